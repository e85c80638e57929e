"""The pixel-pair ("paired") activation layout, without a GPU: the LDS geometry of the F(4x4,3x3) kernels that read it (csrc/rcu_wino4_geom.h, walked
by the host program tests/paired_geometry_check.cpp: every staged unit fetched once, the bank model of the patch reads, reads == what the slot plan
put there), which tensors the planner pairs (rcu_unet_layer_layouts), and the audit of the kernels that write it (conv_wino4_pairs,
up_wino4_pairs: what tests/test_abi_cpu.py and tests/test_upconv4_cpu.py audit for the kernels that do not)."""
import ctypes
import os
import re
import subprocess

import pytest

from plan_rows import DESC_DEFAULTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'reliability-challenges-uncertainty_amd', 'csrc')
NHWC, BLOCKED, PAIRED = 0, 1, 2
W4, UP4, W2, FIRST = 'conv3x3_winograd4<', 'upconv_winograd4<', 'conv3x3_winograd<', 'conv3x3_first<'


def test_paired_lds_geometry_of_every_tile_type(tmp_path):
    exe = str(tmp_path / 'paired_geometry_check')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-I', CSRC, os.path.join(ROOT, 'tests', 'paired_geometry_check.cpp'), '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    assert run.returncode == 0 and run.stdout.strip().endswith('0 failures'), run.stdout


def plan_layouts(height, width, max_batch, options=None, **desc):
    """One dict per layer: name, kernel and the layouts (src1, src2, out, pooled) of its tensors."""
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    lib = _lib.load()
    d = _lib.UnetDesc(height=height, width=width, max_batch=max_batch, **{k: int(v) for k, v in dict(DESC_DEFAULTS, **desc).items()})
    opts = _lib.UnetOptions()
    lib.rcu_unet_default_options(ctypes.byref(opts))
    for key, value in (options or {}).items():
        setattr(opts, key, value)
    handle = ctypes.c_void_p()
    _lib.check(lib.rcu_unet_plan(ctypes.byref(d), ctypes.byref(opts), ctypes.byref(handle)))
    try:
        rows = []
        for i in range(lib.rcu_unet_num_layers(handle)):
            info = _lib.LayerInfo()
            _lib.check(lib.rcu_unet_layer_info(handle, i, ctypes.byref(info)))
            v = [ctypes.c_int32() for _ in range(4)]
            _lib.check(lib.rcu_unet_layer_layouts(handle, i, *[ctypes.byref(x) for x in v]))
            rows.append(dict(name=info.name.decode(), kernel=info.kernel.decode(), layouts=tuple(x.value for x in v)))
        assert lib.rcu_unet_layer_layouts(handle, len(rows), None, None, None, None) == -1
        return rows
    finally:
        lib.rcu_unet_destroy(handle)


def test_headline_plan_pairs_everything_between_the_first_unit_and_the_head():
    rows = plan_layouts(192, 128, 640)
    assert rows[0]['kernel'].startswith(FIRST) and rows[0]['layouts'] == (NHWC, -1, PAIRED, -1)
    assert rows[-1]['name'].startswith('conv_cls.0') and rows[-1]['layouts'] == (PAIRED, -1, NHWC, -1)
    for r in rows[1:-1]:
        assert r['kernel'].startswith((W4, UP4)), r
        assert all(v in (PAIRED, -1) for v in r['layouts']), r
    assert sum(r['layouts'][1] == PAIRED for r in rows) == 4 and sum(r['layouts'][3] == PAIRED for r in rows) == 4


def test_tensors_an_f2_kernel_touches_stay_unpaired():
    rows = plan_layouts(192, 128, 8)
    touched = [r for r in rows if not r['kernel'].startswith((W4, UP4, FIRST))]
    assert any(r['kernel'].startswith(W2) for r in touched)
    for r in touched:
        assert PAIRED not in r['layouts'], r
    # and whatever is paired lies between kernels that can: a unit's output and pooled output alike, the two sources of a unit alike
    for r in rows:
        s1, s2, out, pool = r['layouts']
        assert s2 == -1 or (s1 == PAIRED) == (s2 == PAIRED), r
        assert pool == -1 or (out == PAIRED) == (pool == PAIRED), r


@pytest.mark.parametrize('options, desc', [(dict(pad_levels=1), dict(height=240, width=240)), (dict(act_layout=2), dict(height=192, width=128)),
                                           (dict(act_layout=1), dict(height=192, width=128))])
def test_padded_levels_and_the_blocked_option_pair_nothing(options, desc):
    rows = plan_layouts(desc['height'], desc['width'], 640, options)
    assert all(PAIRED not in r['layouts'] for r in rows)
    if options.get('act_layout') == 2:      # what act_layout = 0 was before the paired layout
        assert all(v in (BLOCKED, -1) for r in rows[1:-1] for v in r['layouts'])
    if options.get('act_layout') == 1:
        assert all(v in (NHWC, -1) for r in rows for v in r['layouts'])


def test_feature_tensor_stays_channels_last():
    rows = plan_layouts(192, 128, 640, provide_features=1)
    assert rows[-1]['layouts'][0] == NHWC and rows[-2]['layouts'][2] == NHWC
    assert rows[-2]['layouts'][0] == PAIRED      # the rest of the plan is not affected


def _asm(tmp_path, source):
    out = str(tmp_path / (source + '.s'))
    subprocess.check_call(['/opt/rocm/bin/hipcc', '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-fno-slp-vectorize', '--cuda-device-only', '-S',
                           os.path.join(CSRC, source), '-o', out], cwd=str(tmp_path))
    return open(out).read()


def _kernel_bodies(text, pattern):
    """name -> the instructions of every kernel whose symbol matches `pattern`"""
    bodies = {}
    for m in re.finditer(r'^(\S*' + pattern + r'\S*):[^\n]*\n(.*?)\n\s*s_endpgm', text, re.S | re.M):
        bodies[m.group(1)] = m.group(2)
    return bodies


@pytest.mark.timeout(900)
@pytest.mark.parametrize('source, paired, plain, n_paired, agprs', [('rcu_wino4.hip', 'conv_wino4_pairs', 'conv_wino4_stream', 5, 256),
                                                                   ('rcu_wino4_up.hip', 'up_wino4_pairs', 'up_wino4_stream', 3, 200)])
def test_paired_kernels_pass_the_accumulator_audit_and_drop_the_lane_trade(tmp_path, source, paired, plain, n_paired, agprs):
    """The kernels that write paired tensors: no scratch, no spill, no compiler-made v_accvgpr_*, the accumulator file as it is (the audits of
    test_abi_cpu.py / test_upconv4_cpu.py, which cover the whole file's text but read the descriptors of the other kernels only) -- and no DPP
    move and fewer selects than the kernel of the same tile that trades lanes."""
    text = _asm(tmp_path, source)
    assert len(re.findall(r'\.amdhsa_kernel (\S*' + paired + r'\S*)', text)) == n_paired
    inside, stray = False, []
    for line in text.splitlines():
        if ';;#ASMSTART' in line:
            inside = True
        elif ';;#ASMEND' in line:
            inside = False
        elif 'v_accvgpr' in line and not inside:
            stray.append(line.strip())
    assert not stray, stray[:5]
    assert 'scratch_' not in text
    meta = text[text.index('amdhsa.kernels'):]
    blocks = [b for b in meta.split('- .agpr_count:')[1:] if paired in b]
    assert len(blocks) == n_paired
    for block in blocks:
        assert int(block.split()[0]) == agprs
        assert int(re.search(r'\.vgpr_spill_count:\s*(\d+)', block).group(1)) == 0
        assert int(re.search(r'\.private_segment_fixed_size:\s*(\d+)', block).group(1)) == 0
    with_trade, without = _kernel_bodies(text, plain), _kernel_bodies(text, paired)
    assert len(without) == n_paired
    for name, body in without.items():
        assert 'quad_perm' not in body, name
        tile = re.search(r'(Wino4Tile|Up4Tile)I\w*?EE', name).group(0)
        twin = [b for n, b in with_trade.items() if tile in n and tile + 'ELb1E' not in n]      # (not the +head kernel: it stores no activations)
        assert twin, name
        print(name, 'v_cndmask', body.count('v_cndmask'), 'against', min(b.count('v_cndmask') for b in twin),
              'instructions', body.count('\n'), 'against', min(b.count('\n') for b in twin))
        # the trade selects which two components a lane sends and which it keeps for each of a tile's 8 stores, four tiles per lane: at least
        # 4 selects x 32 stores = 128 v_cndmask that the paired epilogue has no use for
        assert body.count('v_cndmask') + 100 < min(b.count('v_cndmask') for b in twin), name
