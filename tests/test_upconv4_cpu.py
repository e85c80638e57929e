"""The 25-product F(4x4,3x3) up-convolution (csrc/rcu_wino4_up.hip) without a GPU: its algebra restated in numpy, the planner's choice of it
(rcu_unet_options.upconv_winograd4) and an audit of the code hipcc generates for it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from plan_rows import plan_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Lavin & Gray's F(4x4,3x3), interpolation points 0, +-1, +-2, inf
B4T = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=np.float64)
G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=np.float64)
A4T = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)
KEEP = [0, 1, 3, 4, 5]                   # the positions of a direction that survive: the point -1 (row 2) vanishes on an up-sampled image
VALUE_OF = [0, 1, 2, 2, 3]               # which of the 4 transformed values a surviving position reads
# the reduced transform of a raw low-resolution quadruple (a, b, c, d): rows 0, 1, 4, 5 of B4T applied to (a, b, b, c, c, d)
T4 = np.array([[4, -5, 1, 0], [0, -8, 2, 0], [0, 1, -1, 0], [0, 4, -5, 1]], dtype=np.float64)
SCALE = np.array([1, 1, -3, 1, 1], dtype=np.float64)      # row 3 of B4T gives -3 (b - c): folded into the weights


def upconv25(z, w, bias):
    """nearest x2 -> conv3x3 (padding 1) of z [C, h, w] with weights [O, C, 3, 3] in the 25-product form, tile by tile from the raw 4x4
    low-resolution patch with LOW-RESOLUTION zero padding only.  Returns [O, 2h, 2w] and the number of products per tile and (cin, cout)."""
    c, h, wd = z.shape
    o = w.shape[0]
    u = np.einsum('ir,ocrs,js->ocij', G4, w, G4)[:, :, KEEP][:, :, :, KEEP] * SCALE[:, None] * SCALE[None, :]      # [O, C, 5, 5]
    zp = np.zeros((c, h + 2, wd + 2), dtype=z.dtype)
    zp[:, 1:-1, 1:-1] = z
    at = A4T[:, KEEP]
    out = np.zeros((o, 2 * h, 2 * wd), dtype=z.dtype)
    products = 0
    for ty in range(0, 2 * h, 4):
        for tx in range(0, 2 * wd, 4):
            patch = zp[:, ty // 2:ty // 2 + 4, tx // 2:tx // 2 + 4]                   # low-resolution rows ty/2 - 1 .. ty/2 + 2
            v = np.einsum('ir,crs,js->cij', T4, patch, T4)                             # 16 distinct transformed values per channel
            assert v.shape[1:] == (4, 4)
            v25 = v[:, VALUE_OF][:, :, VALUE_OF]                                        # ... feeding 25 positions
            m = np.einsum('ocij,cij->oij', u, v25)
            products = m.shape[1] * m.shape[2]
            out[:, ty:ty + 4, tx:tx + 4] = np.einsum('pi,oij,qj->opq', at, m, at)
    return out + bias[:, None, None], products


def direct(z, w, bias):
    up = z.repeat(2, axis=1).repeat(2, axis=2)
    c, h, wd = up.shape
    p = np.zeros((c, h + 2, wd + 2), dtype=z.dtype)
    p[:, 1:-1, 1:-1] = up
    out = np.zeros((w.shape[0], h, wd), dtype=z.dtype)
    for r in range(3):
        for s in range(3):
            out += np.einsum('oc,chw->ohw', w[:, :, r, s], p[:, r:r + h, s:s + wd])
    return out + bias[:, None, None]


def test_vanishing_point_and_shared_rows():
    a, b, c, d = np.random.default_rng(0).standard_normal(4)
    t = B4T @ np.array([a, b, b, c, c, d])
    assert abs(t[2]) < 1e-15 and abs(t[3] + 3 * t[4]) < 1e-14
    assert np.allclose(t[[0, 1, 4, 5]], T4 @ np.array([a, b, c, d]), atol=1e-14)


@pytest.mark.parametrize('cin,cout', [(3, 5), (7, 1)])
def test_25_products_match_upsample_then_conv(cin, cout):
    rng = np.random.default_rng(cin)
    z = rng.standard_normal((cin, 6, 10))
    w = rng.standard_normal((cout, cin, 3, 3))
    bias = rng.standard_normal(cout)
    got, products = upconv25(z, w, bias)
    assert products == 25
    ref = direct(z, w, bias)
    assert got.shape == ref.shape == (cout, 12, 20)
    assert np.max(np.abs(got - ref)) < 1e-12


OLD = ['upconv_winograd<S8T4x8,N64,K8>', 'upconv_winograd<S2T8x16,N64,K8>', 'upconv_winograd<T16x16,N64,K8>', 'upconv_winograd<T16x32,N32,K8>']
NEW = ['upconv_winograd4<S8T8x16,N32,K8>', 'upconv_winograd4<S2T16x32,N32,K8>', 'upconv_winograd4<T32x32,N32,K8>', 'upconv_winograd4<T32x32,N32,K8>']
# what the default rule (csrc/rcu_plan.hip, upconv4_wins) takes per plan size of the 192x128 BraTS shape: the per-layer gate admitted every size
# it measured, 160 to 640 samples (profiles/upconv4_layer_gate.txt); the rule keeps to the plans of the pass-group launches, 480 samples and
# up, because a 160-sample plan must give the bits of an 8-sample one (tests/test_gpu_fullsize.py)
DEFAULT_PLANS = {8: OLD, 160: OLD, 320: OLD, 479: OLD, 480: NEW, 640: NEW}


def _ups(rows):
    return [r['kernel'] for r in rows if 'upconv' in r['name']]


def test_planner_takes_the_25_product_upconvolutions_by_option_and_plan_size():
    from rcu_amd import _lib
    lib = _lib.load()
    opts = _lib.UnetOptions()
    lib.rcu_unet_default_options(ctypes.byref(opts))
    assert opts.upconv_winograd4 == 1 and ctypes.sizeof(_lib.UnetOptions) == 8 * 4
    for n, want in DEFAULT_PLANS.items():
        assert _ups(plan_rows(192, 128, n)) == want, n
        assert _ups(plan_rows(192, 128, n, dict(upconv_winograd4=0))) == OLD, n
        assert sum('winograd' in r['kernel'] for r in plan_rows(192, 128, n)) == 22
    small = plan_rows(192, 128, 8, dict(upconv_winograd4=2))
    assert _ups(small) == NEW                                    # all three geometries, whatever the fill
    for r in small:
        if 'upconv' in r['name']:
            assert r['grid'] == (r['height'] // 2, r['width'] // 2)      # the tiles walk the low-resolution level
            assert r['mfma_flops'] == pytest.approx(r['flops'] * 25 / 144, rel=1e-12)      # executed = canonical x 25 / 144
    # everything but the up-convolutions is the option-0 plan
    zero = plan_rows(192, 128, 8, dict(upconv_winograd4=0))
    assert [r for r in small if 'upconv' not in r['name']] == [r for r in zero if 'upconv' not in r['name']]
    assert zero == plan_rows(192, 128, 8)
    # a value outside 0..2 is refused
    desc = _lib.UnetDesc(nb_classes=2, in_channels=4, depth=4, start_filters=32, has_dropout=1, dropout_center=-1, sigma_out=0, bn=1, height=192, width=128,
                         max_batch=8)
    for bad in (3, -1):
        opts.upconv_winograd4 = bad
        handle = ctypes.c_void_p()
        assert lib.rcu_unet_plan(ctypes.byref(desc), ctypes.byref(opts), ctypes.byref(handle)) == -1
        assert b'rcu_unet_options' in lib.rcu_last_error()
    # padded levels (the native 240x240 slices) keep the sub-pixel kernels under every value
    for value in (0, 1, 2):
        native = plan_rows(240, 240, 155, dict(upconv_winograd4=value))
        assert native == plan_rows(240, 240, 155, dict(upconv_winograd4=0))
        assert all(k.startswith('upconv_winograd<') for k in _ups(native)), value
    # a level of exactly one 32x32 tile
    assert _ups(plan_rows(64, 64, 2, dict(upconv_winograd4=2), depth=2)) == ['upconv_winograd4<T32x32,N32,K8>'] * 2


@pytest.mark.timeout(600)
def test_upconv4_kernel_owns_its_accumulator_file(tmp_path):
    """csrc/rcu_wino4_up.hip names its 200 accumulator registers literally in inline assembly, as csrc/rcu_wino4.hip does: the compiler must keep out of
    the accumulator file and spill nothing -- no scratch, no VGPR spill, no v_accvgpr_* outside the asm statements, 200 AGPRs in the descriptor."""
    csrc = os.path.join(ROOT, 'reliability-challenges-uncertainty_amd', 'csrc')
    cmd = ['/opt/rocm/bin/hipcc', '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-fno-slp-vectorize', '--cuda-device-only', '-S',
           os.path.join(csrc, 'rcu_wino4_up.hip'), '-o', str(tmp_path / 'u4.s')]
    subprocess.check_call(cmd, cwd=str(tmp_path))
    text = open(str(tmp_path / 'u4.s')).read()
    assert len(re.findall(r'\.amdhsa_kernel (\S*up_wino4_stream\S*)', text)) == 3
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
    blocks = [b for b in meta.split('- .agpr_count:')[1:] if 'up_wino4_stream' in b]
    assert len(blocks) == 3
    for block in blocks:
        assert int(block.split()[0]) == 200
        assert int(re.search(r'\.vgpr_spill_count:\s*(\d+)', block).group(1)) == 0
        assert int(re.search(r'\.private_segment_fixed_size:\s*(\d+)', block).group(1)) == 0
