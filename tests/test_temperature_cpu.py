"""Temperature scaling without a GPU: the C ABI (symbols, argument validation), the candidate grid, the parabola refinement, loading T and
the YAML surface of the test scripts."""
import ctypes
import json
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('rcu_unet_set_temperature', 'rcu_temperature_nll_workspace_bytes', 'rcu_temperature_nll', 'rcu_temperature_nll_terms')


@pytest.fixture(scope='module')
def lib():
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    return _lib


def test_temperature_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, 'include', 'rcu.h')).read()
    declared = set(re.findall(r'\b(rcu_[a-z0-9_]+)\s*\(', header))
    so = lib.load()
    for name in NAMES:
        assert name in declared and name in lib.SIGNATURES and hasattr(so, name), name


def test_sweep_argument_validation_without_gpu(lib):
    so = lib.load()
    x, t, out, ws = (ctypes.c_void_p(v) for v in (1 << 20, 1 << 30, 1 << 31, 1 << 32))
    betas = (ctypes.c_float * 129)(*([1.0] * 129))

    def refused(status, *words):
        assert status == -1        # RCU_ERR_INVALID
        msg = so.rcu_last_error()
        for w in words:
            assert w in msg, (w, msg)

    def sweep(logits=x, passes=3, n=2, hw=64, c=2, target=t, mask=None, b=betas, k=97, o=out, w=ws):
        return so.rcu_temperature_nll(logits, passes, n, hw, c, target, mask, b, k, o, w, None)

    for k in (0, 129, -1):
        refused(sweep(k=k), b'n_candidates')
    for c in (1, 9, 0):
        refused(sweep(c=c), b'nb_classes')
        refused(so.rcu_temperature_nll_terms(x, 3, 2, 64, c, t, None, 1.0, out, None), b'nb_classes')
    for p in (0, 2049):
        refused(sweep(passes=p), b'passes')
        refused(so.rcu_temperature_nll_terms(x, p, 2, 64, 2, t, None, 1.0, out, None), b'passes')
    refused(sweep(logits=None), b'null')
    refused(sweep(target=None), b'null')
    refused(sweep(o=None), b'null')
    refused(sweep(w=None), b'null')
    refused(sweep(b=None), b'null')
    refused(so.rcu_temperature_nll_terms(x, 3, 2, 64, 2, t, None, 1.0, None, None), b'null')
    refused(sweep(n=0), b'empty')
    refused(sweep(n=1 << 20, hw=1 << 12), b'2^32')
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        bb = (ctypes.c_float * 3)(1.0, bad, 2.0)
        refused(sweep(b=bb, k=3), b'beta[1]')
        refused(so.rcu_temperature_nll_terms(x, 3, 2, 64, 2, t, None, bad, out, None), b'beta')
    assert so.rcu_temperature_nll_workspace_bytes(155 * 240 * 240, 97) >= 99 * 8
    assert so.rcu_temperature_nll_workspace_bytes(64, 97) == 99 * 8


def _plan(lib, sigma_out):
    so = lib.load()
    desc = lib.UnetDesc(nb_classes=2, in_channels=4, depth=2, start_filters=8, has_dropout=1, dropout_center=-1, sigma_out=int(sigma_out),
                        bn=1, height=32, width=32, max_batch=2, residual=0, provide_features=0)
    h = ctypes.c_void_p()
    assert so.rcu_unet_plan(ctypes.byref(desc), None, ctypes.byref(h)) == 0
    return h


def test_set_temperature_validation_without_gpu(lib):
    so = lib.load()
    h = _plan(lib, sigma_out=False)
    try:
        for bad in (0.0, -1.0, float('nan'), float('inf'), -float('inf')):
            assert so.rcu_unet_set_temperature(h, bad) == -1, bad
            assert b'finite' in so.rcu_last_error()
        assert so.rcu_unet_set_temperature(h, 1.5) == 0
        assert so.rcu_unet_set_temperature(h, 1.0) == 0
    finally:
        so.rcu_unet_destroy(h)
    assert so.rcu_unet_set_temperature(None, 1.5) == -1
    h = _plan(lib, sigma_out=True)
    try:
        assert so.rcu_unet_set_temperature(h, 1.5) == -1
        assert b'sigma' in so.rcu_last_error()
    finally:
        so.rcu_unet_destroy(h)


def test_model_set_temperature_validates_and_repacks():
    from rcu_amd.model import UNet
    m = UNet(2, 4, depth=2, start_filters=8)
    assert m.temperature == 1.0
    version = m._weights_version
    m.set_temperature(2)
    assert m.temperature == 2.0 and m._weights_version == version + 1
    for bad in (0, -1, float('nan'), float('inf'), 'x', None, True):
        with pytest.raises(ValueError):
            m.set_temperature(bad)
    assert m.temperature == 2.0
    keys = set(m.state_dict())
    assert not any('temperature' in k for k in keys)
    with pytest.raises(ValueError, match='sigma'):
        UNet(2, 4, depth=2, start_filters=8, sigma_out=True).set_temperature(1.5)


def test_candidate_grid():
    from rcu_amd import calibration as cal
    c = cal.CANDIDATES
    assert len(c) == 97 and all(a < b for a, b in zip(c, c[1:]))
    assert c[48] == 1.0 and c[0] == 0.125 and c[96] == 8.0
    for k, t in enumerate(c):
        assert t == 2.0 ** ((k - 48) / 16)


def test_refine_recovers_the_vertex_of_a_parabola_in_log2_t():
    from rcu_amd import calibration as cal
    for x_star in (-0.3, 0.0, 0.51234, 1.7, -2.93):
        sums = [1e9 + 1e9 * (math.log2(t) - x_star) ** 2 for t in cal.CANDIDATES]
        r = cal.refine(cal.CANDIDATES, sums)
        assert not r.at_edge
        assert abs(math.log2(r.temperature) - x_star) < 1e-9, (x_star, r)
        assert r.index == min(range(97), key=lambda k: abs(math.log2(cal.CANDIDATES[k]) - x_star))


def test_refine_handles_ties_and_flags_both_edges(caplog):
    from rcu_amd import calibration as cal
    c = cal.CANDIDATES
    # a flat minimum over k = 40, 41: the smallest k is k*, the vertex lies half way between the two
    sums = [100 + abs(k - 40.5) * 2 - 1 for k in range(97)]
    sums[40] = sums[41] = 50
    r = cal.refine(c, sums)
    assert r.index == 40 and not r.at_edge
    assert math.log2(r.temperature) == pytest.approx((math.log2(c[40]) + math.log2(c[41])) / 2, abs=1e-12)
    # a flat curve: the smallest k, which is an edge
    r = cal.refine(c, [10] * 97)
    assert r.index == 0 and r.at_edge and r.temperature == c[0]
    # both edges
    caplog.clear()
    with caplog.at_level('WARNING'):
        r = cal.refine(c, list(range(97)))
        assert r.at_edge and r.index == 0 and r.temperature == 0.125
        r = cal.refine(c, list(range(97, 0, -1)))
        assert r.at_edge and r.index == 96 and r.temperature == 8.0
    assert sum('end of the candidate grid' in m for m in caplog.messages) == 2
    # integer sums beyond 2^53 keep their order
    big = [(1 << 60) + abs(k - 30) for k in range(97)]
    assert cal.refine(c, big).index == 30


def test_load_temperature(tmp_path):
    from rcu_amd import calibration as cal
    assert cal.load_temperature(1.5) == 1.5 and cal.load_temperature(2) == 2.0
    good = tmp_path / 't.json'
    good.write_text(json.dumps({'temperature': 0.75, 'voxels': 10}))
    assert cal.load_temperature(str(good)) == 0.75
    assert cal.load_temperature(good) == 0.75
    for bad in (0, -1, float('nan'), float('inf'), None, True, [1.0]):
        with pytest.raises(ValueError):
            cal.load_temperature(bad)
    with pytest.raises(ValueError):
        cal.load_temperature(str(tmp_path / 'missing.json'))
    nokey = tmp_path / 'nokey.json'
    nokey.write_text(json.dumps({'T': 1.5}))
    with pytest.raises(ValueError, match='temperature'):
        cal.load_temperature(str(nokey))
    zero = tmp_path / 'zero.json'
    zero.write_text(json.dumps({'temperature': 0.0}))
    with pytest.raises(ValueError):
        cal.load_temperature(str(zero))


def _context(others, seed=20):
    from rcu_amd import config as cfg
    from rcu_amd import loops
    context = loops.TorchTestContext('cpu')
    context.config = cfg.TestConfiguration()
    context.config.seed = seed
    context.config.others = cfg.OtherParameters().from_dict(others)
    return context


def test_yaml_temperature_reaches_the_model(tmp_path):
    from rcu_amd import scripts
    from rcu_amd.model import UNet
    assert scripts._temperature_hooks(_context(dict(mc=5))) == []
    hooks = scripts._temperature_hooks(_context(dict(mc=5, temperature=1.25)))
    assert len(hooks) == 1 and hooks[0].temperature == 1.25
    path = tmp_path / 'temperature.json'
    path.write_text(json.dumps({'temperature': 0.5}))
    (hook,) = scripts._temperature_hooks(_context(dict(temperature=str(path))))
    ctx = _context({})
    ctx.model = UNet(2, 4, depth=2, start_filters=8)
    hook.end_startup(ctx)
    assert ctx.model.temperature == 0.5
    with pytest.raises(ValueError):
        scripts._temperature_hooks(_context(dict(temperature=-2.0)))
    with pytest.raises(ValueError):
        scripts._temperature_hooks(_context(dict(temperature=str(tmp_path / 'none.json'))))
    # every rank of a sharded run gets the hook: a rank other than the root runs it in its own (otherwise empty) hook
    composed = __import__('rcu_amd.loops', fromlist=['x']).ReducedComposeTestLoopHook([hook])
    ctx.model = UNet(2, 4, depth=2, start_filters=8)
    composed.end_startup(ctx)
    assert ctx.model.temperature == 0.5


YAML = """
config:
  test_name: brats_test_x
  test_dir: {test_dir}
  model_dir: {model_dir}
  seed: 20
  test_at: best
  others:
    model_dir: [{model_dir}]
    temperature: 1.5
meta:
  type: test-config
  version: 0
"""


@pytest.mark.parametrize('script', ['test_ensemble', 'test_aleatoric', 'test_auxiliary_feat', 'test_auxiliary_segm'])
def test_other_scripts_refuse_the_temperature_key(tmp_path, monkeypatch, script):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    path = tmp_path / 'test_brats_x.yaml'
    path.write_text(YAML.format(test_dir=tmp_path / 'out', model_dir=tmp_path / 'train' / 'model_x'))
    with pytest.raises(ValueError, match='others.temperature'):
        getattr(scripts, script)('brats', config_file=str(path), device='cpu')
    assert not (tmp_path / 'out').exists()


def test_fit_script_refuses_tta_and_multi_rank(tmp_path, monkeypatch):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    path = tmp_path / 'fit.yaml'
    path.write_text(YAML.format(test_dir=tmp_path / 'out', model_dir=tmp_path / 'train' / 'model_x')
                    .replace('    temperature: 1.5\n', '    tta: [identity, flip_h]\n'))
    with pytest.raises(ValueError, match='others.tta'):
        scripts.fit_temperature('brats', str(path), device='cpu')
    assert not (tmp_path / 'out').exists()
