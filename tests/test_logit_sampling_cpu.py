"""Test-time logit sampling without a GPU: the C ABI (symbols, argument validation before the device is touched) and the YAML surface of the
test scripts (others.logit_samples, others.is_log_sigma)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('rcu_logit_normals', 'rcu_logit_sampling', 'rcu_unet_forward_sample_sigma_passes')


@pytest.fixture(scope='module')
def lib():
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    return _lib


def test_logit_sampling_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, 'include', 'rcu.h')).read()
    declared = set(re.findall(r'\b(rcu_[a-z0-9_]+)\s*\(', header))
    so = lib.load()
    for name in NAMES:
        assert name in declared and name in lib.SIGNATURES and hasattr(so, name), name
    assert '#define RCU_LOGIT_MAX_SAMPLES 1024' in header and lib.RCU_LOGIT_MAX_SAMPLES == 1024


def _refused(so, status, *words):
    assert status == -1        # RCU_ERR_INVALID
    msg = so.rcu_last_error()
    for w in words:
        assert w in msg, (w, msg)


def test_standalone_argument_validation_without_gpu(lib):
    so = lib.load()
    mu, raw, probs, stats, out = (ctypes.c_void_p(v) for v in (1 << 20, 1 << 30, 1 << 31, 1 << 32, 1 << 33))

    def normals(key=5, first=0, n=2, hw=64, c=2, s=10, o=out):
        return so.rcu_logit_normals(key, first, n, hw, c, s, o, None)

    def sampling(m=mu, r=raw, n=2, hw=64, c=2, log=0, s=10, key=5, first=0, p=probs, st=stats, flags=lib.RCU_MC_EXACT):
        return so.rcu_logit_sampling(m, r, n, hw, c, log, s, key, first, p, st, flags, None)

    for s in (0, -1, 1025):
        _refused(so, normals(s=s), b'samples')
        _refused(so, sampling(s=s), b'samples')
    for c in (0, 9, -1):
        _refused(so, normals(c=c), b'nb_classes')
        _refused(so, sampling(c=c), b'nb_classes')
    _refused(so, normals(hw=1 << 32), b'hw', b'2^32')
    _refused(so, sampling(hw=1 << 32), b'hw', b'2^32')
    _refused(so, normals(n=0), b'empty')
    _refused(so, sampling(hw=0), b'empty')
    _refused(so, normals(o=None), b'null')
    _refused(so, sampling(m=None), b'null')
    _refused(so, sampling(r=None), b'null')
    _refused(so, sampling(p=None, st=None), b'both null')
    _refused(so, sampling(flags=lib.RCU_MC_INPUT_PROBS), b'flags')


def _plan(lib, sigma_out, max_batch=8):
    so = lib.load()
    desc = lib.UnetDesc(nb_classes=2, in_channels=4, depth=2, start_filters=8, has_dropout=1, dropout_center=-1, sigma_out=int(sigma_out),
                        bn=1, height=32, width=32, max_batch=max_batch, residual=0, provide_features=0)
    h = ctypes.c_void_p()
    assert so.rcu_unet_plan(ctypes.byref(desc), None, ctypes.byref(h)) == 0
    return h


def test_forward_argument_validation_without_gpu(lib):
    so = lib.load()
    x, stats, ssum = (ctypes.c_void_p(v) for v in (1 << 20, 1 << 30, 1 << 31))
    keys = (ctypes.c_uint64 * 4)(1, 2, 3, 4)

    def fwd(h, xx=x, n=2, passes=4, k=keys, s=10, st=stats, sm=ssum):
        return so.rcu_unet_forward_sample_sigma_passes(h, xx, n, passes, None, k, 0, s, st, lib.RCU_MC_EXACT, sm, 0, None)

    h = _plan(lib, sigma_out=True)
    try:
        for s in (0, 1025):
            _refused(so, fwd(h, s=s), b'samples')
        _refused(so, fwd(h, n=3), b'max_batch')        # 3 x 4 > 8
        _refused(so, fwd(h, passes=0), b'max_batch')
        _refused(so, fwd(h, n=0), b'max_batch')
        _refused(so, fwd(h, xx=None), b'null')
        _refused(so, fwd(h, k=None), b'null')
        _refused(so, fwd(h, st=None), b'null')
        _refused(so, fwd(h, sm=None), b'null')
    finally:
        so.rcu_unet_destroy(h)
    _refused(so, fwd(None), b'null handle')
    h = _plan(lib, sigma_out=False)
    try:
        _refused(so, fwd(h), b'sigma_out')
    finally:
        so.rcu_unet_destroy(h)


def test_step_constructors_validate_the_sample_count():
    from rcu_amd import steps
    for bad in (-1, 1025, 2.0, '10', True, None):
        with pytest.raises(ValueError, match='logit_samples'):
            steps.AleatoricPredictStep(logit_samples=bad)
        with pytest.raises(ValueError, match='logit_samples'):
            steps.AleatoricMcPredictStep(4, logit_samples=bad)
    assert steps.AleatoricPredictStep(logit_samples=0).logit_samples == 0
    assert steps.AleatoricMcPredictStep(4, logit_samples=1024, seed=3).logit_samples == 1024


def _context(others, seed=20):
    from rcu_amd import config as cfg
    from rcu_amd import loops
    context = loops.TorchTestContext('cpu')
    context.config = cfg.TestConfiguration()
    context.config.seed = seed
    context.config.others = cfg.OtherParameters().from_dict(others)
    return context


def test_aleatoric_steps_follow_the_yaml():
    from rcu_amd import distributed as rdist
    from rcu_amd import scripts, steps
    world = rdist.World()
    (step,) = scripts._aleatoric_steps(_context({}), world)
    assert type(step) is steps.AleatoricPredictStep and step.is_log_sigma is False and step.logit_samples == 0
    (step,) = scripts._aleatoric_steps(_context(dict(is_log_sigma=True)), world)
    assert type(step) is steps.AleatoricPredictStep and step.is_log_sigma is True and step.logit_samples == 0
    # others.mc without logit_samples: not read by the aleatoric script, as before
    (step,) = scripts._aleatoric_steps(_context(dict(mc=4)), world)
    assert type(step) is steps.AleatoricPredictStep and step.logit_samples == 0
    (step,) = scripts._aleatoric_steps(_context(dict(logit_samples=10, is_log_sigma=True), seed=7), world)
    assert type(step) is steps.AleatoricPredictStep and (step.is_log_sigma, step.logit_samples, step.seed) == (True, 10, 7)
    mc, summary = scripts._aleatoric_steps(_context(dict(logit_samples=10, mc=4, is_log_sigma=True), seed=7), world)
    assert type(mc) is steps.AleatoricMcPredictStep and type(summary) is steps.MultiPredictionSummary
    assert (mc.mc_steps, mc.is_log_sigma, mc.logit_samples, mc.seed) == (4, True, 10, 7)
    for bad in (0, 1025, -3, 2.5, '10', True, None, [10]):
        with pytest.raises(ValueError, match='others.logit_samples'):
            scripts._aleatoric_steps(_context(dict(logit_samples=bad)), world)


YAML = """
config:
  test_name: brats_test_x
  test_dir: {test_dir}
  model_dir: {model_dir}
  seed: 20
  test_at: best
  others:
    model_dir: [{model_dir}]
    logit_samples: 10
meta:
  type: test-config
  version: 0
"""


@pytest.mark.parametrize('script', ['test_default', 'test_ensemble', 'test_auxiliary_feat', 'test_auxiliary_segm'])
def test_other_scripts_refuse_the_logit_samples_key(tmp_path, monkeypatch, script):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    path = tmp_path / 'test_brats_x.yaml'
    path.write_text(YAML.format(test_dir=tmp_path / 'out', model_dir=tmp_path / 'train' / 'model_x'))
    kwargs = dict(config_file=str(path), device='cpu')
    with pytest.raises(ValueError, match='others.logit_samples'):
        getattr(scripts, script)('brats', **kwargs)
    assert not (tmp_path / 'out').exists()


def test_fit_script_refuses_the_logit_samples_key(tmp_path, monkeypatch):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    path = tmp_path / 'fit.yaml'
    path.write_text(YAML.format(test_dir=tmp_path / 'out', model_dir=tmp_path / 'train' / 'model_x'))
    with pytest.raises(ValueError, match='others.logit_samples'):
        scripts.fit_temperature('brats', str(path), device='cpu')
    assert not (tmp_path / 'out').exists()
