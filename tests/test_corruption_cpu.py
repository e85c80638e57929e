"""Input corruptions without a GPU: the YAML value's parser, the severity tables against include/rcu.h, the key contract, the host-made taps and
bias coefficients, the C ABI (symbols, argument validation), the script surface and the float64 restatement against its frozen outputs."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import scipy.ndimage

import corruption_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------- parse
def test_parse_accepts_one_mapping_or_a_list_in_order():
    from rcu_amd import corruption as co
    assert co.KINDS == cr.KINDS
    (s,) = co.parse({'kind': 'gaussian_blur', 'severity': 2})
    assert (s.kind, s.code, s.amount, s.severity, s.channels) == ('gaussian_blur', 1, 1.0, 2, None)
    stages = co.parse([{'kind': 'gaussian_blur', 'severity': 2}, {'kind': 'gaussian_noise', 'amount': 0.25},
                       {'kind': 'channel_drop', 'channels': [3, 1]}, {'kind': 'downsample', 'amount': 3}])
    assert [s.kind for s in stages] == ['gaussian_blur', 'gaussian_noise', 'channel_drop', 'downsample']
    assert [s.code for s in stages] == [1, 0, 7, 2]
    assert stages[1].amount == 0.25 and stages[1].severity is None
    assert stages[2].amount == 10.0 and stages[2].channels == (1, 3)
    assert co.parse({'kind': 'channel_drop', 'amount': 6})[0].channels == (1, 2)
    assert len(co.parse([{'kind': 'intensity_shift', 'amount': -0.5}] * 8)) == 8
    for code, kind in enumerate(co.KINDS):
        if kind != 'channel_drop':
            for severity in range(1, 6):
                (s,) = co.parse({'kind': kind, 'severity': severity})
                assert s.code == code and s.amount == co.amount_of(kind, severity) == co.SEVERITY[kind][severity - 1]
    record = co.describe(stages, 20)
    assert json.loads(json.dumps(record)) == record and record['seed'] == 20
    assert record['stages'][0] == {'kind': 'gaussian_blur', 'amount': 1.0, 'severity': 2}
    assert record['stages'][2] == {'kind': 'channel_drop', 'amount': 10.0, 'channels': [1, 3]}


@pytest.mark.parametrize('spec, word', [
    ({'kind': 'fog', 'severity': 1}, 'kind'),
    ({'severity': 1}, 'kind'),
    ({'kind': 'gaussian_blur', 'severity': 1, 'sigma': 2}, 'sigma'),
    ({'kind': 'gaussian_blur', 'severity': 1, 'amount': 1.0}, 'severity'),
    ({'kind': 'gaussian_blur'}, 'severity'),
    ({'kind': 'gaussian_blur', 'severity': 0}, 'severity'),
    ({'kind': 'gaussian_blur', 'severity': 6}, 'severity'),
    ({'kind': 'gaussian_blur', 'severity': 1.5}, 'severity'),
    ({'kind': 'gaussian_blur', 'severity': True}, 'severity'),
    ({'kind': 'channel_drop', 'severity': 1}, 'severity'),
    ({'kind': 'gaussian_noise', 'channels': [0]}, 'channels'),
    ({'kind': 'channel_drop'}, 'channels'),
    ({'kind': 'channel_drop', 'channels': []}, 'channels'),
    ({'kind': 'channel_drop', 'channels': [1, 1]}, 'channels'),
    ({'kind': 'channel_drop', 'channels': [-1]}, 'channels'),
    ({'kind': 'channel_drop', 'channels': [0], 'amount': 1}, 'channels'),
    ({'kind': 'channel_drop', 'amount': 0}, 'amount'),
    ({'kind': 'channel_drop', 'amount': 1.5}, 'amount'),
    ({'kind': 'gaussian_noise', 'amount': -0.1}, 'amount'),
    ({'kind': 'gaussian_blur', 'amount': 0.0}, 'amount'),
    ({'kind': 'gaussian_blur', 'amount': 8.5}, 'amount'),
    ({'kind': 'downsample', 'amount': 1}, 'amount'),
    ({'kind': 'downsample', 'amount': 17}, 'amount'),
    ({'kind': 'contrast', 'amount': 4.5}, 'amount'),
    ({'kind': 'contrast', 'amount': -1}, 'amount'),
    ({'kind': 'intensity_shift', 'amount': float('inf')}, 'amount'),
    ({'kind': 'intensity_shift', 'amount': 'much'}, 'amount'),
    ({'kind': 'bias_field', 'amount': 2.5}, 'amount'),
    ({'kind': 'ghosting', 'amount': 1.5}, 'amount'),
    ('gaussian_blur', 'mapping'),
    ([], 'mapping'),
    ([{'kind': 'ghosting', 'severity': 1}] * 9, '8'),
])
def test_parse_refuses_and_names_the_key(spec, word):
    from rcu_amd import corruption as co
    with pytest.raises(ValueError, match=word):
        co.parse(spec)


def test_severity_tables_equal_the_header_text():
    from rcu_amd import corruption as co
    header = open(os.path.join(ROOT, 'include', 'rcu.h')).read()
    section = header[header.index('Input corruptions (EXTENSION'):]
    found = {}
    for kind, values in re.findall(r'^ \*\s+([a-z_]+)((?:\s+\d+(?:\.\d+)?){5})\s*$', section, flags=re.M):
        found[kind] = tuple(float(v) for v in values.split())
    assert found == {k: tuple(v) for k, v in co.SEVERITY.items()}
    assert set(co.SEVERITY) == set(co.KINDS) - {'channel_drop'}
    assert co.SEVERITY['gaussian_noise'] == (0.1, 0.2, 0.3, 0.5, 0.8) and co.SEVERITY['contrast'] == (0.8, 0.6, 0.45, 0.3, 0.2)
    assert co.SEVERITY['gaussian_blur'] == (0.5, 1, 1.5, 2, 3) and co.SEVERITY['downsample'] == (2, 3, 4, 6, 8)
    assert co.SEVERITY['intensity_shift'] == (0.1, 0.2, 0.3, 0.5, 0.8) and co.SEVERITY['bias_field'] == (0.1, 0.2, 0.3, 0.45, 0.6)
    assert co.SEVERITY['ghosting'] == (0.05, 0.1, 0.15, 0.25, 0.4)
    with pytest.raises(ValueError):
        co.amount_of('channel_drop', 1)
    # the kind codes of the header are the positions in KINDS
    codes = dict(re.findall(r'#define RCU_CORRUPT_([A-Z_]+) (\d+)', header))
    assert [int(codes[k.upper()]) for k in co.KINDS] == list(range(8))


# ------------------------------------------------------------------------------------------- keys, taps, coefficients
def test_corruption_keys_differ_from_every_mask_tta_and_sampling_key():
    from rcu_amd import corruption as co
    from rcu_amd import steps
    for seed in (0, 20, 123456789, 2 ** 40 + 7):
        keys = [co.corruption_seed(seed, s) for s in range(8)]
        assert keys == [(steps.pass_seed(seed, 0) + (16 + s) * 2 ** 40) % (2 ** 63 - 1) for s in range(8)]
        assert len(set(keys)) == 8 and all(0 <= k < 2 ** 63 - 1 for k in keys)
        others = {steps.pass_seed(seed, t) for t in range(0, 2049)}
        others |= {steps.tta_pass_seed(seed, e, t) for e in range(8) for t in range(1, 2049)}
        assert not others & set(keys)
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            co.corruption_seed(20, bad)


@pytest.mark.parametrize('sigma', [0.5, 1, 1.5, 2, 3, 8])
def test_blur_taps_are_scipys_impulse_response(sigma):
    from rcu_amd import corruption as co
    r = int(4 * sigma + 0.5)
    assert co.blur_radius(sigma) == r
    taps = co.blur_taps(sigma)
    assert taps.dtype == np.float64 and taps.shape == (2 * r + 1,)
    line = np.zeros(2 * r + 1)
    line[r] = 1.0
    want = scipy.ndimage.gaussian_filter1d(line, sigma, mode='reflect', truncate=4.0)
    assert np.abs(taps - want).max() <= 1e-15
    assert abs(taps.sum() - 1.0) < 1e-15


def test_bias_coefficients_are_deterministic_normalised_and_differ_by_channel():
    from rcu_amd import corruption as co
    key = co.corruption_seed(20, 0)
    coef = co.bias_coefficients(key, 4)
    assert coef.shape == (4, 8) and coef.dtype == np.float64
    assert np.array_equal(coef, co.bias_coefficients(key, 4))
    assert np.array_equal(coef[:2], co.bias_coefficients(key, 2))
    assert np.abs(np.abs(coef).sum(axis=1) - 1.0).max() < 1e-15
    assert all(not np.array_equal(coef[a], coef[b]) for a in range(4) for b in range(a))
    assert not np.array_equal(coef, co.bias_coefficients(co.corruption_seed(20, 1), 4))
    assert (coef < 0).any() and (coef > 0).any()
    # the restatement the GPU tests compare against is the same function, written twice
    assert np.array_equal(coef, cr.bias_coefficients(key, 4))
    a, b = co.bias_tables(15, 16)
    assert a.shape == (3, 15) and b.shape == (3, 16) and np.all(a[0] == 1.0) and np.all(b[0] == 1.0)
    assert abs(a[1, 0] - np.cos(np.pi * 0.5 / 15)) < 1e-16 and abs(b[2, 15] - np.cos(np.pi * 2 * 15.5 / 16)) < 1e-15


# ------------------------------------------------------------------------------------------- C ABI
def test_corruption_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, 'include', 'rcu.h')).read()
    declared = set(re.findall(r'\b(rcu_[a-z0-9_]+)\s*\(', header))
    so = lib.load()
    for name in ('rcu_corrupt', 'rcu_corrupt_workspace_bytes'):
        assert name in declared and name in lib.SIGNATURES and hasattr(so, name), name
    assert tuple(lib.CORRUPTION_KINDS) == cr.KINDS


def test_corruption_argument_validation_without_gpu(lib):
    so = lib.load()
    x, out, ws = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 40)
    taps = (ctypes.c_float * 9)(*([1.0 / 9] * 9))                # sigma 1: r = 4
    bias = (ctypes.c_float * (32 + 48 + 48))(*([0.125] * 128))   # C = 4, 16 x 16

    def refused(status, *words):
        assert status == -1        # RCU_ERR_INVALID
        msg = so.rcu_last_error()
        assert msg, 'no message'
        for w in words:
            assert w in msg, (w, msg)

    def call(kind, amount, n=2, c=4, h=16, w=16, aux=None, n_aux=0, x_=x, out_=out, ws_=ws):
        return so.rcu_corrupt(x_, n, c, h, w, kind, amount, 7, 2 ** 32 + 5, aux, n_aux, out_, ws_, None)

    # the kind code: never a silent skip
    refused(call(8, 0.1), b'kind')
    refused(call(-1, 0.1), b'kind')
    # pointers, shapes, overlap -- for every kind
    for kind, amount, aux, n_aux in ((0, 0.1, None, 0), (1, 1.0, taps, 9), (2, 2.0, None, 0), (3, 0.5, None, 0), (4, 0.1, None, 0),
                                     (5, 0.3, bias, 128), (6, 0.1, None, 0), (7, 2.0, None, 0)):
        refused(call(kind, amount, aux=aux, n_aux=n_aux, x_=None), b'null')
        refused(call(kind, amount, aux=aux, n_aux=n_aux, out_=None), b'null')
        refused(call(kind, amount, aux=aux, n_aux=n_aux, n=0), b'empty')
        refused(call(kind, amount, aux=aux, n_aux=n_aux, c=0), b'empty')
        refused(call(kind, amount, aux=aux, n_aux=n_aux, out_=x), b'overlap')
        refused(call(kind, amount, aux=aux, n_aux=n_aux, out_=ctypes.c_void_p((1 << 20) + 64)), b'overlap')
        refused(call(kind, float('nan'), aux=aux, n_aux=n_aux), b'finite')
    refused(call(4, 0.1, h=1 << 16, w=1 << 15), b'2^30')
    # the limits of the amounts
    refused(call(0, -0.1), b'gaussian_noise', b'>= 0')
    refused(call(0, 0.1, c=9), b'gaussian_noise', b'channels')
    refused(call(1, 0.0, aux=taps, n_aux=9), b'gaussian_blur', b'(0, 8]')
    refused(call(1, 8.5, aux=taps, n_aux=9), b'gaussian_blur', b'(0, 8]')
    refused(call(1, 4.0, aux=taps, n_aux=33), b'gaussian_blur', b'radius')          # r = 16 = min(H, W)
    refused(call(1, 1.0, aux=taps, n_aux=7), b'aux_host', b'9')
    refused(call(1, 1.0, aux=None, n_aux=9), b'aux_host')
    refused(call(2, 1.9), b'downsample')
    refused(call(2, 17.0), b'downsample')
    refused(call(3, -0.1), b'contrast')
    refused(call(3, 4.1), b'contrast')
    refused(call(3, 0.5, ws_=None), b'workspace')
    refused(call(4, float('inf')), b'finite')
    refused(call(4, 0.1, aux=taps, n_aux=9), b'n_aux')
    refused(call(5, 2.1, aux=bias, n_aux=128), b'bias_field')
    refused(call(5, 0.3, aux=bias, n_aux=127), b'aux_host', b'128')
    refused(call(5, 0.3, aux=bias, n_aux=128, ws_=None), b'workspace')
    refused(call(6, 1.1), b'ghosting')
    refused(call(6, -0.1), b'ghosting')
    refused(call(7, 0.0), b'channel_drop', b'mask')
    refused(call(7, 15.0), b'channel_drop', b'mask')          # all four channels dropped
    refused(call(7, 2.5), b'channel_drop', b'mask')
    refused(call(7, 1.0, c=1), b'channel_drop', b'channels')
    bad = (ctypes.c_float * 9)(*([1.0 / 9] * 8 + [float('nan')]))
    refused(call(1, 1.0, aux=bad, n_aux=9), b'aux_host[8]')
    # workspace sizes
    assert so.rcu_corrupt_workspace_bytes(155, 4, 240, 240, 3) >= 155 * 4 * 8
    assert so.rcu_corrupt_workspace_bytes(155, 4, 240, 240, 5) >= (32 + 720 + 720) * 4
    assert all(so.rcu_corrupt_workspace_bytes(155, 4, 240, 240, k) == 0 for k in (0, 1, 2, 4, 6, 7))


# ------------------------------------------------------------------------------------------- script surface
YAML = """
config:
  test_name: {dataset}_test_x
  test_dir: {test_dir}
  model_dir: {model_dir}
  seed: 20
  test_at: best
  others:
    model_dir: {others_model_dir}
    test_at: best
    prediction_dir: {test_dir}
    corruption: {corruption}
meta:
  type: test-config
  version: 0
"""
SPEC = '[{kind: gaussian_blur, severity: 2}, {kind: gaussian_noise, severity: 3}]'


def _write_config(tmp_path, dataset, script, corruption=SPEC):
    model_dir = tmp_path / 'train' / 'model_x'
    path = tmp_path / 'test_{}_x.yaml'.format(dataset)
    path.write_text(YAML.format(dataset=dataset, test_dir=tmp_path / 'out', model_dir=model_dir, corruption=corruption,
                                others_model_dir='[{}]'.format(model_dir) if script == 'test_ensemble' else model_dir))
    return str(path)


@pytest.mark.parametrize('dataset', ['brats', 'isic'])
@pytest.mark.parametrize('script', ['test_default', 'test_ensemble', 'test_aleatoric', 'test_auxiliary_feat', 'test_auxiliary_segm'])
def test_the_ten_test_scripts_take_the_key(tmp_path, monkeypatch, dataset, script):
    """The corruption step is the first batch step of every script, and the hook that writes corruption.json is among its hooks."""
    from rcu_amd import corruption as co
    from rcu_amd import loops, scripts, steps
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    seen = {}

    def fake_run(context, dataset_, test_steps, write_hook, entries, world=None, startup_hooks=(), subject_hooks=()):
        seen['steps'], seen['hooks'], seen['context'] = list(test_steps), list(startup_hooks), context
        return context

    def fake_loop(self, context, build_test, hook=None):
        seen['steps'], seen['context'], seen['hook'] = list(self.steps), context, hook

    monkeypatch.setattr(scripts, '_run', fake_run)
    monkeypatch.setattr(loops.Test, '__call__', fake_loop)
    monkeypatch.setattr(scripts, '_load_additional_models', lambda context: [])
    monkeypatch.setattr(scripts, '_load_segmentation_model', lambda context: object())
    getattr(scripts, script)(dataset, config_file=_write_config(tmp_path, dataset, script), device='cpu')
    first = seen['steps'][0]
    assert type(first) is steps.CorruptInputStep and first.seed == 20
    assert first.stages == co.parse([{'kind': 'gaussian_blur', 'severity': 2}, {'kind': 'gaussian_noise', 'severity': 3}])
    assert not any(isinstance(s_, steps.CorruptInputStep) for s_ in seen['steps'][1:])
    # corruption.json: what the hook writes when the run starts
    context = seen['context']
    os.makedirs(context.test_dir, exist_ok=True)
    if 'hooks' in seen:
        (hook,) = [h for h in seen['hooks'] if isinstance(h, scripts.CorruptionRecordHook)]
        hook.end_startup(context)
    else:
        seen['hook'].end_startup(context)
    record = json.load(open(os.path.join(context.test_dir, 'corruption.json')))
    assert record == {'seed': 20, 'stages': [{'kind': 'gaussian_blur', 'amount': 1.0, 'severity': 2},
                                             {'kind': 'gaussian_noise', 'amount': 0.3, 'severity': 3}]}


def test_scripts_without_the_key_build_what_they_built_before(tmp_path, monkeypatch):
    from rcu_amd import scripts, steps
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    seen = {}

    def fake_run(context, dataset_, test_steps, write_hook, entries, world=None, startup_hooks=(), subject_hooks=()):
        seen['steps'], seen['hooks'] = list(test_steps), list(startup_hooks)
        return context

    monkeypatch.setattr(scripts, '_run', fake_run)
    path = _write_config(tmp_path, 'brats', 'test_default')
    text = open(path).read()
    open(path, 'w').write(''.join(line for line in text.splitlines(True) if 'corruption' not in line))
    scripts.test_default('brats', config_file=path, device='cpu')
    assert [type(s_) for s_ in seen['steps']] == [steps.SegmentationPredictStep] and seen['hooks'] == []


@pytest.mark.parametrize('bad, word', [('{kind: fog, severity: 1}', 'kind'), ('{kind: gaussian_blur, severity: 2, amount: 1.0}', 'severity'),
                                       ('{kind: ghosting, amount: 3}', 'amount')])
def test_scripts_refuse_a_bad_value_before_anything_is_written(tmp_path, monkeypatch, bad, word):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    with pytest.raises(ValueError, match=r'others\.corruption.*' + word):
        scripts.test_default('brats', config_file=_write_config(tmp_path, 'brats', 'test_default', bad), device='cpu')
    assert not (tmp_path / 'out').exists()


@pytest.mark.parametrize('dataset', ['brats', 'isic'])
def test_the_fit_scripts_refuse_the_key(tmp_path, monkeypatch, dataset):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    with pytest.raises(ValueError, match=r'others\.corruption'):
        scripts.fit_temperature(dataset, _write_config(tmp_path, dataset, 'fit_temperature'), device='cpu')
    assert not (tmp_path / 'out').exists()
    # and the bin-dl entry points of the ten test scripts and the two fit scripts exist
    names = sorted(os.listdir(os.path.join(ROOT, 'bin-dl')))
    assert len([n for n in names if '_test_' in n]) == 10 and len([n for n in names if n.endswith('_fit_temperature.py')]) == 2


def test_the_step_validates_its_arguments():
    from rcu_amd import corruption as co
    from rcu_amd import steps
    step = steps.CorruptInputStep({'kind': 'ghosting', 'severity': 1}, 20)
    assert step.stages == co.parse({'kind': 'ghosting', 'severity': 1}) and isinstance(step, steps.BatchStep)
    assert steps.CorruptInputStep(step.stages, 0).stages == step.stages
    with pytest.raises(ValueError):
        steps.CorruptInputStep({'kind': 'fog', 'severity': 1}, 20)
    with pytest.raises(ValueError):
        steps.CorruptInputStep({'kind': 'ghosting', 'severity': 1}, None)


# ------------------------------------------------------------------------------------------- the restatement against its frozen outputs
def test_reference_reproduces_the_golden_file(golden):
    g = golden('g29_corruptions')
    shape = tuple(int(v) for v in g['golden_shape'])
    assert shape == cr.SHAPES[0] and int(g['key']) == cr.KEY and int(g['first_sample']) == cr.FIRST_SAMPLE
    for s in cr.SHAPES:
        x = g['x_{}x{}x{}'.format(*s)]
        assert x.dtype == np.float32 and x.shape == (3,) + s
        assert np.array_equal(x, cr.make_input(s))
    x = g['x_{}x{}x{}'.format(*shape)]
    names = [str(n) for n in g['cases']]
    assert len(names) == len(cr.CASES)
    for name, (kind, amount) in zip(names, cr.CASES):
        amount = cr.case_amount(kind, amount, shape[0])
        y = cr.reference(kind, x, amount, cr.KEY, cr.FIRST_SAMPLE)
        want = g['y_' + name]
        assert y.dtype == want.dtype and y.shape == want.shape
        assert np.abs(y.astype(np.float64) - want.astype(np.float64)).max() <= 1e-12 * max(1.0, float(np.abs(want).max())), name
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'g29_corruptions.npz')) < 700 * 1024
