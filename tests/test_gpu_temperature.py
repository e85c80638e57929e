"""Temperature scaling on the GPU: the NLL sweep against a float64 numpy oracle and its exact-sum contract, the fit on labels drawn at a known
temperature, T applied through the packed classifier (bit for bit against a pre-divided checkpoint, and against the oracle forward), and the
fit and test scripts end to end (one process, a second run, two ranks, ISIC)."""
import glob
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden_params, golden_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SCALE = 1 << 20
LOGIT_TOL = 2e-6      # test_gpu_parity.py


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _lse(a, axis):
    m = np.max(a, axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def oracle_terms(z, y, beta):
    """float64 l(v) = -log((1/P) sum_t softmax(beta z_t)[y]); z [P, n, C, hw], y [n, hw] (valid classes)."""
    s = beta * z.astype(np.float64)
    logp = s - _lse(s, 2)[:, :, None, :]
    lp = np.take_along_axis(logp, y[None, :, None, :].astype(np.int64), 2)[:, :, 0, :]
    return -(_lse(lp, 0) - math.log(z.shape[0]))


def _case(p, c, n=3, hw=24 * 24, seed=0):
    rng = np.random.RandomState(seed + 100 * p + c)
    z = rng.randn(p, n, c, hw).astype(np.float32) * 3
    z[:, 0, :, :64] = np.sign(rng.randn(p, c, 64)) * 80         # saturated logits: every p_t underflows at beta = 8 on some voxels
    z[:, 0, :, 64:96] = rng.uniform(-80, 80, (p, c, 32))
    y = rng.randint(0, c, (n, hw)).astype(np.uint8)
    return z, y


def _terms(z, y, beta, mask, dev):
    from rcu_amd import _lib
    p, n, c, hw = z.shape
    out = torch.empty(n * hw, dtype=torch.float32, device=dev)
    zt, yt = torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev)
    mt = None if mask is None else torch.from_numpy(mask.astype(np.uint8)).to(dev)
    _lib.check(_lib.load().rcu_temperature_nll_terms(_lib.ptr(zt), p, n, hw, c, _lib.ptr(yt), _lib.ptr(mt), float(beta), _lib.ptr(out),
                                                     _lib.current_stream()))
    return out.cpu().numpy().reshape(n, hw)


def _sweep(z, y, mask, dev, temperatures=None):
    from rcu_amd import calibration as cal
    p, n, c, hw = z.shape
    sweep = cal.NllSweep(dev) if temperatures is None else cal.NllSweep(dev, temperatures)
    sweep.add(torch.from_numpy(z.reshape(p * n, c, hw, 1)).to(dev), torch.from_numpy(y).to(dev),
              None if mask is None else torch.from_numpy(mask).to(dev), passes=p)
    return sweep


@pytest.mark.timeout(600)
@pytest.mark.parametrize('masked', [False, True], ids=['all', 'mask'])
@pytest.mark.parametrize('c', [2, 3])
@pytest.mark.parametrize('p', [1, 3, 20])
def test_sweep_against_the_float64_oracle(dev, p, c, masked):
    from rcu_amd import calibration as cal
    z, y = _case(p, c)
    mask = (np.random.RandomState(5).rand(*y.shape) < 0.6) if masked else None
    sweep = _sweep(z, y, mask, dev)
    sums, means = sweep.sums(), sweep.mean_nll()
    keep = np.ones(y.shape, bool) if mask is None else mask
    assert sweep.voxels == int(keep.sum())
    for k, t in enumerate(cal.CANDIDATES):
        beta = np.float32(1.0 / t)
        terms = _terms(z, y, beta, mask, dev)
        ref = oracle_terms(z, y, float(beta))
        err = np.abs(terms.astype(np.float64) - ref)
        ok = (err <= 1e-5 * np.abs(ref)) | (err <= 2.0 ** -20)
        assert ok[keep].all(), (k, float(err[keep].max()), ref[keep][~ok[keep]][:4], terms[keep][~ok[keep]][:4])
        assert not terms[~keep].any()
        expect = int(np.rint(np.clip(terms[keep].astype(np.float64), 0, 4096) * SCALE).astype(np.int64).sum())
        assert sums[k] == expect, k
        ref_mean = float(np.mean(ref[keep]))
        assert abs(means[k] - ref_mean) <= 1e-5 * ref_mean + 2.0 ** -20, (k, means[k], ref_mean)


@pytest.mark.timeout(300)
def test_sums_do_not_depend_on_the_split(dev):
    from rcu_amd import calibration as cal
    z, y = _case(5, 2, n=6, hw=40 * 40, seed=3)
    mask = np.random.RandomState(9).rand(*y.shape) < 0.7
    whole = _sweep(z, y, mask, dev).sums()
    assert _sweep(z, y, mask, dev).sums() == whole
    for cut in (1, 4):
        sweep = cal.NllSweep(dev)
        for a, b in ((0, cut), (cut, 6)):
            sweep.add(torch.from_numpy(np.ascontiguousarray(z[:, a:b]).reshape(-1, 2, 40, 40)).to(dev), torch.from_numpy(y[a:b]).to(dev),
                      torch.from_numpy(mask[a:b]).to(dev), passes=5)
        assert sweep.sums() == whole, cut


@pytest.mark.timeout(300)
def test_invalid_targets_are_counted_and_refused(dev):
    from rcu_amd import _lib
    from rcu_amd import calibration as cal
    z, y = _case(2, 2, seed=4)
    y[1, :10] = 2
    y[2, 5] = 255
    out = torch.zeros(3, dtype=torch.int64, device=dev)
    ws = torch.empty(_lib.load().rcu_temperature_nll_workspace_bytes(y.size, 1), dtype=torch.uint8, device=dev)
    zt, yt = torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev)
    _lib.check(_lib.load().rcu_temperature_nll(_lib.ptr(zt), 2, 3, y.shape[1], 2, _lib.ptr(yt), None, (ctypes_float1())(1.0), 1, _lib.ptr(out),
                                               _lib.ptr(ws), _lib.current_stream()))
    got = out.cpu().tolist()
    assert got[1] == y.size - 11 and got[2] == 11
    valid = y < 2
    ref = oracle_terms(z, np.where(valid, y, 0), 1.0)
    assert abs(got[0] / SCALE - ref[valid].sum()) <= 1e-5 * ref[valid].sum()
    sweep = cal.NllSweep(dev)
    sweep.add(zt.reshape(6, 2, 24, 24), yt, passes=2)
    with pytest.raises(ValueError, match='11 voxels'):
        sweep.sums()


@pytest.mark.timeout(600)
@pytest.mark.parametrize('masked', [False, True], ids=['all', 'mask'])
@pytest.mark.parametrize('p, c', [(37, 8), (257, 2)])
def test_unstaged_form_against_the_float64_oracle(dev, p, c, masked):
    """P x (C - 1) = 259 floats per voxel do not fit the LDS stage (TN_STAGE_MAX = 256): temperature_nll_kernel<false, ...> reads the
    differences from global memory per candidate.  MC T >= 257 on a binary model, or 37 passes on an 8-class model, take it."""
    from rcu_amd import calibration as cal
    assert p * (c - 1) > 256 >= 36 * 7
    z, y = _case(p, c, n=2)
    mask = (np.random.RandomState(5).rand(*y.shape) < 0.6) if masked else None
    keep = np.ones(y.shape, bool) if mask is None else mask
    sweep = _sweep(z, y, mask, dev)
    sums = sweep.sums()
    assert sweep.voxels == int(keep.sum())
    for k in (0, 48, 96):
        beta = np.float32(1.0 / cal.CANDIDATES[k])
        terms = _terms(z, y, beta, mask, dev)
        ref = oracle_terms(z, y, float(beta))
        err = np.abs(terms.astype(np.float64) - ref)
        ok = (err <= 1e-5 * np.abs(ref)) | (err <= 2.0 ** -20)
        assert ok[keep].all(), (k, float(err[keep].max()), ref[keep][~ok[keep]][:4], terms[keep][~ok[keep]][:4])
        assert not terms[~keep].any()
        expect = int(np.rint(np.clip(terms[keep].astype(np.float64), 0, 4096) * SCALE).astype(np.int64).sum())
        assert sums[k] == expect, k
    # the same voxels added as two calls
    halves = cal.NllSweep(dev)
    for i in range(2):
        halves.add(torch.from_numpy(np.ascontiguousarray(z[:, i:i + 1]).reshape(p, c, 24, 24)).to(dev), torch.from_numpy(y[i:i + 1]).to(dev),
                   None if mask is None else torch.from_numpy(mask[i:i + 1]).to(dev), passes=p)
    assert halves.sums() == sums and halves.voxels == sweep.voxels


def ctypes_float1():
    import ctypes
    return ctypes.c_float * 1


def _draw(z, t0, seed):
    """labels drawn from mean_t softmax(z_t / T0) (binary)."""
    p1 = np.mean(1.0 / (1.0 + np.exp(-(z[:, :, 1] - z[:, :, 0]).astype(np.float64) / t0)), axis=0)
    return (np.random.RandomState(seed).rand(*p1.shape) < p1).astype(np.uint8)


@pytest.mark.timeout(600)
@pytest.mark.parametrize('p', [1, 5])
@pytest.mark.parametrize('t0', [0.5, 2.0])
def test_fit_recovers_a_known_temperature(dev, t0, p):
    from rcu_amd import calibration as cal
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(int(t0 * 10) + p)
    n, hw = 4, 256 * 256
    base = rng.randn(1, n, 2, hw) * 2.5
    z = (base + 0.6 * rng.randn(p, n, 2, hw)).astype(np.float32)
    y = _draw(z, t0, seed=p)
    sweep = _sweep(z, y, None, dev)
    fit = cal.refine(sweep.temperatures, sweep.sums())
    assert not fit.at_edge
    assert abs(fit.temperature / t0 - 1) < 0.03, (fit, t0)
    oracle = [float(np.sum(oracle_terms(z, y, 1.0 / t))) for t in cal.CANDIDATES]
    ofit = cal.refine(cal.CANDIDATES, oracle)
    assert abs(fit.temperature / ofit.temperature - 1) < 0.01, (fit, ofit)
    if t0 == 2.0:
        def ece(t):
            fg = torch.from_numpy(np.mean(1.0 / (1.0 + np.exp(-(z[:, :, 1] - z[:, :, 0]).astype(np.float64) / t)), axis=0).astype(np.float32))
            return ev.ece_binary(fg.reshape(n, 256, 256).to(dev), torch.from_numpy(y.reshape(n, 256, 256)))
        assert ece(fit.temperature) < ece(1.0)


def _g1_model(g, dev, state=None, temperature=None, fuse=True):
    from rcu_amd.model import UNet
    m = UNet(**golden_params(g))
    m.load_state_dict({k: torch.as_tensor(v) for k, v in (state or golden_state(g)).items()})
    m = m.to(dev).eval()
    m.set_fuse_head(fuse)
    if temperature is not None:
        m.set_temperature(temperature)
    return m


def _outputs(m, x, dev):
    from rcu_amd import steps
    out = {'logits': m(x).cpu().numpy()}
    if m.dropout is not None:
        for name, step in (('mc', steps.McPredictStep(4, seed=7)), ('tta', steps.TtaMcPredictStep(['identity', 'flip_h'], mc_steps=2, seed=7))):
            bc = steps.BatchContext({'images': x.clone()}, 0, 0)
            ctx = steps.TorchTestContext('cuda', m)
            step(bc, None, ctx)
            steps.MultiPredictionSummary(do_mi=True, do_var=True)(bc, None, ctx)
            torch.cuda.synchronize()
            for k, v in bc.output.items():
                if torch.is_tensor(v):
                    out[name + ':' + k] = v.cpu().numpy()
    return out


@pytest.mark.timeout(600)
@pytest.mark.parametrize('fuse', [True, False], ids=['fused-head', 'unfused-head'])
def test_set_temperature_is_the_pre_divided_checkpoint(golden, dev, fuse):
    from oracle import unet_oracle as uo
    g = golden('g1_unet_eval')
    params = golden_params(g)
    x = torch.from_numpy(g['x_a']).to(dev)
    plain = _outputs(_g1_model(g, dev, fuse=fuse), x, dev)
    same = _outputs(_g1_model(g, dev, temperature=1.0, fuse=fuse), x, dev)
    for k in plain:
        assert plain[k].tobytes() == same[k].tobytes(), k
    for t in (0.7, 2.5):
        state = dict(golden_state(g))
        for key in ('conv_cls.1.weight', 'conv_cls.1.bias'):
            state[key] = (state[key].astype(np.float64) / t).astype(np.float32)
        scaled = _outputs(_g1_model(g, dev, temperature=t, fuse=fuse), x, dev)
        divided = _outputs(_g1_model(g, dev, state=state, fuse=fuse), x, dev)
        assert sorted(scaled) == sorted(divided)
        for k in scaled:
            assert scaled[k].tobytes() == divided[k].tobytes(), (t, k)
        assert not np.array_equal(scaled['logits'], plain['logits'])
        ref = uo.unet_forward({k: torch.as_tensor(v) for k, v in state.items()}, torch.from_numpy(g['x_a']), None, **params)
        ref = ref.numpy() if torch.is_tensor(ref) else np.asarray(ref)
        assert float(np.max(np.abs(scaled['logits'].astype(np.float64) - ref))) < LOGIT_TOL
    sigma = dict(params, sigma_out=True)
    from rcu_amd.model import UNet
    with pytest.raises(ValueError, match='sigma'):
        UNet(**sigma).set_temperature(1.5)


# ------------------------------------------------------------------------------------------------------------- the scripts
def _written(out_root, suffixes=('.nii.gz', 'metrics.csv')):
    dirs = glob.glob(os.path.join(out_root, '*'))
    assert len(dirs) == 1, dirs
    return {os.path.basename(f): open(f, 'rb').read() for f in sorted(glob.glob(os.path.join(dirs[0], '*'))) if f.endswith(suffixes)}


def _script(name, cfg, env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bin-dl', name), '-config_file', cfg], capture_output=True, text=True, timeout=500,
                       cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def _variant(text, tmp_path, tag, others):
    path = str(tmp_path / 'cfg_{}.yaml'.format(tag))
    with open(path, 'w') as f:
        f.write(text.replace(str(tmp_path / 'out'), str(tmp_path / 'out_{}'.format(tag))).replace('    mc: 2\n', others))
    return path


@pytest.mark.timeout(1800)
def test_brats_fit_and_test_scripts(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_gpu_scripts as tgs
    import test_gpu_tta as tgt
    cfg, vols, _, _ = tgs._setup(tmp_path, mc=2)
    text = open(cfg).read()
    assert '    mc: 2\n' in text
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('WORLD_SIZE', None)
    fits = []
    for tag in ('fit1', 'fit2'):
        r = _script('brats_fit_temperature.py', _variant(text, tmp_path, tag, '    mc: 3\n'), env)
        assert 'temperature:' in r.stdout
        fits.append(_written(str(tmp_path / 'out_{}'.format(tag)), ('temperature.json',))['temperature.json'])
    assert fits[0] == fits[1]
    doc = json.loads(fits[0])
    assert doc['mc'] == 3 and doc['passes'] == 3 and doc['seed'] == 20 and len(doc['curve']) == 97
    assert doc['voxels'] == sum(v[1].size for v in vols.values())
    assert doc['curve'][48][1] == doc['mean_nll_at_1'] and doc['temperature'] > 0
    t = doc['temperature']
    json_path = glob.glob(str(tmp_path / 'out_fit1' / '*' / 'temperature.json'))[0]
    runs = {'json': '    mc: 6\n    temperature: {}\n'.format(json_path), 'float': '    mc: 6\n    temperature: {!r}\n'.format(t), 'none': '    mc: 6\n'}
    written = {}
    for tag, others in runs.items():
        _script('brats_test_default.py', _variant(text, tmp_path, tag, others), env)
        written[tag] = _written(str(tmp_path / 'out_{}'.format(tag)), ('.nii.gz',))
    assert sorted(written['json']) == sorted(written['float']) and len(written['json']) == 2 * len(vols)
    for name in written['json']:
        assert written['json'][name] == written['float'][name], name
    assert any(written['json'][k] != written['none'][k] for k in written['json'] if k.endswith('_probabilities.nii.gz'))
    r = tgt._launch_ranks(os.path.join(ROOT, 'bin-dl', 'brats_test_default.py'), _variant(text, tmp_path, 'two', runs['json']), env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    two = _written(str(tmp_path / 'out_two'), ('.nii.gz',))
    assert sorted(two) == sorted(written['json'])
    for name in two:
        assert two[name] == written['json'][name], name


@pytest.mark.timeout(900)
def test_isic_fit_and_test_scripts_run(tmp_path):
    from PIL import Image
    from oracle import unet_oracle as uo
    from rcu_amd import management as mgt
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_gpu_scripts as tgs
    params = dict(nb_classes=2, in_channels=3, depth=4, start_filters=8, dropout=0.2)
    prefix = tmp_path / 'isic' / 'ISIC-2017_Test_v2'
    img_dir, lab_dir = str(prefix) + '_Data', str(prefix) + '_Part1_GroundTruth'
    os.makedirs(img_dir)
    os.makedirs(lab_dir)
    rng = np.random.RandomState(7)
    for id_ in ('ISIC_0000020', 'ISIC_0000021'):
        Image.fromarray(rng.randint(0, 255, (64, 96, 3)).astype(np.uint8)).save(os.path.join(img_dir, id_ + '.jpg'))
        Image.fromarray(((rng.rand(64, 96) > 0.6) * 255).astype(np.uint8)).save(os.path.join(lab_dir, id_ + '_segmentation.png'))
    mf = mgt.ModelFiles(str(tmp_path / 'train'), 'isic')
    mgt.save_model(mf, 'unet', params, uo.synthetic_state(21, **params))
    text = tgs.ISIC_MC_YAML.format(test_dir=str(tmp_path / 'out'), model_dir=mf.model_dir, dataset=str(prefix))
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    _script('isic_fit_temperature.py', _variant(text, tmp_path, 'fit', '    mc: 2\n'), env)
    doc = json.loads(_written(str(tmp_path / 'out_fit'), ('temperature.json',))['temperature.json'])
    assert doc['voxels'] == 2 * 64 * 96 and doc['passes'] == 2
    json_path = glob.glob(str(tmp_path / 'out_fit' / '*' / 'temperature.json'))[0]
    _script('isic_test_default.py', _variant(text, tmp_path, 'test', '    mc: 2\n    temperature: {}\n'.format(json_path)), env)
    assert len(_written(str(tmp_path / 'out_test'), ('_probabilities.nii.gz',))) == 2
