"""The auxiliary fit on the GPU (include/rcu_fit.h "Auxiliary fit"): rcu_postnet_loss_grad against the float64 restatement of
tests/auxfit_reference.py -- every entry of every gradient within the float32 accumulation bound on its condition sum, the statistics and the loss
within theirs -- its bit-for-bit contract, three Adam steps from the state of fixture G36, and the fit script end to end.

Shapes: voxel counts that are no multiple of 32 or 64 (one slice of 279 voxels; three slices of 1024 + 37, so that a slice has a partial chunk), F = 8
at pitch 32 with NaN in the padding channels, F = 32 with an all-zero channel, L = 1, 3, 4, labels all zero, pitch 64, every pointer one element off
its allocation.  No kernel's grid is capped (a wave per chunk), so there is no case above a cap.

The batches are continuous features, every voxel its own draw, nothing rejected (tests/auxfit_cases.py).  Largest fraction of the gradient bound used
on the MI355X (every test prints its own): 0.050 (one slice of 279 voxels with the dead channel; 0.006 .. 0.038 in the others); the reference's float32
CPU run on the batch of fixture G36 uses 0.028 (tests/test_auxfit_cpu.py).  Three Adam steps: at most 0.37 of the derived tolerance (a BatchNorm
weight of the last hidden unit; 0.05 .. 0.15 elsewhere, below 0.001 for the conv biases)."""
import numpy as np
import pytest
import torch

import auxfit_cases as cases
import auxfit_reference as ref

pytestmark = pytest.mark.gpu

# name -> (seed, n, hw, F, L, pitch, off, zero_channel, all_zero_labels)
CASES = {
    'one_slice_279_zero_channel': (1, 1, 279, 32, 3, 32, 0, 31, False),
    'three_slices_1061_F8_L1': (2, 3, 1061, 8, 1, 32, 0, None, False),
    'three_slices_1061_L4_pitch64_labels0': (3, 3, 1061, 32, 4, 64, 0, None, True),
    'off_by_one_element': (4, 1, 279, 32, 3, 32, 1, 31, False),
    'two_slices_2085_F8_L3': (5, 2, 2085, 8, 3, 32, 0, None, False),
}
_cache = {}


def _case(name):
    """(inputs, float64 reference), computed once per case and shared."""
    if name not in _cache:
        seed, n, hw, F, L, pitch, off, zero, all_zero = CASES[name]
        phi, labels, params, expected = cases.make_inputs(seed, n, hw, F, L, zero_channel=zero, all_zero_labels=all_zero)
        _cache[name] = ((phi, labels, params), expected)
    return _cache[name]


def check_against_reference(got, expected, F, L, tag):
    """Every entry of every output within its bound; prints and returns the largest fraction of the gradient bound used."""
    assert got['flag'] == 0
    grads = ref.unpack(got['grads'], F, L)
    bounds = ref.gradient_bound(expected['cond'])
    worst = 0.0
    for name, _ in ref.packing(F, L):
        g64, bound = expected['grads'][name].reshape(grads[name].shape), bounds[name].reshape(grads[name].shape)
        err = np.abs(grads[name].astype(np.float64) - g64)
        assert np.isfinite(grads[name]).all(), (tag, name)
        frac = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        print('{} {}: largest |g_dev - g64| / bound = {:.4f}'.format(tag, name, frac))
        worst = max(worst, frac)
        assert (err <= bound).all(), (tag, name, frac)
    mu_b, var_b, loss_b = ref.statistics_bounds(expected)
    mu_err, var_err = np.abs(got['mean'] - expected['mu']), np.abs(got['var'] - expected['var'])
    print('{}: mu {:.4f}, var {:.4f}, loss {:.4f} of their bounds'.format(tag, float((mu_err / np.maximum(mu_b, 1e-300)).max()),
                                                                        float((var_err / np.maximum(var_b, 1e-300)).max()),
                                                                        abs(got['loss'] - expected['loss']) / loss_b))
    assert (mu_err <= mu_b).all(), tag
    assert (var_err <= var_b).all(), tag
    assert abs(got['loss'] - expected['loss']) <= loss_b, tag
    return worst


@pytest.mark.parametrize('name', sorted(CASES))
def test_loss_and_gradients_within_the_accumulation_bound(name):
    seed, n, hw, F, L, pitch, off, zero, all_zero = CASES[name]
    (phi, labels, params), expected = _case(name)
    got = cases.device_call(phi, labels, ref.pack(params, F, L), n, hw, F, L, pitch=pitch, off=off)
    worst = check_against_reference(got, expected, F, L, name)
    print('{}: largest fraction of the gradient bound {:.4f}'.format(name, worst))
    if zero is not None:      # nothing flows from a dead input channel
        assert (ref.unpack(got['grads'], F, L)['convs.0.conv2d_batch_relu.conv.weight'][:, zero] == 0).all()


def test_the_outputs_are_a_function_of_the_inputs_bit_for_bit():
    """The call twice, on two streams, at two pitches, with and without garbage in the padding, on and off alignment: equal bits."""
    for name in ('one_slice_279_zero_channel', 'two_slices_2085_F8_L3'):
        seed, n, hw, F, L, pitch, off, zero, all_zero = CASES[name]
        (phi, labels, params), _ = _case(name)
        flat = ref.pack(params, F, L)
        first = cases.device_call(phi, labels, flat, n, hw, F, L, pitch=32, off=0)
        variants = [dict(pitch=32, off=0), dict(pitch=32, off=0, stream=torch.cuda.Stream()), dict(pitch=64, off=0, stream=torch.cuda.Stream()),
                    dict(pitch=32, off=1), dict(pitch=48, off=1, garbage=False)]
        for kw in variants:
            again = cases.device_call(phi, labels, flat, n, hw, F, L, **kw)
            for key in ('grads', 'mean', 'var'):
                assert first[key].tobytes() == again[key].tobytes(), (name, kw, key)
            assert np.float64(first['loss']).tobytes() == np.float64(again['loss']).tobytes(), (name, kw)


def test_a_label_above_one_is_reported():
    from rcu_amd import auxiliary
    from rcu_amd.model import PostNet
    (phi, labels, params), _ = _case('one_slice_279_zero_channel')
    bad = labels.copy()
    bad[100] = 2
    got = cases.device_call(phi, bad, ref.pack(params, 32, 3), 1, 279, 32, 3)
    assert got['flag'] == 1
    net = PostNet(32, 2, nb_convs=3).cuda()
    feats = torch.from_numpy(phi.reshape(1, 9, 31, 32)).cuda().permute(0, 3, 1, 2)
    with pytest.raises(ValueError, match='label >= 2'):
        auxiliary.loss_and_grad(net, feats, torch.from_numpy(bad.reshape(1, 9, 31)).cuda())


def test_loss_and_grad_of_a_module_matches_the_raw_call():
    """rcu_amd.auxiliary.loss_and_grad: the packing of a module's parameters and the names of the gradients it hands back."""
    from rcu_amd import auxiliary
    from rcu_amd.model import PostNet
    (phi, labels, params), expected = _case('one_slice_279_zero_channel')
    net = PostNet(32, 2, nb_convs=3)
    state = net.state_dict()
    for name, value in params.items():
        state[name] = torch.from_numpy(value.reshape(tuple(state[name].shape)))
    net.load_state_dict(state)
    net.cuda()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    feats = torch.from_numpy(phi.reshape(1, 9, 31, 32)).cuda().permute(0, 3, 1, 2)      # the channels-last view UNet.features hands out
    loss, grads, (mean, var) = auxiliary.loss_and_grad(net, feats, torch.from_numpy(labels.reshape(1, 9, 31)).cuda())
    raw = cases.device_call(phi, labels, ref.pack(params, 32, 3), 1, 279, 32, 3)
    unpacked = ref.unpack(raw['grads'], 32, 3)
    assert loss == raw['loss'] and sorted(grads) == sorted(unpacked)
    for name in unpacked:
        assert tuple(grads[name].shape) == tuple(before[name].shape)
        assert grads[name].cpu().numpy().ravel().tobytes() == unpacked[name].ravel().tobytes(), name
    assert mean.cpu().numpy().tobytes() == raw['mean'].tobytes() and var.cpu().numpy().tobytes() == raw['var'].tobytes()
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k


# ------------------------------------------------------------------------------------------------------------------ three Adam steps
def _adam_tolerances(g, F, L, steps, lr):
    """The float64 trajectory of the fixture's batch and, derived from it, how far a float32 device run may be from it after every step.

    Parameters.  Adam's update is lr mhat / (sqrt(vhat) + eps).  A gradient error of at most B_s at the steps s <= t moves mhat by at most
    max_s B_s and sqrt(vhat) by at most max_s B_s, and |mhat| <= sqrt(vhat) up to the bias corrections, so the update of step t moves by at most
    2 lr max_s B_s / (sqrt(vhat_t) + eps), with B_s the gradient bound (1024 + 2) 2^-24 A of step s and vhat_t the reference's.  The float32 arithmetic of
    the step itself adds the one rounding of the stored parameter and those of the update's few operations per step (2^-24 (|p| + 8 lr)).  The gradient of steps 2 and 3 is taken at
    parameters that differ by these tolerances; that second-order term (lr |dg/dp| tol) is far inside the factor (1024 + 2) and is left out.
    For a conv bias B / (|g| + eps) is large -- its gradient is zero in exact arithmetic -- and the tolerance says what is true: Adam moves it by up to lr
    per step in the direction of the rounding residue.

    Running statistics.  mu_t moves with the parameters of step t: per layer, du = tol_W max|a| + |W| da (the part that varies over the voxels) plus
    tol_b (a constant shift, which the variance and xhat do not see); |d var| <= 4 sigma du + 4 du^2; |d xhat| <= 2 du / sigma + max|xhat| |d var| /
    (2 sigma^2); da of the next layer = |gamma| |d xhat| + tol_gamma max|xhat| + tol_beta.  The bounds of the statistics themselves (mu, var) are added, and
    the momentum weights 0.1 0.9^(steps - t) sum the steps."""
    state = {k[len('sd0::'):]: np.asarray(v, dtype=np.float64) for k, v in g.items() if k.startswith('sd0::')}
    names = [name for name, _ in ref.packing(F, L)]
    params = {name: state[name].reshape(shape) for name, shape in ref.packing(F, L)}
    m = {name: np.zeros_like(params[name]) for name in names}
    v = {name: np.zeros_like(params[name]) for name in names}
    tol = {name: np.zeros_like(params[name]) for name in names}
    worst_b = {name: np.zeros_like(params[name]) for name in names}
    N = g['phi'].shape[0]
    rm_tol, rv_tol = np.zeros((L, F)), np.zeros((L, F))
    for t in range(1, steps + 1):
        r = ref.loss_and_grad(g['phi'], g['labels'], params, L)
        mu_b, var_b, _ = ref.statistics_bounds(r)
        da = np.zeros(F)
        for k in range(L):
            base = 'convs.{}.conv2d_batch_relu.'.format(k)
            sigma = np.sqrt(r['var'][k] + ref.EPS)
            du = tol[base + 'conv.weight'] @ np.abs(r['a'][k]).max(0) + np.abs(params[base + 'conv.weight']) @ da
            dvar = 4 * sigma * du + 4 * du * du
            xmax = np.abs(r['xhat'][k]).max(0)
            dxhat = 2 * du / sigma + xmax * dvar / (2 * sigma * sigma)
            da = np.abs(params[base + 'bn.weight']) * dxhat + tol[base + 'bn.weight'] * xmax + tol[base + 'bn.bias']
            weight = 0.1 * 0.9 ** (steps - t)
            rm_tol[k] += weight * (mu_b[k] + du + tol[base + 'conv.bias'])
            rv_tol[k] += weight * (var_b[k] + dvar) * N / (N - 1)
        bounds = ref.gradient_bound(r['cond'])
        params, m, v = ref.adam_step(params, r['grads'], m, v, t, lr=lr)
        for name in names:
            worst_b[name] = np.maximum(worst_b[name], bounds[name].reshape(worst_b[name].shape))
            vhat = v[name] / (1 - 0.999 ** t)
            tol[name] = tol[name] + 2 * lr * worst_b[name] / (np.sqrt(vhat) + 1e-8) + ref.U * (np.abs(params[name]) + 8 * lr)
    return tol, rm_tol, rv_tol


def test_three_adam_steps_from_the_fixture_state(golden):
    """rcu_amd.auxiliary.Fitter -- the kernels, torch's running-statistics update and torch.optim.Adam on the device -- against the float64 state the
    reference's own modules reach after three steps (fixture G36), every parameter and running statistic within the tolerance derived above."""
    from rcu_amd import auxiliary
    from rcu_amd.model import PostNet
    g = golden('g36_auxfit')
    n, h, w, F, L, steps = (int(x) for x in g['shape'])
    lr = float(g['lr'])
    net = PostNet(F, 2, nb_convs=L)
    net.load_state_dict({k[len('sd0::'):]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith('sd0::')})
    feats = torch.from_numpy(g['phi'].reshape(n, h, w, F)).cuda().permute(0, 3, 1, 2)
    labels = torch.from_numpy(g['labels'].reshape(n, h, w)).cuda()
    fitter = auxiliary.Fitter(net, lr, torch.device('cuda'))
    losses = torch.zeros(steps, dtype=torch.float64, device='cuda')
    for t in range(steps):
        assert fitter.step(feats, labels, losses[t:]) == n * h * w
    fitter.close()
    assert not net.training and all(not p.requires_grad and p.grad is None for p in net.parameters())
    final = {k: v.cpu().numpy() for k, v in net.state_dict().items()}
    tol, rm_tol, rv_tol = _adam_tolerances(g, F, L, steps, lr)
    loss_b = (ref.CHUNK + 2) * ref.U * float(np.max(g['losses'])) * 2      # mean |l| = the loss (l >= 0); the later losses also move with the parameters
    assert (np.abs(losses.cpu().numpy() - g['losses']) <= loss_b).all()
    for name, shape in ref.packing(F, L):
        err = np.abs(final[name].astype(np.float64).reshape(shape) - g['sd3::' + name].reshape(shape))
        print('{}: largest fraction of the Adam tolerance {:.4f}'.format(name, float((err / tol[name]).max())))
        assert (err <= tol[name]).all(), name
        assert (final[name].reshape(shape) != g['sd0::' + name].reshape(shape)).any(), name
    for k in range(L):
        bn = 'convs.{}.conv2d_batch_relu.bn.'.format(k)
        assert (np.abs(final[bn + 'running_mean'] - g['sd3::' + bn + 'running_mean']) <= rm_tol[k]).all(), k
        assert (np.abs(final[bn + 'running_var'] - g['sd3::' + bn + 'running_var']) <= rv_tol[k]).all(), k
        assert int(final[bn + 'num_batches_tracked']) == steps == int(g['sd3::' + bn + 'num_batches_tracked'])
    # the module is ready for inference: its fused eval-mode kernel sees the new weights
    out = net(feats)
    assert tuple(out.shape) == (n, 2, h, w) and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------------------------ the script, end to end
def test_fit_script_then_the_unchanged_test_script(tmp_path, monkeypatch):
    """bin-dl/brats_fit_auxiliary_feat.py, run as the command line runs it, for two epochs on the tiny dataset of tests/test_gpu_scripts.py, then brats_test_auxiliary_feat.py on the
    directory it wrote.  The losses of the CSV against tests/auxfit_reference.py on the same batches -- the ones the script handed to the fit,
    recorded on the way -- with the frozen U-Net's own features and arg-max as inputs, float64 Adam between the steps: within the loss bound."""
    import csv
    import glob
    import json
    import os
    import yaml
    import test_gpu_scripts as tgs
    from test_gpu_density import tgs_model
    from rcu_amd import auxiliary, density, scripts
    from rcu_amd.model import PostNet
    cfg, vols, states, params = tgs._setup(tmp_path)
    seen = []
    fit = auxiliary.fit_auxiliary_feat

    def recording(model, postnet, batches, epochs, **kw):
        def walk():
            seen.append([])
            for images, target in batches():
                seen[-1].append((images.clone(), target.clone()))
                yield images, target
        return fit(model, postnet, walk, epochs, **kw)

    monkeypatch.setattr(scripts.auxiliary_mod, 'fit_auxiliary_feat', recording)
    cfg_fit = tgs._with_others(cfg, 'fit', auxiliary_fit=dict(epochs=2, lr=1e-3, nb_convs=2))
    # the command line itself, bin-dl/brats_fit_auxiliary_feat.py -config_file X, executed in this process
    import runpy
    import sys
    entry = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'bin-dl', 'brats_fit_auxiliary_feat.py')
    monkeypatch.setattr(sys, 'argv', [entry, '-config_file', cfg_fit])
    runpy.run_path(entry, run_name='__main__')
    fit_dir = glob.glob(str(tmp_path / 'out_fit' / '*'))[0]
    doc = json.load(open(os.path.join(fit_dir, 'auxiliary_fit.json')))
    rows = doc['rows']
    table = list(csv.DictReader(open(os.path.join(fit_dir, 'auxiliary_fit.csv'))))
    total = sum(v[0].shape[0] * v[0].shape[1] * v[0].shape[2] for v in vols.values())
    assert [r['epoch'] for r in table] == ['1', '2'] and list(table[0]) == ['epoch', 'steps', 'voxels', 'error_fraction', 'mean_loss']
    assert len(seen) == 2 and all(int(r['voxels']) == total and int(r['steps']) == len(seen[0]) for r in table)      # no slice of it is black
    assert (doc['epochs'], doc['nb_convs'], doc['lr'], doc['in_channels'], doc['test_at']) == (2, 2, 1e-3, 32, 'best')
    model_dir = doc['postnet_model_dir']
    found = sorted(os.path.basename(f) for f in glob.glob(os.path.join(model_dir, 'checkpoints', '*.pth')))
    assert found == ['checkpoint_ep001.pth', 'checkpoint_ep002-best.pth', 'checkpoint_ep002.pth']

    net = PostNet(32, 2, nb_convs=2)
    seed = yaml.safe_load(open(cfg_fit))['config'].get('seed') or 0
    torch.manual_seed(int(seed))      # the script re-initialises the PostNet under the YAML seed
    for module in net.modules():
        if hasattr(module, 'reset_parameters'):
            module.reset_parameters()
    names = [name for name, _ in ref.packing(32, 2)]
    p = {name: value.numpy().astype(np.float64) for name, value in net.state_dict().items() if name in names}
    m, v = {name: np.zeros_like(p[name]) for name in names}, {name: np.zeros_like(p[name]) for name in names}
    unet = tgs_model(params, states[0])
    t = 0
    for epoch, batches in enumerate(seen):
        losses, bounds = [], []
        for images, target in batches:
            with density.eval_features(unet):
                logits = unet(images.float().cuda())
                e = auxiliary.error_target(logits, target.cuda()).cpu().numpy().reshape(-1)
                phi = unet.features.permute(0, 2, 3, 1).reshape(-1, 32).cpu().numpy()
            r = ref.loss_and_grad(phi, e, p, 2)
            t += 1
            p, m, v = ref.adam_step(p, r['grads'], m, v, t, lr=1e-3)
            losses.append(r['loss']), bounds.append(ref.statistics_bounds(r)[2])
        got = rows[epoch]
        assert float(table[epoch]['mean_loss']) == got['mean_loss'] and len(got['losses']) == len(losses)
        print('epoch {}: mean loss {:.9f}, reference {:.9f}, bound {:.3g}; largest step fraction {:.4f}'.format(
            epoch + 1, got['mean_loss'], float(np.mean(losses)), float(np.mean(bounds)),
            max(abs(a - b) / c for a, b, c in zip(got['losses'], losses, bounds))))
        assert all(abs(a - b) <= c for a, b, c in zip(got['losses'], losses, bounds))
        assert abs(got['mean_loss'] - float(np.mean(losses))) <= float(np.mean(bounds))
        assert abs(got['error_fraction'] - float(table[epoch]['error_fraction'])) == 0 and 0 < got['error_fraction'] < 1
    assert rows[1]['mean_loss'] < rows[0]['mean_loss']

    # the unchanged test script on what the fit wrote
    with open(cfg) as f:
        text = f.read()
    seg_dir = [ln.split('model_dir: ')[1] for ln in text.splitlines() if ln.startswith('  model_dir: ')][0]
    text = text.replace('model_dir: ' + seg_dir, 'model_dir: ' + model_dir).replace('  others: {}\n', '  others:\n    model_dir: {}\n    test_at: best\n'.format(seg_dir))
    cfg_feat = str(tmp_path / 'test_feat.yaml')
    with open(cfg_feat, 'w') as f:
        f.write(text)
    assert yaml.safe_load(open(cfg_feat))['config']['model_dir'] == model_dir
    ctx = scripts.test_auxiliary_feat('brats', cfg_feat)
    for name, (images, labels, props) in vols.items():
        conf, pred = tgs._confidence(ctx, name)
        assert conf.dtype == np.float32 and conf.shape == labels.shape and np.isfinite(conf).all() and 0 <= conf.min() and conf.max() <= 1
