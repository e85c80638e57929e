"""The auxiliary fit without a GPU (include/rcu_fit.h "Auxiliary fit"): the float64 restatement tests/auxfit_reference.py against fixture G36 (the
reference's own PostNet, nn.CrossEntropyLoss and torch.optim.Adam, tests/golden/generate_auxfit.py) and against torch.autograd on a fresh float64
restatement; the second header's symbols, its argument validation and the untouched prototypes of include/rcu.h; the packing table; the stream-order
table of the second header; the fit script's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import auxfit_cases as cases
import auxfit_reference as ref
from test_density_scripts_cpu import _context, _yaml_with
from test_stream_order_cpu import prototypes, stream_entry_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT_NAMES = ('rcu_postnet_fit_param_count', 'rcu_postnet_fit_workspace_bytes', 'rcu_postnet_loss_grad')


@pytest.fixture(scope='module')
def g36(golden):
    g = golden('g36_auxfit')
    n, h, w, F, L, steps = (int(v) for v in g['shape'])
    state = {k[len('sd0::'):]: v for k, v in g.items() if k.startswith('sd0::')}
    return g, (n, h, w, F, L, steps), state, ref.loss_and_grad(g['phi'], g['labels'], state, L)


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64).reshape(np.shape(a))
    return bool((np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))).all())


def test_reference_reproduces_the_fixture_to_1e_12(g36):
    g, (n, h, w, F, L, steps), state, got = g36
    assert g['phi'].shape == (n * h * w, F) and (g['phi'][:, F - 1] == 0).all() and set(np.unique(g['labels'])) == {0, 1}
    assert _close(got['loss'], g['loss']) and _close(got['mu'], g['mu']) and _close(got['var'], g['var'])
    for name, shape in ref.packing(F, L):
        assert _close(got['grads'][name], g['g64::' + name]), name
        assert _close(got['cond'][name], g['cond::' + name]), name
        assert np.isfinite(g['g32::' + name]).all()
    # a conv bias in front of a train-mode BatchNorm has no gradient
    for k in range(L):
        assert np.abs(g['g64::convs.{}.conv2d_batch_relu.conv.bias'.format(k)]).max() < 1e-14


def test_reference_fit_steps_reproduce_three_adam_steps_of_the_fixture(g36):
    """Parameters, running statistics and num_batches_tracked after three Adam steps.  The conv biases -- and the running means, which carry them
    -- are excepted from 1e-12: their gradient is zero in exact arithmetic, float64 leaves ~1e-17 of either sign, and Adam's lr g / (|g| + 1e-8)
    amplifies the difference of two such residues by lr / eps = 1e4 per step; they are held to 1e-10."""
    g, (n, h, w, F, L, steps), state, _ = g36
    full = {k: v for k, v in state.items()}
    final, losses = ref.fit_steps(g['phi'], g['labels'], full, L, steps, lr=float(g['lr']))
    assert _close(losses, g['losses'])
    assert sorted(final) == sorted(k[len('sd3::'):] for k in g if k.startswith('sd3::'))
    for name, value in final.items():
        loose = name.endswith('conv.bias') or name.endswith('running_mean')
        assert _close(value, g['sd3::' + name], 1e-10 if loose else 1e-12), name
        if name.endswith('num_batches_tracked'):
            assert int(value) == steps == int(g['sd3::' + name])
    moved = max(float(np.abs(final[name] - state[name].reshape(final[name].shape)).max()) for name, _ in ref.packing(F, L))
    assert 0.5e-4 < moved < 3.5e-4      # three steps of at most lr each


def test_fixture_float32_run_sits_well_inside_the_gradient_bound(g36):
    """The reference's float32 CPU run against the bound the device is held to: the fraction it uses is the yardstick the README quotes."""
    g, (n, h, w, F, L, steps), state, got = g36
    bounds = ref.gradient_bound(got['cond'])
    worst = 0.0
    for name, _ in ref.packing(F, L):
        err = np.abs(g['g32::' + name].astype(np.float64) - g['g64::' + name]).reshape(bounds[name].shape)
        assert (err <= bounds[name]).all(), name
        worst = max(worst, float((err / np.maximum(bounds[name], 1e-300)).max()))
    print('float32 reference run: largest fraction of the gradient bound {:.4f}'.format(worst))
    assert worst < 0.5


def test_per_voxel_du_and_a_match_autograd_on_a_fresh_float64_restatement():
    """torch.nn modules of our own (not the fixture's), float64, train mode: the gradient autograd leaves at every conv output is du, every conv
    input is a, the parameter gradients and the BatchNorm modules' running statistics are the reference's."""
    n, hw, F, L = 2, 150, 8, 2
    phi, labels, params, got = cases.make_inputs(7, n, hw, F, L)
    convs = [torch.nn.Conv2d(F, F, 1).double() for _ in range(L)]
    norms = [torch.nn.BatchNorm2d(F).double().train() for _ in range(L)]
    last = torch.nn.Conv2d(F, 2, 1).double()
    with torch.no_grad():
        for k in range(L):
            base = 'convs.{}.conv2d_batch_relu.'.format(k)
            convs[k].weight.copy_(torch.from_numpy(params[base + 'conv.weight'].reshape(F, F, 1, 1)))
            convs[k].bias.copy_(torch.from_numpy(params[base + 'conv.bias']))
            norms[k].weight.copy_(torch.from_numpy(params[base + 'bn.weight']))
            norms[k].bias.copy_(torch.from_numpy(params[base + 'bn.bias']))
        last.weight.copy_(torch.from_numpy(params['conv_logits.weight'].reshape(2, F, 1, 1)))
        last.bias.copy_(torch.from_numpy(params['conv_logits.bias']))
    a = torch.from_numpy(phi).double().reshape(n, hw, 1, F).permute(0, 3, 1, 2)
    us, inputs = [], []
    for k in range(L):
        inputs.append(a)
        u = convs[k](a)
        u.retain_grad()
        us.append(u)
        a = torch.relu(norms[k](u))
    inputs.append(a)
    loss = torch.nn.functional.cross_entropy(last(a), torch.from_numpy(labels.astype(np.int64)).reshape(n, hw, 1))
    loss.backward()
    flat = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()      # noqa: E731
    assert _close(got['loss'], float(loss.detach()))
    for k in range(L):
        base = 'convs.{}.conv2d_batch_relu.'.format(k)
        assert _close(got['du'][k], flat(us[k].grad), 1e-13) and _close(got['a'][k], flat(inputs[k]), 1e-13), k
        assert _close(got['grads'][base + 'conv.weight'], convs[k].weight.grad.numpy().reshape(F, F))
        assert _close(got['grads'][base + 'bn.weight'], norms[k].weight.grad.numpy()) and _close(got['grads'][base + 'bn.bias'], norms[k].bias.grad.numpy())
        rm, rv, nbt = ref.update_running(np.zeros(F), np.ones(F), 0, got['mu'][k], got['var'][k], n * hw)
        assert _close(rm, norms[k].running_mean.numpy()) and _close(rv, norms[k].running_var.numpy()) and nbt == int(norms[k].num_batches_tracked)
    assert _close(got['a'][L], flat(inputs[L]), 1e-13) and _close(got['grads']['conv_logits.weight'], last.weight.grad.numpy().reshape(2, F))


def test_the_synthetic_batches_are_continuous_and_unfiltered():
    phi, labels, params, expected = cases.make_inputs(1, 1, 279, 32, 3, zero_channel=31)
    again = cases.make_inputs(1, 1, 279, 32, 3, zero_channel=31)
    assert phi.tobytes() == again[0].tobytes() and labels.tobytes() == again[1].tobytes()
    assert len(np.unique(phi, axis=0)) == 279 and (phi[:, 31] == 0).all() and 0 < labels.mean() < 1
    ratio = np.abs(phi[:, :31].mean(0)) / phi[:, :31].std(0)
    assert ratio.max() > 10 and (phi[:, ::4] >= 0).all()      # |mu| >> sigma somewhere, as the variance has to survive it
    assert expected['var'].min() > 0 and np.isfinite(expected['loss'])


# ------------------------------------------------------------------------------------------------------------------ C ABI
def _header(name):
    with open(os.path.join(ROOT, 'include', name)) as f:
        return f.read()


def test_the_second_header_declares_what_the_library_exports():
    from rcu_amd import _lib
    declared = [name for name, _ in prototypes(_header('rcu_fit.h'))]
    assert set(FIT_NAMES) <= set(declared) and set(declared) == set(_lib.FIT_SIGNATURES)
    lib = _lib.load()
    for name in FIT_NAMES:
        assert name in _lib.FIT_SIGNATURES and name not in _lib.SIGNATURES and hasattr(lib, name), name
    params = dict(prototypes(_header('rcu_fit.h')))['rcu_postnet_loss_grad']
    assert len(params) == len(_lib.FIT_SIGNATURES['rcu_postnet_loss_grad'][1]) == 15 and params[-1] == 'void* stream'
    assert '#include "rcu.h"' in _header('rcu_fit.h') and 'RCU_POSTNET_FIT_MAX_CONVS 4' in _header('rcu_fit.h')


def test_the_first_header_gained_no_prototype():
    """include/rcu.h is as tests/stream_order.py and rcu_amd._lib.SIGNATURES describe it, name for name: the fit's entry points are declared in the
    second header alone (a stream-taking prototype added to rcu.h would need a row in an existing test file)."""
    import stream_order as so
    from rcu_amd import _lib
    declared = [name for name, _ in prototypes(_header('rcu.h'))]
    assert set(declared) == set(_lib.SIGNATURES) and not set(declared) & set(FIT_NAMES)
    assert set(stream_entry_points(_header('rcu.h'))) == set(so.CASES) | set(so.EXEMPT)
    assert not any(name in _header('rcu.h') for name in FIT_NAMES) and 'rcu_fit' not in _header('rcu.h')


def test_arguments_are_checked_without_a_device():
    from rcu_amd import _lib
    lib = _lib.load()
    assert lib.rcu_postnet_fit_param_count(32, 3) == ref.param_count(32, 3) == 3426 and lib.rcu_postnet_fit_param_count(8, 1) == ref.param_count(8, 1)
    for bad in ((0, 3), (33, 3), (32, 0), (32, 5)):
        assert lib.rcu_postnet_fit_param_count(*bad) == 0 and lib.rcu_postnet_fit_workspace_bytes(bad[0], bad[1], 2, 100) == 0
    assert lib.rcu_postnet_fit_workspace_bytes(32, 3, 1, 1) == 0 and lib.rcu_postnet_fit_workspace_bytes(32, 3, 0, 10) == 0
    small, large = lib.rcu_postnet_fit_workspace_bytes(32, 3, 1, 1024), lib.rcu_postnet_fit_workspace_bytes(32, 3, 3, 1025)
    assert 0 < small < large and small % 256 == 0
    p = ctypes.c_void_p(1 << 20)      # never dereferenced: every call below is refused first
    odd = ctypes.c_void_p((1 << 20) + 4)

    def call(features=p, pitch=32, F=32, n=2, hw=100, labels=p, L=3, params=p, grads=p, loss=p, mean=p, var=p, flags=p, ws=p):
        status = lib.rcu_postnet_loss_grad(features, pitch, F, n, hw, labels, L, params, grads, loss, mean, var, flags, ws, None)
        return status, lib.rcu_last_error().decode()

    for kw, word in ((dict(features=None), 'null argument'), (dict(flags=None), 'null argument'), (dict(F=0), 'F must be in 1..32'),
                     (dict(F=33), 'F must be in 1..32'), (dict(pitch=28), 'channel_pitch'), (dict(pitch=34), 'channel_pitch'),
                     (dict(F=8, pitch=8), 'channel_pitch must be >= 32'), (dict(L=0), 'nb_convs'), (dict(L=5), 'nb_convs must be in 1..4'),
                     (dict(n=0), 'n and hw'), (dict(n=1, hw=1), 'N = n \\* hw >= 2'), (dict(n=1 << 21, hw=1 << 20), 'below 2\\^40'),
                     (dict(loss=odd), 'loss_dev and workspace_dev must be 8-byte aligned'), (dict(ws=odd), '8-byte aligned'),
                     (dict(features=ctypes.c_void_p((1 << 20) + 2)), '4-byte aligned')):
        status, message = call(**kw)
        assert status == _lib.RCU_ERR_INVALID and re.search(word, message) and message.startswith('rcu_postnet_loss_grad: '), (kw, message)


def test_the_packing_table_is_the_state_dict(g36):
    from rcu_amd import auxiliary
    from rcu_amd.model import PostNet
    for F, L in ((32, 3), (8, 1), (5, 4)):
        net = PostNet(F, 2, nb_convs=L)
        table = auxiliary.packing(F, L)
        named = dict(net.named_parameters())
        assert [name for name, _ in table] == [name for name, _ in ref.packing(F, L)]
        assert sorted(named) == sorted(name for name, _ in table)
        assert all(tuple(named[name].shape) == tuple(shape) for name, shape in table)
        assert [name for name, _ in auxiliary._ordered_parameters(net)] == [name for name, _ in table]
        assert sum(int(np.prod(shape)) for _, shape in table) == ref.param_count(F, L)
        extra = sorted(set(net.state_dict()) - set(named))
        assert extra == sorted('convs.{}.conv2d_batch_relu.bn.{}'.format(k, s) for k in range(L) for s in ('running_mean', 'running_var', 'num_batches_tracked'))
        assert len(auxiliary._batch_norms(net)) == L
    text = _header('rcu_fit.h')
    for piece in ('convs.k.conv2d_batch_relu.conv.weight [F][F]', 'convs.k.conv2d_batch_relu.conv.bias [F]', 'convs.k.conv2d_batch_relu.bn.weight [F]',
                  'convs.k.conv2d_batch_relu.bn.bias [F]', 'conv_logits.weight [2][F]', 'conv_logits.bias [2]'):
        assert piece in text, piece
    order = [text.index(p) for p in ('conv.weight [F][F]', 'conv.bias [F]', 'bn.weight [F]', 'bn.bias [F]', 'conv_logits.weight', 'conv_logits.bias')]
    assert order == sorted(order)
    g, (n, h, w, F, L, steps), state, _ = g36
    flat = ref.pack(state, F, L)
    assert flat.dtype == np.float32 and all(np.array_equal(v.ravel(), state[k].ravel()) for k, v in ref.unpack(flat, F, L).items())


def test_the_module_refuses_what_the_kernels_do_not_take():
    from rcu_amd import auxiliary
    from rcu_amd.model import PostNet
    with pytest.raises(ValueError, match='dropout'):
        auxiliary._check_postnet(PostNet(32, 2, nb_convs=3, dropout=0.1))
    with pytest.raises(ValueError, match='nb_classes = 2'):
        auxiliary._check_postnet(PostNet(32, 3))
    with pytest.raises(ValueError, match='1..32 feature channels'):
        auxiliary._check_postnet(PostNet(64, 2))
    with pytest.raises(ValueError, match='nb_convs in 1..4'):
        auxiliary._check_postnet(PostNet(32, 2, nb_convs=5))
    with pytest.raises(ValueError, match='PostNet'):
        auxiliary._check_postnet(torch.nn.Conv2d(4, 2, 1))
    with pytest.raises(RuntimeError, match='only runs on the GPU'):
        auxiliary.loss_and_grad(PostNet(32, 2), torch.zeros(1, 32, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))
    logits = torch.tensor([[[[1.0, 2.0, 0.5]], [[1.0, 1.0, 0.7]]]])      # a tie goes to class 0: the first maximum
    target = torch.tensor([[[0, 3, 0]]])
    assert auxiliary.error_target(logits, target).tolist() == [[[0, 1, 1]]] and auxiliary.error_target(logits, target).dtype == torch.uint8


# ------------------------------------------------------------------------------------------------------------------ stream order
def test_every_stream_taking_prototype_of_the_second_header_has_a_row():
    import stream_order as so
    import stream_order_fit as sof
    found = stream_entry_points(_header('rcu_fit.h'))
    assert 'rcu_postnet_loss_grad' in found and found['rcu_postnet_loss_grad'] == []
    assert all(set(hosts) <= set(sof.CASES[name].hosts) for name, hosts in found.items() if name in sof.CASES)
    assert sorted(sof.CASES) == sorted(found) and all(len(case.variants) >= 1 and callable(case.build) for case in sof.CASES.values())
    assert not set(sof.CASES) & (set(so.CASES) | set(so.EXEMPT)), 'the rows of the second header live in a table of their own'


# ------------------------------------------------------------------------------------------------------------------ the script
def _no_world(monkeypatch):
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)


def test_the_key_is_a_row_this_script_alone_takes():
    from rcu_amd import scripts
    rows = [row for row in scripts._OTHERS if row.name == 'auxiliary_fit']
    assert len(rows) == 1 and rows[0].scripts == frozenset(('fit_auxiliary_feat',))
    assert 'auxiliary_fit' in [row.name for row in scripts._OTHERS if 'fit_auxiliary_feat' in row.scripts]
    assert scripts.fit_auxiliary_feat.__test__ is False


@pytest.mark.parametrize('others, word', [
    ('    mc: 20\n', 'others.mc: the auxiliary fit is one eval-mode pass'), ('    tta: [identity]\n', 'others.tta: the auxiliary fit'),
    ('    temperature: 1.5\n', 'others.temperature .*fit_auxiliary_feat script does not take it'),
    ('    agreement: true\n', 'others.agreement .*fit_auxiliary_feat script does not take it'),
    ('    mc_adaptive: {check_at: [5], tolerance: 0.01}\n', 'others.mc_adaptive .*fit_auxiliary_feat script does not take it'),
    ('    logit_samples: 4\n', 'others.logit_samples .*fit_auxiliary_feat script does not take it'),
    ('    corruption: gaussian_noise\n', 'others.corruption .*fit_auxiliary_feat script does not take it'),
    ('    density: d.npz\n', 'others.density .*fit_auxiliary_feat script does not take it'),
    ('    laplace: l.npz\n', 'others.laplace .*fit_auxiliary_feat script does not take it')])
def test_fit_script_refuses_every_other_row_by_name(tmp_path, monkeypatch, others, word):
    from rcu_amd import scripts
    _no_world(monkeypatch)
    with pytest.raises(ValueError, match=word):
        scripts.fit_auxiliary_feat('brats', _yaml_with(tmp_path, others + '    auxiliary_fit: {epochs: 2}\n'), device='cpu')
    assert not (tmp_path / 'out').exists()


@pytest.mark.parametrize('script', ['test_default', 'test_ensemble', 'test_aleatoric', 'test_auxiliary_feat', 'test_auxiliary_segm', 'fit_temperature',
                                    'fit_density', 'fit_laplace'])
def test_other_scripts_refuse_the_key(tmp_path, monkeypatch, script):
    from rcu_amd import scripts
    _no_world(monkeypatch)
    path = _yaml_with(tmp_path, '    model_dir: [{}]\n    auxiliary_fit: {{epochs: 2}}\n'.format(tmp_path / 'train' / 'model_x'))
    with pytest.raises(ValueError, match='others.auxiliary_fit.*the {} script does not take it'.format(script.replace('test_', ''))):
        if script.startswith('fit_'):
            getattr(scripts, script)('brats', str(path), device='cpu')
        elif script == 'test_default':
            scripts.test_default('brats', str(path), None, device='cpu')
        else:
            getattr(scripts, script)('brats', config_file=str(path), device='cpu')
    assert not (tmp_path / 'out').exists()


def test_fit_script_runs_in_one_process_and_checks_its_options(monkeypatch):
    from rcu_amd import distributed as rdist
    from rcu_amd import scripts
    monkeypatch.setattr(scripts, '_context', lambda device, config_file: (_context(dict()), rdist.World(rank=0, world=2)))
    with pytest.raises(ValueError, match='the auxiliary_feat fit runs in one process'):
        scripts.fit_auxiliary_feat('brats', 'unused.yaml', device='cpu')
    with pytest.raises(ValueError, match='brats'):
        scripts.fit_auxiliary_feat('other', 'x.yaml')
    assert scripts._auxiliary_fit_options(_context(dict())) == (1, 1e-4, 3)
    assert scripts._auxiliary_fit_options(_context(dict(auxiliary_fit=dict(epochs=4, lr='2e-4', nb_convs=2)))) == (4, 2e-4, 2)
    for value, word in ((dict(steps=3), 'takes epochs, lr, nb_convs; got steps'), (dict(epochs=0), 'epochs must be an integer >= 1'),
                        (dict(epochs=True), 'epochs'), (dict(nb_convs=5), 'nb_convs must be an integer in 1..4'), (dict(lr=0), 'lr must be a number > 0'),
                        (dict(lr='fast'), 'lr must be a number > 0')):
        with pytest.raises(ValueError, match='others.auxiliary_fit.*' + word):
            scripts._auxiliary_fit_options(_context(dict(auxiliary_fit=value)))
    with pytest.raises(ValueError, match='UNet'):
        scripts._check_auxiliary_model(torch.nn.Conv2d(4, 2, 1))


@pytest.mark.parametrize('dataset', ['brats', 'isic'])
def test_entry_points_wrap_the_fit(dataset):
    text = open(os.path.join(ROOT, 'bin-dl', '{}_fit_auxiliary_feat.py'.format(dataset))).read()
    assert "scripts.fit_auxiliary_feat('{}', args.config_file)".format(dataset) in text and "add_argument('-config_file'" in text
