"""Last-layer Laplace without a GPU (include/rcu.h "Last-layer Laplace"): tests/laplace_reference.py against the independent witnesses of fixture
G35 (torch autograd's Hessian, numpy.linalg.inv, numpy.linalg.slogdet), rcu_amd.laplace.fit_from_moments against the reference and under any
slice order or batching, the file round trip, and every refusal."""
import itertools

import numpy as np
import pytest
import torch

import laplace_reference as ref

CASES = ((24, 3), (32, 2), (40, 4), (64, 2))
RTOL = 1e-9


@pytest.fixture(scope='module')
def g35(golden):
    return golden('g35_laplace')


def _case(g, F, C):
    tag = '{}_{}'.format(F, C)
    return {k[:-len(tag) - 1]: v for k, v in g.items() if k.endswith('_' + tag)}


def _theta(c):
    return np.concatenate([c['W'], c['w0'][:, None]], 1).astype(np.float64)


def _close(a, b, rtol=RTOL):
    scale = float(np.abs(b).max())
    assert float(np.abs(a - b).max()) <= rtol * scale, (float(np.abs(a - b).max()), scale)


@pytest.mark.parametrize('F, C', CASES)
def test_the_reference_hessian_is_autograds(g35, F, C):
    c = _case(g35, F, C)
    p64 = ref.softmax(c['z'])
    w, S, G = ref.moments(c['psi'], p64)
    H = ref.hessian(ref.fsum_slices(w), ref.fsum_slices(S), ref.fsum_slices(G))
    _close(H, c['H'])
    D, dead = F + 1, int(g35['dead_channel'])
    assert not H[[k * D + dead for k in range(C)]].any(), 'the dead channel was meant to leave zero rows'
    # with the float32 probabilities the device reads, the Hessian moves by their rounding alone
    w32, S32, G32 = ref.moments(c['psi'], c['p32'])
    _close(ref.hessian(ref.fsum_slices(w32), ref.fsum_slices(S32), ref.fsum_slices(G32)), c['H'], rtol=1e-5)


@pytest.mark.parametrize('F, C', CASES)
def test_a_saturated_voxel_has_no_curvature_in_float32(g35, F, C):
    c = _case(g35, F, C)
    s, v = (int(k) for k in g35['saturated'])
    om = ref.omega(c['p32'])
    assert om.dtype == np.float32 and not om[s, v].any() and sorted(c['p32'][s, v].tolist()) == [0.0] * (C - 1) + [1.0]
    # the float32 weights are what the definition says, operation by operation
    p = c['p32']
    for q, (a, b) in enumerate(ref.pairs(C)):
        want = np.multiply(p[..., a], np.subtract(np.float32(1), p[..., a])) if a == b else np.negative(np.multiply(p[..., a], p[..., b]))
        assert om[..., q].tobytes() == want.astype(np.float32).tobytes()
    assert (om[..., [q for q, (a, b) in enumerate(ref.pairs(C)) if a == b]] >= 0).all()


@pytest.mark.parametrize('F, C', CASES)
def test_the_reference_variance_is_the_inverse_hessians(g35, F, C):
    c = _case(g35, F, C)
    fit = ref.fit(*ref.moments(c['psi'], ref.softmax(c['z'])), _theta(c), float(c['scale']), float(c['tau']))
    pred = ref.predictive(fit['A'], fit['b'], fit['kappa'], c['psi'].reshape(-1, F), c['z'].reshape(-1, C))
    want = c['s2'].reshape(-1, C)
    assert float(np.abs(pred['s2'] / want - 1.0).max()) <= RTOL
    assert (np.tril(fit['A'], -1) == 0).all(), 'A is the transposed Cholesky factor: upper triangular'
    assert (fit['kappa'] > 0).all() and (pred['s2'] >= fit['kappa'][None] * (1 - 1e-12)).all()
    assert np.abs(pred['p'].sum(1) - 1).max() < 1e-12 and (pred['zt'] * c['z'].reshape(-1, C) >= 0).all()


@pytest.mark.parametrize('F, C', CASES)
def test_the_evidence_argmax_is_slogdets(g35, F, C):
    c = _case(g35, F, C)
    tau, scores = ref.evidence_tau(float(c['scale']) * c['H'], _theta(c))
    assert tau == float(c['evtau'])
    assert float(np.abs(np.array(scores) - c['evscores']).max()) <= RTOL * float(np.abs(c['evscores']).max())
    assert ref.GRID[0] < tau < ref.GRID[-1], 'the maximiser was meant to lie inside the grid'


# ------------------------------------------------------------------------------------------------------------------- package
def _bits(fit):
    return [getattr(fit, name).tobytes() for name in ('H', 'Sigma', 'A', 'b', 'kappa')] + [fit.tau]


@pytest.mark.parametrize('F, C', CASES)
@pytest.mark.parametrize('prior', [None, 'evidence'])
def test_fit_from_moments_is_the_reference(g35, F, C, prior):
    from rcu_amd import laplace
    c = _case(g35, F, C)
    moments = ref.moments(c['psi'], c['p32'])
    prior = float(c['tau']) if prior is None else prior
    ours = laplace.fit_from_moments(*moments, _theta(c), float(c['scale']), prior, temperature=1.0, voxels=192)
    theirs = ref.fit(*moments, _theta(c), float(c['scale']), prior)
    assert ours.tau == theirs['tau'] and (ours.F, ours.C, ours.voxels) == (F, C, 192)
    for name in ('H', 'Sigma', 'A', 'b', 'kappa'):
        _close(getattr(ours, name), theirs[name], rtol=1e-9)
    a32, b32, k32 = ours.float32_parameters()
    assert a32.dtype == b32.dtype == k32.dtype == np.float32 and a32.shape == (C, F, F)


def test_fit_from_moments_gives_the_same_bits_for_any_order_and_batching(g35):
    from rcu_amd import laplace
    c = _case(g35, 24, 3)
    rng = np.random.default_rng(5)
    # nine slices of very different magnitude: a plain sum would depend on the order
    scales = 10.0 ** rng.uniform(-2, 2, 9)
    psi = np.concatenate([c['psi']] * 3) * scales[:, None, None].astype(np.float32)
    p = np.concatenate([c['p32']] * 3)
    w, S, G = ref.moments(psi, p)
    first = None
    for order in itertools.islice(itertools.permutations(range(9)), 0, 40320, 4481):
        order = list(order)
        fit = laplace.fit_from_moments(w[order], S[order], G[order], _theta(c), 1.0, 'evidence')
        first = first or _bits(fit)
        assert _bits(fit) == first
    as_tensors = laplace.fit_from_moments(torch.from_numpy(w), torch.from_numpy(S), torch.from_numpy(G), _theta(c), 1.0, 'evidence')
    assert _bits(as_tensors) == first
    plain = ref.hessian(w.sum(0), S.sum(0), G.sum(0))
    assert not np.array_equal(plain, as_tensors.H), 'the slices were meant to make a plain sum round differently'


def test_the_file_round_trip(g35, tmp_path):
    from rcu_amd import laplace
    c = _case(g35, 32, 2)
    fit = laplace.fit_from_moments(*ref.moments(c['psi'], c['p32']), _theta(c), 0.25, 'evidence', temperature=1.7, voxels=192)
    path = tmp_path / 'laplace.npz'
    laplace.save_laplace(fit, path)
    back = laplace.load_laplace(str(path))
    assert _bits(back) == _bits(fit)
    assert back.as_dict() == fit.as_dict() == {'F': 32, 'C': 2, 'tau': fit.tau, 'hessian_scale': 0.25, 'temperature': 1.7, 'voxels': 192}
    with np.load(path, allow_pickle=False) as doc:
        assert sorted(doc.files) == sorted(['H', 'Sigma', 'A', 'b', 'kappa', 'tau', 'hessian_scale', 'temperature', 'voxels'])
    np.savez(tmp_path / 'other.npz', A=fit.A)
    with pytest.raises(ValueError, match='cannot be read: no H, Sigma'):
        laplace.load_laplace(tmp_path / 'other.npz')
    with pytest.raises(ValueError, match='cannot be read'):
        laplace.load_laplace(tmp_path / 'missing.npz')
    (tmp_path / 'text.npz').write_text('no archive')
    with pytest.raises(ValueError, match='cannot be read'):
        laplace.load_laplace(tmp_path / 'text.npz')


def test_every_refusal_names_its_cause(g35):
    from rcu_amd import laplace, steps
    from rcu_amd.model import UNet
    c = _case(g35, 32, 2)
    moments = ref.moments(c['psi'], c['p32'])
    theta = _theta(c)
    for bad in (0, -1.0, float('nan'), float('inf'), True, 'large'):
        with pytest.raises(ValueError, match='hessian_scale must be'):
            laplace.fit_from_moments(*moments, theta, bad, 1.0)
    for bad in (0, -2.0, float('nan'), True, 'marginal', None):
        with pytest.raises(ValueError, match='prior_precision must be'):
            laplace.fit_from_moments(*moments, theta, 1.0, bad)
    with pytest.raises(ValueError, match=r'theta must be \[C, F \+ 1\] = \[2, 33\]'):
        laplace.fit_from_moments(*moments, theta[:, :-1], 1.0, 1.0)
    with pytest.raises(ValueError, match='expected w'):
        laplace.fit_from_moments(moments[0], moments[1], moments[2][:, :, :-1], theta, 1.0, 1.0)
    with pytest.raises(ValueError, match='4 pairs'):
        laplace.fit_from_moments(np.zeros((1, 4)), np.zeros((1, 4, 3)), np.zeros((1, 4, 3, 3)), np.zeros((2, 4)), 1.0, 1.0)
    with pytest.raises(ValueError, match='not finite'):
        laplace.fit_from_moments(moments[0], moments[1], np.full_like(moments[2], np.inf), theta, 1.0, 1.0)
    for classes in (1, 5, 8):
        with pytest.raises(ValueError, match='2..4 classes, got {}'.format(classes)):
            laplace.pairs(classes)
    assert laplace.pairs(3) == ref.pairs(3) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    fit = laplace.fit_from_moments(*moments, theta, 1.0, 1.0)

    # the model's side
    params = dict(in_channels=4, depth=2, dropout=0.05)
    with pytest.raises(ValueError, match='needs a rcu_amd.model.UNet'):
        laplace.check_model(torch.nn.Conv2d(4, 2, 1), fit)
    with pytest.raises(ValueError, match='sigma_out model'):
        laplace.check_model(UNet(nb_classes=2, start_filters=32, sigma_out=True, **params), fit)
    with pytest.raises(ValueError, match='F = 32, C = 2; the model has start_filters = 24, nb_classes = 2'):
        laplace.check_model(UNet(nb_classes=2, start_filters=24, **params), fit)
    with pytest.raises(ValueError, match='F = 32, C = 2; the model has start_filters = 32, nb_classes = 3'):
        laplace.check_model(UNet(nb_classes=3, start_filters=32, **params), fit)
    for classes in (1, 5):
        with pytest.raises(ValueError, match='2..4 classes, got {}'.format(classes)):
            laplace.check_model(UNet(nb_classes=classes, start_filters=32, **params))
    scaled = UNet(nb_classes=2, start_filters=32, **params)
    assert laplace.check_model(scaled, fit) == (32, 2)
    scaled.set_temperature(1.5)
    with pytest.raises(ValueError, match='made at temperature 1.0, the model runs at 1.5'):
        laplace.check_model(scaled, fit)
    theta_scaled = laplace.classifier_parameters(scaled)
    scaled.set_temperature(1.0)
    assert theta_scaled.shape == (2, 33) and np.array_equal(theta_scaled * 1.5, laplace.classifier_parameters(scaled))

    # the step's own arguments
    with pytest.raises(ValueError, match='needs a laplace.LaplaceFit'):
        steps.LaplacePredictStep(dict(A=fit.A))
    with pytest.raises(ValueError, match='link must be one of probit, sample'):
        steps.LaplacePredictStep(fit, link='logistic')
    with pytest.raises(ValueError, match="link='sample' needs samples >= 1"):
        steps.LaplacePredictStep(fit, link='sample')
    with pytest.raises(ValueError, match='logit_samples must be an integer'):
        steps.LaplacePredictStep(fit, link='sample', samples=2.5)
    with pytest.raises(ValueError, match='integer seed'):
        steps.LaplacePredictStep(fit, seed='x')
    assert steps.LaplacePredictStep(fit, link='sample', samples=4, seed=3).samples == 4
    with pytest.raises(ValueError, match='A must be'):
        laplace.LaplaceFit(fit.H, fit.Sigma, fit.A[0], fit.b, fit.kappa, 1.0, 1.0, 1.0, 0)
    with pytest.raises(ValueError, match='do not have the shapes'):
        laplace.LaplaceFit(fit.H[:-1], fit.Sigma, fit.A, fit.b, fit.kappa, 1.0, 1.0, 1.0, 0)
