"""Feature-space density without a GPU (include/rcu.h "Feature-space density"): the float64 reference against the scipy witnesses of fixture G32,
the host-side fit of rcu_amd.density (exactly rounded sums, ridge, refusals, shared covariance, the .npz round trip) and the C symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

import density_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = (8, 32, 64)


@pytest.fixture(scope='module')
def g32(golden):
    return golden('g32_density')


@pytest.fixture(scope='module')
def density():
    from rcu_amd import density
    return density


def _labels(g, K):
    return {1: np.zeros_like(g['labels2']), 2: g['labels2'], 3: g['labels3']}[K]


@pytest.mark.parametrize('F', FS)
def test_reference_energies_equal_the_scipy_witness(g32, F):
    phi = g32['phi_{}'.format(F)]
    for K, key in ((1, 'e1_{}'), (2, 'e_{}'), (3, 'e3_{}')):
        fit = ref.fit(*ref.moments(phi, _labels(g32, K), K), ridge=float(g32['ridge']))
        e, _ = ref.energy(fit['A'], fit['b'], fit['k'], phi.reshape(-1, F))
        want = g32[key.format(F)].reshape(-1)
        worst = float(np.max(np.abs(e - want) / np.abs(want)))
        print('F = {}, K = {}: largest relative difference to the witness {:.3e}'.format(F, K, worst))
        assert worst <= 1e-10, (F, K, worst)


@pytest.mark.parametrize('F', FS)
def test_reference_moments_and_fit_equal_the_fixture(g32, density, F):
    phi = g32['phi_{}'.format(F)]
    n, S, G = ref.moments(phi, g32['labels2'], 2)
    assert np.array_equal(n, g32['n_{}'.format(F)])
    np.testing.assert_allclose(S, g32['S_{}'.format(F)], rtol=1e-13, atol=1e-11)
    np.testing.assert_allclose(G, g32['G_{}'.format(F)], rtol=1e-13, atol=1e-11)
    assert int(n[2, 1]) == 0      # the slice that lacks a class
    for fit in (ref.fit(n, S, G), density.fit_from_moments(n, S, G).__dict__):
        np.testing.assert_allclose(fit['mu'], g32['mu_{}'.format(F)], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(fit['k'], g32['k_{}'.format(F)], rtol=1e-11)
        scale = np.abs(g32['A_{}'.format(F)]).max()
        np.testing.assert_allclose(fit['A'], g32['A_{}'.format(F)], rtol=0, atol=1e-8 * scale)
        assert np.array_equal(fit['A'], np.tril(fit['A']))
    mine, theirs = density.fit_from_moments(n, S, G), ref.fit(n, S, G)
    for name in ('mu', 'cov', 'A', 'b', 'k'):
        np.testing.assert_allclose(getattr(mine, name), theirs[name], rtol=1e-12, atol=1e-12 * np.abs(theirs[name]).max())
    assert (mine.F, mine.K, mine.voxels, list(mine.n)) == (F, 2, 3 * 312, [int(v) for v in n.sum(0)])
    assert mine.as_dict()['counts'] == [int(v) for v in n.sum(0)] and mine.as_dict()['ridge'] == 1e-6


def _bits(fit):
    return [getattr(fit, name).tobytes() for name in ('n', 'mu', 'cov', 'A', 'b', 'k')]


@pytest.mark.parametrize('F', (8, 32))
def test_fit_is_invariant_under_slice_order_and_batching(g32, density, F):
    """The fsum property: the same per-slice moments in any order, or concatenated from any batches, give the same bits."""
    phi = g32['phi_{}'.format(F)].astype(np.float64)
    # nine slices whose sums do not round alike: the fixture's three, and two rescaled copies (a plain left-to-right sum depends on their order)
    phis = np.concatenate([phi, phi * 1.0e3 * np.pi, phi * 1.0e-3 / 7.0])
    labels = np.concatenate([g32['labels2']] * 3)
    n, S, G = ref.moments(phis, labels, 2)
    base = _bits(density.fit_from_moments(n, S, G))
    rng = np.random.default_rng(5)
    orders = [np.arange(9)[::-1], rng.permutation(9), rng.permutation(9)]
    assert any(not np.array_equal(np.cumsum(S[o], 0)[-1], np.cumsum(S, 0)[-1]) for o in orders), 'the plain sum does not see the order: weak data'
    for order in orders:
        assert _bits(density.fit_from_moments(n[order], S[order], G[order])) == base
    for cuts in ((9,), (4, 5), (1, 8), (2, 3, 4)):      # the moments of the batches, concatenated as fit_density concatenates them
        edges = np.cumsum((0,) + cuts)
        parts = [ref.moments(phis[a:b], labels[a:b], 2) for a, b in zip(edges[:-1], edges[1:])]
        assert _bits(density.fit_from_moments(*(np.concatenate([p[i] for p in parts]) for i in range(3)))) == base


def test_ridge_lets_the_dead_channel_through(g32, density):
    F, dead = 32, int(g32['dead_channel'])
    n, S, G = (g32[k.format(F)] for k in ('n_{}', 'S_{}', 'G_{}'))
    with pytest.raises(ValueError, match='class 0.*positive definite'):
        density.fit_from_moments(n, S, G, ridge=0.0)
    fit = density.fit_from_moments(n, S, G)
    plain = fit.cov[:, dead, dead] / (np.trace(fit.cov, axis1=1, axis2=2) / F)
    np.testing.assert_allclose(plain, 1e-6, rtol=1e-5)      # the channel's own variance is exactly zero: what is left is the ridge
    assert np.all(np.abs(fit.A[:, dead, dead]) > 100.0) and np.all(np.isfinite(fit.A)) and np.all(np.isfinite(fit.k))
    for c in range(2):
        L = np.linalg.inv(fit.A[c])
        np.testing.assert_allclose(L @ L.T, fit.cov[c], rtol=0, atol=1e-9 * np.abs(fit.cov[c]).max())
    with pytest.raises(ValueError, match='ridge'):
        density.fit_from_moments(n, S, G, ridge=-1.0)


def test_a_class_with_too_few_voxels_is_refused_by_name(g32, density):
    F = 64
    n, S, G = ref.moments(g32['phi_64'][:1, :150], g32['labels3'][:1, :150], 3)
    assert (n.sum(0) <= F).any()
    first = int(np.argmax(n.sum(0) <= F))
    with pytest.raises(ValueError, match='class {} has {} voxels'.format(first, int(n.sum(0)[first]))):
        density.fit_from_moments(n, S, G)
    n8, S8, G8 = ref.moments(g32['phi_8'], g32['labels3'], 3)
    density.fit_from_moments(n8, S8, G8)
    n8[:, 1] = 0
    with pytest.raises(ValueError, match='class 1 has 0 voxels'):
        density.fit_from_moments(n8, S8, G8)
    with pytest.raises(ValueError, match='expected n'):
        density.fit_from_moments(n[0], S, G)


@pytest.mark.parametrize('F', (8, 32))
def test_shared_covariance_is_the_pooled_formula(g32, density, F):
    n, S, G = ref.moments(g32['phi_{}'.format(F)], g32['labels3'], 3)
    fit = density.fit_from_moments(n, S, G, shared_covariance=True)
    assert fit.shared_covariance
    x = g32['phi_{}'.format(F)].reshape(-1, F).astype(np.float64)
    y = g32['labels3'].reshape(-1)
    pooled = np.zeros((F, F))
    for c in range(3):
        xc = x[y == c]
        mu = xc.mean(0)
        pooled += (xc - mu).T @ (xc - mu)       # n_c Sigma_c, centred form
    pooled /= x.shape[0]
    pooled += 1e-6 * (np.trace(pooled) / F) * np.eye(F)
    for c in range(3):
        np.testing.assert_allclose(fit.cov[c], pooled, rtol=0, atol=1e-10 * np.abs(pooled).max())
        assert np.array_equal(fit.cov[c], fit.cov[0]) and np.array_equal(fit.A[c], fit.A[0])
    # one covariance: the classes' constants differ by their log priors alone
    np.testing.assert_allclose(fit.k - fit.k[0], np.log(fit.n / fit.voxels) - np.log(fit.n[0] / fit.voxels), rtol=0, atol=1e-13)
    theirs = ref.fit(n, S, G, shared_covariance=True)
    np.testing.assert_allclose(fit.A, theirs['A'], rtol=1e-12, atol=1e-12 * np.abs(theirs['A']).max())


def test_save_and_load_round_trip_the_bits(g32, density, tmp_path):
    n, S, G = (g32[k.format(32)] for k in ('n_{}', 'S_{}', 'G_{}'))
    for shared in (False, True):
        fit = density.fit_from_moments(n, S, G, ridge=3e-6, shared_covariance=shared)
        path = tmp_path / 'density_{}.npz'.format(int(shared))
        density.save_density(fit, path)
        back = density.load_density(str(path))
        assert _bits(back) == _bits(fit)
        assert (back.ridge, back.shared_covariance, back.F, back.K, back.voxels) == (3e-6, shared, 32, 2, fit.voxels)
        a32, b32, k32 = back.float32_parameters()
        assert a32.dtype == b32.dtype == k32.dtype == np.float32 and np.array_equal(a32, fit.A.astype(np.float32))
    with pytest.raises(ValueError, match='cannot be read'):
        density.load_density(str(tmp_path / 'missing.npz'))
    np.savez(str(tmp_path / 'other.npz'), mu=np.zeros((2, 4)))
    with pytest.raises(ValueError, match='cannot be read'):
        density.load_density(str(tmp_path / 'other.npz'))


def test_host_side_refusals_need_no_gpu(density):
    import torch
    with pytest.raises(RuntimeError, match='only runs on the GPU'):
        density.feature_moments(torch.zeros(1, 8, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8), 2)
    with pytest.raises(ValueError, match='nb_classes'):
        density.feature_moments(torch.zeros(1, 8, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8), 9)
    with pytest.raises(ValueError, match='UNet'):
        density.fit_density(torch.nn.Conv2d(1, 1, 1), [])
    from rcu_amd import steps
    with pytest.raises(ValueError, match='DensityFit'):
        steps.DensityPredictStep({'A': 1})


def test_c_symbols_have_the_documented_signatures():
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'rcu.h')).read()
    assert 'Feature-space density' in header
    flat = re.sub(r'/\*.*?\*/', ' ', header, flags=re.S)
    flat = re.sub(r'\s+', ' ', flat)
    want = {
        'rcu_density_moments_workspace_bytes': 'size_t rcu_density_moments_workspace_bytes(size_t n, size_t hw, int F, int K);',
        'rcu_density_moments': 'int rcu_density_moments(const float* features_dev, int channel_pitch, int F, const uint8_t* labels_dev , size_t n, '
                               'size_t hw, int K, int64_t* n_out_dev , double* S_out_dev , double* G_out_dev , void* workspace_dev, void* stream);',
        'rcu_density_energy': 'int rcu_density_energy(const float* features_dev, int channel_pitch, int F, size_t n_voxels, int K, const float* A_dev , '
                              'const float* b_dev , const float* k_dev , float* energy_dev , float* d2_dev , void* stream);',
    }
    for name, text in want.items():
        assert text in flat, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == text.count(',') + 1, name
    so = _lib.load()
    assert re.search(r'#define RCU_DENSITY_CHUNK (\d+)', header).group(1) == str(ref.CHUNK)
    # the workspace: one record per chunk of RCU_DENSITY_CHUNK voxels; 0 for arguments out of range
    small, large = so.rcu_density_moments_workspace_bytes(3, ref.CHUNK, 32, 2), so.rcu_density_moments_workspace_bytes(3, ref.CHUNK + 1, 32, 2)
    assert 0 < small < large and so.rcu_density_moments_workspace_bytes(3, 100, 65, 2) == 0 and so.rcu_density_moments_workspace_bytes(3, 100, 8, 9) == 0
    # every argument is checked before the device is touched
    p = ctypes.c_void_p(4096)
    for args, word in (((p, 32, 65, 10, 2, p, p, p, p, None, None), b'F must be'), ((p, 30, 32, 10, 2, p, p, p, p, None, None), b'channel_pitch'),
                       ((p, 34, 32, 10, 2, p, p, p, p, None, None), b'channel_pitch'), ((p, 32, 32, 10, 9, p, p, p, p, None, None), b'K must be'),
                       ((p, 32, 32, 0, 2, p, p, p, p, None, None), b'n_voxels'), ((None, 32, 32, 10, 2, p, p, p, p, None, None), b'null'),
                       ((ctypes.c_void_p(4100), 32, 32, 10, 2, p, p, p, p, None, None), b'16-byte')):
        assert so.rcu_density_energy(*args) == -1 and word in so.rcu_last_error(), word
    for args, word in (((p, 32, 0, p, 1, 10, 2, p, p, p, p, None), b'F must be'), ((p, 8, 12, p, 1, 10, 2, p, p, p, p, None), b'channel_pitch'),
                       ((p, 32, 32, p, 1, 10, 0, p, p, p, p, None), b'K must be'), ((p, 32, 32, p, 0, 10, 2, p, p, p, p, None), b'n must be'),
                       ((p, 32, 32, p, 1, 10, 2, p, p, p, None, None), b'null')):
        assert so.rcu_density_moments(*args) == -1 and word in so.rcu_last_error(), word
