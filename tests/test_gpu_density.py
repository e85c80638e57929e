"""Feature-space density on the GPU (include/rcu.h "Feature-space density"): the moments kernel and the energy kernel against the float64
reference with the bounds of their float32 arithmetic, their bit-for-bit contracts (a slice's rows / a voxel's energy are functions of that slice /
voxel alone), the predict step and the fit on a synthetic U-Net, and the scripts end to end.

Largest fractions of the bounds used on the MI355X (every test prints its own): moments 0.013, d2 0.028, energy 0.026 (README, "Feature-space
density")."""
import ctypes
import csv
import glob
import json
import os

import numpy as np
import pytest
import torch

import density_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PITCH = {8: 32, 32: 32, 64: 64}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda')


@pytest.fixture(scope='module')
def g32(golden):
    return golden('g32_density')


def _labels(g, K):
    return {1: np.zeros_like(g['labels2']), 2: g['labels2'], 3: g['labels3']}[K]


def _at_pitch(phi, pitch, seed=1):
    """[..., F] -> float32 [..., pitch] with finite garbage planted in the padding channels."""
    out = (np.random.default_rng(seed).standard_normal(phi.shape[:-1] + (pitch,)) * 1.0e3).astype(np.float32)
    out[..., :phi.shape[-1]] = phi
    return out


def _moments(x, pitch, F, labels, n, hw, K, dev):
    """rcu_density_moments on device tensors (any views: their data_ptr is what the kernel gets) -> numpy (n, S, G)."""
    from rcu_amd import _lib
    lib = _lib.load()
    counts = torch.full((n, K), -1, device=dev, dtype=torch.int64)
    S = torch.full((n, K, F), float('nan'), device=dev, dtype=torch.float64)
    G = torch.full((n, K, F, F), float('nan'), device=dev, dtype=torch.float64)
    ws = torch.empty(lib.rcu_density_moments_workspace_bytes(n, hw, F, K) // 8, device=dev, dtype=torch.float64)
    _lib.check(lib.rcu_density_moments(ctypes.c_void_p(x.data_ptr()), pitch, F, ctypes.c_void_p(labels.data_ptr()), n, hw, K, _lib.ptr(counts),
                                       _lib.ptr(S), _lib.ptr(G), _lib.ptr(ws), _lib.current_stream()))
    return counts.cpu().numpy(), S.cpu().numpy(), G.cpu().numpy()


def _check_moments(got, phi, labels, K, tag):
    counts, S, G = got
    rn, rS, rG = ref.moments(phi, labels, K)
    bS, bG = ref.moment_bounds(phi, labels, K)
    assert np.array_equal(counts, rn), tag
    assert np.isfinite(S).all() and np.isfinite(G).all(), tag
    eS, eG = np.abs(S - rS), np.abs(G - rG)
    assert (eS <= bS).all() and (eG <= bG).all(), (tag, float((eS - bS).max()), float((eG - bG).max()))
    assert np.array_equal(G, np.swapaxes(G, 2, 3)), tag          # both triangles, the same bits
    used = max(float((eS[bS > 0] / bS[bS > 0]).max()), float((eG[bG > 0] / bG[bG > 0]).max()))
    print('moments {}: largest fraction of the bound used {:.4f}'.format(tag, used))
    return used


@pytest.mark.parametrize('K', [2, 3])
@pytest.mark.parametrize('F', [8, 32, 64])
@pytest.mark.parametrize('hw', [279, 312])
def test_moments_against_the_reference(dev, g32, hw, F, K):
    phi = g32['phi_{}'.format(F)][:, :hw]
    labels = np.ascontiguousarray(_labels(g32, K)[:, :hw])
    assert (ref.moments(phi, labels, K)[0] == 0).any(), 'a slice was meant to lack a class'
    x = torch.from_numpy(_at_pitch(phi, PITCH[F])).to(dev)
    got = _moments(x, PITCH[F], F, torch.from_numpy(labels).to(dev), 3, hw, K, dev)
    _check_moments(got, phi, labels, K, 'hw={} F={} K={}'.format(hw, F, K))


@pytest.mark.parametrize('F, K', [(32, 2), (64, 3), (20, 8)])
def test_moments_over_several_chunks(dev, F, K):
    """hw beyond two chunks of RCU_DENSITY_CHUNK voxels, odd: three float32 chunk sums are promoted and added in float64, (c0 + c1) + c2."""
    hw = 2 * ref.CHUNK + 279
    rng = np.random.default_rng(F + K)
    phi = (rng.standard_normal((3, hw, F)) * rng.uniform(0.2, 3.0, F) + rng.standard_normal(F)).astype(np.float32)
    labels = rng.integers(0, K, (3, hw)).astype(np.uint8)
    labels[1][labels[1] == K - 1] = 0
    pitch = (F + 3) // 4 * 4 + 4
    x = torch.from_numpy(_at_pitch(phi, pitch)).to(dev)
    got = _moments(x, pitch, F, torch.from_numpy(labels).to(dev), 3, hw, K, dev)
    _check_moments(got, phi, labels, K, 'hw={} F={} K={}'.format(hw, F, K))


@pytest.mark.parametrize('F, hw', [(8, 279), (32, 279), (64, 312), (32, 2 * 1024 + 279)])
def test_moments_of_a_slice_do_not_depend_on_the_batch_or_the_pointers(dev, g32, F, hw):
    K, pitch = 3, PITCH[F]
    if hw <= 312:
        phi, labels = g32['phi_{}'.format(F)][:, :hw], np.ascontiguousarray(g32['labels3'][:, :hw])
    else:
        rng = np.random.default_rng(3)
        phi, labels = rng.standard_normal((3, hw, F)).astype(np.float32), rng.integers(0, K, (3, hw)).astype(np.uint8)
    x = torch.from_numpy(_at_pitch(phi, pitch)).to(dev)
    y = torch.from_numpy(labels).to(dev)
    batch = _moments(x, pitch, F, y, 3, hw, K, dev)
    alone = _moments(x[1], pitch, F, y[1], 1, hw, K, dev)
    # the same three slices one slice into a larger allocation (an odd hw leaves the label pointer unaligned), other garbage in the padding
    big_x = torch.from_numpy(_at_pitch(np.concatenate([phi[2:], phi, phi[:1]]), pitch, seed=7)).to(dev)
    big_y = torch.from_numpy(np.concatenate([labels[2:], labels, labels[:1]])).to(dev)
    moved = _moments(big_x[1:], pitch, F, big_y[1:], 3, hw, K, dev)
    first = _moments(big_x[2:], pitch, F, big_y[2:], 2, hw, K, dev)       # ... and as the first of two
    for a, b, m, f in zip(batch, alone, moved, first):
        assert a[1].tobytes() == b[0].tobytes() == m[1].tobytes() == f[0].tobytes()
        assert a.tobytes() == m.tobytes()


def test_a_label_beyond_the_classes_is_an_error(dev, g32):
    from rcu_amd import _lib, density
    phi = g32['phi_8']
    x = torch.from_numpy(_at_pitch(phi, 32)).to(dev)
    y = torch.from_numpy(g32['labels3']).to(dev)
    with pytest.raises(_lib.RcuError, match='label >= K'):
        _moments(x, 32, 8, y, 3, 312, 2, dev)
    feats = x.reshape(3, 24, 13, 32)[..., :8].permute(0, 3, 1, 2)
    with pytest.raises(ValueError, match='labels must lie in 0..1'):
        density.feature_moments(feats, y.reshape(3, 24, 13), 2)
    counts, S, G = density.feature_moments(feats, y.reshape(3, 24, 13), 3)
    _check_moments((counts.cpu().numpy(), S.cpu().numpy(), G.cpu().numpy()), phi, g32['labels3'], 3, 'wrapper F=8 K=3')


# ------------------------------------------------------------------------------------------------------------------- energy
def _fit(g32, F, K):
    from rcu_amd import density
    return density.fit_from_moments(*ref.moments(g32['phi_{}'.format(F)], _labels(g32, K), K), ridge=float(g32['ridge']))


def _energy(x, pitch, F, nvox, fit, dev, with_d2=True):
    from rcu_amd import _lib
    a, b, k = fit.device_parameters(dev)
    e = torch.full((nvox,), float('nan'), device=dev, dtype=torch.float32)
    d2 = torch.full((nvox, fit.K), float('nan'), device=dev, dtype=torch.float32) if with_d2 else None
    _lib.check(_lib.load().rcu_density_energy(ctypes.c_void_p(x.data_ptr()), pitch, F, nvox, fit.K, _lib.ptr(a), _lib.ptr(b), _lib.ptr(k), _lib.ptr(e),
                                              _lib.ptr(d2), _lib.current_stream()))
    return e.cpu().numpy(), None if d2 is None else d2.cpu().numpy()


def _check_energy(e, d2, fit, phi, tag):
    a32, b32, k32 = fit.float32_parameters()
    re, rd2 = ref.energy(a32, b32, k32, phi)
    bound = ref.energy_bounds(a32, b32, phi)
    tol = ref.energy_tolerance(bound, re)
    assert np.isfinite(e).all(), tag
    ee = np.abs(e - re)
    used_e = float((ee / tol).max())
    used_d = 0.0
    if d2 is not None:
        ed = np.abs(d2 - rd2)
        used_d = float((ed / bound).max())
        assert (ed <= bound).all(), (tag, used_d)
    print('energy {}: largest fraction of the bound used d2 {:.4f}, energy {:.4f}'.format(tag, used_d, used_e))
    assert (ee <= tol).all(), (tag, used_e)
    return used_d, used_e


def _probe_voxels(g32, F, nvox):
    """The fixture's voxels; a few pushed off the data (scaled, and off the dead channel's constant) so that large distances are met too."""
    phi = g32['phi_{}'.format(F)].reshape(-1, F)[:nvox].copy()
    phi[5::23] *= 3.0
    phi[7::31, int(g32['dead_channel'])] += 0.01
    return phi


@pytest.mark.parametrize('K', [1, 2, 3])
@pytest.mark.parametrize('F', [8, 32, 64])
@pytest.mark.parametrize('nvox', [279, 3 * 312])
def test_energy_against_the_reference(dev, g32, nvox, F, K):
    fit = _fit(g32, F, K)
    assert np.abs(fit.A).max() > 100.0, 'the dead channel was meant to make the fit ill-conditioned'
    phi = _probe_voxels(g32, F, nvox)
    x = torch.from_numpy(_at_pitch(phi, PITCH[F])).to(dev)
    e, d2 = _energy(x, PITCH[F], F, nvox, fit, dev)
    _check_energy(e, d2, fit, phi, 'nvox={} F={} K={}'.format(nvox, F, K))
    # the witness of the fixture (scipy, float64 fit) on the untouched voxels: the float32 parameters and arithmetic stay close to it
    key = {1: 'e1_{}', 2: 'e_{}', 3: 'e3_{}'}[K].format(F)
    plain = np.ones(nvox, bool)
    plain[5::23] = False
    plain[7::31] = False
    assert np.abs(e[plain] - g32[key].reshape(-1)[:nvox][plain]).max() < 0.05


@pytest.mark.parametrize('F, K', [(8, 2), (32, 3), (64, 2), (13, 2), (45, 3)])
def test_energy_of_a_voxel_does_not_depend_on_the_call(dev, g32, F, K):
    if F in (8, 32, 64):
        fit, phi, pitch = _fit(g32, F, K), _probe_voxels(g32, F, 936), PITCH[F]
    else:      # channel counts that are no multiple of 4: the last float4 of a voxel is cut
        from rcu_amd import density
        wide = g32['phi_64'][..., 4:4 + F]
        fit, phi, pitch = density.fit_from_moments(*ref.moments(wide, _labels(g32, K), K)), np.ascontiguousarray(wide.reshape(-1, F)), (F + 3) // 4 * 4
    small = phi[:279]
    alone, alone_d2 = _energy(torch.from_numpy(_at_pitch(small, pitch)).to(dev), pitch, F, 279, fit, dev)
    _check_energy(alone, alone_d2, fit, small, 'alone F={} K={}'.format(F, K))
    without, _ = _energy(torch.from_numpy(_at_pitch(small, pitch, seed=9)).to(dev), pitch, F, 279, fit, dev, with_d2=False)
    assert without.tobytes() == alone.tobytes()
    # the same 279 voxels as voxels 37 .. 315 of a larger call (37: no multiple of the 32 voxels a wave takes), and called at that offset
    big = torch.from_numpy(_at_pitch(np.concatenate([phi[300:337], small, phi[400:936]]), pitch, seed=5)).to(dev)
    whole, whole_d2 = _energy(big, pitch, F, big.shape[0], fit, dev)
    assert whole[37:37 + 279].tobytes() == alone.tobytes() and whole_d2[37:37 + 279].tobytes() == alone_d2.tobytes()
    sub, _ = _energy(big[37:], pitch, F, 279, fit, dev)
    assert sub.tobytes() == alone.tobytes()


@pytest.mark.parametrize('F', [8, 32, 64])
def test_energy_of_the_mean_is_minus_k(dev, g32, F):
    from rcu_amd import density
    for c in range(2):
        phi = g32['phi_{}'.format(F)].reshape(-1, F)[g32['labels2'].reshape(-1) == c]
        fit = density.fit_from_moments(*ref.moments(phi[None], np.zeros((1, phi.shape[0]), np.uint8), 1))
        mu = fit.mu.astype(np.float32)
        e, d2 = _energy(torch.from_numpy(_at_pitch(mu, PITCH[F])).to(dev), PITCH[F], F, 1, fit, dev)
        a32, b32, k32 = fit.float32_parameters()
        bound = ref.energy_bounds(a32, b32, mu)
        assert abs(float(e[0]) + float(k32[0])) <= float(ref.energy_tolerance(bound, -k32.astype(np.float64))[0]), (F, c, e, k32)
        assert 0.0 <= float(d2[0, 0]) <= float(bound[0, 0])


# ------------------------------------------------------------------------------------------------------------- step and fit
PARAMS = dict(nb_classes=2, in_channels=4, depth=2, start_filters=32, dropout=0.05)


def _unet(dev, seed=11, **over):
    from oracle import unet_oracle as uo
    from rcu_amd.model import UNet
    params = dict(PARAMS, **over)
    m = UNet(**params)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in uo.synthetic_state(seed, **params).items()})
    return m.to(dev).eval()


def _fit_bits(fit):
    return [getattr(fit, name).tobytes() for name in ('n', 'mu', 'cov', 'A', 'b', 'k')]


@pytest.mark.parametrize('shape', [(32, 32), (64, 32), (40, 24)])      # (40 x 24: level 0 is padded to whole tiles, the tap hands a compact copy out)
def test_fit_and_step_on_a_synthetic_unet(dev, shape):
    from rcu_amd import density, steps
    h, w = shape
    m = _unet(dev)
    g = torch.Generator().manual_seed(h + w)
    images = torch.randn(6, 4, h, w, generator=g).to(dev)
    target = (torch.rand(6, h, w, generator=g) < 0.35).to(torch.uint8).to(dev)
    fits = []
    for cuts in ((6,), (4, 2), (1, 5)):
        edges = np.cumsum((0,) + cuts)
        fits.append(density.fit_density(m, [(images[a:b], target[a:b]) for a, b in zip(edges[:-1], edges[1:])]))
        assert m.provide_features is False and not m.mc_active()
    assert _fit_bits(fits[0]) == _fit_bits(fits[1]) == _fit_bits(fits[2])
    fit = fits[0]
    assert (fit.F, fit.K, fit.voxels) == (32, 2, 6 * h * w) and int(fit.n.sum()) == 6 * h * w

    ctx = steps.TorchTestContext('cuda', m)
    bc = steps.BatchContext({'images': images.cpu().clone()}, 0, 0)
    steps.DensityPredictStep(fit)(bc, None, ctx)
    feats = m.features.cpu()           # the host round trip, before any other forward
    energy = bc.output['density']
    assert tuple(energy.shape) == (6, 1, h, w) and energy.dtype == torch.float32 and m.provide_features is False
    plain = steps.BatchContext({'images': images.cpu().clone()}, 0, 0)
    steps.SegmentationPredictStep(do_probs=True)(plain, None, ctx)
    for key in ('logits', 'probabilities'):
        assert bc.output[key].cpu().numpy().tobytes() == plain.output[key].cpu().numpy().tobytes(), key
    again, d2 = density.energy(fit, feats.to(dev), with_d2=True)
    assert again.cpu().numpy().tobytes() == energy.cpu().numpy().tobytes()
    phi = feats.permute(0, 2, 3, 1).reshape(-1, 32).numpy()
    _check_energy(energy.cpu().numpy().reshape(-1), d2.cpu().numpy().reshape(-1, 2), fit, phi, 'step {}x{}'.format(h, w))
    # the fit itself against the float64 reference on the same features (the moments are within their float32 bound: a loose check here)
    theirs = ref.fit(*ref.moments(phi.reshape(6, h * w, 32), target.cpu().numpy().reshape(6, h * w), 2))
    np.testing.assert_allclose(fit.mu, theirs['mu'], rtol=0, atol=1e-4 * np.abs(theirs['mu']).max())
    # refusals
    with pytest.raises(ValueError, match='F = 32'):
        steps.DensityPredictStep(fit)(steps.BatchContext({'images': images.cpu()}, 0, 0), None, steps.TorchTestContext('cuda', _unet(dev, start_filters=8)))
    with pytest.raises(ValueError, match='UNet'):
        steps.DensityPredictStep(fit)(steps.BatchContext({'images': images.cpu()}, 0, 0), None, steps.TorchTestContext('cuda', torch.nn.Conv2d(4, 2, 1)))


# ------------------------------------------------------------------------------------------------------------------ scripts
def _nii(ctx):
    return {os.path.basename(f): open(f, 'rb').read() for f in sorted(glob.glob(os.path.join(ctx.test_dir, '*.nii.gz')))}


def test_fit_script_then_the_default_script_with_and_without_the_key(tmp_path):
    import test_gpu_scripts as tgs
    from rcu_amd import density, nifti, scripts, steps
    cfg, vols, states, params = tgs._setup(tmp_path)
    fit = scripts.fit_density('brats', tgs._with_others(cfg, 'fit'))
    fit_dir = glob.glob(str(tmp_path / 'out_fit' / '*'))[0]
    npz = os.path.join(fit_dir, 'density.npz')
    doc = json.load(open(os.path.join(fit_dir, 'density.json')))
    assert (doc['F'], doc['K'], doc['ridge'], doc['test_at']) == (32, 2, 1e-6, 'best') and doc['model_dir'] and len(doc['counts']) == 2
    assert doc['voxels'] == sum(v[1].size for v in vols.values()) == sum(doc['counts'])
    assert doc['counts'][1] == sum(int((v[1] > 0).sum()) for v in vols.values())
    assert _fit_bits(density.load_density(npz)) == _fit_bits(fit)

    without = scripts.test_default('brats', tgs._with_others(cfg, 'plain'), None)
    with_key = scripts.test_default('brats', tgs._with_others(cfg, 'density', density=npz), None)
    a, b = _nii(without), _nii(with_key)
    assert len(a) == 2 * len(vols) and sorted(b) == sorted(list(a) + ['{}_density.nii.gz'.format(name) for name in vols])
    for name in a:
        assert a[name] == b[name], name
    assert open(os.path.join(without.test_dir, 'metrics.csv'), 'rb').read() == open(os.path.join(with_key.test_dir, 'metrics.csv'), 'rb').read()
    # the map holds the step's energies
    m = tgs_model(params, states[0])
    for name, (images, _, props) in vols.items():
        got, rprops = nifti.read(os.path.join(with_key.test_dir, name + '_density.nii.gz'))
        bc = steps.BatchContext({'images': torch.from_numpy(images).permute(0, 3, 1, 2).contiguous()}, 0, 0)
        steps.DensityPredictStep(fit)(bc, None, steps.TorchTestContext('cuda', m))
        assert got.dtype == np.float32 and rprops == props and got.tobytes() == bc.output['density'][:, 0].cpu().numpy().tobytes()

    # under dataset shift: the run completes and writes the map (no claim about its values)
    shifted = scripts.test_default('brats', tgs._with_others(cfg, 'shift', density=npz, corruption=[dict(kind='gaussian_noise', severity=5)]), None)
    c = _nii(shifted)
    assert sorted(c) == sorted(b) and all(np.isfinite(nifti.read(os.path.join(shifted.test_dir, n + '_density.nii.gz'))[0]).all() for n in vols)
    assert any(c[k] != b[k] for k in c if k.endswith('_density.nii.gz'))

    # the evaluation on the run as type `density`
    gt = tmp_path / 'gt' / 'HGG'
    for name, (images, labels, props) in vols.items():
        (gt / name).mkdir(parents=True)
        for mod, arr in (('flair', images[..., 0]), ('t1', images[..., 1]), ('t2', images[..., 2]), ('t1ce', images[..., 3]), ('seg', labels * 4)):
            nifti.write(str(gt / name / '{}_{}.nii.gz'.format(name, mod)), arr, props)
    scripts.eval_uncertainty('brats', {'density': with_key.test_dir}, str(tmp_path / 'gt'), str(tmp_path / 'eval'), actions=('minmax', 'ue_curves'),
                             expected_subjects=list(vols))
    written = glob.glob(str(tmp_path / 'eval' / '**' / '*.csv'), recursive=True)
    assert any('minmax' in f for f in written) and sum('density' in os.path.basename(f) for f in written) >= 2, written
    numbers = 0
    for f in written:
        for row in csv.reader(open(f)):
            for cell in row:
                try:
                    value = float(cell)
                except ValueError:
                    continue
                numbers += 1
                assert np.isfinite(value), (f, row)
    assert numbers > 20


def tgs_model(params, state):
    from rcu_amd.model import UNet
    m = UNet(**params)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    return m.to('cuda').eval()
