"""Nearest-neighbour feature uncertainty on the GPU (include/rcu_knn.h): rcu_knn_distances against exact integers and against the float64
reference within the bound of its float32 arithmetic, its bit-for-bit purity contracts (a voxel's distances are a function of that voxel and the
bank rows alone), the grid cap, the sampling keys against the numpy Philox, the fit's independence of batching, the predict step, and the scripts
end to end.

Largest fraction of the bound E = (2 F + 8) 2^-24 (|xhat| + |b|)^2 used on the MI355X (the tolerance test prints its own): 0.080, at F = 5
with normalisation (README, "Nearest-neighbour feature uncertainty")."""
import ctypes
import csv
import glob
import json
import os

import numpy as np
import pytest
import torch

import knn_reference as ref

pytestmark = pytest.mark.gpu
PITCH = {1: 4, 5: 8, 32: 32}
GRID_CAP_VOXELS = 2048 * 512      # KNN_GRID_CAP workgroups x 4 waves x KNN_GROUPS groups x 32 voxels (csrc/rcu_knn.hip)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda')


@pytest.fixture(scope='module')
def g37(golden):
    return golden('g37_knn')


def _at_pitch(phi, pitch, fill=None, seed=1):
    """[n, F] -> float32 [n, pitch] with finite garbage (or ``fill``) planted in the padding channels."""
    out = (np.random.default_rng(seed).standard_normal((phi.shape[0], pitch)) * 1.0e3).astype(np.float32)
    if fill is not None:
        out[:] = fill
    out[:, :phi.shape[1]] = phi
    return out


def _call(x, pitch, F, nvox, rows, sq, k, normalize, with_d2=True):
    """rcu_knn_distances on device tensors (any views: their data_ptr is what the kernel gets) -> numpy (score [nvox], d2 [nvox, k] or None)."""
    from rcu_amd import _lib
    lib = _lib.load()
    score = torch.full((nvox,), float('nan'), device=x.device, dtype=torch.float32)
    d2 = torch.full((nvox, k), float('nan'), device=x.device, dtype=torch.float32) if with_d2 else None
    _lib.check(lib.rcu_knn_distances(ctypes.c_void_p(x.data_ptr()), pitch, F, nvox, _lib.ptr(rows), _lib.ptr(sq), rows.shape[0], k, int(normalize),
                                     _lib.ptr(score), _lib.ptr(d2), _lib.current_stream()))
    return score.cpu().numpy(), None if d2 is None else d2.cpu().numpy()


def _run(phi, rows, sq, k, normalize, dev, pitch=None, fill=None, with_d2=True):
    pitch = PITCH.get(phi.shape[1], 32) if pitch is None else pitch
    x = torch.from_numpy(_at_pitch(phi, pitch, fill)).to(dev)
    return _call(x, pitch, phi.shape[1], phi.shape[0], torch.from_numpy(rows).to(dev), torch.from_numpy(sq).to(dev), k, normalize, with_d2)


def _check_score(score, d2):
    """score is sqrtf of the kernel's own d2_(k): within 2^-23 relative of the exact square root."""
    exact = np.sqrt(d2[:, -1].astype(np.float64))
    assert (np.abs(score.astype(np.float64) - exact) <= 2.0 ** -23 * exact).all()


# ------------------------------------------------------------------------------------------------------------------ exact case
@pytest.mark.parametrize('M', [1, 31, 32, 33, 100])
def test_integer_features_give_the_integer_distances_exactly(dev, M):
    """normalize = 0, features and bank integers in 0..15 at F = 32: every product and sum is exact in float32 (at most 2 x 32 x 225), so all k
    outputs equal the integer reference."""
    rng = np.random.default_rng(100 + M)
    bank = rng.integers(0, 16, (M, 32))
    rows, sq = bank.astype(np.float32), (bank * bank).sum(1).astype(np.float32)
    phi_all = rng.integers(0, 16, (12480, 32))
    phi_all[:M] = bank[rng.permutation(M)]      # (members of the bank: distance 0)
    for nvox in (1, 31, 33, 12480):
        phi = phi_all[:nvox]
        want = np.sort(((phi[:, None, :] - bank[None, :, :]) ** 2).sum(-1), axis=1)
        for k in (1, 2, 8):
            if k > M:
                continue
            score, d2 = _run(phi.astype(np.float32), rows, sq, k, 0, dev)
            assert np.array_equal(d2.astype(np.int64), want[:, :k]) and (d2 == np.floor(d2)).all(), (M, nvox, k)
            assert score.tobytes() == np.sqrt(d2[:, -1]).tobytes(), (M, nvox, k)      # (np.sqrt on float32 is correctly rounded)


# ------------------------------------------------------------------------------------------------------------------ tolerance
@pytest.mark.parametrize('normalize', [0, 1])
@pytest.mark.parametrize('F', [1, 5, 32])
def test_distances_within_the_bound_of_the_float32_arithmetic(dev, g37, F, normalize):
    """Continuous post-ReLU-like features with per-channel scales (fixture G37: zero vectors, bank rows planted equal to query voxels, duplicated
    bank rows).  For j = 1..k: |d2_dev,(j) - d2_ref,(j)| <= max_m E(v, m); no neighbour identity is asserted."""
    phi, bank = g37['phi_{}'.format(F)], g37['bank_{}'.format(F)]
    rows, sq = ref.bank_parameters(bank, normalize)
    assert rows.tobytes() == g37['rows_{}_{}'.format(F, normalize)].tobytes() and sq.tobytes() == g37['sq_{}_{}'.format(F, normalize)].tobytes()
    assert not phi[:2].any() and not bank[0].any() and np.array_equal(bank[1:6], phi[2:7]) and np.array_equal(bank[6], bank[8])
    k = 8
    score, d2 = _run(phi, rows, sq, k, normalize, dev)
    want, bound = ref.neighbours(phi, rows, k, normalize), ref.error_bound(phi, rows, normalize)
    err = np.abs(d2.astype(np.float64) - want)
    used = float((err / bound[:, None]).max())
    print('knn F = {} normalize = {}: largest fraction of the bound used {:.4f}'.format(F, normalize, used))
    assert np.isfinite(d2).all() and (d2 >= 0).all() and (np.diff(d2, axis=1) >= 0).all()
    assert (err <= bound[:, None]).all(), used
    _check_score(score, d2)
    # a planted row is at distance ~0 of its voxel; a zero voxel under normalize stays zero: its distance to the zero row is exactly 0
    assert (d2[2:7, 0] <= bound[2:7]).all()
    assert d2[0, 0] == 0.0 and d2[1, 0] == 0.0
    # a duplicated row counts as often as it is there: against the three equal rows alone every voxel sees one distance three times
    _, dup = _run(phi, rows[6:9], sq[6:9], 3, normalize, dev)
    assert np.array_equal(dup[:, 0], dup[:, 1]) and np.array_equal(dup[:, 0], dup[:, 2])
    # the witness of the fixture, through the reference
    assert (np.abs(want - g37['d2_{}_{}'.format(F, normalize)]) <= 1e-12 * np.maximum(1.0, want)).all()


# ------------------------------------------------------------------------------------------------------------------ purity
def test_purity_contracts_hold_bit_for_bit(dev, g37):
    rng = np.random.default_rng(5)
    for F, normalize, k in ((32, 1, 8), (5, 0, 3), (32, 0, 5), (1, 1, 2)):
        phi, bank = g37['phi_{}'.format(F)], g37['bank_{}'.format(F)]
        rows, sq = ref.bank_parameters(bank, normalize)
        score, d2 = _run(phi, rows, sq, k, normalize, dev)
        # permuting the voxels permutes the outputs
        p = rng.permutation(phi.shape[0])
        s2, d22 = _run(phi[p], rows, sq, k, normalize, dev)
        assert s2.tobytes() == score[p].tobytes() and d22.tobytes() == d2[p].tobytes(), (F, 'voxel permutation')
        # a voxel alone, and in a launch of another size
        s3, d23 = _run(phi[100:133], rows, sq, k, normalize, dev)
        assert s3.tobytes() == score[100:133].tobytes() and d23.tobytes() == d2[100:133].tobytes(), (F, 'launch size')
        # permuting the bank rows changes no bit
        q = rng.permutation(rows.shape[0])
        s4, d24 = _run(phi, rows[q], sq[q], k, normalize, dev)
        assert s4.tobytes() == score.tobytes() and d24.tobytes() == d2.tobytes(), (F, 'bank permutation')
        # a NULL d2_dev changes no other bit
        s5, none = _run(phi, rows, sq, k, normalize, dev, with_d2=False)
        assert none is None and s5.tobytes() == score.tobytes(), (F, 'NULL d2_dev')
        # another pitch, NaN in the padding channels
        s6, d26 = _run(phi, rows, sq, k, normalize, dev, pitch=64, fill=np.float32('nan'))
        assert s6.tobytes() == score.tobytes() and d26.tobytes() == d2.tobytes(), (F, 'pitch 64 with NaN padding')
        # a pointer one 16-byte unit off the allocation
        pitch = PITCH[F]
        buf = torch.full((4 + phi.shape[0] * pitch,), float('nan'), device=dev, dtype=torch.float32)
        buf[4:] = torch.from_numpy(_at_pitch(phi, pitch)).to(dev).reshape(-1)
        s7, d27 = _call(buf[4:], pitch, F, phi.shape[0], torch.from_numpy(rows).to(dev), torch.from_numpy(sq).to(dev), k, normalize)
        assert s7.tobytes() == score.tobytes() and d27.tobytes() == d2.tobytes(), (F, 'offset pointer')
        # other k: the same distances
        for other in (1, 8):
            _, d28 = _run(phi, rows, sq, other, normalize, dev)
            m = min(k, other)
            assert d28[:, :m].tobytes() == np.ascontiguousarray(d2[:, :m]).tobytes(), (F, 'k', other)


def test_rows_of_a_small_bank_inside_a_larger_one_with_far_extras(dev, g37):
    """M = 33 (one row in the second tile) against the same rows inside M = 100 -- other tiles, other positions -- with extras that are far away."""
    phi, bank = g37['phi_32'], g37['bank_32'][:33]
    rng = np.random.default_rng(9)
    extras = (g37['bank_32'][33:] + np.float32(1.0e3)).astype(np.float32)
    rows, sq = ref.bank_parameters(bank, 0)
    order = rng.permutation(33)
    big = np.concatenate([extras[:40], bank[order[:20]], extras[40:], bank[order[20:]]])
    big_rows, big_sq = ref.bank_parameters(big, 0)
    assert big_rows.shape[0] == 100
    for k in (1, 8):
        score, d2 = _run(phi, rows, sq, k, 0, dev)
        s2, d22 = _run(phi, big_rows, big_sq, k, 0, dev)
        assert float(d2.max()) < 1.0e5 < float(ref.squared_distances(phi, extras, 0).min())
        assert s2.tobytes() == score.tobytes() and d22.tobytes() == d2.tobytes(), k


def test_more_than_one_staged_piece_of_the_bank(dev):
    """M = 600 is three staged pieces of 256 rows, the last one ragged; the nearest rows are planted in the last piece and the last tile."""
    rng = np.random.default_rng(77)
    phi = np.maximum(rng.normal(0.3, 1.0, (700, 32)), 0.0).astype(np.float32)
    bank = np.maximum(rng.normal(0.3, 1.0, (600, 32)), 0.0).astype(np.float32)
    bank[590:600] = phi[:10]
    for normalize in (0, 1):
        rows, sq = ref.bank_parameters(bank, normalize)
        score, d2 = _run(phi, rows, sq, 5, normalize, dev)
        want, bound = ref.neighbours(phi, rows, 5, normalize), ref.error_bound(phi, rows, normalize)
        assert (np.abs(d2 - want) <= bound[:, None]).all() and (d2[:10, 0] <= bound[:10]).all()
        _check_score(score, d2)


# ------------------------------------------------------------------------------------------------------------------ grid cap
def test_voxels_beyond_the_grid_cap(dev):
    """The grid is capped at 2048 workgroups of 512 voxels: one shape just above it (a second trip for the first workgroups, a ragged last group),
    small M and F."""
    nvox = GRID_CAP_VOXELS + 512 + 37
    rng = np.random.default_rng(3)
    phi = rng.integers(0, 64, (nvox, 1)).astype(np.float32)
    bank = np.array([[3.0], [40.0], [41.0]], dtype=np.float32)
    rows, sq = ref.bank_parameters(bank, 0)
    score, d2 = _run(phi, rows, sq, 2, 0, dev)
    want = np.sort((phi.astype(np.int64) - bank.astype(np.int64).T) ** 2, axis=1)[:, :2]
    assert np.array_equal(d2.astype(np.int64), want)
    assert score.tobytes() == np.sqrt(d2[:, 1]).tobytes()


# ------------------------------------------------------------------------------------------------------------------ keys
def test_sample_keys_are_the_numpy_philox_integer_for_integer(dev, g37):
    from rcu_amd import knn
    assert knn.knn_seed(7) == ref.knn_seed(7) and knn.knn_seed(0) == 32 << 40
    for seed, index, hw in ((7, [0, 1, 154], 1061), (7, [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5], 40), (12345, [2 ** 40 + 9], 1), (3, [5, 2], 57600)):
        got = knn.sample_keys(len(index), hw, index, seed, device=dev)
        assert got.dtype == torch.int64 and tuple(got.shape) == (len(index), hw) and got.is_cuda
        want = ref.slice_keys(seed, index, hw)
        assert np.array_equal(got.cpu().numpy(), want) and int(got.min()) >= 0
    # the fixture's table: single probes, the pixel index up to 2^31 - 1 taken from a longer slice is not affordable here, so v is small
    for seed, g, v, key in zip(g37['key_seed'], g37['key_g'], g37['key_v'], g37['key63']):
        if int(v) < 60000:
            assert int(knn.sample_keys(1, int(v) + 1, [int(g)], int(seed), device=dev)[0, int(v)]) == int(key)
    with pytest.raises(ValueError, match='slice_index'):
        knn.sample_keys(2, 4, [1], 0, device=dev)


# ------------------------------------------------------------------------------------------------------------------ step and fit
PARAMS = dict(nb_classes=2, in_channels=4, depth=2, start_filters=32, dropout=0.05)


def _unet(dev, seed=11, **over):
    from oracle import unet_oracle as uo
    from rcu_amd.model import UNet
    params = dict(PARAMS, **over)
    m = UNet(**params)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in uo.synthetic_state(seed, **params).items()})
    return m.to(dev).eval()


def _bank_bits(bank):
    return [getattr(bank, name).tobytes() for name in ('features', 'labels', 'key63', 'g', 'v')] + [bank.normalize, bank.per_class, bank.seed]


def test_fit_does_not_depend_on_batching_and_the_step_keeps_the_default_bits(dev):
    from rcu_amd import knn, steps
    h, w = 40, 24      # (level 0 is padded to whole tiles: the tap hands a compact copy out)
    m = _unet(dev)
    g = torch.Generator().manual_seed(64)
    images = torch.randn(6, 4, h, w, generator=g).to(dev)
    target = (torch.rand(6, h, w, generator=g) < 0.35).to(torch.uint8).to(dev)
    ones = [(images[i:i + 1], target[i:i + 1], i) for i in range(6)]
    threes = [(images[0:3], target[0:3], 0), (images[3:6], target[3:6], 3)]
    banks = [knn.fit_knn(m, batches, 50, 9) for batches in (ones, ones[::-1], threes, threes[::-1], [(images, target)])]
    assert m.provide_features is False and not m.mc_active()
    for other in banks[1:]:
        assert _bank_bits(other) == _bank_bits(banks[0])
    bank = banks[0]
    assert (bank.F, bank.M, bank.counts(), bank.per_class, bank.seed, bank.normalize) == (32, 100, [50, 50], (50, 50), 9, True)
    # the rows are the reference's selection, and hold the tapped features of those voxels
    labels = target.cpu().numpy().reshape(6, h * w)
    want = ref.select_bank(labels, ref.slice_keys(9, range(6), h * w), (50, 50))
    for got, expected in zip((bank.labels, bank.key63, bank.g, bank.v), want):
        assert np.array_equal(got.astype(np.int64), expected)
    with knn.eval_features(m):
        m(images)
        feats = m.features.permute(0, 2, 3, 1).reshape(6, h * w, 32).cpu().numpy()
    assert bank.features.tobytes() == np.ascontiguousarray(feats[bank.g, bank.v]).tobytes()
    # a class with fewer voxels than asked for gives all of them; a class without a voxel is refused by name
    few = knn.fit_knn(m, [(images[:1], target[:1])], [10, 5000], 9)
    assert few.counts() == [10, int(target[:1].sum())]
    with pytest.raises(ValueError, match='class 1 has no voxel'):
        knn.fit_knn(m, [(images[:1], torch.zeros_like(target[:1]))], 10, 9)

    ctx = steps.TorchTestContext('cuda', m)
    bc = steps.BatchContext({'images': images.cpu().clone()}, 0, 0)
    steps.KnnPredictStep(bank, 5)(bc, None, ctx)
    tapped = m.features.cpu()           # the host round trip, before any other forward
    score = bc.output['knn']
    assert tuple(score.shape) == (6, 1, h, w) and score.dtype == torch.float32 and m.provide_features is False
    plain = steps.BatchContext({'images': images.cpu().clone()}, 0, 0)
    steps.SegmentationPredictStep(do_probs=True)(plain, None, ctx)
    for key in ('logits', 'probabilities'):
        assert bc.output[key].cpu().numpy().tobytes() == plain.output[key].cpu().numpy().tobytes(), key
    again, d2 = knn.distances(bank, tapped.to(dev), 5, with_neighbours=True)
    assert again.cpu().numpy().tobytes() == score.cpu().numpy().tobytes() and tuple(d2.shape) == (6, h, w, 5)
    phi = tapped.permute(0, 2, 3, 1).reshape(-1, 32).numpy()
    rows, sq = bank.float32_parameters()
    assert rows.tobytes() == ref.bank_parameters(bank.features, True)[0].tobytes() and sq.tobytes() == ref.bank_parameters(bank.features, True)[1].tobytes()
    want, bound = ref.neighbours(phi, rows, 5, True), ref.error_bound(phi, rows, True)
    got = d2.cpu().numpy().reshape(-1, 5)
    assert (np.abs(got - want) <= bound[:, None]).all()
    _check_score(score.cpu().numpy().reshape(-1), got)
    # the bank's own voxels are at distance ~0 of a row
    flat = got.reshape(6, h * w, 5)
    assert (flat[bank.g, bank.v, 0] <= bound.reshape(6, h * w)[bank.g, bank.v]).all()
    # refusals
    with pytest.raises(ValueError, match='F = 32'):
        steps.KnnPredictStep(bank, 5)(steps.BatchContext({'images': images.cpu()}, 0, 0), None, steps.TorchTestContext('cuda', _unet(dev, start_filters=8)))
    with pytest.raises(ValueError, match='UNet'):
        steps.KnnPredictStep(bank, 5)(steps.BatchContext({'images': images.cpu()}, 0, 0), None, steps.TorchTestContext('cuda', torch.nn.Conv2d(4, 2, 1)))
    with pytest.raises(ValueError, match='k must be an integer in 1..8'):
        steps.KnnPredictStep(bank, 9)


# ------------------------------------------------------------------------------------------------------------------ scripts
def _nii(ctx):
    return {os.path.basename(f): open(f, 'rb').read() for f in sorted(glob.glob(os.path.join(ctx.test_dir, '*.nii.gz')))}


def test_fit_script_then_the_default_script_with_and_without_the_key(tmp_path):
    import test_gpu_scripts as tgs
    from test_gpu_density import tgs_model
    from rcu_amd import knn, nifti, scripts, steps
    cfg, vols, states, params = tgs._setup(tmp_path)
    bank = scripts.fit_knn('brats', tgs._with_others(cfg, 'fit', knn_bank=dict(per_class=64)))
    fit_dir = glob.glob(str(tmp_path / 'out_fit' / '*'))[0]
    npz = os.path.join(fit_dir, 'knn.npz')
    doc = json.load(open(os.path.join(fit_dir, 'knn.json')))
    assert (doc['F'], doc['per_class'], doc['normalize'], doc['test_at']) == (32, [64, 64], True, 'best') and doc['model_dir']
    assert doc['counts'][0] == 64 and 1 <= doc['counts'][1] <= 64 and doc['M'] == sum(doc['counts']) == bank.M
    assert _bank_bits(knn.load_knn(npz)) == _bank_bits(bank)
    slices = sum(v[1].shape[0] for v in vols.values())
    assert 0 <= int(bank.g.min()) and int(bank.g.max()) < slices

    without = scripts.test_default('brats', tgs._with_others(cfg, 'plain'), None)
    with_key = scripts.test_default('brats', tgs._with_others(cfg, 'knn', knn=npz, knn_k=3), None)
    a, b = _nii(without), _nii(with_key)
    assert len(a) == 2 * len(vols) and sorted(b) == sorted(list(a) + ['{}_knn.nii.gz'.format(name) for name in vols])
    for name in a:
        assert a[name] == b[name], name
    assert open(os.path.join(without.test_dir, 'metrics.csv'), 'rb').read() == open(os.path.join(with_key.test_dir, 'metrics.csv'), 'rb').read()
    record = json.load(open(os.path.join(with_key.test_dir, 'knn.json')))
    assert (record['k'], record['M'], record['file']) == (3, bank.M, npz) and not os.path.exists(os.path.join(without.test_dir, 'knn.json'))
    # the map holds the step's distances
    m = tgs_model(params, states[0])
    for name, (images, _, props) in vols.items():
        got, rprops = nifti.read(os.path.join(with_key.test_dir, name + '_knn.nii.gz'))
        bc = steps.BatchContext({'images': torch.from_numpy(images).permute(0, 3, 1, 2).contiguous()}, 0, 0)
        steps.KnnPredictStep(bank, 3)(bc, None, steps.TorchTestContext('cuda', m))
        assert got.dtype == np.float32 and rprops == props and got.tobytes() == bc.output['knn'][:, 0].cpu().numpy().tobytes()
        assert np.isfinite(got).all() and (got >= 0).all()

    # under dataset shift and with a temperature: the run completes and writes the map (no claim about its values)
    shifted = scripts.test_default('brats', tgs._with_others(cfg, 'shift', knn=npz, temperature=1.5,
                                                             corruption=[dict(kind='gaussian_noise', severity=5)]), None)
    c = _nii(shifted)
    assert sorted(c) == sorted(b) and all(np.isfinite(nifti.read(os.path.join(shifted.test_dir, n + '_knn.nii.gz'))[0]).all() for n in vols)
    assert any(c[k] != b[k] for k in c if k.endswith('_knn.nii.gz'))

    # the evaluation on the run as type `knn`
    gt = tmp_path / 'gt' / 'HGG'
    for name, (images, labels, props) in vols.items():
        (gt / name).mkdir(parents=True)
        for mod, arr in (('flair', images[..., 0]), ('t1', images[..., 1]), ('t2', images[..., 2]), ('t1ce', images[..., 3]), ('seg', labels * 4)):
            nifti.write(str(gt / name / '{}_{}.nii.gz'.format(name, mod)), arr, props)
    scripts.eval_uncertainty('brats', {'knn': with_key.test_dir}, str(tmp_path / 'gt'), str(tmp_path / 'eval'), actions=('minmax', 'ue_curves'),
                             expected_subjects=list(vols))
    written = glob.glob(str(tmp_path / 'eval' / '**' / '*.csv'), recursive=True)
    assert any('minmax' in f for f in written) and sum('knn' in os.path.basename(f) for f in written) >= 2, written
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
