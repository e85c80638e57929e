"""The squared distance transform, the border shell, the boundary table and the surface distances on the GPU: on the fixture volumes against
the reference's and scipy's arrays (fixture G24), on shapes that stress the three passes, across slab widths, on a native-size volume;
`SubjectBatch.metrics(want=('boundary',))`, the 'boundary' action end to end and the border entries of `Loader.get_data`.  Every
comparison is integer or byte equality unless a tolerance is stated."""
import math
import os

import numpy as np
import pytest
import torch

from test_boundary_cpu import (CASES, NONE, ONE, TOL, as_cells, brute_force_edt_sq, golden, histogram_of, numpy_boundary_table, numpy_surface,
                               quantise, separable_edt_sq)
from test_gpu_ue_curves import _all_csv, _rows, _tree

pytestmark = pytest.mark.gpu
SLAB_WIDTHS = (0, 1, 2, 4, 8, 16, 32, 64)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture()
def set_slab_width():
    from rcu_amd import _lib
    lib = _lib.load()

    def setter(width):
        _lib.check(lib.rcu_edt_set_slab_width(width))
    yield setter
    lib.rcu_edt_set_slab_width(0)


def same_histogram(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3


def numpy_surface_histogram(prediction, target):
    sp, st = numpy_surface(prediction), numpy_surface(target)
    return histogram_of(separable_edt_sq(st)[sp].astype(np.int64), separable_edt_sq(sp)[st].astype(np.int64))


# --------------------------------------------------------------------------------------------------------------- 1. the fixture
def check_fixture_volume(ev, g, name, edt_in, edt_out, border11, border23, hist, table3, table10):
    assert edt_in.dtype == np.uint32 and np.array_equal(edt_in, g[name + '_edt_sq_in']), name
    assert np.array_equal(edt_out, g[name + '_edt_sq_out']), name
    for (distance, mask), tag in ((border11, '11'), (border23, '23')):
        assert distance.dtype == np.float64 and mask.dtype == bool and distance.shape == mask.shape == g[name + '_target'].shape
        assert distance.tobytes() == g[name + '_dist' + tag].tobytes(), (name, tag)          # the reference's float64 distance, bit for bit
        assert np.array_equal(mask, g[name + '_mask' + tag]), (name, tag)
    assert same_histogram(hist, histogram_of(g[name + '_sq_p_to_t'], g[name + '_sq_t_to_p'])), name
    m = ev.surface_distance_metrics(hist)
    for key in ('hd', 'hd95', 'assd'):
        assert abs(m[key] - float(g[name + '_' + key])) <= TOL, (name, key)
    assert np.array_equal(as_cells(table3), g[name + '_table_r3']) and np.array_equal(as_cells(table10), g[name + '_table_r10']), name


def test_fixture_volumes_one_by_one(dev):
    from rcu_amd import evaluation as ev
    g = golden()
    for name in CASES:
        pr, tg, unc = g[name + '_prediction'], g[name + '_target'], g[name + '_uncertainty']
        check_fixture_volume(ev, g, name, ev.distance_transform_sq(tg), ev.distance_transform_sq(tg, invert=True), ev.boarder_mask(tg, 1, 1),
                             ev.boarder_mask(tg, 2, 3), ev.surface_distance_histograms(pr, tg)[0], ev.boundary_table(pr, tg, unc, bands=3)[0],
                             ev.boundary_table(pr, tg, unc, bands=10)[0])
    # device tensors in, device tensors out
    tg = torch.from_numpy(g['box_target']).to(dev)
    d = ev.distance_transform_sq(tg)
    assert d.is_cuda and np.array_equal(d.cpu().numpy().view(np.uint32), g['box_edt_sq_in'])
    distance, mask = ev.boarder_mask(tg, 1, 1)
    assert distance.is_cuda and mask.dtype == torch.bool and distance.cpu().numpy().tobytes() == g['box_dist11'].tobytes()


def test_fixture_volumes_as_one_batch(dev):
    """Volumes of one shape go through every kernel as one batch: the box case, its prediction as a second target, and both flipped."""
    from rcu_amd import evaluation as ev
    g = golden()
    pr, tg, unc = g['box_prediction'], g['box_target'], g['box_uncertainty']
    targets = np.stack([tg, pr, tg[::-1].copy(), pr[:, ::-1].copy()])
    predictions = np.stack([pr, tg, pr[::-1].copy(), tg[:, ::-1].copy()])
    uncs = np.stack([unc, unc, unc[::-1].copy(), unc[:, ::-1].copy()])
    edt_in, edt_out = ev.distance_transform_sq(targets, n_volumes=4), ev.distance_transform_sq(targets, n_volumes=4, invert=True)
    hists = ev.surface_distance_histograms(predictions, targets, n_volumes=4)
    tables3, tables10 = ev.boundary_table(predictions, targets, uncs, bands=3, n_volumes=4), ev.boundary_table(predictions, targets, uncs, bands=10, n_volumes=4)
    assert tables3.shape == (4, 2, 4) and tables10.shape == (4, 2, 11)
    check_fixture_volume(ev, g, 'box', edt_in[0], edt_out[0], ev.boarder_mask(tg, 1, 1), ev.boarder_mask(tg, 2, 3), hists[0], tables3[0], tables10[0])
    for v in range(4):       # the batch is the volumes one by one
        assert np.array_equal(edt_in[v], ev.distance_transform_sq(targets[v])) and np.array_equal(edt_out[v], ev.distance_transform_sq(targets[v], invert=True))
        assert same_histogram(hists[v], ev.surface_distance_histograms(predictions[v], targets[v])[0])
        assert tables10[v].tobytes() == ev.boundary_table(predictions[v], targets[v], uncs[v], bands=10)[0].tobytes()
    # a flipped volume has the flipped transform, and the same multisets and cells
    assert np.array_equal(edt_in[2], edt_in[0][::-1]) and same_histogram(hists[2], hists[0]) and tables3[2].tobytes() == tables3[0].tobytes()
    assert same_histogram(hists[1], (hists[0][0], hists[0][2], hists[0][1]))       # prediction and target swapped: the directions swap


# ------------------------------------------------------------------------------------------- 2. shapes that stress the passes
SHAPES = ((1, 1, 1), (1, 1, 300), (300, 1, 2), (2, 300, 3), (5, 7, 9), (3, 70, 130), (33, 65, 17), (1, 16, 64), (4, 64, 64))


def stress_features(shape, rng):
    """name -> feature set (bool)."""
    n = int(np.prod(shape))
    corner = np.zeros(shape, dtype=bool)
    corner[-1, -1, -1] = True
    hole = np.ones(shape, dtype=bool)
    hole.reshape(-1)[n // 3] = False
    return {'half': rng.rand(*shape) < 0.5, 'sparse': rng.rand(*shape) < 0.001, 'corner': corner, 'hole': hole,
            'all': np.ones(shape, dtype=bool), 'none': np.zeros(shape, dtype=bool)}


@pytest.mark.parametrize('shape', SHAPES)
def test_shapes_that_stress_the_passes(dev, shape):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(sum(shape))
    for name, feature in stress_features(shape, rng).items():
        expect = separable_edt_sq(feature)
        if feature.size <= 700:
            assert np.array_equal(expect, brute_force_edt_sq(feature)), (shape, name)
        if name == 'all':
            assert not expect.any()
        if name == 'none' or not feature.any():
            assert np.all(expect == NONE)
        if name == 'corner':       # the largest distances there are: every extent's square
            assert int(expect.reshape(-1)[0]) == sum((e - 1) ** 2 for e in shape)
        # the features are the zeros of the mask ... or, inverted, its non-zeros (values other than 1 too)
        got = ev.distance_transform_sq((~feature).astype(np.uint8) * 7)
        assert got.dtype == np.uint32 and got.shape == shape and np.array_equal(got, expect), (shape, name)
        assert np.array_equal(ev.distance_transform_sq(feature.astype(np.uint8) * 3, invert=True), expect), (shape, name, 'invert')


# --------------------------------------------------------------------------------------------------------------- 3. a batch
def test_volumes_of_a_batch_never_see_each_other(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(8)
    shape = (4, 9, 70)
    features = np.zeros((3,) + shape, dtype=bool)
    features[1, 2, 4, 33] = True
    features[2] = rng.rand(*shape) < 0.3
    features[2, -1] = True                    # a whole slice of features right behind volume 1 ...
    features[2, 0] = True                     # ... and none of it may be seen from volume 1 (or 0)
    got = ev.distance_transform_sq((~features).astype(np.uint8), n_volumes=3)
    assert np.all(got[0] == NONE)
    z, y, x = np.indices(shape)
    assert np.array_equal(got[1].astype(np.int64), (z - 2) ** 2 + (y - 4) ** 2 + (x - 33) ** 2)
    assert np.array_equal(got[2], separable_edt_sq(features[2]))
    # the border shell and the table of a one-class volume: NONE is +inf
    distance, mask = ev.boarder_mask(np.zeros(shape, dtype=np.uint8), 1, 1)
    assert np.all(np.isinf(distance)) and not mask.any()


# --------------------------------------------------------------------------------------------------------- 4. launch geometry
def test_distances_do_not_depend_on_the_slab_width(dev, set_slab_width):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(4)
    shape = (3, 70, 130)
    masks = np.stack([rng.rand(*shape) < 0.5, rng.rand(*shape) < 0.999, rng.rand(*shape) < 0.01]).astype(np.uint8)
    reference = None
    for width in SLAB_WIDTHS:
        set_slab_width(width)
        got = ev.distance_transform_sq(masks, n_volumes=3).tobytes() + ev.distance_transform_sq(masks, n_volumes=3, invert=True).tobytes()
        if reference is None:
            reference = got
            assert np.array_equal(ev.distance_transform_sq(masks[1]), separable_edt_sq(masks[1] == 0))
        assert got == reference, width


# ------------------------------------------------------------------------------------------------------ 5. the boundary table
def table_case(rng, shape=(5, 40, 48)):
    z, y, x = np.indices(shape)
    target = (((z - 2) ** 2 * 9 + (y - 18) ** 2 + (x - 20) ** 2 <= 150) | (rng.rand(*shape) < 0.003)).astype(np.uint8) * 2
    prediction = (np.roll(target, 2, axis=2) != 0) ^ (rng.rand(*shape) < 0.02)
    return prediction.astype(np.uint8), target


def test_map_forms_equal_the_numpy_quantisation(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(51)
    prediction, target = table_case(rng)
    unc = rng.rand(*target.shape)
    flat = unc.reshape(-1)
    flat[:64] = (np.arange(64) + 0.5) / ONE                          # exact ties
    flat[64:72] = [0.0, -0.0, 1.0, 1.5, -2.0, np.nan, np.inf, -np.inf]        # NaN and values out of range
    flat[100:200] = np.round(flat[100:200], 3)
    for dtype in (np.float64, np.float32):
        u = unc.astype(dtype)
        for bands in (1, 3, 64):
            got = ev.boundary_table(prediction, target, u, bands=bands)
            assert got.shape == (1, 2, bands + 1)
            assert np.array_equal(as_cells(got[0]), numpy_boundary_table(prediction, target, quantise(u), bands)), (dtype, bands)
            again = ev.boundary_table(torch.from_numpy(prediction).to(dev), torch.from_numpy(target).to(dev), torch.from_numpy(u).to(dev), bands=bands)
            assert again.tobytes() == got.tobytes()
    # without an uncertainty the sums stay 0, the counts are the same
    plain = as_cells(ev.boundary_table(prediction, target, bands=3)[0])
    full = numpy_boundary_table(prediction, target, None, 3)
    assert np.array_equal(plain, full) and not plain[..., 2:].any() and plain[..., 1].sum() == int(((prediction != 0) != (target != 0)).sum())
    with pytest.raises(ValueError):
        ev.boundary_table(prediction, target, bands=65)


def test_probability_form_equals_the_map_form_on_the_device_entropy(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(53)
    prediction, target = table_case(rng)
    p = rng.rand(*target.shape).astype(np.float32)
    special = np.array([0.0, 1.0, 0.5, 1e-7, 0.999999, np.float32(1e-45), np.nextafter(np.float32(0.5), np.float32(0))], dtype=np.float32)
    p.reshape(-1)[:special.size] = special
    p.reshape(-1)[special.size:3000] = (rng.rand(3000 - special.size) * 1e-4).astype(np.float32)      # peaked
    entropy = ev.normalised_entropy(p)                                # device float64 map: rcu_normalised_entropy's output
    for bands in (1, 3, 64):
        direct = ev.boundary_table(prediction, target, foreground_probability=p, bands=bands)
        assert direct.tobytes() == ev.boundary_table(prediction, target, entropy, bands=bands).tobytes()
        assert direct.tobytes() == ev.boundary_table(prediction, target, ev.EntropyOfProbability(p), bands=bands).tobytes()
        assert np.array_equal(as_cells(direct[0]), numpy_boundary_table(prediction, target, quantise(entropy.cpu().numpy()), bands))


def test_a_target_without_foreground_lands_in_the_last_band(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(55)
    shape = (5, 40, 48)
    prediction, unc = (rng.rand(*shape) < 0.1).astype(np.uint8), rng.rand(*shape)
    for bands in (1, 64):
        cells = as_cells(ev.boundary_table(prediction, np.zeros(shape, dtype=np.uint8), unc, bands=bands)[0])
        q = quantise(unc)
        assert list(cells[0, bands]) == [prediction.size, int(prediction.sum()), int(q.sum()), int(q[prediction != 0].sum())]
        cells[0, bands] = 0
        assert not cells.any()


# ------------------------------------------------------------------------------------------------------ 6. surface distances
def test_surface_distances_by_hand(dev):
    from rcu_amd import evaluation as ev
    shape = (6, 8, 20)
    rng = np.random.RandomState(61)
    blob = np.zeros(shape, dtype=np.uint8)
    blob[1:5, 2:7, 3:15] = 1
    empty = np.zeros(shape, dtype=np.uint8)
    hist = ev.surface_distance_histograms(empty, blob)[0]
    m = ev.surface_distance_metrics(hist)
    assert math.isnan(m['hd']) and math.isnan(m['hd95']) and math.isnan(m['assd'])
    assert (m['n_surface_prediction'], m['n_surface_target']) == (0, int(numpy_surface(blob).sum())) and list(hist[0]) == [NONE]
    m = ev.surface_distance_metrics(ev.surface_distance_histograms(blob, blob)[0])
    assert (m['hd'], m['hd95'], m['assd']) == (0.0, 0.0, 0.0) and m['n_surface_prediction'] == m['n_surface_target'] > 0
    a, b = np.zeros((13, 5, 4), dtype=np.uint8), np.zeros((13, 5, 4), dtype=np.uint8)
    a[0, 0, 0], b[12, 4, 3] = 1, 1                                     # 3-4-12 apart
    hist = ev.surface_distance_histograms(a, b)[0]
    assert list(hist[0]) == [169] and list(hist[1]) == [1] and list(hist[2]) == [1]
    m = ev.surface_distance_metrics(hist)
    assert (m['hd'], m['hd95'], m['assd']) == (13.0, 13.0, 13.0)
    # random maps, odd shape, a batch with an empty member: the multisets of the numpy restatement
    shape = (3, 17, 67)
    predictions = np.stack([rng.rand(*shape) < 0.4, np.zeros(shape, dtype=bool), rng.rand(*shape) < 0.9]).astype(np.uint8)
    targets = np.stack([rng.rand(*shape) < 0.05, rng.rand(*shape) < 0.5, rng.rand(*shape) < 0.7]).astype(np.uint8)
    hists = ev.surface_distance_histograms(predictions, targets, n_volumes=3)
    for v in (0, 2):
        assert same_histogram(hists[v], numpy_surface_histogram(predictions[v], targets[v])), v
        m = ev.surface_distance_metrics(hists[v])
        both = np.sqrt(np.concatenate([np.repeat(hists[v][0], hists[v][1]), np.repeat(hists[v][0], hists[v][2])]).astype(np.float64))
        assert m['hd'] == both.max() and m['hd95'] == float(np.percentile(both, 95)) and abs(m['assd'] - both.mean()) <= TOL
    assert list(hists[1][0]) == [NONE] and int(hists[1][1].sum()) == 0 and int(hists[1][2].sum()) == int(numpy_surface(targets[1]).sum())


# ------------------------------------------------------------------------------------------------------------ 7. native size
def test_native_size_volume_equals_scipy(dev):
    from scipy import ndimage
    from rcu_amd import evaluation as ev
    shape = (155, 240, 240)
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    rng = np.random.RandomState(105)
    mask = ((((z - 85) / 28.0) ** 2 + ((y - 85) / 40.0) ** 2 + ((x - 128) / 38.0) ** 2 <= 1.0) | (rng.rand(*shape) < 0.002)).astype(np.uint8)
    expect = np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.uint32)      # the only scipy call at this size
    m_dev = torch.from_numpy(mask).to(dev)
    got = ev.distance_transform_sq(m_dev).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, expect) and int(expect.max()) > 20 ** 2
    # the other transform has no scipy call: the blob's far corner by hand, and the features are zeros
    out = ev.distance_transform_sq(m_dev, invert=True).cpu().numpy().view(np.uint32)
    assert not out[mask != 0].any() and out[mask == 0].all() and not np.any(out == NONE)
    where = np.argwhere(mask != 0).astype(np.int64)
    for corner in ((0, 0, 0), (154, 239, 239), (154, 0, 239)):
        assert int(out[corner]) == int(((where - np.array(corner)) ** 2).sum(1).min())


# ------------------------------------------------------------------------------------------------------- 8. SubjectBatch
def test_subject_batch_metrics_with_boundary(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(3)
    batch = ev.SubjectBatch(4, 12 * 20)
    subjects = []
    for slot, shape in enumerate(((12, 20), (20, 12), (12, 20), (2, 6, 20))):       # one size, three shapes
        p = rng.rand(*shape).astype(np.float32)
        pr, tg = (p > 0.6).astype(np.uint8), (rng.rand(*shape) < 0.3).astype(np.uint8)
        batch.put(slot, p, pr, tg)
        subjects.append((p, pr, tg))
    batch.upload()
    plain = batch.metrics(want=('minmax', 'ue', 'ue_hist'), levels=16)
    more = batch.metrics(want=('minmax', 'ue', 'ue_hist', 'boundary'), levels=16, bands=4)
    assert set(more) == set(plain) | {'boundary'} and len(more['boundary']) == 4
    for key in ('min', 'max', 'counts', 'ue_hist'):
        assert plain[key].dtype == more[key].dtype and plain[key].tobytes() == more[key].tobytes(), key
    for slot, (p, pr, tg) in enumerate(subjects):
        table, surface, off_border = more['boundary'][slot]
        assert table.tobytes() == ev.boundary_table(pr, tg, foreground_probability=p, bands=4)[0].tobytes()
        assert np.array_equal(as_cells(table), numpy_boundary_table(pr, tg, quantise(ev.normalised_entropy(p).cpu().numpy()), 4))
        assert same_histogram(surface, ev.surface_distance_histograms(pr, tg)[0]) and same_histogram(surface, numpy_surface_histogram(pr, tg))
        _, shell = ev.boarder_mask(tg, 1, 1)
        expect = ev.uncertainty_histogram_from_p(pr, tg, p, 16, mask=~shell)[0]
        assert off_border.dtype == expect.dtype and off_border.tobytes() == expect.tobytes()
        assert int(off_border.sum()) == int((~shell).sum()) == tg.size - int(as_cells(table)[:, 0, 0].sum())
    with pytest.raises(ValueError):
        batch.metrics(want=('boundary',), bands=0)


def test_subject_batch_all_scans_in_one_call_over_two_shapes(dev):
    """Every scan of ``metrics`` in ONE call on a batch of two shapes, the odd shape in the middle slot (the gathered copy of the per-shape
    grouping): each entry is what the public one-volume function returns for that subject in its own shape, integer for integer, and
    the floats (min / max, the reliability histogram's confidence sums) bit for bit.  4320 voxels per subject: more than one labelling
    tile (4 x 8 x 32) along every axis, more than one line per slab of the distance transform."""
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(11)
    shapes = ((6, 20, 36), (6, 36, 20), (6, 20, 36))
    batch = ev.SubjectBatch(3, 6 * 20 * 36)
    subjects = []
    for slot, shape in enumerate(shapes):
        p = rng.rand(*shape).astype(np.float32)
        pr = (p > 0.5).astype(np.uint8)
        blob = np.zeros(shape, dtype=np.uint8)
        blob[1:5, shape[1] // 4:shape[1] // 4 * 3, shape[2] // 4:shape[2] // 4 * 3] = 1
        tg = np.roll(blob, (slot % 2, 2 + slot, -3), axis=(0, 1, 2))       # a shifted blob: both classes, and errors of both kinds
        assert 0 < int(tg.sum()) < tg.size and ((pr != tg) & (tg != 0)).any() and ((pr != tg) & (tg == 0)).any()
        batch.put(slot, p, pr, tg)
        subjects.append((p, pr, tg))
    batch.upload()
    res = batch.metrics(want=('minmax', 'ece', 'ue', 'ue_hist', 'components', 'boundary'), levels=1000, bands=3, connectivity=26)
    assert set(res) == {'min', 'max', 'hist', 'counts', 'ue_hist', 'components', 'boundary'}
    for slot, (p, pr, tg) in enumerate(subjects):
        assert res['min'][slot].tobytes() == p.min().tobytes() and res['max'][slot].tobytes() == p.max().tobytes(), slot
        count, sum_conf, sum_pos = ev.calibration_histogram(p, tg, 10)
        print(slot, 'sum_conf', [v.hex() for v in res['hist'][1][slot]], [v.hex() for v in sum_conf[0]])
        assert np.array_equal(res['hist'][0][slot], count[0]) and np.array_equal(res['hist'][2][slot], sum_pos[0]), slot
        assert res['hist'][1][slot].dtype == np.float64 and res['hist'][1][slot].tobytes() == sum_conf[0].tobytes(), slot
        assert int(count.sum()) == tg.size
        assert np.array_equal(res['counts'][slot], ev.uncertainty_counts_from_p(pr, tg, p)[0]), slot
        expect = ev.uncertainty_histogram_from_p(pr, tg, p, 1000)[0]
        assert res['ue_hist'][slot].dtype == expect.dtype and np.array_equal(res['ue_hist'][slot], expect), slot
        of_prediction, of_target = res['components'][slot]
        assert of_prediction.tobytes() == ev.component_table(pr, tg, ev.EntropyOfProbability(p), 26)[0].tobytes() and len(of_prediction) >= 1, slot
        assert of_target.tobytes() == ev.component_table(tg, pr, None, 26)[0].tobytes() and len(of_target) >= 1, slot
        table, surface, off_border = res['boundary'][slot]
        assert table.tobytes() == ev.boundary_table(pr, tg, foreground_probability=p, bands=3)[0].tobytes(), slot
        assert same_histogram(surface, ev.surface_distance_histograms(pr, tg)[0]), slot
        expect = ev.uncertainty_histogram_from_p(pr, tg, p, 1000, mask=~ev.boarder_mask(tg, 1, 1)[1])[0]
        assert off_border.dtype == expect.dtype and np.array_equal(off_border, expect) and 0 < int(off_border.sum()) < tg.size, slot


# ----------------------------------------------------------------------------------------------------------- 9. end to end
def test_boundary_action_end_to_end(dev, tmp_path):
    from rcu_amd import evalrun, evaluation as ev
    rng = np.random.RandomState(5)
    subjects = ['Brats18_{}_1'.format(c) for c in 'ABCDEFGHI']
    gt_dir, run_dir, truth = _tree(tmp_path, subjects, 'probabilities', rng)
    gts = evalrun.collect_brats_ground_truth(gt_dir)
    entry = evalrun.get_eval_data('baseline_mc', run_dir, gts, expected_subjects=subjects)
    old = ['minmax', 'ece_dice', 'calib', 'bnf_ue', 'ue_curves', 'components']
    base = str(tmp_path / 'eval')
    evalrun.evaluate_runs([entry], old + ['boundary'], base, 'foreground', bands=3, levels=50)
    fused = _all_csv(base)
    mine = {k: v for k, v in fused.items() if os.path.basename(k).startswith('eval_boundary')}
    assert sorted(os.path.basename(k) for k in mine) == ['eval_boundary_bands_baseline_mc.csv', 'eval_boundary_baseline_mc.csv',
                                                         'eval_boundary_pooled_baseline_mc.csv']
    assert all(os.path.dirname(k) == evalrun.UNCERTAINTY_NAME for k in mine) and len(fused) == 14 + 3 + 3 + 3
    # the plain loop writes the same bytes; batches of 1 and 8 the same pooled and bands files (and the same rows)
    for tag, kwargs in (('plain', dict(fused=False)), ('b1', dict(batch_subjects=1)), ('b8', dict(batch_subjects=8))):
        other = str(tmp_path / ('eval_' + tag))
        evalrun.evaluate_runs([entry], old + ['boundary'], other, 'foreground', bands=3, levels=50, **kwargs)
        assert _all_csv(other) == fused, tag
    # the other actions' files do not feel the new one
    without = str(tmp_path / 'eval_old')
    evalrun.evaluate_runs([entry], old, without, 'foreground', levels=50)
    assert _all_csv(without) == {k: v for k, v in fused.items() if k not in mine}
    # contents
    rows = _rows(os.path.join(base, 'uncertainty', 'eval_boundary_baseline_mc.csv'))
    assert [r['subject_name'] for r in rows] == sorted(subjects)
    off = [k + '_off_border' for k in ev.UE_CURVE_KEYS]
    assert list(rows[0]) == ['test_id', 'subject_name'] + list(ev.BOUNDARY_TABLE_KEYS) + ['hd', 'hd95', 'assd'] + off
    tables, hists = [], []
    for r in rows:
        conf, pred, tgt = truth[r['subject_name']]
        table = ev.boundary_table(pred, tgt, foreground_probability=conf, bands=3)[0]
        assert np.array_equal(as_cells(table), numpy_boundary_table(pred, tgt, quantise(ev.normalised_entropy(conf).cpu().numpy()), 3))
        bm = ev.boundary_metrics(table)
        sm = ev.surface_distance_metrics(numpy_surface_histogram(pred, tgt))
        shell = (separable_edt_sq(tgt == 0).astype(np.int64) <= 1) & (separable_edt_sq(tgt != 0).astype(np.int64) <= 1)
        hist = ev.uncertainty_histogram_from_p(pred, tgt, conf, 50, mask=~shell)[0]
        cm = ev.ue_curve_metrics(hist)
        assert {k: r[k] for k in ev.BOUNDARY_TABLE_KEYS} == {k: str(bm[k]) for k in ev.BOUNDARY_TABLE_KEYS}
        assert {k: r[k] for k in ('hd', 'hd95', 'assd')} == {k: str(sm[k]) for k in ('hd', 'hd95', 'assd')}
        assert {k: r[k + '_off_border'] for k in ev.UE_CURVE_KEYS} == {k: str(cm[k]) for k in ev.UE_CURVE_KEYS}
        tables.append(table)
        hists.append(hist)
    (row,) = _rows(os.path.join(base, 'uncertainty', 'eval_boundary_pooled_baseline_mc.csv'))
    total = ev.add_boundary_tables(tables)
    bm, cm = ev.boundary_metrics(total), ev.ue_curve_metrics(sum(hists))
    assert row['test_id'] == 'baseline_mc' and {k: row[k] for k in ev.BOUNDARY_TABLE_KEYS} == {k: str(bm[k]) for k in ev.BOUNDARY_TABLE_KEYS}
    assert {k: row[k + '_off_border'] for k in ev.UE_CURVE_KEYS} == {k: str(cm[k]) for k in ev.UE_CURVE_KEYS}
    bands = _rows(os.path.join(base, 'uncertainty', 'eval_boundary_bands_baseline_mc.csv'))
    assert [(int(b['side']), int(b['band'])) for b in bands] == [(s, k) for s in range(2) for k in range(4)]
    assert [[int(b[k]) for k in ('voxels', 'errors', 'unc_sum', 'unc_err_sum')] for b in bands] == as_cells(total).reshape(8, 4).tolist()
    # the pooled files do not depend on the subject order
    entry_rev = evalrun.get_eval_data('baseline_mc', run_dir, gts, expected_subjects=subjects)
    entry_rev.subject_files = entry_rev.subject_files[::-1]
    rev = str(tmp_path / 'eval_rev')
    evalrun.evaluate_runs([entry_rev], ['boundary'], rev, 'foreground', batch_subjects=4, bands=3, levels=50)
    for name in ('eval_boundary_pooled_baseline_mc.csv', 'eval_boundary_bands_baseline_mc.csv'):
        assert _all_csv(rev)[os.path.join('uncertainty', name)] == fused[os.path.join('uncertainty', name)]


def test_boundary_action_on_a_sigma_run(dev, tmp_path):
    """The map-based path: a 'sigma' run is rescaled with the run's global min / max (written by the minmax action) before it is summed."""
    from rcu_amd import evalrun, evaluation as ev
    rng = np.random.RandomState(6)
    subjects = ['Brats18_S_1', 'Brats18_T_1']
    gt_dir, run_dir, truth = _tree(tmp_path, subjects, 'sigma', rng)
    gts = evalrun.collect_brats_ground_truth(gt_dir)
    entry = evalrun.get_eval_data('aleatoric', run_dir, gts, expected_subjects=subjects)
    base = str(tmp_path / 'eval')
    evalrun.evaluate_runs([entry], ['minmax'], base, 'foreground')        # the global rescale reads the file this writes
    evalrun.evaluate_runs([entry], ['boundary'], base, 'foreground', bands=2)
    mm = evalrun.read_min_max(os.path.join(base, 'minmax', 'eval_summary_minmax_aleatoric.csv'))
    bands = _rows(os.path.join(base, 'uncertainty', 'eval_boundary_bands_aleatoric_globalrescale.csv'))
    total = sum(numpy_boundary_table(pred, tgt, quantise(ev.rescale_uncertainties(sigma, mm[0], mm[1])), 2) for sigma, pred, tgt in truth.values())
    assert [[int(b[k]) for k in ('voxels', 'errors', 'unc_sum', 'unc_err_sum')] for b in bands] == total.reshape(6, 4).tolist()
    assert len(_rows(os.path.join(base, 'uncertainty', 'eval_boundary_aleatoric_globalrescale.csv'))) == 2


# ------------------------------------------------------------------------------------------------------------ 10. the loader
def test_loader_fills_the_border_entries(dev, tmp_path):
    from rcu_amd import evalrun, evaluation as ev
    rng = np.random.RandomState(7)
    subjects = ['Brats18_L_1', 'Brats18_M_1']
    gt_dir, run_dir, truth = _tree(tmp_path, subjects, 'probabilities', rng)
    entry = evalrun.get_eval_data('baseline_mc', run_dir, evalrun.collect_brats_ground_truth(gt_dir), expected_subjects=subjects)
    loader = evalrun.Loader()
    plain = loader.get_data(entry.subject_files[0], evalrun.Loader.Params('probabilities'))
    assert 'target_boarder' not in plain and 'prediction_distance' not in plain
    for sf in entry.subject_files:
        conf, pred, tgt = truth[sf.subject]
        to_eval = loader.get_data(sf, evalrun.Loader.Params('probabilities', need_gt_dist_and_boarder=True, need_prediction_dist_and_boarder=True))
        for key, label_map in (('target', tgt), ('prediction', pred)):
            d_in, d_out = separable_edt_sq(label_map == 0).astype(np.int64), separable_edt_sq(label_map != 0).astype(np.int64)
            boarder, distance = to_eval[key + '_boarder'], to_eval[key + '_distance']      # the mask under *_boarder, the distance under *_distance
            assert boarder.dtype == bool and np.array_equal(boarder, (d_in <= 1) & (d_out <= 1))
            assert distance.dtype == np.float64 and np.array_equal(distance, np.sqrt((d_in + d_out).astype(np.float64)))
        assert 'target_boarder' in loader.cached and 'prediction_distance' in loader.cached          # cached per subject
        to_eval['uncertainty'] = ev.normalised_entropy(conf).cpu().numpy()
        results = {}
        ev.UncertaintyErrorDiceNumpy(0.5, with_mask=True)(to_eval, results)
        tp, tn, fp, fn, tpu, tnu, fpu, fnu = ev.uncertainty(pred, tgt, to_eval['uncertainty'] > 0.5, mask=~to_eval['target_boarder'])
        assert tp + tn + fp + fn == int((~to_eval['target_boarder']).sum())
        assert results == {'precision': ev.error_precision(tpu, tnu, fpu, fnu), 'recall': ev.error_recall(fp, fn, fpu, fnu),
                           'dice': ev.error_dice(fp, fn, tpu, tnu, fpu, fnu)}
        unmasked = {}
        ev.UncertaintyErrorDiceNumpy(0.5)(to_eval, unmasked)
        assert unmasked != results
