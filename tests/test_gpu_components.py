"""Connected components on the GPU: rcu_cc_label / rcu_cc_compact / rcu_cc_relabel / rcu_cc_table against the numpy restatement and
scipy's labels and sums (fixture G23), on shapes that stress the tiling, on a native-size batch, across tile settings; the three forms of
the uncertainty source; SubjectBatch.metrics with 'components'; the 'components' evaluation action end to end.  Every comparison is
integer equality (or byte equality of files)."""
import os
import shutil

import numpy as np
import pytest
import torch

from test_components_cpu import ONE, as_rows, as_table, dense_of, fixture_cases, numpy_labels, numpy_table, same_metrics
from test_gpu_ue_curves import _all_csv, _rows, _tree

pytestmark = pytest.mark.gpu
TILES = ((0, 0, 0), (1, 1, 1), (2, 3, 5), (8, 8, 16), (1, 16, 64), (1, 1, 1024), (3, 1, 7))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture()
def set_tile():
    from rcu_amd import _lib
    so = _lib.load()

    def call(tile):
        _lib.check(so.rcu_cc_set_tile(*tile))
    yield call
    so.rcu_cc_set_tile(0, 0, 0)


def check_volume(ev, mask, conn, n_volumes=1, what=''):
    """Canonical labels, dense labels, counts and the plain table of a mask (or a batch) against the numpy restatement."""
    canonical = ev.canonical_labels(mask, conn, n_volumes)
    dense, counts = ev.connected_components(mask, conn, n_volumes)
    tables = ev.component_table(mask, connectivity=conn, n_volumes=n_volumes)
    assert canonical.dtype == np.int32 and dense.dtype == np.int32 and canonical.shape == dense.shape == mask.shape
    assert counts.dtype == np.int64 and counts.shape == (n_volumes,) and len(tables) == n_volumes
    volumes = [mask] if n_volumes == 1 else list(mask)
    for v, vol in enumerate(volumes):
        expect = numpy_labels(vol, conn)
        got = canonical if n_volumes == 1 else canonical[v]
        assert np.array_equal(got, expect), (what, conn, v)
        expect_dense, k = dense_of(expect)
        assert np.array_equal(dense if n_volumes == 1 else dense[v], expect_dense) and int(counts[v]) == k, (what, conn, v)
        assert np.array_equal(as_rows(tables[v]), numpy_table(vol, connectivity=conn, labels=expect)), (what, conn, v)
    return canonical, counts


# ------------------------------------------------------------------------------------------------------ fixture volumes
def test_fixture_volumes_one_by_one(dev):
    from rcu_amd import evaluation as ev
    for name, conn, pred, target, unc, ref in fixture_cases():
        for which, mask, other, u in (('pred', pred, target, unc), ('target', target, pred, None)):
            dense, counts = ev.connected_components(mask, conn)
            assert np.array_equal(dense, ref[which + '_labels']) and int(counts[0]) == len(ref[which + '_table']), (name, conn, which)
            (table,) = ev.component_table(mask, other, u, conn)
            assert table.dtype == ev.COMPONENT_DTYPE
            assert np.array_equal(as_rows(table), ref[which + '_table']), (name, conn, which)
            check_volume(ev, mask, conn, what=name)
        # the metrics of the device's tables are those of scipy's
        got = ev.component_metrics(ev.component_table(pred, target, unc, conn)[0], ev.component_table(target, pred, None, conn)[0])
        assert same_metrics(got, ev.component_metrics(as_table(ref['pred_table']), as_table(ref['target_table'])))


def test_fixture_volumes_as_batches(dev):
    """The three 12 x 17 x 9 volumes as one batch, in two orders, with repeated members: a volume's labels and rows do not feel its neighbours."""
    from rcu_amd import evaluation as ev
    cases = {(name, conn): (pred, target, unc, ref) for name, conn, pred, target, unc, ref in fixture_cases()}
    for conn in (6, 26):
        for order in (('d10', 'd30', 'd60'), ('d60', 'd10', 'd60', 'd30', 'd10')):
            pred = np.stack([cases[(n, conn)][0] for n in order])
            target = np.stack([cases[(n, conn)][1] for n in order])
            unc = np.stack([cases[(n, conn)][2] for n in order])
            v = len(order)
            dense, counts = ev.connected_components(pred, conn, n_volumes=v)
            tables = ev.component_table(pred, target, unc, conn, n_volumes=v)
            for i, n in enumerate(order):
                ref = cases[(n, conn)][3]
                assert np.array_equal(dense[i], ref['pred_labels']) and int(counts[i]) == len(ref['pred_table'])
                assert np.array_equal(as_rows(tables[i]), ref['pred_table']), (conn, order, i)
    # device tensors in, device labels out
    pred = torch.from_numpy(np.stack([cases[(n, 26)][0] for n in ('d10', 'd30')])).to(dev)
    dense, counts = ev.connected_components(pred, 26, n_volumes=2)
    assert isinstance(dense, torch.Tensor) and dense.is_cuda and dense.dtype == torch.int32
    assert np.array_equal(dense[1].cpu().numpy(), cases[('d30', 26)][3]['pred_labels'])


# ------------------------------------------------------------------------------------------- shapes that stress the tiling
def serpentine(shape):
    """A one-voxel-wide band through the whole volume: every other row along x of every other plane, neighbouring rows joined at
    alternating ends, neighbouring planes by a single voxel: one component under either connectivity, through very long chains."""
    d, h, w = shape
    m = np.zeros(shape, dtype=np.uint8)
    m[::2, ::2, :] = 1
    for j, y in enumerate(range(1, h - 1, 2)):
        m[::2, y, (w - 1) if j % 2 == 0 else 0] = 1
    m[1:d - 1:2, 0, 0] = 1
    return m


def stress_masks(shape):
    d, h, w = shape
    z, y, x = np.indices(shape)
    out = {'empty': np.zeros(shape, dtype=np.uint8), 'full': np.full(shape, 7, dtype=np.uint8),
           'checkerboard': ((z + y + x) % 2 == 0).astype(np.uint8), 'serpentine': serpentine(shape)}
    # voxels that meet at corners only, along the main diagonal -- through the corners where the default tiles (4 x 8 x 32, 1 x 16 x 64) meet
    # as well --, and along an anti-diagonal of the last plane (edge contacts)
    diag = np.zeros(shape, dtype=np.uint8)
    for k in range(min(h, w)):
        diag[min(k, d - 1), k, k] = 1
    for k in range(min(h, w)):
        diag[d - 1, k, w - 1 - k] = 1
    out['diagonal'] = diag
    rng = np.random.RandomState(h * w + d)
    out['random30'] = (rng.rand(*shape) < 0.3).astype(np.uint8)
    return out


SHAPES = ((9, 19, 70), (1, 37, 150), (5, 8, 33), (13, 3, 2), (1, 1, 300), (4, 8, 32))


@pytest.mark.parametrize('shape', SHAPES)
def test_shapes_that_stress_the_tiling(dev, shape):
    from rcu_amd import evaluation as ev
    n = int(np.prod(shape))
    for name, mask in stress_masks(shape).items():
        for conn in (6, 26):
            canonical, counts = check_volume(ev, mask, conn, what=(name, shape))
            if name == 'empty':
                assert int(counts[0]) == 0 and not canonical.any()
            if name == 'full':
                assert int(counts[0]) == 1 and np.all(canonical == 1)
            if name == 'checkerboard':       # no two of its voxels share a face; with two or more axes they all meet at edges
                one = conn == 26 and sum(e > 1 for e in shape) >= 2
                assert int(counts[0]) == (1 if one else int(mask.sum())) and int(mask.sum()) == (n + 1) // 2, (shape, conn)
            if name == 'serpentine':
                assert int(counts[0]) == 1, (shape, conn)
    # 2-D input (depth 1 by shape) is the same computation as the [1, H, W] volume
    if shape[0] == 1:
        mask = stress_masks(shape)['random30']
        for conn in (6, 26):
            assert np.array_equal(ev.canonical_labels(mask[0], conn), ev.canonical_labels(mask, conn)[0])


def test_volume_boundaries_of_a_batch_separate_components(dev):
    """Foreground in the last plane / row of one volume and the first of the next: adjacent in memory, never connected."""
    from rcu_amd import evaluation as ev
    shape = (3, 5, 40)
    batch = np.zeros((4,) + shape, dtype=np.uint8)
    batch[0, -1], batch[1, 0], batch[1, -1, -1, -1], batch[2, 0, 0, 0], batch[3] = 1, 1, 1, 1, 1
    for conn in (6, 26):
        canonical, counts = check_volume(ev, batch, conn, n_volumes=4, what='boundaries')
        assert list(counts) == [1, 2, 1, 1]
        assert canonical[1, 0, 0, 0] == 1 and canonical[2, 0, 0, 0] == 1 and canonical[3].min() == 1 == canonical[3].max()
        assert canonical[0, -1, 0, 0] == 2 * 5 * 40 + 1                   # indices restart in every volume
    # rows that wrap: the end of one row and the start of the next are neighbours in memory only
    img = np.zeros((1, 6, 33), dtype=np.uint8)
    img[0, :, 0], img[0, :, -1] = 1, 1
    img[0, ::2, 0] = 0
    for conn in (6, 26):
        check_volume(ev, img, conn, what='wrap')


def test_labels_and_tables_do_not_depend_on_the_tile(dev, set_tile):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(31)
    shape = (11, 21, 45)
    masks = np.stack([(rng.rand(*shape) < 0.25).astype(np.uint8), stress_masks(shape)['serpentine'], (rng.rand(*shape) < 0.6).astype(np.uint8)])
    other = (rng.rand(*masks.shape) < 0.4).astype(np.uint8)
    p = rng.rand(*masks.shape).astype(np.float32)
    image = (rng.rand(70, 130) < 0.45).astype(np.uint8)
    for conn in (6, 26):
        reference = None
        for tile in TILES:
            set_tile(tile)
            got = (ev.canonical_labels(masks, conn, 3).tobytes(), [t.tobytes() for t in ev.component_table(masks, other, ev.EntropyOfProbability(p), conn, 3)],
                   ev.canonical_labels(image, conn).tobytes())
            if reference is None:
                reference = got
                set_tile((0, 0, 0))
                for v in range(3):
                    assert np.array_equal(ev.canonical_labels(masks[v], conn), numpy_labels(masks[v], conn))
            assert got == reference, (conn, tile)


# ------------------------------------------------------------------------------------------------- the uncertainty sources
def test_map_forms_equal_the_numpy_quantisation(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(41)
    shape = (2, 10, 30, 50)
    mask = (rng.rand(*shape) < 0.4).astype(np.uint8)
    other = (rng.rand(*shape) < 0.5).astype(np.uint8) * 5
    unc = rng.rand(*shape)
    flat = unc.reshape(-1)
    flat[:64] = (np.arange(64) + 0.5) / ONE                          # exact ties
    flat[64:72] = [0.0, -0.0, 1.0, 1.5, -2.0, np.nan, np.inf, -np.inf]
    flat[100:200] = np.round(flat[100:200], 3)
    mask.reshape(-1)[:220] = 1                                        # the special values are inside components
    for dtype in (np.float64, np.float32):
        u = unc.astype(dtype)
        for conn in (6, 26):
            tables = ev.component_table(mask, other, u, conn, n_volumes=2)
            for v in range(2):
                assert np.array_equal(as_rows(tables[v]), numpy_table(mask[v], other[v], u[v], conn)), (dtype, conn, v)
            # device tensors give the same table
            again = ev.component_table(torch.from_numpy(mask).to(dev), torch.from_numpy(other).to(dev), torch.from_numpy(u).to(dev), conn, n_volumes=2)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(again, tables))


def test_probability_form_equals_the_map_form_on_the_device_entropy(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(43)
    shape = (3, 7, 40, 36)
    mask = (rng.rand(*shape) < 0.06).astype(np.uint8)               # sparse: hundreds of components under either connectivity
    other = (rng.rand(*shape) < 0.5).astype(np.uint8)
    p = rng.rand(*shape).astype(np.float32)
    special = np.array([0.0, 1.0, 0.5, 1e-7, 0.999999, np.float32(1e-45), np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))],
                       dtype=np.float32)
    p.reshape(-1)[:special.size] = special
    p.reshape(-1)[special.size:5000] = (rng.rand(5000 - special.size) * 1e-4).astype(np.float32)      # peaked
    mask.reshape(-1)[:5000:3] = 1
    entropy = ev.normalised_entropy(p)                                # device float64 map: rcu_normalised_entropy's output
    assert entropy.dtype == torch.float64
    for conn in (6, 26):
        direct = ev.component_table(mask, other, ev.EntropyOfProbability(p), conn, n_volumes=3)
        via_map = ev.component_table(mask, other, entropy, conn, n_volumes=3)
        assert sum(len(t) for t in direct) > 100
        for a, b in zip(direct, via_map):
            assert a.tobytes() == b.tobytes(), conn
        host = entropy.cpu().numpy()
        for v in range(3):
            assert np.array_equal(as_rows(direct[v]), numpy_table(mask[v], other[v], host[v], conn))
            assert int(direct[v]['unc_max'].max()) <= ONE


# ------------------------------------------------------------------------------------------------------ native size
def native_batch():
    """8 x 155 x 240 x 240: an ellipsoid blob (shifted per volume) plus sparse noise, some of it touching the blob."""
    shape = (155, 240, 240)
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    out = np.zeros((8,) + shape, dtype=np.uint8)
    for v in range(8):
        rng = np.random.RandomState(100 + v)
        blob = ((z - 70 - 3 * v) / 28.0) ** 2 + ((y - 110 + 5 * v) / 40.0) ** 2 + ((x - 128) / (33.0 + v)) ** 2 <= 1.0
        out[v] = blob | (rng.rand(*shape) < 0.002)
    return out


def test_native_size_batch(dev):
    from rcu_amd import evaluation as ev
    masks = native_batch()
    v, n = 8, 155 * 240 * 240
    rng = np.random.RandomState(9)
    other = np.roll(masks, 7, axis=3)
    p = rng.rand(2, n).astype(np.float32)[np.arange(8) % 2].reshape(masks.shape)        # two probability maps, alternating
    m_dev, o_dev, p_dev = torch.from_numpy(masks).to(dev), torch.from_numpy(other).to(dev), torch.from_numpy(p).to(dev)
    canonical = ev._labels_on_device(m_dev.reshape(v, n), (155, 240, 240), 26)
    dense, counts = ev.connected_components(m_dev, 26, n_volumes=v)
    tables = ev.component_table(m_dev, o_dev, ev.EntropyOfProbability(p_dev), 26, n_volumes=v)
    pick = 5
    expect = numpy_labels(masks[pick], 26)
    assert np.array_equal(canonical[pick].cpu().numpy().reshape(masks[pick].shape), expect)
    expect_dense, k = dense_of(expect)
    assert int(counts[pick]) == k and k > 1000 and np.array_equal(dense[pick].cpu().numpy(), expect_dense)
    entropy = ev.normalised_entropy(p_dev[pick]).cpu().numpy()
    rows = numpy_table(masks[pick], other[pick], entropy, 26, labels=expect)
    assert np.array_equal(as_rows(tables[pick]), rows)
    assert int(rows[:, 1].max()) > 100000                                              # the blob is one component of > 1e5 voxels
    for i in range(v):
        assert int(tables[i]['voxels'].astype(np.int64).sum()) == int(masks[i].astype(bool).sum()) and len(tables[i]) == int(counts[i])
    # the batch is the volumes one by one: volume 0 and 7 alone, and under 6-connectivity
    for i in (0, 7):
        alone = ev.component_table(m_dev[i], o_dev[i], ev.EntropyOfProbability(p_dev[i]), 26)[0]
        assert alone.tobytes() == tables[i].tobytes()
    six = ev._labels_on_device(m_dev[pick].reshape(1, n), (155, 240, 240), 6).cpu().numpy().reshape(masks[pick].shape)
    assert np.array_equal(six, numpy_labels(masks[pick], 6))


# ------------------------------------------------------------------------------------------------------ SubjectBatch
def test_subject_batch_metrics_with_components(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(3)
    shape, count = (6, 14, 20), 3
    n = int(np.prod(shape))
    batch = ev.SubjectBatch(count, n, with_mask=True)
    subjects = []
    for slot in range(count):
        p = rng.rand(*shape).astype(np.float32)
        pr, tg, m = (p > 0.6).astype(np.uint8), (rng.rand(*shape) < 0.3).astype(np.uint8), (rng.rand(*shape) < 0.6).astype(np.uint8)
        batch.put(slot, p, pr, tg, m)
        subjects.append((p, pr, tg))
    batch.upload()
    plain = batch.metrics(want=('minmax', 'ece', 'ue', 'ue_hist'))
    more = batch.metrics(want=('minmax', 'ece', 'ue', 'ue_hist', 'components'), connectivity=6)
    assert set(more) == set(plain) | {'components'}
    for key in ('min', 'max', 'counts', 'ue_hist'):
        assert plain[key].dtype == more[key].dtype and plain[key].tobytes() == more[key].tobytes(), key
    for a, b in zip(plain['hist'], more['hist']):
        assert a.tobytes() == b.tobytes()
    assert len(more['components']) == count
    for slot, (p, pr, tg) in enumerate(subjects):
        of_pred, of_target = more['components'][slot]
        assert of_pred.tobytes() == ev.component_table(pr, tg, ev.EntropyOfProbability(p), 6)[0].tobytes()
        assert of_target.tobytes() == ev.component_table(tg, pr, None, 6)[0].tobytes()
        assert np.array_equal(as_rows(of_target), numpy_table(tg, pr, None, 6))
    # subjects of one size and two shapes in one batch: each is labelled in its own shape
    batch2 = ev.SubjectBatch(2, 12 * 20)
    a, b = (rng.rand(12, 20) < 0.5).astype(np.uint8), (rng.rand(20, 12) < 0.5).astype(np.uint8)
    batch2.put(0, a.astype(np.float32), a, a)
    batch2.put(1, b.astype(np.float32), b, b)
    batch2.upload()
    got = batch2.metrics(want=('components',))['components']
    assert np.array_equal(as_rows(got[0][1]), numpy_table(a, a, None, 26)) and np.array_equal(as_rows(got[1][1]), numpy_table(b, b, None, 26))


# ----------------------------------------------------------------------------------------------------------- end to end
def test_components_action_end_to_end(dev, tmp_path):
    from rcu_amd import evalrun, evaluation as ev
    rng = np.random.RandomState(5)
    subjects = ['Brats18_{}_1'.format(c) for c in 'ABCDEFGHI']
    gt_dir, run_dir, truth = _tree(tmp_path, subjects, 'probabilities', rng)
    gts = evalrun.collect_brats_ground_truth(gt_dir)
    entry = evalrun.get_eval_data('baseline_mc', run_dir, gts, expected_subjects=subjects)
    old = ['minmax', 'ece_dice', 'calib', 'bnf_ue', 'ue_curves']
    base = str(tmp_path / 'eval')
    evalrun.evaluate_runs([entry], old + ['components'], base, 'foreground')
    fused = _all_csv(base)
    mine = {k: v for k, v in fused.items() if os.path.basename(k).startswith('eval_component')}
    assert sorted(os.path.basename(k) for k in mine) == ['eval_component_list_baseline_mc.csv', 'eval_components_baseline_mc.csv',
                                                         'eval_components_pooled_baseline_mc.csv']
    assert all(os.path.dirname(k) == evalrun.UNCERTAINTY_NAME for k in mine) and len(fused) == 14 + 3 + 3
    # the plain loop and every batch size write the same bytes
    for tag, kwargs in (('plain', dict(fused=False)), ('b1', dict(batch_subjects=1)), ('b3', dict(batch_subjects=3)), ('b8', dict(batch_subjects=8))):
        other = str(tmp_path / ('eval_' + tag))
        evalrun.evaluate_runs([entry], old + ['components'], other, 'foreground', **kwargs)
        assert _all_csv(other) == fused, tag
    # the four default actions' and ue_curves' files do not feel the new one
    without = str(tmp_path / 'eval_old')
    evalrun.evaluate_runs([entry], old, without, 'foreground')
    assert _all_csv(without) == {k: v for k, v in fused.items() if k not in mine}
    # the action alone
    alone = str(tmp_path / 'eval_alone')
    evalrun.evaluate_runs([entry], ['components'], alone, 'foreground')
    assert _all_csv(alone) == mine
    # contents
    rows = _rows(os.path.join(base, 'uncertainty', 'eval_components_baseline_mc.csv'))
    assert [r['subject_name'] for r in rows] == sorted(subjects)
    assert list(rows[0]) == ['test_id', 'subject_name'] + list(ev.COMPONENT_METRIC_KEYS)
    listed = _rows(os.path.join(base, 'uncertainty', 'eval_component_list_baseline_mc.csv'))
    pooled_p, pooled_t, at = [], [], 0
    for r in rows:
        conf, pred, tgt = truth[r['subject_name']]
        pt = ev.component_table(pred, tgt, ev.EntropyOfProbability(conf))[0]
        tt = ev.component_table(tgt, pred)[0]
        assert np.array_equal(as_rows(tt), numpy_table(tgt, pred, None, 26))
        assert np.array_equal(as_rows(pt)[:, :3], numpy_table(pred, tgt, None, 26)[:, :3])
        expect = ev.component_metrics(pt, tt)
        assert {k: r[k] for k in ev.COMPONENT_METRIC_KEYS} == {k: str(v) for k, v in expect.items()}
        assert int(r['n_components']) == len(pt)
        for k, row in enumerate(pt):
            line = listed[at + k]
            assert (line['subject'], int(line['component']), int(line['root_index']), int(line['voxels']), int(line['target_voxels'])) == \
                   (r['subject_name'], k + 1, int(row['root']), int(row['voxels']), int(row['other_voxels']))
            assert float(line['mean_uncertainty']) == int(row['unc_sum']) / (int(row['voxels']) * ONE) and int(line['is_fp']) == int(row['other_voxels'] == 0)
            assert float(line['max_uncertainty']) == int(row['unc_max']) / ONE
        at += len(pt)
        pooled_p.append(pt)
        pooled_t.append(tt)
    assert at == len(listed)
    (row,) = _rows(os.path.join(base, 'uncertainty', 'eval_components_pooled_baseline_mc.csv'))
    expect = ev.component_metrics(np.concatenate(pooled_p), np.concatenate(pooled_t))
    assert {k: row[k] for k in ev.COMPONENT_METRIC_KEYS} == {k: str(v) for k, v in expect.items()} and row['test_id'] == 'baseline_mc'
    # the pooled file does not depend on the subject order; connectivity and levels reach the action
    entry_rev = evalrun.get_eval_data('baseline_mc', run_dir, gts, expected_subjects=subjects)
    entry_rev.subject_files = entry_rev.subject_files[::-1]
    rev = str(tmp_path / 'eval_rev')
    evalrun.evaluate_runs([entry_rev], ['components'], rev, 'foreground', batch_subjects=4)
    name = os.path.join('uncertainty', 'eval_components_pooled_baseline_mc.csv')
    assert _all_csv(rev)[name] == fused[name]
    six = str(tmp_path / 'eval_six')
    evalrun.evaluate_runs([entry], ['components'], six, 'foreground', connectivity=6, levels=64)
    rows6 = _rows(os.path.join(six, 'uncertainty', 'eval_components_baseline_mc.csv'))
    conf, pred, tgt = truth[rows6[0]['subject_name']]
    expect = ev.component_metrics(ev.component_table(pred, tgt, ev.EntropyOfProbability(conf), 6)[0], ev.component_table(tgt, pred, None, 6)[0], 64)
    assert {k: rows6[0][k] for k in ev.COMPONENT_METRIC_KEYS} == {k: str(v) for k, v in expect.items()}
    assert int(rows6[0]['n_components']) > int(rows[0]['n_components'])
    six_plain = str(tmp_path / 'eval_six_plain')
    evalrun.evaluate_runs([entry], ['components'], six_plain, 'foreground', connectivity=6, levels=64, fused=False)
    assert _all_csv(six_plain) == _all_csv(six)


def test_components_action_on_a_sigma_run(dev, tmp_path):
    """The map-based path: a 'sigma' run is rescaled with the run's global min / max (written by the minmax action) before it is summed."""
    from rcu_amd import evalrun, evaluation as ev
    rng = np.random.RandomState(6)
    subjects = ['Brats18_S_1', 'Brats18_T_1', 'Brats18_U_1']
    gt_dir, run_dir, truth = _tree(tmp_path, subjects, 'sigma', rng)
    gts = evalrun.collect_brats_ground_truth(gt_dir)
    entry = evalrun.get_eval_data('aleatoric', run_dir, gts, expected_subjects=subjects)
    assert entry.confidence_entry == 'sigma'
    base = str(tmp_path / 'eval')
    evalrun.evaluate_runs([entry], ['minmax'], base, 'foreground')        # the global rescale reads the file this writes
    evalrun.evaluate_runs([entry], ['components'], base, 'foreground')
    mm = evalrun.read_min_max(os.path.join(base, 'minmax', 'eval_summary_minmax_aleatoric.csv'))
    rows = _rows(os.path.join(base, 'uncertainty', 'eval_components_aleatoric_globalrescale.csv'))
    assert [r['subject_name'] for r in rows] == sorted(subjects)
    pooled_p, pooled_t = [], []
    for r in rows:
        sigma, pred, tgt = truth[r['subject_name']]
        prepared = ev.rescale_uncertainties(sigma, mm[0], mm[1])
        pt, tt = as_table(numpy_table(pred, tgt, prepared, 26)), as_table(numpy_table(tgt, pred, None, 26))
        expect = ev.component_metrics(pt, tt)
        assert {k: r[k] for k in ev.COMPONENT_METRIC_KEYS} == {k: str(v) for k, v in expect.items()}
        pooled_p.append(pt)
        pooled_t.append(tt)
    (row,) = _rows(os.path.join(base, 'uncertainty', 'eval_components_pooled_aleatoric_globalrescale.csv'))
    expect = ev.component_metrics(np.concatenate(pooled_p), np.concatenate(pooled_t))
    assert {k: row[k] for k in ev.COMPONENT_METRIC_KEYS} == {k: str(v) for k, v in expect.items()}
    assert os.path.exists(os.path.join(base, 'uncertainty', 'eval_component_list_aleatoric_globalrescale.csv'))
    shutil.rmtree(base)
