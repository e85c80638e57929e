"""The component-pair table on the GPU (rcu_cc_pairs) against np.unique over the stacked label pairs, under stress (64 distinct keys per
wave, every wave on one slot), across capacities, hashes and batchings; lesion_tables against the scipy-made fixture G27; SubjectBatch.metrics
with 'lesions'; the 'lesions' evaluation action end to end against the mask-based procedure of the fixture's generator.  Every table
comparison is integer equality (or byte equality of files)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from test_gpu_components import serpentine
from test_gpu_ue_curves import _all_csv, _rows, _tree
from test_lesions_cpu import CASES, CONFIGS, ONE, close, component_rows, fixture, numpy_pairs, pair_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture()
def hash_shift():
    from rcu_amd import _lib
    so = _lib.load()

    def call(shift):
        _lib.check(so.rcu_cc_pairs_set_hash_shift(shift))
    yield call
    so.rcu_cc_pairs_set_hash_shift(0)


@pytest.fixture(scope='module')
def checkerboard(dev):
    """64^3 under 6-connectivity: 131,072 one-voxel components; (mask, dense labels, canonical labels, the pair table numpy finds)."""
    from rcu_amd import evaluation as ev
    z, y, x = np.indices((64, 64, 64))
    mask = ((z + y + x) % 2 == 0).astype(np.uint8)
    dense, counts = ev.connected_components(mask, 6)
    assert int(counts[0]) == 131072
    canonical = ev.canonical_labels(mask, 6)
    return mask, dense, canonical, numpy_pairs(dense, canonical)


def raw_pairs(dev, a, b, inside, capacity, guard=256):
    """rcu_cc_pairs into a buffer with guard bytes on either side -> (counters [V, 2], slots [V, capacity, 4] int64 as they lie, guards intact)."""
    from rcu_amd import _lib
    so = _lib.load()
    v, n = a.shape
    nbytes = so.rcu_cc_pairs_bytes(capacity, v)
    assert nbytes == ((v * capacity * 16 + 255) & ~255) + ((v * 8 + 255) & ~255)
    buffer = torch.full((guard + nbytes + guard,), 0xA5, device=dev, dtype=torch.uint8)
    a_dev, b_dev = torch.from_numpy(np.ascontiguousarray(a)).to(dev), torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    i_dev = None if inside is None else torch.from_numpy(np.ascontiguousarray(inside)).to(dev)
    _lib.check(so.rcu_cc_pairs(_lib.ptr(a_dev), _lib.ptr(b_dev), _lib.ptr(i_dev), n, v, capacity, buffer.data_ptr() + guard, _lib.current_stream()))
    host = buffer.cpu().numpy()
    intact = bool((host[:guard] == 0xA5).all() and (host[guard + nbytes:] == 0xA5).all())
    body = host[guard:guard + nbytes]
    slot_bytes = (v * capacity * 16 + 255) & ~255
    slots = body[:v * capacity * 16].view(np.uint32).reshape(v, capacity, 4).astype(np.int64)
    counters = body[slot_bytes:slot_bytes + 8 * v].view(np.uint32).reshape(v, 2).astype(np.int64)
    return counters, slots, intact


def random_labels(rng, shape, density, ids):
    out = np.where(rng.rand(*shape) < density, rng.choice(ids, size=shape), 0).astype(np.int32)
    out[rng.rand(*shape) < 0.02] = -7           # negative values count as background
    return out


# ------------------------------------------------------------------------------------------------------- pairs vs numpy
@pytest.mark.parametrize('shape', ((3, 7, 70), (1, 5, 129), (2, 16, 64)))
def test_pairs_equal_numpy_unique(dev, shape):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(sum(shape))
    few, many = np.array([1, 2, 3, 65535, 65536, 70001, (1 << 31) - 1]), np.concatenate([np.arange(1, 400), [65536 + 5, 1 << 20, (1 << 31) - 2]])
    seen = 0
    for batch in (1, 3):
        for density, ids_a, ids_b in ((0.08, many, few), (0.95, few, few), (0.9, many, many), (0.5, few, many)):
            full = (batch,) + shape
            a, b = random_labels(rng, full, density, ids_a), random_labels(rng, full, density, ids_b)
            inside = (rng.rand(*full) < 0.4).astype(np.uint8) * 9
            arrays = (a, b, inside) if batch > 1 else (a[0], b[0], inside[0])
            with_inside = ev.component_pairs(*arrays, n_volumes=batch)
            without = ev.component_pairs(arrays[0], arrays[1], n_volumes=batch)
            assert len(with_inside) == len(without) == batch
            for v in range(batch):
                assert with_inside[v].dtype == ev.PAIR_DTYPE
                assert np.array_equal(pair_rows(with_inside[v]), numpy_pairs(a[v], b[v], inside[v])), (shape, batch, density, v)
                assert np.array_equal(pair_rows(without[v]), numpy_pairs(a[v], b[v])), (shape, batch, density, v)
                seen += len(with_inside[v])
            # device tensors in: the same table
            again = ev.component_pairs(*(torch.from_numpy(x).to(dev) for x in arrays), n_volumes=batch)
            assert all(p.tobytes() == q.tobytes() for p, q in zip(again, with_inside))
    assert seen > 1000
    # nothing to pair: empty tables
    zero = np.zeros(shape, dtype=np.int32)
    assert len(ev.component_pairs(zero, np.ones(shape, dtype=np.int32))[0]) == 0 and len(ev.component_pairs(-np.ones(shape, dtype=np.int32), zero + 3)[0]) == 0
    with pytest.raises(ValueError):
        ev.component_pairs(zero, zero.reshape(-1)[:-1])
    for capacity in (100, 32, 1 << 27):
        with pytest.raises(ValueError):
            ev.component_pairs(zero, zero, capacity=capacity)


def test_checkerboard_stress_64_distinct_keys_per_wave(dev, checkerboard):
    from rcu_amd import evaluation as ev
    mask, dense, canonical, expect = checkerboard
    assert len(expect) == 131072 and np.all(expect[:, 2] == 1)
    (got,) = ev.component_pairs(dense, canonical, inside=mask)
    assert np.array_equal(pair_rows(got)[:, :3], expect[:, :3]) and np.all(got['inside_voxels'] == 1)
    # the two numberings pair up one to one, in the same order: label k is the component whose first voxel is canonical label's index
    assert np.array_equal(got['a'], np.arange(1, 131073)) and np.all(np.diff(got['b'].astype(np.int64)) > 0)


def test_serpentine_contention_every_wave_on_one_slot(dev):
    from rcu_amd import evaluation as ev
    band = serpentine((16, 64, 128))
    labels, counts = ev.connected_components(band, 26)
    assert int(counts[0]) == 1
    ones = np.ones(band.shape, dtype=np.int32)
    (got,) = ev.component_pairs(labels, ones, inside=band)
    assert pair_rows(got).tolist() == [[1, 1, int(band.sum()), int(band.sum())]]
    (got,) = ev.component_pairs(ones * 77777, ones * 3, inside=band)          # every voxel of every wave
    assert pair_rows(got).tolist() == [[77777, 3, band.size, int(band.sum())]]


def test_volumes_of_a_batch_do_not_mix(dev):
    from rcu_amd import evaluation as ev
    shape = (3, 4, 5, 40)
    a, b = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32)
    a[0, :2], b[0, 1:3] = 5, 9              # the same ids in every volume, other extents
    a[1, :, :3], b[1, :, 2:] = 5, 9
    a[2, -1, -1, -1], b[2, -1, -1, -1] = 5, 9
    a[2, 0, 0, 0] = 5                       # (b is background there)
    got = ev.component_pairs(a, b, n_volumes=3)
    assert [pair_rows(t).tolist() for t in got] == [[[5, 9, 5 * 40, 0]], [[5, 9, 4 * 1 * 40, 0]], [[5, 9, 1, 0]]]
    for v in range(3):
        assert ev.component_pairs(a[v], b[v])[0].tobytes() == got[v].tobytes()


def test_identity_cross_check_without_a_host_oracle(dev):
    """Every component of P & D lies in exactly one component of P and one of D: summing the sizes of the components of P & D by the pair
    of labels at their first voxels must give the pair table, integer for integer."""
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(12)
    shape = (10, 30, 50)
    target = (rng.rand(*shape) < 0.004).astype(np.uint8)
    for conn in (6, 26):
        for radius in (1, 3):
            prediction = (rng.rand(*shape) < (0.2 if conn == 6 else 0.05)).astype(np.uint8)          # hundreds of components under either connectivity
            d = (ev.distance_transform_sq(target, invert=True) <= radius * radius).astype(np.uint8)
            p_labels, _ = ev.connected_components(prediction, conn)
            d_labels, _ = ev.connected_components(d, conn)
            (pairs,) = ev.component_pairs(p_labels, d_labels, inside=target)
            (both,) = ev.component_table(prediction & d, target, connectivity=conn)
            roots = both['root'].astype(np.int64)
            keys = (p_labels.reshape(-1)[roots].astype(np.int64) << 32) | d_labels.reshape(-1)[roots].astype(np.int64)
            unique, inverse = np.unique(keys, return_inverse=True)
            voxels, inside = np.zeros(len(unique), dtype=np.int64), np.zeros(len(unique), dtype=np.int64)
            np.add.at(voxels, inverse, both['voxels'].astype(np.int64))
            np.add.at(inside, inverse, both['other_voxels'].astype(np.int64))
            expect = np.stack([unique >> 32, unique & 0xffffffff, voxels, inside], axis=1)
            assert len(expect) > 15 and np.array_equal(pair_rows(pairs), expect), (conn, radius)


# ------------------------------------------------------------------------------------------------------------- capacity
def test_a_full_table_drops_voxels_and_writes_nothing_outside_itself(dev, checkerboard):
    mask, dense, canonical, expect = checkerboard
    a = np.stack([dense, np.roll(dense, 2, axis=0)]).reshape(2, -1)          # (a shift by two planes keeps the parity: other partners)
    b = np.stack([canonical, canonical]).reshape(2, -1)
    counters, slots, intact = raw_pairs(dev, a, b, None, 64)
    assert intact
    for v in range(2):
        total = int(((a[v] > 0) & (b[v] > 0)).sum())
        assert counters[v, 0] == 64 and counters[v, 1] > 0
        claimed = slots[v][slots[v][:, 0] != 0]
        assert len(claimed) == 64 and len({(r[0], r[1]) for r in claimed.tolist()}) == 64
        assert int(claimed[:, 2].sum()) + int(counters[v, 1]) == total              # a voxel is in the table or counted as dropped
        known = {(r[0], r[1]): r[2] for r in numpy_pairs(a[v], b[v]).tolist()}
        assert all(known[(r[0], r[1])] == r[2] and r[3] == 0 for r in claimed.tolist())
    # a table that holds everything: the counters say so
    counters, slots, intact = raw_pairs(dev, a, b, mask.reshape(1, -1).repeat(2, 0), 1 << 18)
    assert intact and counters.tolist() == [[131072, 0], [131072, 0]]
    for v in range(2):
        claimed = slots[v][slots[v][:, 0] != 0]
        order = np.lexsort((claimed[:, 1], claimed[:, 0]))
        assert np.array_equal(claimed[order], numpy_pairs(a[v], b[v], mask))


def test_component_pairs_retries_until_the_table_holds_everything(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(8)
    shape = (2, 8, 32, 64)
    a, b = rng.randint(1, 101, shape).astype(np.int32), rng.randint(1, 101, shape).astype(np.int32)
    assert ev.pair_capacity(100, 100) == 1024
    got = ev.component_pairs(a, b, n_volumes=2)                        # the default capacity of 1024 slots: > 7000 pairs per volume
    small = ev.component_pairs(a, b, n_volumes=2, capacity=64)
    for v in range(2):
        expect = numpy_pairs(a[v], b[v])
        assert len(expect) > 7000 and np.array_equal(pair_rows(got[v]), expect) and small[v].tobytes() == got[v].tobytes()


def test_a_table_that_just_fits_under_the_degraded_hash(dev, hash_shift):
    from rcu_amd import evaluation as ev
    n = 3 * 7 * 70
    i = np.arange(n)
    a, b = (i % 8 + 1).astype(np.int32).reshape(3, 7, 70), ((i // 8) % 8 + 100000).astype(np.int32).reshape(3, 7, 70)
    expect = numpy_pairs(a, b)
    assert len(expect) == 64
    reference = None
    for shift in (0, 40, 58, 61, 63):             # 63: two start slots for 64 pairs
        hash_shift(shift)
        counters, slots, intact = raw_pairs(dev, a.reshape(1, -1), b.reshape(1, -1), None, 64)
        assert intact and counters.tolist() == [[64, 0]], shift
        order = np.lexsort((slots[0][:, 1], slots[0][:, 0]))
        assert np.array_equal(slots[0][order], expect), shift
        (got,) = ev.component_pairs(a, b, capacity=64)
        assert np.array_equal(pair_rows(got), expect), shift
        reference = reference or got.tobytes()
        assert got.tobytes() == reference
    # long chains in a larger table as well
    hash_shift(63)
    rng = np.random.RandomState(4)
    a, b = rng.randint(0, 40, (2, 16, 64)).astype(np.int32), rng.randint(0, 40, (2, 16, 64)).astype(np.int32)
    (got,) = ev.component_pairs(a, b, capacity=2048)
    assert np.array_equal(pair_rows(got), numpy_pairs(a, b)) and len(got) > 900


# ---------------------------------------------------------------------------------------------------------- determinism
def test_runs_and_batchings_give_identical_sorted_tables(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(21)
    shape = (3, 9, 19, 70)
    a, b = rng.randint(-2, 60, shape).astype(np.int32), rng.randint(-2, 9, shape).astype(np.int32)
    inside = (rng.rand(*shape) < 0.5).astype(np.uint8)
    first = ev.component_pairs(a, b, inside, n_volumes=3)
    second = ev.component_pairs(a, b, inside, n_volumes=3)
    alone = [ev.component_pairs(a[v], b[v], inside[v])[0] for v in range(3)]
    other_capacity = ev.component_pairs(a, b, inside, n_volumes=3, capacity=1 << 14)
    for v in range(3):
        assert first[v].tobytes() == second[v].tobytes() == alone[v].tobytes() == other_capacity[v].tobytes()
        assert np.array_equal(pair_rows(first[v]), numpy_pairs(a[v], b[v], inside[v]))


# ------------------------------------------------------------------------------------------------- lesion_tables on G27
def test_lesion_tables_equal_the_fixture(dev):
    from rcu_amd import evaluation as ev
    g = fixture()
    rng = np.random.RandomState(27)
    for name in CASES:
        pred, target, unc = g[name + '_prediction'], g[name + '_target'], g[name + '_uncertainty']
        p = rng.rand(*pred.shape).astype(np.float32)
        for conn, radius in CONFIGS:
            tag = '{}_c{}_r{}_'.format(name, conn, radius)
            ((components, lesions, pairs),) = ev.lesion_tables(pred, target, unc, conn, radius)
            assert components.dtype == lesions.dtype == ev.COMPONENT_DTYPE and pairs.dtype == ev.PAIR_DTYPE
            assert np.array_equal(component_rows(components), g[tag + 'pred_table']), tag
            assert np.array_equal(component_rows(lesions), g[tag + 'lesion_table']), tag
            assert np.array_equal(pair_rows(pairs), g[tag + 'pairs']), tag
            assert components.tobytes() == ev.component_table(pred, target, unc, conn)[0].tobytes()
            # the entropy of a probability map in registers: the table of its materialised map; lesions and pairs do not feel the uncertainty
            direct = ev.lesion_tables(pred, target, ev.EntropyOfProbability(p), conn, radius)[0]
            via_map = ev.lesion_tables(pred, target, ev.normalised_entropy(p), conn, radius)[0]
            assert all(x.tobytes() == y.tobytes() for x, y in zip(direct, via_map))
            assert direct[1].tobytes() == lesions.tobytes() and direct[2].tobytes() == pairs.tobytes()
            none = ev.lesion_tables(pred, target, None, conn, radius)[0]
            assert np.array_equal(component_rows(none[0])[:, :3], g[tag + 'pred_table'][:, :3]) and not none[0]['unc_sum'].any()
    # a batch: the two 8 x 9 x 10 volumes, one without a target voxel (its squared distances are EDT_NONE: no lesion), one without a prediction
    pred, target = np.stack([g['notarget_prediction'], g['nopred_prediction']]), np.stack([g['notarget_target'], g['nopred_target']])
    unc = np.stack([g['notarget_uncertainty'], g['nopred_uncertainty']])
    for conn, radius in CONFIGS:
        batch = ev.lesion_tables(torch.from_numpy(pred).to(dev), torch.from_numpy(target).to(dev), torch.from_numpy(unc).to(dev), conn, radius, n_volumes=2)
        for v, name in enumerate(('notarget', 'nopred')):
            tag = '{}_c{}_r{}_'.format(name, conn, radius)
            assert np.array_equal(component_rows(batch[v][0]), g[tag + 'pred_table']) and np.array_equal(component_rows(batch[v][1]), g[tag + 'lesion_table'])
            assert np.array_equal(pair_rows(batch[v][2]), g[tag + 'pairs'])
        assert len(batch[0][1]) == 0 and len(batch[0][2]) == 0 and len(batch[1][0]) == 0
    for bad in (-1, 1.5, 46341):
        with pytest.raises(ValueError):
            ev.lesion_tables(pred[0], target[0], merge_radius=bad)


def test_subject_batch_metrics_with_lesions(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(3)
    shape, count = (6, 14, 20), 3
    batch = ev.SubjectBatch(count, int(np.prod(shape)))
    subjects = []
    for slot in range(count):
        p = rng.rand(*shape).astype(np.float32)
        pr, tg = (p > 0.6).astype(np.uint8), (rng.rand(*shape) < 0.05).astype(np.uint8)
        batch.put(slot, p, pr, tg)
        subjects.append((p, pr, tg))
    batch.upload()
    plain = batch.metrics(want=('minmax', 'ue', 'components'), connectivity=6)
    more = batch.metrics(want=('minmax', 'ue', 'components', 'lesions'), connectivity=6, merge_radius=2)
    only = batch.metrics(want=('lesions',), connectivity=6, merge_radius=2)
    assert set(more) == set(plain) | {'lesions'} and set(only) == {'lesions'}
    for key in ('min', 'max', 'counts'):
        assert plain[key].tobytes() == more[key].tobytes()
    for slot, (p, pr, tg) in enumerate(subjects):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(plain['components'][slot], more['components'][slot]))
        expect = ev.lesion_tables(pr, tg, ev.EntropyOfProbability(p), 6, 2)[0]
        for got in (more['lesions'][slot], only['lesions'][slot]):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, expect))
        assert more['lesions'][slot][0].tobytes() == more['components'][slot][0].tobytes()       # one labelling of the prediction for both


# ----------------------------------------------------------------------------------------------------------- end to end
def _generator():
    spec = importlib.util.spec_from_file_location('generate_lesions', os.path.join(ROOT, 'tests', 'golden', 'generate_lesions.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_lesions_action_end_to_end(dev, tmp_path):
    from rcu_amd import evalrun, evaluation as ev
    gen = _generator()
    rng = np.random.RandomState(5)
    subjects = ['Brats18_{}_1'.format(c) for c in 'ABCDEFGHI']
    gt_dir, run_dir, truth = _tree(tmp_path, subjects, 'probabilities', rng)
    gts = evalrun.collect_brats_ground_truth(gt_dir)
    entry = evalrun.get_eval_data('baseline_mc', run_dir, gts, expected_subjects=subjects)
    options = dict(levels=20, connectivity=6, merge_radius=0, min_lesion_voxels=2, match_iou=0.5)
    base = str(tmp_path / 'eval')
    evalrun.evaluate_runs([entry], ['lesions'], base, 'foreground', **options)
    fused = _all_csv(base)
    assert sorted(fused) == [os.path.join('uncertainty', f) for f in ('eval_lesion_curve_baseline_mc.csv', 'eval_lesion_list_baseline_mc.csv',
                                                                       'eval_lesions_baseline_mc.csv', 'eval_lesions_pooled_baseline_mc.csv')]
    # the plain loop and other batch sizes write the same bytes
    for tag, kwargs in (('plain', dict(fused=False)), ('b1', dict(batch_subjects=1)), ('b4', dict(batch_subjects=4))):
        other = str(tmp_path / ('eval_' + tag))
        evalrun.evaluate_runs([entry], ['lesions'], other, 'foreground', **options, **kwargs)
        assert _all_csv(other) == fused, tag
    # next to 'components': its files are those of 'components' alone, the lesions' files those of 'lesions' alone
    comp_alone, together = str(tmp_path / 'eval_components'), str(tmp_path / 'eval_both')
    evalrun.evaluate_runs([entry], ['components'], comp_alone, 'foreground', **options)
    evalrun.evaluate_runs([entry], ['components', 'lesions'], together, 'foreground', **options)
    both = _all_csv(together)
    assert both == {**_all_csv(comp_alone), **fused} and len(both) == 3 + 4
    together_plain = str(tmp_path / 'eval_both_plain')
    evalrun.evaluate_runs([entry], ['components', 'lesions'], together_plain, 'foreground', fused=False, **options)
    assert _all_csv(together_plain) == both
    # contents: the mask-based procedure of the fixture's generator on the same arrays
    rows = _rows(os.path.join(base, 'uncertainty', 'eval_lesions_baseline_mc.csv'))
    assert [r['subject_name'] for r in rows] == sorted(subjects) and list(rows[0]) == ['test_id', 'subject_name'] + list(ev.LESION_METRIC_KEYS)
    listed = _rows(os.path.join(base, 'uncertainty', 'eval_lesion_list_baseline_mc.csv'))
    oracle_subjects, at = [], 0
    for r in rows:
        conf, pred, tgt = truth[r['subject_name']]
        entropy = ev.normalised_entropy(conf).cpu().numpy()
        p_labels, l_labels, pred_table, _, _ = gen.tables(pred, tgt, entropy, 6, 0)
        subject = (p_labels, l_labels, tgt != 0, pred_table[:, 3] / (pred_table[:, 1] * np.float64(ONE)))
        oracle_subjects.append(subject)
        metrics, _, lesions = gen.evaluate([subject], 20, 0.5, 2)
        for key, expect in zip(gen.METRIC_KEYS, metrics):
            assert close(float(r[key]), expect), (r['subject_name'], key, r[key], float(expect))
        assert int(r['n_lesions']) == len(lesions[0]) > 0
        for line, expect in zip(listed[at:at + len(lesions[0])], lesions[0]):
            assert line['subject'] == r['subject_name'] and all(close(float(line[k]), e) for k, e in zip(gen.LIST_KEYS, expect))
        at += len(lesions[0])
    assert at == len(listed)
    metrics, curve, _ = gen.evaluate(oracle_subjects, 20, 0.5, 2)
    (row,) = _rows(os.path.join(base, 'uncertainty', 'eval_lesions_pooled_baseline_mc.csv'))
    assert row['test_id'] == 'baseline_mc' and all(close(float(row[k]), e) for k, e in zip(gen.METRIC_KEYS, metrics))
    lines = _rows(os.path.join(base, 'uncertainty', 'eval_lesion_curve_baseline_mc.csv'))
    assert len(lines) == 21 and [float(l['threshold']) for l in lines] == [k / 20 for k in range(21)]
    for line, expect in zip(lines, curve):
        assert all(close(float(line[k]), e) for k, e in zip(gen.CURVE_KEYS, expect))
    # the pooled files do not depend on the subject order
    entry_rev = evalrun.get_eval_data('baseline_mc', run_dir, gts, expected_subjects=subjects)
    entry_rev.subject_files = entry_rev.subject_files[::-1]
    rev = str(tmp_path / 'eval_rev')
    evalrun.evaluate_runs([entry_rev], ['lesions'], rev, 'foreground', batch_subjects=4, **options)
    for name in ('eval_lesions_pooled_baseline_mc.csv', 'eval_lesion_curve_baseline_mc.csv'):
        assert _all_csv(rev)[os.path.join('uncertainty', name)] == fused[os.path.join('uncertainty', name)]
    # a merge radius reaches the action: the first subject's row under a dilation of one voxel, fused and plain
    merged, merged_plain = str(tmp_path / 'eval_r1'), str(tmp_path / 'eval_r1_plain')
    evalrun.evaluate_runs([entry], ['lesions'], merged, 'foreground', **dict(options, merge_radius=1))
    evalrun.evaluate_runs([entry], ['lesions'], merged_plain, 'foreground', fused=False, **dict(options, merge_radius=1))
    assert _all_csv(merged) == _all_csv(merged_plain) and _all_csv(merged) != fused
    first = _rows(os.path.join(merged, 'uncertainty', 'eval_lesions_baseline_mc.csv'))[0]
    conf, pred, tgt = truth[first['subject_name']]
    p_labels, l_labels, pred_table, _, _ = gen.tables(pred, tgt, ev.normalised_entropy(conf).cpu().numpy(), 6, 1)
    metrics, _, _ = gen.evaluate([(p_labels, l_labels, tgt != 0, pred_table[:, 3] / (pred_table[:, 1] * np.float64(ONE)))], 20, 0.5, 2)
    assert all(close(float(first[k]), e) for k, e in zip(gen.METRIC_KEYS, metrics)) and int(first['n_lesions']) < int(rows[0]['n_lesions'])


def test_lesions_action_on_images(dev, tmp_path):
    """An ISIC-shaped run: 2-D subjects are depth 1 (the 8-neighbourhood under connectivity 26, a Euclidean disc as the dilation)."""
    from rcu_amd import evalrun, evaluation as ev
    gen = _generator()
    subjects = ['Brats18_{}_1'.format(c) for c in 'PQRST']
    gt_dir, run_dir, truth = _tree(tmp_path, subjects, 'probabilities', np.random.RandomState(9), shape=(24, 32))
    entry = evalrun.get_eval_data('baseline', run_dir, evalrun.collect_brats_ground_truth(gt_dir), expected_subjects=subjects)
    options = dict(levels=50, connectivity=26, merge_radius=1, min_lesion_voxels=0, match_iou=0.5)
    base, plain = str(tmp_path / 'eval'), str(tmp_path / 'eval_plain')
    evalrun.evaluate_runs([entry], ['components', 'lesions'], base, '', batch_subjects=2, **options)
    evalrun.evaluate_runs([entry], ['components', 'lesions'], plain, '', fused=False, **options)
    files = _all_csv(base)
    assert files == _all_csv(plain) and len(files) == 3 + 4
    rows = _rows(os.path.join(base, 'uncertainty', 'eval_lesions_baseline.csv'))
    assert [r['subject_name'] for r in rows] == sorted(subjects)
    oracle_subjects = []
    for r in rows:
        conf, pred, tgt = truth[r['subject_name']]
        assert pred.ndim == 2
        p_labels, l_labels, pred_table, _, _ = gen.tables(pred, tgt, ev.normalised_entropy(conf).cpu().numpy(), 26, 1)
        oracle_subjects.append((p_labels, l_labels, tgt != 0, pred_table[:, 3] / (pred_table[:, 1] * np.float64(ONE))))
        metrics, _, _ = gen.evaluate(oracle_subjects[-1:], 50, 0.5, 0)
        assert all(close(float(r[k]), e) for k, e in zip(gen.METRIC_KEYS, metrics)), r['subject_name']
    metrics, curve, _ = gen.evaluate(oracle_subjects, 50, 0.5, 0)
    (row,) = _rows(os.path.join(base, 'uncertainty', 'eval_lesions_pooled_baseline.csv'))
    assert all(close(float(row[k]), e) for k, e in zip(gen.METRIC_KEYS, metrics)) and int(row['n_lesions']) > 0
    lines = _rows(os.path.join(base, 'uncertainty', 'eval_lesion_curve_baseline.csv'))
    assert len(lines) == 51 and all(close(float(line[k]), e) for line, expect in zip(lines, curve) for k, e in zip(gen.CURVE_KEYS, expect))
