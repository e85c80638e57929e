"""The calibration level histogram on the GPU: rcu_calib_curve against the numpy definition (fixture G26), on ragged and misaligned batches,
its invariants, the NLL terms, the worst cases of the hot-level aggregation; SubjectBatch.metrics with 'calib_levels'; the 'calib_curves'
evaluation action end to end (fused and plain loop, batch sizes, subject order, a 'sigma' run, --recalibrate_from)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_calib_curves_cpu import CASES, numpy_calibration_levels, numpy_levels_of, numpy_thresholds
from test_gpu_ue_curves import _all_csv, _rows, _tree

pytestmark = pytest.mark.gpu
LEVELS = (2, 10, 1000, 1365, 1366, 4096)       # 1365 | 1366: the narrow | wide workgroup
P_FLOOR = 2.0 ** -23
L_MAX = 23 * np.log(2.0)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def device_terms(p, target, levels):
    """rcu_calib_curve_terms -> (level int32 [n], l float32 [n]) on the host."""
    from rcu_amd import _lib
    p, target = p.reshape(-1), target.reshape(-1)
    level = torch.empty(p.numel(), device=p.device, dtype=torch.int32)
    nll = torch.empty(p.numel(), device=p.device, dtype=torch.float32)
    _lib.check(_lib.load().rcu_calib_curve_terms(_lib.ptr(p), _lib.ptr(target), p.numel(), levels, _lib.ptr(level), _lib.ptr(nll), _lib.current_stream()))
    return level.cpu().numpy(), nll.cpu().numpy()


def check_against_numpy(ev, p, target, levels, mask=None, n_volumes=1):
    """The GPU's integers of a batch equal the definition's, volume by volume (the NLL column apart); -> (levels, totals)."""
    got, totals = ev.calibration_levels(p, target, levels, mask=mask, n_volumes=n_volumes)
    assert got.dtype == np.uint64 and got.shape == (n_volumes, 3, levels) and totals.dtype == np.uint64 and totals.shape == (n_volumes, 2, 4)
    host = [None if a is None else (a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).reshape(n_volumes, -1) for a in (p, target, mask)]
    for v in range(n_volumes):
        want, want_totals = numpy_calibration_levels(host[0][v], host[1][v], levels, None if host[2] is None else host[2][v])
        assert np.array_equal(got[v], want), (levels, v)
        assert np.array_equal(totals[v, :, :3], want_totals), (levels, v)
    return got, totals


@pytest.mark.parametrize('levels', LEVELS)
def test_equals_the_numpy_definition_on_the_fixtures(dev, levels):
    from rcu_amd import evaluation as ev
    g = load_golden('g26_calib_curves')
    for tag in CASES:
        for mask in (None, g[tag + '_mask']):
            check_against_numpy(ev, g[tag + '_p'], g[tag + '_target'], levels, mask)
    # a [..., 2] probability map goes through _foreground as calibration_histogram's does
    p = g['a_p']
    two = ev.calibration_levels(np.stack([1 - p, p], axis=-1), g['a_target'], levels)
    one = ev.calibration_levels(p, g['a_target'], levels)
    assert np.array_equal(two[0], one[0]) and np.array_equal(two[1], one[1])


@pytest.mark.parametrize('n', (1, 16383, 16385, 65541))
def test_small_ragged_misaligned_batches(dev, n):
    """Three volumes whose length is no multiple of 4 (misaligned heads, ragged tails, the partial and the whole block of both workgroup
    sizes), bases offset by one element (everything element by element), a volume that is masked out entirely, NaN, -1 and 2 among the values."""
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(n)
    v = 3
    p = rng.rand(v, n).astype(np.float32)
    p[:, ::5] = np.round(p[:, ::5], 3)                   # many values on (or an ulp from) a threshold
    flat = p.reshape(-1)
    flat[:min(6, flat.size)] = [np.nan, -1.0, 2.0, 0.0, 1.0, 0.5][:min(6, flat.size)]
    target = (rng.rand(v, n) < 0.3).astype(np.uint8) * 7
    mask = (rng.rand(v, n) < 0.7).astype(np.uint8)
    mask[1] = 0
    for levels in (1000, 4096):
        for m in (None, mask):
            got, totals = check_against_numpy(ev, p, target, levels, m, n_volumes=v)
            if m is not None:
                assert not got[1].any() and not totals[1].any()
        # the same batch behind one stray element: no array is 16-byte (4-byte) aligned
        shifted = [torch.cat([torch.zeros(1, dtype=t.dtype), t.reshape(-1)]).to(dev)[1:] for t in (torch.from_numpy(p), torch.from_numpy(target), torch.from_numpy(mask))]
        assert shifted[0].data_ptr() % 16 == 4 and shifted[1].data_ptr() % 4 == 1
        check_against_numpy(ev, shifted[0], shifted[1], levels, shifted[2], n_volumes=v)
        check_against_numpy(ev, shifted[0], shifted[1], levels, None, n_volumes=v)


def test_invariants_of_the_integers(dev):
    from rcu_amd import _lib, evaluation as ev
    rng = np.random.RandomState(12)
    v, n = 4, 40003
    p = rng.rand(v, n).astype(np.float32)
    p[2] = (rng.rand(n) * 1e-3).astype(np.float32)
    target = (rng.rand(v, n) < 0.3).astype(np.uint8)
    mask = (rng.rand(v, n) < 0.6).astype(np.uint8)
    so = _lib.load()
    for levels in (1000, 4096):
        whole, totals = ev.calibration_levels(p, target, levels, mask=mask, n_volumes=v)
        assert np.array_equal(whole[:, 2].sum(axis=1), totals[:, 0, 1] + totals[:, 1, 1])
        assert np.array_equal(whole[:, :2].sum(axis=(1, 2)), mask.sum(axis=1).astype(np.uint64))
        assert np.array_equal(whole[:, 0].sum(axis=1), totals[:, 0, 0]) and np.array_equal(whole[:, 1].sum(axis=1), totals[:, 1, 0])
        for vol in range(v):      # a batch equals its volumes one by one
            one, one_totals = ev.calibration_levels(p[vol], target[vol], levels, mask=mask[vol])
            assert np.array_equal(one[0], whole[vol]) and np.array_equal(one_totals[0], totals[vol])
        # two disjoint halves add up to the whole
        half = (rng.rand(v, n) < 0.5).astype(np.uint8)
        a, ta = ev.calibration_levels(p, target, levels, mask=mask * half, n_volumes=v)
        b, tb = ev.calibration_levels(p, target, levels, mask=mask * (1 - half), n_volumes=v)
        assert np.array_equal(a + b, whole) and np.array_equal(ta + tb, totals)
        try:      # every launch geometry gives the same integers
            for blocks in (1, 2):
                _lib.check(so.rcu_calib_curve_set_blocks_per_workgroup(blocks))
                other, other_totals = ev.calibration_levels(p, target, levels, mask=mask, n_volumes=v)
                assert np.array_equal(other, whole) and np.array_equal(other_totals, totals), blocks
        finally:
            so.rcu_calib_curve_set_blocks_per_workgroup(0)


def test_nll_terms_and_their_sum(dev):
    from rcu_amd import evaluation as ev
    g = load_golden('g26_calib_curves')
    rng = np.random.RandomState(13)
    extra = np.concatenate([rng.rand(5000), rng.rand(2000) * 1e-6, 1 - rng.rand(2000) * 1e-6, [0.0, 1.0, 2.0 ** -23, 2.0 ** -24, 1 - 2.0 ** -24,
                                                                                              np.nan, -1.0, 2.0]]).astype(np.float32)
    p = np.concatenate([g[tag + '_p'].reshape(-1) for tag in CASES] + [extra])
    target = (rng.rand(p.size) < 0.4).astype(np.uint8)
    mask = (rng.rand(p.size) < 0.7).astype(np.uint8)
    y = target != 0
    with np.errstate(invalid='ignore'):
        py = np.where(y, p, np.float32(1) - p).astype(np.float32)
        ref = np.clip(-np.log(np.fmax(py.astype(np.float64), P_FLOOR)), 0.0, L_MAX)       # fmax: a NaN probability counts as the floor
    for levels in (1000, 1365, 4095, 4096):
        level, l = device_terms(torch.from_numpy(p).to(dev), torch.from_numpy(target).to(dev), levels)
        assert np.array_equal(level, numpy_levels_of(p, levels))
        t = numpy_thresholds(levels)      # every threshold of this grid with its float32 neighbours: t_k -> k, the value below -> k - 1
        probes = np.concatenate([t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(2))])
        probe_level, _ = device_terms(torch.from_numpy(probes).to(dev), torch.zeros(probes.size, dtype=torch.uint8, device=dev), levels)
        k = np.arange(1, levels)
        assert np.array_equal(probe_level, np.concatenate([k, k - 1, k])) and np.array_equal(probe_level, numpy_levels_of(probes, levels))
        assert l.dtype == np.float32 and l.min() >= 0 and l.max() <= np.float32(L_MAX)
        err = np.abs(l.astype(np.float64) - ref)
        print('levels', levels, 'largest NLL term error', err.max(), 'largest relative', (err / np.maximum(ref, 1e-30))[ref > 2.0 ** -20].max())
        assert np.all((err <= 1e-5 * np.abs(ref)) | (err <= 2.0 ** -20))
        fixed = np.rint(l.astype(np.float64) * 2.0 ** 20).astype(np.uint64)       # l * 2^20 is exact in float32 and in float64
        for m in (None, mask):
            hist, totals = ev.calibration_levels(p, target, levels, mask=m)
            keep = np.ones(p.size, dtype=bool) if m is None else m != 0
            assert [int(totals[0, c, 3]) for c in (0, 1)] == [int(fixed[keep & ~y].sum()), int(fixed[keep & y].sum())]
            got = ev.calibration_curve_metrics(hist[0], totals[0], bins=1)
            assert abs(got['nll'] - ref[keep].mean()) <= 1e-5 * ref[keep].mean() + 2.0 ** -20


@pytest.mark.parametrize('levels', (1000, 4096))
def test_peaked_worst_cases_of_the_aggregation(dev, levels):
    """One volume of 65,536 voxels with one p: a single hot level takes everything.  Then every 32nd voxel elsewhere, every wave's FIRST lane
    among them: the hot level is never the first lane's."""
    from rcu_amd import evaluation as ev
    n = 65536
    for p0 in (np.float32(3e-4), np.float32(0.7311), np.float32(1.0)):
        p = np.full(n, p0, dtype=np.float32)
        target = np.zeros(n, dtype=np.uint8)
        got, totals = check_against_numpy(ev, p, target, levels)
        k = int(numpy_levels_of(p[:1], levels)[0])
        assert int(got[0, 0, k]) == n and int(got[0, :2].sum()) == n and int(totals[0, 0, 0]) == n
        p[::32] = np.float32(0.25) if p0 != np.float32(0.25) else np.float32(0.5)
        target[::3] = 1
        got, _ = check_against_numpy(ev, p, target, levels)
        assert int(got[0, :2, k].sum()) == n - n // 32
        # the rare level moves through the volume: every lane is the odd one somewhere
        p = np.full(n, p0, dtype=np.float32)
        p[::33] = rng_levels(levels, p[::33].size)
        check_against_numpy(ev, p, target, levels, mask=(np.arange(n) % 5 != 0).astype(np.uint8))


def rng_levels(levels, count):
    """`count` values spread over all levels."""
    return ((np.random.RandomState(levels).randint(0, levels, count) + 0.5) / levels).astype(np.float32)


def test_subject_batch_metrics_with_the_calibration_levels(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(3)
    count, n = 3, 24 * 24 * 24 + 5
    subjects = []
    for with_mask in (True, False):
        batch = ev.SubjectBatch(count, n, with_mask=with_mask)
        for slot in range(count):
            p = rng.rand(n).astype(np.float32) if slot else (rng.rand(n) * 1e-3).astype(np.float32)
            pr, tg, m = (p > 0.5).astype(np.uint8), (rng.rand(n) < 0.3).astype(np.uint8), (rng.rand(n) < 0.6).astype(np.uint8)
            batch.put(slot, p, pr, tg, m if with_mask else None)
            subjects.append((p, tg, m if with_mask else None))
        batch.upload()
        plain = batch.metrics(want=('minmax', 'ece', 'ue'))
        more = batch.metrics(want=('minmax', 'ece', 'ue', 'calib_levels'))
        assert set(more) == set(plain) | {'calib_levels', 'calib_totals'}
        for key in ('min', 'max', 'counts'):
            assert plain[key].tobytes() == more[key].tobytes(), key
        for a, b in zip(plain['hist'], more['hist']):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        assert more['calib_levels'].dtype == np.uint64 and more['calib_levels'].shape == (count, 3, 1000) and more['calib_totals'].shape == (count, 2, 4)
        for slot, (p, tg, m) in enumerate(subjects[-count:]):        # the mask of the 'ece' scan
            levels, totals = ev.calibration_levels(p, tg, mask=m)
            assert np.array_equal(more['calib_levels'][slot], levels[0]) and np.array_equal(more['calib_totals'][slot], totals[0])
            merged = levels[0, :2].sum(axis=0).reshape(10, 100).sum(axis=1)
            assert np.array_equal(merged.astype(np.int64), more['hist'][0][slot])
        assert batch.metrics(want=('calib_levels',), levels=64)['calib_levels'].shape == (count, 3, 64)


# ----------------------------------------------------------------------------------------------------------- end to end
def _calib_files(files):
    return {k: v for k, v in files.items() if os.path.basename(k).startswith(('eval_calib_curves_', 'eval_calib_levels_'))}


def test_calib_curves_action_end_to_end(dev, tmp_path):
    from rcu_amd import evalrun, evaluation as ev, nifti
    rng = np.random.RandomState(5)
    subjects = ['Brats18_{}_1'.format(c) for c in 'ABCDEFGHI']
    gt_dir, run_dir, truth = _tree(tmp_path, subjects, 'probabilities', rng)
    gts = evalrun.collect_brats_ground_truth(gt_dir)
    entry = evalrun.get_eval_data('baseline_mc', run_dir, gts, expected_subjects=subjects)
    old = ['minmax', 'ece_dice', 'calib', 'bnf_ue', 'ue_curves']
    new = old + ['calib_curves']
    base = str(tmp_path / 'eval')
    evalrun.evaluate_runs([entry], new, base, 'foreground')
    fused = _all_csv(base)
    calib_files = _calib_files(fused)
    names = ['eval_calib_curves_baseline_mc.csv', 'eval_calib_curves_pooled_baseline_mc.csv', 'eval_calib_levels_baseline_mc.csv']
    assert sorted(os.path.basename(k) for k in calib_files) == names and all(os.path.dirname(k) == evalrun.CALIB_NAME for k in calib_files)
    # the plain loop writes the same bytes; batch sizes and the subject order do not reach the pooled and the levels file
    plain = str(tmp_path / 'eval_plain')
    evalrun.evaluate_runs([entry], new, plain, 'foreground', fused=False)
    assert _all_csv(plain) == fused
    entry_rev = evalrun.get_eval_data('baseline_mc', run_dir, gts, expected_subjects=subjects)
    entry_rev.subject_files = entry_rev.subject_files[::-1]
    for tag, which, kwargs in (('b1', entry, dict(batch_subjects=1)), ('b4', entry, dict(batch_subjects=4)), ('rev', entry_rev, dict(batch_subjects=4))):
        other = str(tmp_path / ('eval_' + tag))
        evalrun.evaluate_runs([which], ['calib_curves'], other, 'foreground', **kwargs)
        files = _all_csv(other)
        assert set(files) == set(calib_files)
        for name in names[1:]:
            assert files[os.path.join(evalrun.CALIB_NAME, name)] == fused[os.path.join(evalrun.CALIB_NAME, name)], (tag, name)
        if which is entry:
            assert files == calib_files, tag
    # the other actions' files do not feel the new one
    without = str(tmp_path / 'eval_old')
    evalrun.evaluate_runs([entry], old, without, 'foreground')
    assert _all_csv(without) == {k: v for k, v in fused.items() if k not in calib_files}
    # contents: per-subject rows, the pooled row, the levels file
    rows = _rows(os.path.join(base, evalrun.CALIB_NAME, names[0]))
    assert [r['subject_name'] for r in rows] == sorted(subjects) and list(rows[0]) == ['test_id', 'subject_name'] + list(ev.CALIB_CURVE_KEYS)
    pooled_levels, pooled_totals = np.zeros((3, 1000), dtype=object), np.zeros((2, 4), dtype=object)
    hist10 = [np.zeros(10, dtype=np.int64), np.zeros(10), np.zeros(10, dtype=np.int64)]
    for r in rows:
        conf, pred, tgt = truth[r['subject_name']]
        sub = r['subject_name']
        mask = nifti.read(os.path.join(gt_dir, 'HGG', sub, sub + '_t2.nii.gz'))[0] > 0
        levels, totals = ev.calibration_levels(conf, tgt, mask=mask)
        expect = ev.calibration_curve_metrics(levels[0], totals[0])
        assert {k: r[k] for k in ev.CALIB_CURVE_KEYS} == {k: str(v) for k, v in expect.items()}
        assert int(r['n']) == int(mask.sum()) and int(r['n_pos']) == int((tgt[mask] != 0).sum())
        pooled_levels, pooled_totals = pooled_levels + levels[0].astype(object), pooled_totals + totals[0].astype(object)
        for acc, part in zip(hist10, ev.calibration_histogram(conf, tgt, 10, mask=mask)):
            acc += part[0]
    (row,) = _rows(os.path.join(base, evalrun.CALIB_NAME, names[1]))
    expect = ev.calibration_curve_metrics(pooled_levels, pooled_totals)
    assert {k: row[k] for k in ev.CALIB_CURVE_KEYS} == {k: str(v) for k, v in expect.items()} and row['test_id'] == 'baseline_mc'
    ece10 = ev.ece_from_histogram(*hist10)
    print('pooled ece', float(row['ece']), 'of the summed 10-bin histograms', ece10)
    assert abs(float(row['ece']) - ece10) <= 1e-9
    level_rows = _rows(os.path.join(base, evalrun.CALIB_NAME, names[2]))
    assert list(level_rows[0]) == list(evalrun.CALIB_LEVELS_COLUMNS) and [int(r['level']) for r in level_rows] == list(range(1000))
    assert [np.float32(r['threshold']) for r in level_rows[1:]] == list(ev.calibration_thresholds(1000)) and float(level_rows[0]['threshold']) == 0.0
    assert [int(r['n_neg']) for r in level_rows] == list(pooled_levels[0]) and [int(r['n_pos']) for r in level_rows] == list(pooled_levels[1])
    assert [float(r['isotonic']) for r in level_rows] == list(ev.isotonic_levels(pooled_levels))
    for r, n_neg, n_pos, conf in zip(level_rows, *pooled_levels):
        if n_neg + n_pos:
            assert float(r['mean_confidence']) == conf / ((n_neg + n_pos) << 32) and float(r['positive_fraction']) == n_pos / (n_neg + n_pos)
        else:
            assert r['mean_confidence'] == '' and r['positive_fraction'] == ''
    # a second evaluation judged under the first run's isotonic map: three more columns, every other column's text unchanged
    recal = str(tmp_path / 'eval_recal')
    evalrun.evaluate_runs([entry], ['calib_curves'], recal, 'foreground', recalibrate_from=os.path.join(base, evalrun.CALIB_NAME, names[2]))
    for name in names[:2]:
        before, after = _rows(os.path.join(base, evalrun.CALIB_NAME, name)), _rows(os.path.join(recal, evalrun.CALIB_NAME, name))
        assert list(after[0]) == list(before[0]) + list(ev.CALIB_RECAL_KEYS) and len(after) == len(before)
        for b, a in zip(before, after):
            assert {k: a[k] for k in b} == b
            assert all(np.isfinite(float(a[k])) for k in ev.CALIB_RECAL_KEYS)
    assert _all_csv(recal)[os.path.join(evalrun.CALIB_NAME, names[2])] == fused[os.path.join(evalrun.CALIB_NAME, names[2])]
    (after,) = _rows(os.path.join(recal, evalrun.CALIB_NAME, names[1]))
    assert float(after['ece_recal']) <= 1e-12       # the pooled run under its own map: every pooled block's value is its positive fraction
    with pytest.raises(ValueError):
        evalrun.evaluate_runs([entry], ['calib_curves'], str(tmp_path / 'eval_bad'), 'foreground', levels=500,
                              recalibrate_from=os.path.join(base, evalrun.CALIB_NAME, names[2]))
    # a run whose ECE actions and calib_curves disagree about the mask cannot happen through get_actions; other level counts and bins
    few = str(tmp_path / 'eval_64')
    evalrun.evaluate_runs([entry], ['calib_curves'], few, '', levels=64, calib_bins=16, mass_bins=4)
    assert len(_rows(os.path.join(few, evalrun.CALIB_NAME, names[2]))) == 64
    (row64,) = _rows(os.path.join(few, evalrun.CALIB_NAME, names[1]))
    assert int(row64['n']) == sum(truth[s][0].size for s in subjects)       # no brain mask without 'foreground'


def test_calib_curves_action_on_a_sigma_run(dev, tmp_path):
    """A 'sigma' run is rescaled on the host and takes the plain loop; its rows are those of the prepared probabilities."""
    from rcu_amd import evalrun, evaluation as ev
    rng = np.random.RandomState(6)
    subjects = ['Brats18_S_1', 'Brats18_T_1', 'Brats18_U_1']
    gt_dir, run_dir, truth = _tree(tmp_path, subjects, 'sigma', rng)
    gts = evalrun.collect_brats_ground_truth(gt_dir)
    entry = evalrun.get_eval_data('aleatoric', run_dir, gts, expected_subjects=subjects)
    assert entry.confidence_entry == 'sigma'
    base = str(tmp_path / 'eval')
    evalrun.evaluate_runs([entry], ['minmax'], base, '')        # the global rescale reads the file this writes
    evalrun.evaluate_runs([entry], ['calib', 'calib_curves'], base, '')
    actions = evalrun.get_actions(['calib', 'calib_curves'], os.path.join(base, evalrun.MINMAX_NAME), base, '')
    for a in actions:
        a.setup_eval(entry)
    assert not evalrun._fusable(entry, actions) and actions[0].id_ == actions[1].id_
    run_id = actions[1].id_
    rows = _rows(os.path.join(base, evalrun.CALIB_NAME, 'eval_calib_curves_{}.csv'.format(run_id)))
    bins = _rows(os.path.join(base, evalrun.CALIB_NAME, 'eval_calibration_{}.csv'.format(run_id)))
    assert [r['subject_name'] for r in rows] == sorted(subjects)
    for r, b in zip(rows, bins):      # the same prepared map as the 'calib' action's: its 10-bin ECE
        assert int(r['n']) == truth[r['subject_name']][0].size and abs(float(r['ece']) - float(b['ece'])) <= 1e-9
    assert len(_rows(os.path.join(base, evalrun.CALIB_NAME, 'eval_calib_levels_{}.csv'.format(run_id)))) == 1000
    (pooled,) = _rows(os.path.join(base, evalrun.CALIB_NAME, 'eval_calib_curves_pooled_{}.csv'.format(run_id)))
    assert int(pooled['n']) == sum(int(r['n']) for r in rows) and 0 <= float(pooled['brier']) <= 1
