"""The uncertainty level histogram on the GPU: rcu_unc_hist / rcu_unc_hist_from_p against the numpy definition and the reference-made counts
(fixtures G9, G22), against rcu_unc_counts, at the level boundaries, on native-size batches; SubjectBatch.metrics with 'ue_hist'; the
'ue_curves' evaluation action end to end (fused and plain loop, batch sizes, a 'sigma' run)."""
import csv
import glob
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_ue_curves_cpu import SCRIPT_THRESHOLDS, boundary_index, counts_at, levels_of, numpy_histogram

pytestmark = pytest.mark.gpu
LEVELS = (2, 20, 1000, 4096)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def levels_of_sorted(u, levels):
    """levels_of for large arrays: #{k : t_k < u} by binary search (NaN -> 0)."""
    bounds = np.arange(1, levels, dtype=np.float64) / np.float64(levels)
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    return np.where(np.isnan(u), 0, np.searchsorted(bounds, u, side='left')).astype(np.int64)


def fixture_volumes():
    g9, g22 = load_golden('g9_uncertainty'), load_golden('g22_ue_curves')
    out = [('g9', g9['prediction'], g9['target'], g9['uncertainty'], g9['mask'], g9['counts'], None)]
    for tag in 'abc':
        out.append(('g22' + tag, g22[tag + '_prediction'], g22[tag + '_target'], g22[tag + '_uncertainty'], g22[tag + '_mask'],
                    g22[tag + '_counts'][0], g22[tag + '_counts'][1]))
    return out


def test_binary_search_restatement_is_the_definition():
    g = load_golden('g22_ue_curves')
    for levels in LEVELS:
        assert np.array_equal(levels_of_sorted(g['c_uncertainty'], levels), levels_of(g['c_uncertainty'], levels))


@pytest.mark.parametrize('levels', LEVELS)
def test_histogram_equals_the_numpy_definition_on_the_fixtures(dev, levels):
    from rcu_amd import evaluation as ev
    for name, pr, tg, unc, mask, counts, masked_counts in fixture_volumes():
        for m in (None, mask):
            for dtype in (np.float64, np.float32):
                u = unc.astype(dtype)
                got = ev.uncertainty_histogram(pr, tg, u, levels, mask=m)
                assert got.dtype == np.uint64 and got.shape == (1, 4, levels)
                assert np.array_equal(got[0], numpy_histogram(pr, tg, u, levels, mask=m)), (name, levels, dtype, m is not None)
            # float64 map: the suffix sums are the reference's counts wherever the grid holds the script's threshold
            got = ev.uncertainty_histogram(pr, tg, unc, levels, mask=m)[0]
            ref = counts if m is None else masked_counts
            for i, thr in enumerate(SCRIPT_THRESHOLDS):
                k = boundary_index(thr, levels)
                if k is not None and ref is not None:
                    assert counts_at(got, k) == list(ref[i]), (name, levels, thr)
    g9 = load_golden('g9_uncertainty')
    if levels == 1000:
        got = ev.uncertainty_histogram(g9['prediction'], g9['target'], g9['uncertainty'], levels, mask=g9['mask'])[0]
        assert counts_at(got, 500) == list(g9['masked_counts_thr05'])


def test_suffix_sums_equal_unc_counts_on_a_ragged_batch(dev):
    """3 volumes of 1,000,003 voxels: an odd volume length (misaligned heads, ragged tails) beyond one workgroup's share; every launch
    geometry gives the same integers."""
    from rcu_amd import _lib, evaluation as ev
    rng = np.random.RandomState(7)
    v, n, levels = 3, 1000003, 1000
    unc = rng.rand(v, n)
    unc[:, ::7] = np.round(unc[:, ::7], 3)               # many values exactly on (or an ulp from) a boundary
    unc[0, :5] = [0.0, 1.0, np.nan, -1.0, 2.0]
    pr, tg = (rng.rand(v, n) < 0.5).astype(np.uint8), (rng.rand(v, n) < 0.3).astype(np.uint8) * 3
    mask = (rng.rand(v, n) < 0.7).astype(np.uint8)
    ks = (1, 2, 50, 100, 333, 500, 501, 750, 950, 997, 998, 999)
    thresholds = [k / levels for k in ks]
    so = _lib.load()
    try:
        for dtype in (np.float64, np.float32):
            u = unc.astype(dtype)
            for m in (None, mask):
                counts = ev.uncertainty_counts(pr, tg, u, thresholds, mask=m, n_volumes=v)
                hists = []
                for blocks in (0, 1, 3, 64):
                    _lib.check(so.rcu_unc_hist_set_blocks_per_workgroup(blocks))
                    hists.append(ev.uncertainty_histogram(pr, tg, u, levels, mask=m, n_volumes=v))
                for h in hists[1:]:
                    assert np.array_equal(h, hists[0])
                for vol in range(v):
                    for i, k in enumerate(ks):
                        assert counts_at(hists[0][vol], k) == list(counts[vol, i]), (dtype, vol, k)
        # the wide-workgroup form (B > 1365) on the same batch against the numpy definition
        got = ev.uncertainty_histogram(pr, tg, unc, 4096, mask=mask, n_volumes=v)
        for vol in range(v):
            keep = mask[vol] != 0
            level = levels_of_sorted(unc[vol][keep], 4096)
            cell = np.where(tg[vol][keep] != 0, np.where(pr[vol][keep] != 0, 0, 3), np.where(pr[vol][keep] != 0, 2, 1))
            assert np.array_equal(got[vol], np.bincount(cell * 4096 + level, minlength=4 * 4096).reshape(4, 4096).astype(np.uint64))
    finally:
        so.rcu_unc_hist_set_blocks_per_workgroup(0)


def test_every_boundary_value_lands_in_its_level(dev):
    """G22 (c)'s probe values, each as a volume of its own (one voxel: every head / tail case of the 16-byte path on the way)."""
    from rcu_amd import evaluation as ev
    g = load_golden('g22_ue_curves')
    special = g['c_uncertainty'].reshape(-1)[g['c_special_index']]
    expect = g['c_special_level']
    n = special.size
    zeros = np.zeros(n, dtype=np.uint8)
    got = ev.uncertainty_histogram(zeros, zeros, special, 1000, n_volumes=n)
    assert got.shape == (n, 4, 1000)
    assert np.array_equal(got.sum(axis=(1, 2)), np.ones(n, dtype=np.uint64))
    assert np.array_equal(got[:, 1, :].argmax(axis=1), expect)           # t_k -> k - 1, next above -> k, NaN and negative -> 0, above 1 -> B - 1
    assert np.array_equal(got[:, 1, :].max(axis=1), np.ones(n, dtype=np.uint64))
    # the same values in one volume, in the other grids
    for levels in (2, 20, 4096):
        got = ev.uncertainty_histogram(zeros, zeros, special, levels)[0]
        assert np.array_equal(got[1], np.bincount(levels_of(special, levels), minlength=levels).astype(np.uint64))


def _from_p_equals_map(ev, p, pr, tg, levels, mask=None, n_volumes=1):
    direct = ev.uncertainty_histogram_from_p(pr, tg, p, levels, mask=mask, n_volumes=n_volumes)
    via_map = ev.uncertainty_histogram(pr, tg, ev.normalised_entropy(p), levels, mask=mask, n_volumes=n_volumes)
    assert direct.shape == via_map.shape == (n_volumes, 4, levels)
    assert np.array_equal(direct, via_map)
    return direct


def peaked(rng, shape):
    """About 97 % of the voxels with p < 1e-4 or p > 1 - 1e-4 (the recipe of G22 (b))."""
    p = rng.rand(*shape).astype(np.float32)
    tiny = (rng.rand(*shape) * 1e-4).astype(np.float32)
    return np.where(rng.rand(*shape) < 0.97, np.where(rng.rand(*shape) < 0.9, tiny, np.float32(1) - tiny), p).astype(np.float32)


def test_from_p_equals_the_map_based_path(dev):
    from rcu_amd import evaluation as ev
    g = load_golden('g22_ue_curves')
    for tag in 'ab':
        for levels in LEVELS:
            for m in (None, g[tag + '_mask']):
                h = _from_p_equals_map(ev, g[tag + '_p'], g[tag + '_prediction'], g[tag + '_target'], levels, mask=m)
        # an EntropyOfProbability is routed to the from-p kernel
        routed = ev.uncertainty_histogram(g[tag + '_prediction'], g[tag + '_target'], ev.EntropyOfProbability(g[tag + '_p']), 4096, mask=g[tag + '_mask'])
        assert np.array_equal(routed, h)
    special = np.array([0.0, 1.0, 0.5, 1e-7, 0.999999, np.float32(1e-45)] + [np.nextafter(np.float32(0.5), np.float32(k)) for k in (0, 1)],
                       dtype=np.float32)
    assert special[5] > 0 and special[5] == np.finfo(np.float32).smallest_subnormal
    zeros = np.zeros(special.size, dtype=np.uint8)
    for levels in LEVELS:
        h = _from_p_equals_map(ev, special, zeros, zeros, levels, n_volumes=special.size)
        level = h[:, 1, :].argmax(axis=1)
        assert list(level[:2]) == [0, 0] and level[2] == levels - 1 and level[5] == 0       # entropy 0 at p = 0 and 1, 1 at p = 0.5
    # every float32 in a stretch around two boundaries of B = 1000 and at the ends of [0, 1]
    bits = np.concatenate([np.arange(0, 4096), np.arange(0x3F800000 - 4096, 0x3F800000 + 8),
                           np.arange(0x3DE00000, 0x3DE00000 + 65536), np.arange(0x3F000000 - 32768, 0x3F000000 + 32768)]).astype(np.uint32)
    p = bits.view(np.float32)
    zeros = np.zeros(p.size, dtype=np.uint8)
    for levels in (1000, 4096):
        _from_p_equals_map(ev, p, zeros, zeros, levels)


def test_from_p_on_native_size_batches(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(11)
    shape = (2, 155, 240, 240)
    tg = (rng.rand(*shape) < 0.3).astype(np.uint8)
    for name, p in (('peaked', peaked(rng, shape)), ('uniform', rng.rand(*shape).astype(np.float32))):
        pr = (p > 0.5).astype(np.uint8)
        for levels in (1000, 4096):
            h = _from_p_equals_map(ev, p, pr, tg, levels, n_volumes=2)
            assert [int(v) for v in h.sum(axis=(1, 2))] == [155 * 240 * 240] * 2
            if name == 'peaked':
                # p < 1e-4 has an entropy below 1.5e-3: the lowest two (B = 1000) / eight (B = 4096) levels hold nearly everything
                assert int(h[:, :, :levels // 500].sum()) > 0.9 * p.size
    # one native-size volume with every voxel identical: the single cell [tn][0] holds N exactly
    n = 155 * 240 * 240
    for levels in (1000, 4096):
        for p0 in (np.float32(1e-8), np.float32(0.0)):
            h = ev.uncertainty_histogram_from_p(torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev),
                                                torch.full((n,), float(p0), dtype=torch.float32, device=dev), levels)
            assert int(h[0, 1, 0]) == n and int(h.sum()) == n
        h = ev.uncertainty_histogram(torch.ones(n, dtype=torch.uint8, device=dev), torch.ones(n, dtype=torch.uint8, device=dev),
                                     torch.full((n,), 2.0, dtype=torch.float64, device=dev), levels)
        assert int(h[0, 0, levels - 1]) == n and int(h.sum()) == n


def test_subject_batch_metrics_with_the_level_histogram(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(3)
    count, n = 3, 24 * 24 * 24 + 5
    batch = ev.SubjectBatch(count, n, with_mask=True)
    subjects = []
    for slot in range(count):
        p = peaked(rng, (n,)) if slot else rng.rand(n).astype(np.float32)
        pr, tg, m = (p > 0.5).astype(np.uint8), (rng.rand(n) < 0.3).astype(np.uint8), (rng.rand(n) < 0.6).astype(np.uint8)
        batch.put(slot, p, pr, tg, m)
        subjects.append((p, pr, tg))
    batch.upload()
    plain = batch.metrics(want=('minmax', 'ece', 'ue'))
    more = batch.metrics(want=('minmax', 'ece', 'ue', 'ue_hist'))
    assert set(more) == set(plain) | {'ue_hist'} and 'ue_hist' not in plain
    for key in ('min', 'max', 'counts'):
        assert plain[key].dtype == more[key].dtype and plain[key].tobytes() == more[key].tobytes(), key
    for a, b in zip(plain['hist'], more['hist']):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert more['ue_hist'].dtype == np.uint64 and more['ue_hist'].shape == (count, 4, 1000)
    for slot, (p, pr, tg) in enumerate(subjects):        # no mask, like the 'ue' scan
        assert np.array_equal(more['ue_hist'][slot], ev.uncertainty_histogram_from_p(pr, tg, p)[0])
        for i, thr in enumerate(SCRIPT_THRESHOLDS):      # the base counts of the table-based scan of the same batch
            assert counts_at(more['ue_hist'][slot], boundary_index(thr, 1000))[:4] == list(more['counts'][slot, i, :4])
    assert batch.metrics(want=('ue_hist',), levels=64)['ue_hist'].shape == (count, 4, 64)


# ----------------------------------------------------------------------------------------------------------- end to end
def _all_csv(root):
    return {os.path.relpath(f, root): open(f, 'rb').read() for f in sorted(glob.glob(os.path.join(root, '**', '*.csv'), recursive=True))}


def _rows(path):
    with open(path, newline='') as f:
        return list(csv.DictReader(f))


def _tree(tmp_path, subjects, entry_name, rng, shape=(6, 16, 16)):
    """A tiny BraTS-style tree: ground truth under gt/HGG/<subject>/, predictions + the run's confidence entry under pred/."""
    from rcu_amd import nifti
    gt_root, run_dir = tmp_path / 'gt' / 'HGG', tmp_path / ('pred_' + entry_name)
    run_dir.mkdir(parents=True)
    truth = {}
    for sub in subjects:
        (gt_root / sub).mkdir(parents=True, exist_ok=True)
        t2 = (rng.rand(*shape) * (rng.rand(*shape) > 0.3)).astype(np.float32)
        seg = (rng.rand(*shape) < 0.3).astype(np.uint8) * rng.randint(1, 5, shape).astype(np.uint8)
        if entry_name == 'probabilities':
            conf = rng.rand(*shape).astype(np.float32)
            pred = (conf > 0.5).astype(np.uint8)
        else:
            conf = (rng.rand(*shape).astype(np.float32) * 2.5 + 0.1)
            pred = (rng.rand(*shape) > 0.5).astype(np.uint8)
        for mod, arr in (('flair', t2), ('t1', t2), ('t2', t2), ('t1ce', t2), ('seg', seg)):
            nifti.write(str(gt_root / sub / '{}_{}.nii.gz'.format(sub, mod)), arr)
        nifti.write(str(run_dir / '{}_{}.nii.gz'.format(sub, entry_name)), conf)
        nifti.write(str(run_dir / '{}_prediction.nii.gz'.format(sub)), pred)
        truth[sub] = (conf, pred, (seg > 0).astype(np.uint8))
    return str(tmp_path / 'gt'), str(run_dir), truth


def test_ue_curves_action_end_to_end(dev, tmp_path):
    from rcu_amd import evalrun, evaluation as ev
    rng = np.random.RandomState(5)
    subjects = ['Brats18_{}_1'.format(c) for c in 'ABCDEFGHI']
    gt_dir, run_dir, truth = _tree(tmp_path, subjects, 'probabilities', rng)
    gts = evalrun.collect_brats_ground_truth(gt_dir)
    entry = evalrun.get_eval_data('baseline_mc', run_dir, gts, expected_subjects=subjects)
    old, new = ['minmax', 'ece_dice', 'calib', 'bnf_ue'], ['minmax', 'ece_dice', 'calib', 'bnf_ue', 'ue_curves']
    base = str(tmp_path / 'eval')
    evalrun.evaluate_runs([entry], new, base, 'foreground')
    fused = _all_csv(base)
    ue_files = {k: v for k, v in fused.items() if os.path.basename(k).startswith('eval_ue_')}
    assert sorted(os.path.basename(k) for k in ue_files) == ['eval_ue_curves_baseline_mc.csv', 'eval_ue_curves_pooled_baseline_mc.csv',
                                                             'eval_ue_levels_baseline_mc.csv']
    assert all(os.path.dirname(k) == evalrun.UNCERTAINTY_NAME for k in ue_files) and len(fused) == 14 + 3
    # the plain loop and every batch size write the same bytes
    for tag, kwargs in (('plain', dict(fused=False)), ('b1', dict(batch_subjects=1)), ('b3', dict(batch_subjects=3)), ('b8', dict(batch_subjects=8))):
        other = str(tmp_path / ('eval_' + tag))
        evalrun.evaluate_runs([entry], new, other, 'foreground', **kwargs)
        assert _all_csv(other) == fused, tag
    # the four old actions' files do not feel the new one
    without = str(tmp_path / 'eval_old')
    evalrun.evaluate_runs([entry], old, without, 'foreground')
    assert _all_csv(without) == {k: v for k, v in fused.items() if k not in ue_files}
    # the action alone, and another number of levels
    alone = str(tmp_path / 'eval_alone')
    evalrun.evaluate_runs([entry], ['ue_curves'], alone, 'foreground')
    assert _all_csv(alone) == ue_files
    # contents: per-subject rows, the pooled row, the levels file
    rows = _rows(os.path.join(base, 'uncertainty', 'eval_ue_curves_baseline_mc.csv'))
    assert [r['subject_name'] for r in rows] == sorted(subjects)
    assert list(rows[0]) == ['test_id', 'subject_name'] + list(ev.UE_CURVE_KEYS)
    pooled = np.zeros((4, 1000), dtype=np.uint64)
    for r in rows:
        conf, pred, tgt = truth[r['subject_name']]
        h = ev.uncertainty_histogram_from_p(pred, tgt, conf)[0]
        pooled += h
        expect = ev.ue_curve_metrics(h)
        assert {k: r[k] for k in ev.UE_CURVE_KEYS} == {k: str(v) for k, v in expect.items()}
        assert int(r['n']) == conf.size and int(r['n_errors']) == int((pred != tgt).sum())
    (row,) = _rows(os.path.join(base, 'uncertainty', 'eval_ue_curves_pooled_baseline_mc.csv'))
    assert {k: row[k] for k in ev.UE_CURVE_KEYS} == {k: str(v) for k, v in ev.ue_curve_metrics(pooled).items()} and row['test_id'] == 'baseline_mc'
    levels = _rows(os.path.join(base, 'uncertainty', 'eval_ue_levels_baseline_mc.csv'))
    assert list(levels[0]) == ['level', 'threshold', 'tp', 'tn', 'fp', 'fn'] and len(levels) == 1000
    assert [int(r['level']) for r in levels] == list(range(1000)) and [float(r['threshold']) for r in levels] == [k / 1000 for k in range(1000)]
    assert np.array_equal(np.array([[int(r[c]) for r in levels] for c in ('tp', 'tn', 'fp', 'fn')], dtype=np.uint64), pooled)
    # the pooled files do not depend on the subject order either
    entry_rev = evalrun.get_eval_data('baseline_mc', run_dir, gts, expected_subjects=subjects)
    entry_rev.subject_files = entry_rev.subject_files[::-1]
    rev = str(tmp_path / 'eval_rev')
    evalrun.evaluate_runs([entry_rev], ['ue_curves'], rev, 'foreground', batch_subjects=4)
    for name in ('eval_ue_curves_pooled_baseline_mc.csv', 'eval_ue_levels_baseline_mc.csv'):
        assert _all_csv(rev)[os.path.join('uncertainty', name)] == fused[os.path.join('uncertainty', name)]
    few = str(tmp_path / 'eval_64')
    evalrun.evaluate_runs([entry], ['ue_curves'], few, 'foreground', levels=64)
    assert len(_rows(os.path.join(few, 'uncertainty', 'eval_ue_levels_baseline_mc.csv'))) == 64


def test_ue_curves_action_on_a_sigma_run(dev, tmp_path):
    """The map-based path: a 'sigma' run is rescaled with the run's global min / max (written by the minmax action) before it is binned."""
    from rcu_amd import evalrun, evaluation as ev
    rng = np.random.RandomState(6)
    subjects = ['Brats18_S_1', 'Brats18_T_1', 'Brats18_U_1']
    gt_dir, run_dir, truth = _tree(tmp_path, subjects, 'sigma', rng)
    gts = evalrun.collect_brats_ground_truth(gt_dir)
    entry = evalrun.get_eval_data('aleatoric', run_dir, gts, expected_subjects=subjects)
    assert entry.confidence_entry == 'sigma'
    base = str(tmp_path / 'eval')
    evalrun.evaluate_runs([entry], ['minmax'], base, 'foreground')        # the global rescale reads the file this writes
    evalrun.evaluate_runs([entry], ['ue_curves'], base, 'foreground')
    mm = evalrun.read_min_max(os.path.join(base, 'minmax', 'eval_summary_minmax_aleatoric.csv'))
    rows = _rows(os.path.join(base, 'uncertainty', 'eval_ue_curves_aleatoric_globalrescale.csv'))
    assert [r['subject_name'] for r in rows] == sorted(subjects)
    pooled = np.zeros((4, 1000), dtype=np.uint64)
    for r in rows:
        sigma, pred, tgt = truth[r['subject_name']]
        prepared = ev.rescale_uncertainties(sigma, mm[0], mm[1])
        h = numpy_histogram(pred, tgt, prepared, 1000)
        pooled += h
        expect = ev.ue_curve_metrics(h)
        assert float(r['auroc']) == expect['auroc'] and float(r['aurc']) == expect['aurc'] and int(r['n_errors']) == expect['n_errors']
    (row,) = _rows(os.path.join(base, 'uncertainty', 'eval_ue_curves_pooled_aleatoric_globalrescale.csv'))
    assert float(row['auroc']) == ev.ue_curve_metrics(pooled)['auroc']
    assert os.path.exists(os.path.join(base, 'uncertainty', 'eval_ue_levels_aleatoric_globalrescale.csv'))
    shutil.rmtree(base)
