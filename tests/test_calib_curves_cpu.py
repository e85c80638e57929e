"""The calibration level histogram and the metrics derived from it without a GPU: the thresholds and the C ABI's argument checks, the
definition restated in numpy and pinned to the reference's reliability histograms and to scikit-learn's Brier score and isotonic fit
(fixture G26), the identities of `calibration_curve_metrics`, and the evaluation action's registration."""
import csv
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('rcu_calib_curve_thresholds', 'rcu_calib_curve_workspace_bytes', 'rcu_calib_curve', 'rcu_calib_curve_terms',
         'rcu_calib_curve_set_blocks_per_workgroup')
CASES = ('a', 'b', 'c')
SELECTIONS = ('nomask', 'masked')
Q_ONE = 1 << 32
# Sums of at most about 2 B float64 terms in [0, 1] on both sides; 2 * 4096 * 2^-53 < 1e-12: rounding, not slack.
TOL = 1e-12
# The confidence sums of the level histogram are off by at most 2^-33 per voxel (Q(p) = rint(p * 2^32)), the Brier score by three such
# roundings per voxel (Q of class 1, Q2 of both classes): below 4e-10 on the mean, whatever the number of voxels.
TOL_FIXED = 1e-9


# --------------------------------------------------------------------------------------- the definition, in plain numpy
def numpy_thresholds(levels):
    """t_k, k = 1..levels-1: the smallest float32 >= k * ((1 + 1e-8) / levels) -- the edges of np.linspace(0, 1 + 1e-8, levels + 1)."""
    edges = np.arange(1, levels, dtype=np.float64) * ((1.0 + 1e-8) / levels)
    t = edges.astype(np.float32)
    low = t.astype(np.float64) < edges
    t[low] = np.nextafter(t[low], np.float32(2.0))
    return t


def numpy_levels_of(p, levels):
    """level(p) = #{k : p >= t_k}; NaN compares false: level 0."""
    p = np.asarray(p, dtype=np.float32).reshape(-1)
    return np.where(np.isnan(p), 0, np.searchsorted(numpy_thresholds(levels), p, side='right')).astype(np.int64)


def fixed_q(x):
    """rint(x * 2^32) of float64 x in [0, 1], ties to even, as uint64."""
    return np.rint(x * 4294967296.0).astype(np.uint64)


def numpy_calibration_levels(p, target, levels, mask=None):
    """-> (levels uint64 [3, B], totals uint64 [2, 3]: n_y, sum Q, sum Q2 per class) by the definition of include/rcu.h, rcu_calib_curve."""
    p = np.asarray(p, dtype=np.float32).reshape(-1)
    y = np.asarray(target).reshape(-1) != 0
    level = numpy_levels_of(p, levels)
    with np.errstate(invalid='ignore'):
        c = np.clip(np.where(np.isnan(p), 0.0, p.astype(np.float64)), 0.0, 1.0)
    q, q2 = fixed_q(c), fixed_q(c * c)
    if mask is not None:
        keep = np.asarray(mask).reshape(-1) != 0
        y, level, q, q2 = y[keep], level[keep], q[keep], q2[keep]
    out = np.zeros((3, levels), dtype=np.uint64)
    out[0] = np.bincount(level[~y], minlength=levels)
    out[1] = np.bincount(level[y], minlength=levels)
    np.add.at(out[2], level, q)
    totals = np.array([[int(sel.sum()), int(q[sel].sum(dtype=np.uint64)), int(q2[sel].sum(dtype=np.uint64))] for sel in (~y, y)], dtype=np.uint64)
    return out, totals


def with_nll(totals3):
    """[2, 3] totals -> [2, 4] with a zero NLL sum (the NLL needs the device's logf: tests/test_gpu_calib_curves.py)."""
    return np.concatenate([np.asarray(totals3, dtype=np.uint64), np.zeros((2, 1), dtype=np.uint64)], axis=1)


def fixture_case(tag, sel):
    g = load_golden('g26_calib_curves')
    return g, g[tag + '_p'], g[tag + '_target'], (g[tag + '_mask'] if sel == 'masked' else None)


# ------------------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope='module')
def lib():
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    return _lib


def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, 'include', 'rcu.h')).read()
    declared = set(re.findall(r'\b(rcu_[a-z0-9_]+)\s*\(', header))
    so = lib.load()
    for name in NAMES:
        assert name in declared and name in lib.SIGNATURES and hasattr(so, name), name
    assert 'RCU_CALIB_CURVE_MAX_LEVELS 4096' in header and lib.RCU_CALIB_CURVE_MAX_LEVELS == 4096
    assert 'rcu_calib_curve.hip' in open(os.path.join(os.path.dirname(lib.__file__), 'csrc', 'Makefile')).read()


@pytest.mark.parametrize('levels,bins', [(1000, 10), (1000, 20), (1000, 500), (20, 10), (30, 15), (1365, 5), (1366, 2), (4096, 2), (4096, 32), (4095, 1365)])
def test_thresholds_of_a_divisor_are_thresholds_of_the_levels(lib, levels, bins):
    """t_{k B / n} of B levels is bit-equal to t_k of n bins: merging B / n consecutive levels gives the n-bin histogram for every float32 p."""
    fine, coarse = numpy_thresholds(levels), numpy_thresholds(bins)
    assert fine.dtype == np.float32 and fine.size == levels - 1 and np.all(np.diff(fine) > 0)
    assert np.array_equal(fine[levels // bins - 1::levels // bins].view(np.uint32), coarse.view(np.uint32))
    # the library's host function is the restatement, and for n <= 32 the existing rcu_ece_thresholds
    assert np.array_equal(np.array(lib.calib_curve_thresholds(levels)[:levels - 1], dtype=np.float32).view(np.uint32), fine.view(np.uint32))
    if bins <= lib.RCU_MAX_BINS and bins > 1:
        assert np.array_equal(np.array(lib.ece_thresholds(bins)[:bins - 1], dtype=np.float32).view(np.uint32), coarse.view(np.uint32))


def test_thresholds_equal_the_ece_thresholds_up_to_32_bins(lib):
    for levels in range(2, lib.RCU_MAX_BINS + 1):
        assert list(lib.calib_curve_thresholds(levels)[:levels - 1]) == list(lib.ece_thresholds(levels)[:levels - 1]), levels
    # p = 0.5 sits in level 499 of 1000 and in bin 4 of 10, p = 1 in the last level, NaN and negatives in level 0
    probe = np.array([0.5, 1.0, np.nan, -1.0, 0.0, 2.0], dtype=np.float32)
    assert list(numpy_levels_of(probe, 1000)) == [499, 999, 0, 0, 0, 999] and list(numpy_levels_of(probe, 10)) == [4, 9, 0, 0, 0, 9]


def test_argument_validation_without_gpu(lib):
    so = lib.load()
    p, tg, m, out, tot, ws = (ctypes.c_void_p(v) for v in (1 << 20, 1 << 24, 1 << 25, 1 << 26, 1 << 30, 1 << 31))

    def refused(status, *words):
        assert status == -1        # RCU_ERR_INVALID
        msg = so.rcu_last_error()
        for w in words:
            assert w in msg, (w, msg)

    def scan(p_=p, target=tg, mask=None, n=1000, v=2, levels=1000, o=out, t=tot, w=ws):
        return so.rcu_calib_curve(p_, target, mask, n, v, levels, o, t, w, None)

    def terms(p_=p, target=tg, n=1000, levels=1000, lv=out, nl=tot):
        return so.rcu_calib_curve_terms(p_, target, n, levels, lv, nl, None)

    name = b'rcu_calib_curve:'
    for levels in (1, 0, -5, 4097, 1 << 20):
        refused(scan(levels=levels), name, b'levels')
        refused(terms(levels=levels), b'rcu_calib_curve_terms:', b'levels')
        refused(so.rcu_calib_curve_thresholds(levels, (ctypes.c_float * 8)()), b'rcu_calib_curve_thresholds:', b'levels')
    refused(scan(None), name, b'null', b'p_foreground_dev')
    refused(scan(target=None), name, b'null', b'target_dev')
    refused(scan(o=None), name, b'null', b'levels_dev')
    refused(scan(t=None), name, b'null', b'totals_dev')
    refused(scan(w=None), name, b'null', b'workspace_dev')
    refused(scan(n=0), name, b'n_per_volume')
    for v in (0, -1, 65536):
        refused(scan(v=v), name, b'n_volumes')
    refused(scan(None, levels=1), name, b'levels')      # levels are judged first, with every other argument bad as well
    refused(terms(None), b'rcu_calib_curve_terms:', b'null', b'p_foreground_dev')
    refused(terms(target=None), b'rcu_calib_curve_terms:', b'null', b'target_dev')
    refused(terms(lv=None), b'rcu_calib_curve_terms:', b'null', b'level_dev')
    refused(terms(nl=None), b'rcu_calib_curve_terms:', b'null', b'nll_dev')
    refused(terms(n=0), b'rcu_calib_curve_terms:', b'n must')
    refused(so.rcu_calib_curve_thresholds(10, None), b'rcu_calib_curve_thresholds:', b'null')
    refused(so.rcu_calib_curve_set_blocks_per_workgroup(-1), b'negative')
    for levels in (2, 1000, 4096):
        assert so.rcu_calib_curve_workspace_bytes(155 * 240 * 240, 8, levels) >= 4 * (levels + 1)
    assert so.rcu_calib_curve_workspace_bytes(1000, 1, 1) == 0 and so.rcu_calib_curve_workspace_bytes(1000, 1, 4097) == 0


# ------------------------------------------------------------------------------- the restatement against the yardsticks
@pytest.mark.parametrize('sel', SELECTIONS)
@pytest.mark.parametrize('tag', CASES)
def test_merged_levels_are_the_reference_histogram(tag, sel):
    from rcu_amd import evaluation as ev
    g, p, target, mask = fixture_case(tag, sel)
    levels, totals = numpy_calibration_levels(p, target, 1000, mask)
    n = p.size if mask is None else int(np.count_nonzero(mask))
    assert int(levels[:2].sum()) == n == int(totals[:, 0].sum()) and int(levels[2].sum()) == int(totals[:, 1].sum())
    for bins in (10, 20):
        merged = levels[:2].sum(axis=0).reshape(bins, -1).sum(axis=1)
        non_zero = g['{}_bins_non_zero{}_{}'.format(tag, bins, sel)]
        assert np.array_equal(merged != 0, non_zero)
        assert np.array_equal(merged[non_zero].astype(np.int64), g['{}_bins_count{}_{}'.format(tag, bins, sel)])
        positives = levels[1].reshape(bins, -1).sum(axis=1)[non_zero]
        assert np.array_equal(positives / merged[non_zero], g['{}_bins_positive_fraction{}_{}'.format(tag, bins, sel)])
        got = ev.calibration_curve_metrics(levels, with_nll(totals), bins=bins)
        ref = float(g['{}_ece{}_{}'.format(tag, bins, sel)])
        print(tag, sel, bins, 'ece', got['ece'], 'reference', ref, 'difference', got['ece'] - ref)
        assert abs(got['ece'] - ref) <= TOL_FIXED
        gaps = np.abs(g['{}_bins_avg_confidence{}_{}'.format(tag, bins, sel)] - g['{}_bins_positive_fraction{}_{}'.format(tag, bins, sel)])
        assert abs(got['mce'] - gaps.max()) <= TOL_FIXED
    # other grids contain the same histograms
    for fine in (20, 4096 // 4 * 5, 4000):
        other, _ = numpy_calibration_levels(p, target, fine, mask)
        assert np.array_equal(other[:2].sum(axis=0).reshape(10, -1).sum(axis=1), levels[:2].sum(axis=0).reshape(10, -1).sum(axis=1))


@pytest.mark.parametrize('sel', SELECTIONS)
@pytest.mark.parametrize('tag', CASES)
def test_brier_score_matches_scikit_learn(tag, sel):
    from rcu_amd import evaluation as ev
    g, p, target, mask = fixture_case(tag, sel)
    levels, totals = numpy_calibration_levels(p, target, 1000, mask)
    got = ev.calibration_curve_metrics(levels, with_nll(totals))
    ref = float(g['{}_brier_{}'.format(tag, sel)])
    print(tag, sel, 'brier', got['brier'], 'scikit-learn', ref, 'difference', got['brier'] - ref)
    assert abs(got['brier'] - ref) <= TOL_FIXED
    keep = np.ones(p.size, dtype=bool) if mask is None else mask.reshape(-1)
    y, q = target.reshape(-1)[keep].astype(np.float64), p.reshape(-1)[keep].astype(np.float64)
    assert got['n'] == y.size and got['n_pos'] == int(y.sum())
    assert abs(got['bias'] - (q.mean() - y.mean())) <= TOL_FIXED and got['nll'] == 0.0


@pytest.mark.parametrize('sel', SELECTIONS)
@pytest.mark.parametrize('tag', CASES)
def test_isotonic_map_matches_scikit_learn(tag, sel):
    from rcu_amd import evaluation as ev
    g, p, target, mask = fixture_case(tag, sel)
    levels, totals = numpy_calibration_levels(p, target, 1000, mask)
    got = ev.isotonic_levels(levels)
    filled = g['{}_isotonic_levels_{}'.format(tag, sel)]
    assert got.shape == (1000,) and got.dtype == np.float64 and np.all(np.diff(got) >= 0) and got.min() >= 0 and got.max() <= 1
    assert np.array_equal(np.flatnonzero(levels[:2].sum(axis=0)), filled)
    ref = g['{}_isotonic_{}'.format(tag, sel)]
    assert np.abs(got[filled] - ref[filled]).max() <= TOL
    # an empty level takes the value of the nearest non-empty level below, leading empty levels the first value
    below = np.searchsorted(filled, np.arange(1000), side='right') - 1
    assert np.array_equal(got, got[filled][np.maximum(below, 0)])
    # a run's own map: the Brier score of the isotonic predictions
    recal = ev.calibration_curve_metrics(levels, with_nll(totals), recalibration=got)
    assert abs(recal['brier_recal'] - float(g['{}_isotonic_brier_{}'.format(tag, sel)])) <= TOL
    assert list(recal) == list(ev.CALIB_CURVE_KEYS + ev.CALIB_RECAL_KEYS)
    assert recal['ece_recal'] <= TOL       # the isotonic fit is calibrated on its own data: every pooled block's value is its positive fraction
    assert {k: recal[k] for k in ev.CALIB_CURVE_KEYS} == ev.calibration_curve_metrics(levels, with_nll(totals))
    gc = np.clip(got, 2.0 ** -23, 1 - 2.0 ** -23)
    n0, n1 = levels[0].astype(np.float64), levels[1].astype(np.float64)
    assert abs(recal['nll_recal'] + (n1 * np.log(gc) + n0 * np.log1p(-gc)).sum() / (n0.sum() + n1.sum())) <= 1e-9 * max(1.0, recal['nll_recal'])


def test_isotonic_pools_violators_and_fills_gaps():
    from rcu_amd import evaluation as ev
    levels = np.zeros((3, 8), dtype=np.uint64)
    levels[0] = [0, 1, 0, 1, 3, 0, 0, 0]
    levels[1] = [0, 1, 0, 0, 1, 0, 4, 0]       # positive fractions 1/2, 0, 1/4, 1 at levels 1, 3, 4, 6
    assert list(ev.isotonic_levels(levels)) == [2 / 7] * 6 + [1.0, 1.0]      # the first three pool to (1 + 0 + 1) / (2 + 1 + 4)
    assert np.all(np.isnan(ev.isotonic_levels(np.zeros((3, 8), dtype=np.uint64))))
    with pytest.raises(ValueError):
        ev.isotonic_levels(np.zeros((4, 8), dtype=np.uint64))


@pytest.mark.parametrize('tag', CASES)
def test_murphy_decomposition_is_the_brier_score_of_the_level_mean_forecast(tag):
    from rcu_amd import evaluation as ev
    g, p, target, mask = fixture_case(tag, 'masked')
    for levels_n in (10, 1000):
        levels, totals = numpy_calibration_levels(p, target, levels_n, mask)
        got = ev.calibration_curve_metrics(levels, with_nll(totals), bins=10)
        keep = mask.reshape(-1)
        y, level = target.reshape(-1)[keep].astype(np.float64), numpy_levels_of(p, levels_n)[keep]
        n_l = levels[:2].sum(axis=0).astype(np.float64)
        forecast = np.divide(levels[2].astype(np.float64) / Q_ONE, n_l, out=np.zeros(levels_n), where=n_l > 0)
        brier_of_means = np.mean((forecast[level] - y) ** 2)
        assert abs(got['brier_reliability'] - got['brier_resolution'] + got['brier_uncertainty'] - brier_of_means) <= TOL
        assert got['brier_reliability'] >= 0 and got['brier_resolution'] >= 0 and abs(got['brier_uncertainty'] - y.mean() * (1 - y.mean())) <= TOL


def test_equal_mass_and_ks_against_voxelwise_restatements():
    """On a map whose every voxel has a level of its own the level-resolution definitions are the voxel-wise ones."""
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(4)
    levels_n, n = 4096, 500
    p = ((rng.permutation(levels_n)[:n] + 0.5) / levels_n).astype(np.float32)
    target = (rng.rand(n) < p).astype(np.uint8)
    levels, totals = numpy_calibration_levels(p, target, levels_n)
    assert levels[:2].sum(axis=0).max() == 1
    for mass_bins in (1, 7, 10, 500):
        got = ev.calibration_curve_metrics(levels, with_nll(totals), bins=2, mass_bins=mass_bins)
        order = np.argsort(p)
        q, y = p[order].astype(np.float64), target[order].astype(np.float64)
        groups = np.minimum(mass_bins - 1, (mass_bins * np.arange(n)) // n)
        ace = sum(abs((q[groups == b] - y[groups == b]).sum()) for b in range(mass_bins)) / n
        assert abs(got['ace'] - ace) <= TOL_FIXED
        assert abs(got['ks'] - np.abs(np.cumsum(q - y)).max() / n) <= TOL_FIXED
    one = ev.calibration_curve_metrics(levels, with_nll(totals), bins=1, mass_bins=1)
    assert abs(one['ace'] - abs(one['bias'])) <= TOL and abs(one['ece'] - abs(one['bias'])) <= TOL_FIXED and one['ks'] >= one['ace'] - TOL


def test_an_empty_selection_gives_nan_not_an_exception():
    from rcu_amd import evaluation as ev
    levels, totals = np.zeros((3, 1000), dtype=np.uint64), np.zeros((2, 4), dtype=np.uint64)
    for recal in (None, np.linspace(0, 1, 1000)):
        got = ev.calibration_curve_metrics(levels, totals, recalibration=recal)
        assert got['n'] == 0 and got['n_pos'] == 0
        assert all(math.isnan(v) for k, v in got.items() if k not in ('n', 'n_pos'))
        assert list(got) == list(ev.CALIB_CURVE_KEYS + (ev.CALIB_RECAL_KEYS if recal is not None else ()))
    # one class only: everything is defined
    p = np.array([0.25, 0.75], dtype=np.float32)
    levels, totals = numpy_calibration_levels(p, np.zeros(2, dtype=np.uint8), 10)
    got = ev.calibration_curve_metrics(levels, with_nll(totals))
    assert got['brier'] == (0.0625 + 0.5625) / 2 and got['brier_uncertainty'] == 0.0 and got['bias'] == 0.5 and not any(math.isnan(v) for v in got.values())
    for bad in (dict(bins=3), dict(bins=0), dict(mass_bins=0), dict(recalibration=np.zeros(11))):
        with pytest.raises(ValueError):
            ev.calibration_curve_metrics(levels, with_nll(totals), **bad)
    with pytest.raises(ValueError):
        ev.calibration_curve_metrics(levels, np.zeros((2, 4), dtype=np.uint64))       # totals of other voxels than the histogram's


def test_pooled_metrics_do_not_depend_on_the_order_of_addition():
    from rcu_amd import evaluation as ev
    parts = []
    for tag in CASES:
        for sel in SELECTIONS:
            _, p, target, mask = fixture_case(tag, sel)
            levels, totals = numpy_calibration_levels(p, target, 1000, mask)
            totals = with_nll(totals)
            totals[:, 3] = totals[:, 0] * np.uint64(12345)
            parts.append((levels.astype(object) << 31, totals.astype(object) << 31))      # beyond 2^63: Python integers throughout
    rows = []
    for order in (range(len(parts)), reversed(range(len(parts))), (3, 0, 5, 1, 4, 2)):
        levels, totals = np.zeros((3, 1000), dtype=object), np.zeros((2, 4), dtype=object)
        for i in order:
            levels, totals = levels + parts[i][0], totals + parts[i][1]
        assert int(levels[2].sum()) > 1 << 64
        rows.append(ev.calibration_curve_metrics(levels, totals, bins=20, mass_bins=15))
    assert rows[0] == rows[1] == rows[2]
    # scaling every integer leaves the ratios where they were: the pooled arithmetic does not overflow or lose the integers
    small = [np.sum([part[k] >> 31 for part in parts], axis=0) for k in (0, 1)]
    unscaled = ev.calibration_curve_metrics(small[0], small[1], bins=20, mass_bins=15)
    for key in ('brier', 'nll', 'bias', 'ece', 'mce', 'ace', 'ks'):
        assert abs(rows[0][key] - unscaled[key]) <= TOL, key


# ------------------------------------------------------------------------------------------------------- the action
def _levels_file(path, levels):
    from rcu_amd import evalrun
    with open(path, 'w', newline='') as f:
        writer = csv.writer(f)
        writer.writerow(evalrun.CALIB_LEVELS_COLUMNS)
        for level in range(levels):
            writer.writerow([level, level / levels, 1, 1, 0.5, 0.5, level / (levels - 1)])


def test_action_is_registered_and_not_a_default(tmp_path):
    from rcu_amd import evalrun, evaluation as ev
    base = str(tmp_path / 'eval')
    (action,) = evalrun.get_actions(['calib_curves'], os.path.join(base, evalrun.MINMAX_NAME), base, 'foreground')
    assert isinstance(action, evalrun.CalibCurvesAction) and action.need_mask and (action.levels, action.calib_bins, action.mass_bins) == (1000, 10, 10)
    assert action.out_dir == os.path.join(base, evalrun.CALIB_NAME) and os.path.isdir(action.out_dir)
    assert action.recalibration is None and tuple(action.keys) == ev.CALIB_CURVE_KEYS
    actions = evalrun.get_actions(['minmax', 'calib_curves'], os.path.join(base, evalrun.MINMAX_NAME), base, '', levels=64, calib_bins=16, mass_bins=5)
    assert [type(a).__name__ for a in actions] == ['SaveMinMaxAction', 'CalibCurvesAction']
    assert not actions[1].need_mask and (actions[1].levels, actions[1].calib_bins, actions[1].mass_bins) == (64, 16, 5)
    default = evalrun.get_actions(['minmax', 'ece_dice', 'calib', 'bnf_ue'], os.path.join(base, evalrun.MINMAX_NAME), base, '')
    assert not any(isinstance(a, evalrun.CalibCurvesAction) for a in default)
    source = open(os.path.join(ROOT, 'bin-eval', 'eval_uncertainty.py')).read()
    for flag in ('--calib_bins', '--mass_bins', '--recalibrate_from'):
        assert flag in source


def test_action_refuses_bins_that_do_not_divide_the_levels(tmp_path):
    from rcu_amd import evalrun
    base = str(tmp_path / 'eval')
    for levels, bins in ((1000, 3), (1000, 0), (64, 10), (10, 20)):
        with pytest.raises(ValueError):
            evalrun.get_actions(['calib_curves'], os.path.join(base, evalrun.MINMAX_NAME), base, '', levels=levels, calib_bins=bins)
    for levels in (1, 4097):
        with pytest.raises(ValueError):
            evalrun.get_actions(['calib_curves'], os.path.join(base, evalrun.MINMAX_NAME), base, '', levels=levels, calib_bins=1)
    with pytest.raises(ValueError):
        evalrun.get_actions(['calib_curves'], os.path.join(base, evalrun.MINMAX_NAME), base, '', mass_bins=0)
    # the other actions do not look at the option
    evalrun.get_actions(['ue_curves'], os.path.join(base, evalrun.MINMAX_NAME), base, '', calib_bins=3)


def test_action_refuses_a_recalibration_file_of_another_level_count(tmp_path):
    from rcu_amd import evalrun, evaluation as ev
    base = str(tmp_path / 'eval')
    path = str(tmp_path / 'eval_calib_levels_validation.csv')
    _levels_file(path, 64)
    with pytest.raises(ValueError, match='levels'):
        evalrun.get_actions(['calib_curves'], os.path.join(base, evalrun.MINMAX_NAME), base, '', recalibrate_from=path)
    (action,) = evalrun.get_actions(['calib_curves'], os.path.join(base, evalrun.MINMAX_NAME), base, '', levels=64, calib_bins=8, recalibrate_from=path)
    assert np.array_equal(action.recalibration, np.arange(64) / 63) and tuple(action.keys) == ev.CALIB_CURVE_KEYS + ev.CALIB_RECAL_KEYS
