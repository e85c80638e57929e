"""The uncertainty level histogram and the threshold-free uncertainty-error metrics without a GPU: the C ABI's argument checks, the
definition of a level restated in numpy and pinned to the reference-made counts (fixtures G9, G22), `ue_curve_metrics` against
scikit-learn's stored values and against voxel-wise restatements, and the evaluation action's registration."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('rcu_unc_hist_workspace_bytes', 'rcu_unc_hist', 'rcu_unc_hist_from_p')
SCRIPT_THRESHOLDS = (0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95)
# Both sides of a metric comparison are sums of at most about 2 B float64 terms in [0, 1]; 2 * 4096 * 2^-53 < 1e-12: rounding, not slack.
TOL = 1e-12


# --------------------------------------------------------------------------------------- the definition, in plain numpy
def levels_of(u, levels):
    """level(u) = #{k in 1..levels-1 : u > t_k}, t_k = (double)k / (double)levels, compared in float64; NaN compares false."""
    bounds = np.arange(1, levels, dtype=np.float64) / np.float64(levels)
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    with np.errstate(invalid='ignore'):
        return (u[:, None] > bounds[None, :]).sum(axis=1).astype(np.int64)


def cells_of(prediction, target):
    pr, tg = np.asarray(prediction).reshape(-1) != 0, np.asarray(target).reshape(-1) != 0
    return np.where(tg, np.where(pr, 0, 3), np.where(pr, 2, 1))      # tp 0, tn 1, fp 2, fn 3


def numpy_histogram(prediction, target, uncertainty, levels, mask=None):
    cell, level = cells_of(prediction, target), levels_of(uncertainty, levels)
    if mask is not None:
        keep = np.asarray(mask).reshape(-1) != 0
        cell, level = cell[keep], level[keep]
    return np.bincount(cell * levels + level, minlength=4 * levels).reshape(4, levels).astype(np.uint64)


def counts_at(hist, k):
    """tp, tn, fp, fn, tpu, tnu, fpu, fnu for the threshold t_k: base counts = row sums, uncertain = the sums over the levels >= k."""
    h = np.asarray(hist).astype(np.int64)
    return list(h.sum(axis=1)) + list(h[:, k:].sum(axis=1))


def boundary_index(thr, levels):
    """k with t_k == thr exactly (the script's literal IS the boundary), or None when the grid has no such boundary."""
    k = int(round(thr * levels))
    return k if 1 <= k < levels and float(np.float64(k) / np.float64(levels)) == thr else None


# ------------------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope='module')
def lib():
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    return _lib


def test_histogram_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, 'include', 'rcu.h')).read()
    declared = set(re.findall(r'\b(rcu_[a-z0-9_]+)\s*\(', header))
    so = lib.load()
    for name in NAMES:
        assert name in declared and name in lib.SIGNATURES and hasattr(so, name), name
    assert 'RCU_UNC_HIST_MAX_LEVELS 4096' in header and lib.RCU_UNC_HIST_MAX_LEVELS == 4096
    # the header states the definition and the caveat of the from-p path
    assert '(double)k / (double)B' in header and 'logf' in header[header.index('rcu_unc_hist_from_p'):]


def test_histogram_argument_validation_without_gpu(lib):
    so = lib.load()
    u, pr, tg, m, out, ws = (ctypes.c_void_p(v) for v in (1 << 20, 1 << 24, 1 << 25, 1 << 26, 1 << 30, 1 << 31))

    def refused(status, *words):
        assert status == -1        # RCU_ERR_INVALID
        msg = so.rcu_last_error()
        for w in words:
            assert w in msg, (w, msg)

    def hist(unc=u, is64=1, prediction=pr, target=tg, mask=None, n=1000, v=2, levels=1000, o=out, w=ws):
        return so.rcu_unc_hist(unc, is64, prediction, target, mask, n, v, levels, o, w, None)

    def hist_p(p=u, prediction=pr, target=tg, mask=None, n=1000, v=2, levels=1000, o=out, w=ws):
        return so.rcu_unc_hist_from_p(p, prediction, target, mask, n, v, levels, o, w, None)

    for fn, name, map_name in ((hist, b'rcu_unc_hist:', b'unc_dev'), (hist_p, b'rcu_unc_hist_from_p:', b'p_foreground_dev')):
        for levels in (1, 0, -5, 4097, 1 << 20):
            refused(fn(levels=levels), name, b'levels')
        refused(fn(None), name, b'null', map_name)
        refused(fn(prediction=None), name, b'null', b'prediction_dev')
        refused(fn(target=None), name, b'null', b'target_dev')
        refused(fn(o=None), name, b'null', b'hist_dev')
        refused(fn(w=None), name, b'null', b'workspace_dev')
        refused(fn(n=0), name, b'n_per_volume')
        for v in (0, -1):
            refused(fn(v=v), name, b'n_volumes')
        # levels are judged first, with every other argument bad as well: nothing is dereferenced
        refused(fn(None, levels=1), name, b'levels')
    for levels in (2, 1000, 4096):
        assert so.rcu_unc_hist_workspace_bytes(155 * 240 * 240, 8, levels) >= 8
    assert so.rcu_unc_hist_workspace_bytes(1000, 1, 1) == 0 and so.rcu_unc_hist_workspace_bytes(1000, 1, 4097) == 0


def test_entropy_arithmetic_has_one_definition():
    """The five lines of ToEntropy's arithmetic live in one device function that both kernels call."""
    csrc = os.path.join(ROOT, 'reliability-challenges-uncertainty_amd', 'csrc')
    shared = open(os.path.join(csrc, 'rcu_entropy.h')).read()
    assert 'logf(f)' in shared and '__forceinline__' in shared
    for name, fn in (('rcu_calib.hip', 'normalised_entropy_of_p'), ('rcu_unc_hist.hip', 'entropy_nats_of_p')):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "rcu_entropy.h"' in text and fn in text, name
        assert 'logf(' not in text, name        # no second copy of the arithmetic


# ------------------------------------------------------------------------------ the identity against the reference's counts
def test_suffix_sums_reproduce_the_reference_counts_g9():
    g = load_golden('g9_uncertainty')
    assert tuple(g['thresholds']) == SCRIPT_THRESHOLDS
    for levels in (1000, 20, 100):
        h = numpy_histogram(g['prediction'], g['target'], g['uncertainty'], levels)
        assert int(h.sum()) == g['uncertainty'].size
        hit = 0
        for i, thr in enumerate(SCRIPT_THRESHOLDS):
            k = boundary_index(thr, levels)
            if k is None:
                continue
            hit += 1
            assert counts_at(h, k) == list(g['counts'][i]), (levels, thr)
        assert hit == 11, (levels, hit)        # k / 20, k / 100 and k / 1000 all round to the literals' doubles
    h = numpy_histogram(g['prediction'], g['target'], g['uncertainty'], 1000, mask=g['mask'])
    assert counts_at(h, 500) == list(g['masked_counts_thr05'])


@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_suffix_sums_reproduce_the_reference_counts_g22(tag):
    g = load_golden('g22_ue_curves')
    assert tuple(g['thresholds']) == SCRIPT_THRESHOLDS and int(g['levels']) == 1000
    pr, tg, unc, mask = (g['{}_{}'.format(tag, k)] for k in ('prediction', 'target', 'uncertainty', 'mask'))
    assert unc.dtype == np.float64
    for levels in (1000, 20, 100):
        for which, m in ((0, None), (1, mask)):
            h = numpy_histogram(pr, tg, unc, levels, mask=m)
            assert [boundary_index(t, 1000) for t in SCRIPT_THRESHOLDS] == [50, 100, 200, 300, 400, 500, 600, 700, 800, 900, 950]
            for i, thr in enumerate(SCRIPT_THRESHOLDS):
                k = boundary_index(thr, levels)
                if k is not None:
                    assert counts_at(h, k) == list(g['{}_counts'.format(tag)][which, i]), (levels, thr, which)


def test_boundary_values_land_where_the_definition_says():
    g = load_golden('g22_ue_curves')
    unc = g['c_uncertainty'].reshape(-1)
    level = levels_of(unc, 1000)
    special, expect = unc[g['c_special_index']], g['c_special_level']
    assert np.array_equal(level[g['c_special_index']], expect)
    t = np.arange(1, 1000, dtype=np.float64) / 1000.0
    # the layout of the probe: t_k -> k - 1, the float64 below -> k - 1, the float64 above -> k; then 0, -0, 1, 1 + 1e-9, -1e-9, NaN
    assert np.array_equal(special[:999], t) and np.array_equal(expect[:999], np.arange(0, 999))
    assert np.array_equal(special[999:1998], np.nextafter(t, 0.0)) and np.array_equal(expect[999:1998], np.arange(0, 999))
    assert np.array_equal(special[1998:2997], np.nextafter(t, 1.0)) and np.array_equal(expect[1998:2997], np.arange(1, 1000))
    assert list(expect[2997:]) == [0, 0, 999, 999, 0, 0] and np.isnan(special[-1]) and special[-2] < 0 and special[-3] > 1
    # the script's literals are the boundaries, bit for bit
    for thr in SCRIPT_THRESHOLDS:
        assert t[boundary_index(thr, 1000) - 1] == thr


# ------------------------------------------------------------------------------------------------------- ue_curve_metrics
def voxelwise_metrics(error, level, levels):
    """aurc, eaurc, ue_dice_max, ue_dice_max_threshold restated voxel by voxel (sorting, no histogram)."""
    from rcu_amd import evaluation as ev
    error, level = np.asarray(error, dtype=bool), np.asarray(level)
    n, n_err = error.size, int(error.sum())
    order = np.argsort(level, kind='stable')
    lv, er = level[order], error[order]
    # coverage points: after each whole level
    ends = np.nonzero(np.r_[lv[1:] != lv[:-1], True])[0]        # last index of each level present
    cum_err = np.cumsum(er)
    aurc = ideal = 0.0
    prev = -1
    risks, ideals = [], []
    for end in ends:
        accepted = int(end) + 1
        weight = (accepted - (prev + 1)) / n
        risks.append(weight * (int(cum_err[end]) / accepted))
        ideals.append(weight * (max(0, accepted - (n - n_err)) / accepted))
        prev = int(end)
    aurc, ideal = math.fsum(risks), math.fsum(ideals)
    best, best_thr = None, None
    for k in range(1, levels):
        unc = level >= k
        d = ev.error_dice(n_err, 0, int((unc & ~error).sum()), 0, int((unc & error).sum()), 0)       # (errors as fp, correct as tp: the formula sums them)
        if best is None or d > best:
            best, best_thr = d, k / levels
    return aurc, aurc - ideal, best, best_thr


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_metrics_match_scikit_learn_and_the_voxelwise_restatement(tag):
    from rcu_amd import evaluation as ev
    g = load_golden('g22_ue_curves')
    pr, tg, unc = (g['{}_{}'.format(tag, k)] for k in ('prediction', 'target', 'uncertainty'))
    for levels in (1000,):
        h = numpy_histogram(pr, tg, unc, levels)
        m = ev.ue_curve_metrics(h)
        assert list(m) == ['n', 'n_errors', 'auroc', 'auprc', 'aurc', 'eaurc', 'ue_dice_max', 'ue_dice_max_threshold'] == list(ev.UE_CURVE_KEYS)
        error = (pr != tg).reshape(-1)
        assert m['n'] == error.size and m['n_errors'] == int(error.sum())
        print(tag, 'auroc', m['auroc'], float(g[tag + '_auroc']), 'auprc', m['auprc'], float(g[tag + '_auprc']))
        assert abs(m['auroc'] - float(g[tag + '_auroc'])) <= TOL
        assert abs(m['auprc'] - float(g[tag + '_auprc'])) <= TOL
        aurc, eaurc, dice, thr = voxelwise_metrics(error, levels_of(unc, levels), levels)
        print(tag, 'aurc', m['aurc'], aurc, 'eaurc', m['eaurc'], eaurc, 'dice', m['ue_dice_max'], dice, m['ue_dice_max_threshold'], thr)
        assert abs(m['aurc'] - aurc) <= TOL and abs(m['eaurc'] - eaurc) <= TOL
        assert abs(m['ue_dice_max'] - dice) <= TOL and m['ue_dice_max_threshold'] == thr
        assert -TOL <= m['eaurc'] <= m['aurc'] <= 1.0


def test_metrics_of_other_grids_match_the_voxelwise_restatement():
    from rcu_amd import evaluation as ev
    g = load_golden('g22_ue_curves')
    pr, tg, unc = g['a_prediction'], g['a_target'], g['a_uncertainty']
    error = (pr != tg).reshape(-1)
    for levels in (2, 20, 4096):
        m = ev.ue_curve_metrics(numpy_histogram(pr, tg, unc, levels))
        level = levels_of(unc, levels)
        aurc, eaurc, dice, thr = voxelwise_metrics(error, level, levels)
        assert abs(m['aurc'] - aurc) <= TOL and abs(m['eaurc'] - eaurc) <= TOL
        assert abs(m['ue_dice_max'] - dice) <= TOL and m['ue_dice_max_threshold'] == thr
        # auroc by its definition, pair counting: P(level of an error > level of a correct voxel) + P(equal) / 2
        le, lc = np.bincount(level[error], minlength=levels), np.bincount(level[~error], minlength=levels)
        below = np.cumsum(lc) - lc
        pairs2 = sum(int(le[l]) * (2 * int(below[l]) + int(lc[l])) for l in range(levels))
        assert abs(m['auroc'] - pairs2 / (2 * int(le.sum()) * int(lc.sum()))) <= TOL


def test_perfect_and_inverted_rankings():
    from rcu_amd import evaluation as ev
    h = np.zeros((4, 10), dtype=np.uint64)
    h[1, 0], h[0, 1], h[2, 8], h[3, 9] = 50, 30, 12, 8       # correct voxels certain, errors uncertain
    m = ev.ue_curve_metrics(h)
    assert m['auroc'] == 1.0 and m['auprc'] == 1.0 and m['eaurc'] == 0.0 and m['ue_dice_max'] == 1.0
    assert m['ue_dice_max_threshold'] == 0.2                    # the SMALLEST threshold with Dice 1: u > 0.2 keeps exactly the errors
    assert m['n'] == 100 and m['n_errors'] == 20
    m = ev.ue_curve_metrics(h[:, ::-1])
    assert m['auroc'] == 0.0 and m['eaurc'] > 0.0


def test_undefined_cases_are_nan_never_an_exception():
    from rcu_amd import evaluation as ev
    empty = np.zeros((4, 16), dtype=np.uint64)
    m = ev.ue_curve_metrics(empty)
    assert m['n'] == 0 and m['n_errors'] == 0
    assert all(math.isnan(m[k]) for k in ('auroc', 'auprc', 'aurc', 'eaurc'))
    assert m['ue_dice_max'] == ev.error_dice(0, 0, 0, 0, 0, 0) == 1.0
    no_errors = empty.copy()
    no_errors[0, 3], no_errors[1, 0] = 5, 7
    m = ev.ue_curve_metrics(no_errors)
    assert math.isnan(m['auroc']) and math.isnan(m['auprc']) and m['aurc'] == 0.0 and m['eaurc'] == 0.0
    only_errors = empty.copy()
    only_errors[2, 3], only_errors[3, 9] = 5, 7
    m = ev.ue_curve_metrics(only_errors)
    assert math.isnan(m['auroc']) and abs(m['auprc'] - 1.0) <= TOL and abs(m['aurc'] - 1.0) <= TOL and m['eaurc'] == 0.0
    with pytest.raises(ValueError):
        ev.ue_curve_metrics(np.zeros((3, 16)))


def test_histograms_pool_by_addition():
    """The metrics of two subjects' summed histogram are those of the concatenated voxels."""
    from rcu_amd import evaluation as ev
    g = load_golden('g22_ue_curves')
    ha = numpy_histogram(g['a_prediction'], g['a_target'], g['a_uncertainty'], 1000)
    hb = numpy_histogram(g['b_prediction'], g['b_target'], g['b_uncertainty'], 1000)
    both = numpy_histogram(np.concatenate([g['a_prediction'].reshape(-1), g['b_prediction'].reshape(-1)]),
                           np.concatenate([g['a_target'].reshape(-1), g['b_target'].reshape(-1)]),
                           np.concatenate([g['a_uncertainty'].reshape(-1), g['b_uncertainty'].reshape(-1)]), 1000)
    assert np.array_equal(ha + hb, both)
    pooled, direct = ev.ue_curve_metrics(ha + hb), ev.ue_curve_metrics(both)
    assert pooled == direct
    error = np.concatenate([(g[t + '_prediction'] != g[t + '_target']).reshape(-1) for t in 'ab'])
    level = np.concatenate([levels_of(g[t + '_uncertainty'], 1000) for t in 'ab'])
    aurc, eaurc, dice, thr = voxelwise_metrics(error, level, 1000)
    assert abs(pooled['aurc'] - aurc) <= TOL and abs(pooled['eaurc'] - eaurc) <= TOL and abs(pooled['ue_dice_max'] - dice) <= TOL
    assert pooled['ue_dice_max_threshold'] == thr


# ------------------------------------------------------------------------------------------------------------ the action
def test_action_is_registered_and_not_a_default(tmp_path):
    from rcu_amd import evalrun
    base = str(tmp_path / 'eval')
    actions = evalrun.get_actions(['ue_curves'], os.path.join(base, evalrun.MINMAX_NAME), base, 'foreground')
    assert len(actions) == 1 and isinstance(actions[0], evalrun.UeCurvesAction) and actions[0].levels == 1000
    assert (actions[0].rescale_confidence, actions[0].rescale_sigma) == ('subject', 'global')
    assert os.path.isdir(os.path.join(base, evalrun.UNCERTAINTY_NAME))
    actions = evalrun.get_actions(['minmax', 'ue_curves'], os.path.join(base, evalrun.MINMAX_NAME), base, '', levels=64)
    assert [type(a).__name__ for a in actions] == ['SaveMinMaxAction', 'UeCurvesAction'] and actions[1].levels == 64
    assert evalrun.metrics_wanted(actions) == (['minmax', 'ue_hist'], (0.5,), False)
    for bad in (1, 4097):
        with pytest.raises(ValueError):
            evalrun.get_actions(['ue_curves'], os.path.join(base, evalrun.MINMAX_NAME), base, '', levels=bad)
    # the script's default action list is unchanged, and its help names the new action and --levels
    script = open(os.path.join(ROOT, 'bin-eval', 'eval_uncertainty.py')).read()
    assert "acts = args.act or ['minmax', 'ece_dice', 'calib', 'bnf_ue']" in script
    assert 'ue_curves' in script and "'--levels'" in script
    import inspect
    from rcu_amd import scripts
    assert inspect.signature(scripts.eval_uncertainty).parameters['actions'].default == ('minmax', 'ece_dice', 'calib', 'bnf_ue')
