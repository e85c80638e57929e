"""The squared distance transform, the border shell, the surface distances and the boundary table without a GPU: the definitions restated
in numpy (a brute-force transform) and pinned to scipy's and the reference's arrays (fixture G24), `surface_distance_metrics` and
`boundary_metrics` against the fixture's floats, the C ABI's argument checks, the evaluation action's files and its registration."""
import csv
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('rcu_edt_sq', 'rcu_border_mask', 'rcu_boundary_table', 'rcu_surface_distance_bins', 'rcu_surface_distance_workspace_bytes',
         'rcu_surface_distance_hist', 'rcu_edt_set_slab_width')
CASES = ('box', 'blobs', 'face', 'rand', 'img')
ONE = 1 << 24
NONE = 0xFFFFFFFF
# hd, hd95 and assd are one square root resp. one interpolation of two of them resp. a sum of a few thousand float64 terms below 20 divided
# once; the fixture's side sums scipy's floats in another order.  The issue sets 1e-12.
TOL = 1e-12


# --------------------------------------------------------------------------------------- the definitions, in plain numpy
def brute_force_edt_sq(feature):
    """uint32 squared distance to the nearest True voxel of ``feature`` (up to 3 axes), NONE without one: every voxel against every feature."""
    feature = np.asarray(feature, dtype=bool)
    shape3 = (1,) * (3 - feature.ndim) + feature.shape
    out = np.full(feature.size, NONE, dtype=np.uint32)
    where = np.argwhere(feature.reshape(shape3)).astype(np.int64)
    if where.size:
        voxels = np.indices(shape3).reshape(3, -1).T.astype(np.int64)
        for first in range(0, len(voxels), 256):
            chunk = voxels[first:first + 256]
            out[first:first + 256] = ((chunk[:, None, :] - where[None, :, :]) ** 2).sum(-1).min(1)
    return out.reshape(feature.shape)


def separable_edt_sq(feature):
    """The same transform by the three separable passes (exact integers, NONE saturating): what larger test volumes are checked against."""
    feature = np.asarray(feature, dtype=bool)
    shape3 = (1,) * (3 - feature.ndim) + feature.shape
    big = np.int64(1) << 40
    f = np.where(feature.reshape(shape3), 0, big).astype(np.int64)
    for axis in (2, 1, 0):
        n = shape3[axis]
        idx = np.arange(n, dtype=np.int64)
        sq = (idx[:, None] - idx[None, :]) ** 2                       # [i, j]
        moved = np.moveaxis(f, axis, -1)                               # [..., j]
        best = np.full(moved.shape, big, dtype=np.int64)
        for j in range(n):                                             # (memory stays small)
            best = np.minimum(best, moved[..., j:j + 1] + sq[:, j])
        f = np.moveaxis(best, -1, axis)
    return np.where(f >= big, NONE, f).astype(np.uint32).reshape(feature.shape)


def quantise(u):
    with np.errstate(invalid='ignore'):
        q = np.rint(np.clip(np.asarray(u, dtype=np.float64), 0.0, 1.0) * np.float64(ONE))
    return np.where(np.isnan(q), 0, q).astype(np.int64)


def numpy_surface(a):
    """The voxels of a with a face neighbour outside a inside the volume."""
    a = np.asarray(a) != 0
    s = np.zeros(a.shape, dtype=bool)
    for axis in range(a.ndim):
        for lo in (True, False):
            here = [slice(None)] * a.ndim
            there = [slice(None)] * a.ndim
            here[axis], there[axis] = (slice(1, None), slice(None, -1)) if lo else (slice(None, -1), slice(1, None))
            s[tuple(here)] |= a[tuple(here)] & ~a[tuple(there)]
    return s


def numpy_boundary_table(prediction, target, q, bands, d_sq=None):
    """int64 [2, bands + 1, 4]: voxels, errors, unc_sum, unc_err_sum per (side, band); band k: k^2 < d <= (k + 1)^2, the last: d > bands^2."""
    tg = np.asarray(target) != 0
    if d_sq is None:
        d_in, d_out = separable_edt_sq(~tg).astype(np.int64), separable_edt_sq(tg).astype(np.int64)
        d_sq = np.where((d_in == NONE) | (d_out == NONE), np.int64(NONE), d_in + d_out)
    error = (np.asarray(prediction) != 0) != tg
    band = np.full(tg.shape, bands, dtype=np.int64)
    for k in range(bands - 1, -1, -1):
        band[d_sq <= (k + 1) ** 2] = k
    table = np.zeros((2, bands + 1, 4), dtype=np.int64)
    q = np.zeros(tg.shape, dtype=np.int64) if q is None else q
    for s in range(2):
        for b in range(bands + 1):
            cell = (tg == bool(s)) & (band == b)
            table[s, b] = [cell.sum(), (cell & error).sum(), q[cell].sum(), q[cell & error].sum()]
    return table


def as_cells(table):
    """A structured table of rcu_amd.evaluation.BOUNDARY_DTYPE -> the [..., 4] int64 layout of the fixture."""
    return np.stack([table[k].astype(np.int64) for k in ('voxels', 'errors', 'unc_sum', 'unc_err_sum')], axis=-1)


def as_table(cells):
    from rcu_amd import evaluation as ev
    cells = np.asarray(cells, dtype=np.int64)
    out = np.zeros(cells.shape[:-1], dtype=ev.BOUNDARY_DTYPE)
    for i, k in enumerate(('voxels', 'errors', 'unc_sum', 'unc_err_sum')):
        out[k] = cells[..., i]
    return out


def histogram_of(sq_p_to_t, sq_t_to_p):
    """Two lists of squared distances -> the (sq_values, count_p_to_t, count_t_to_p) of surface_distance_histograms."""
    values = np.unique(np.concatenate([sq_p_to_t, sq_t_to_p])).astype(np.int64)
    return (values, np.array([(sq_p_to_t == v).sum() for v in values], dtype=np.int64),
            np.array([(sq_t_to_p == v).sum() for v in values], dtype=np.int64))


def golden():
    g = load_golden('g24_boundary')
    assert tuple(str(c) for c in g['cases']) == CASES
    return g


# ------------------------------------------------------------------------------------- the restatement against the fixture
def test_brute_force_transform_reproduces_scipy():
    g = golden()
    for name in CASES:
        target = g[name + '_target']
        assert (target != 0).any() and (target == 0).any(), name
        for feature, key in ((target == 0, '_edt_sq_in'), (target != 0, '_edt_sq_out')):
            brute = brute_force_edt_sq(feature)
            assert brute.dtype == np.uint32 and np.array_equal(brute, g[name + key]), (name, key)
            assert np.array_equal(separable_edt_sq(feature), brute), (name, key)
    assert g['img_target'].ndim == 2
    assert np.all(brute_force_edt_sq(np.zeros((2, 3, 4), dtype=bool)) == NONE) and np.all(separable_edt_sq(np.zeros((2, 3, 4), dtype=bool)) == NONE)


def test_fixture_is_consistent_with_the_reference_shell():
    g = golden()
    for name in CASES:
        d_in, d_out = g[name + '_edt_sq_in'].astype(np.int64), g[name + '_edt_sq_out'].astype(np.int64)
        assert np.all((d_in == 0) != (d_out == 0))                     # one of the two is always 0
        # sqrt of the exact integer in float64 is the reference's distance, bit for bit; the masks are integer comparisons
        assert np.array_equal(np.sqrt((d_in + d_out).astype(np.float64)), g[name + '_dist11'])
        assert np.array_equal(g[name + '_dist23'], g[name + '_dist11'])
        assert np.array_equal((d_in <= 1) & (d_out <= 1), g[name + '_mask11']) and g[name + '_mask11'].dtype == bool
        assert np.array_equal((d_in <= 4) & (d_out <= 9), g[name + '_mask23'])
        for which in ('prediction', 'target'):
            assert np.array_equal(numpy_surface(g[name + '_' + which]), g[name + '_surface_' + which]), (name, which)
        assert np.array_equal(g[name + '_surface_target'], (g[name + '_target'] != 0) & (d_in == 1))
        sp, st = g[name + '_surface_prediction'], g[name + '_surface_target']
        assert np.array_equal(np.sort(brute_force_edt_sq(st)[sp].astype(np.int64)), g[name + '_sq_p_to_t'])
        assert np.array_equal(np.sort(brute_force_edt_sq(sp)[st].astype(np.int64)), g[name + '_sq_t_to_p'])
        q = quantise(g[name + '_uncertainty'])
        for bands in (3, 10):
            table = numpy_boundary_table(g[name + '_prediction'], g[name + '_target'], q, bands)
            assert np.array_equal(table, g['{}_table_r{}'.format(name, bands)]), (name, bands)
            assert table[:, 0, 0].sum() == g[name + '_mask11'].sum()   # band 0 of both sides is the reference's border shell
            assert table[..., 0].sum() == g[name + '_target'].size


# ------------------------------------------------------------------------------------------------ the host arithmetic
def test_surface_distance_metrics_match_the_fixture():
    from rcu_amd import evaluation as ev
    g = golden()
    for name in CASES:
        hist = histogram_of(g[name + '_sq_p_to_t'], g[name + '_sq_t_to_p'])
        m = ev.surface_distance_metrics(hist)
        assert set(m) == set(ev.SURFACE_DISTANCE_KEYS)
        assert m['n_surface_prediction'] == int(g[name + '_surface_prediction'].sum()) and m['n_surface_target'] == int(g[name + '_surface_target'].sum())
        for key in ('hd', 'hd95', 'assd'):
            print(name, key, m[key], float(g[name + '_' + key]))
            assert abs(m[key] - float(g[name + '_' + key])) <= TOL, (name, key)


def test_surface_distance_metrics_by_hand():
    from rcu_amd import evaluation as ev
    empty = np.zeros(0, dtype=np.int64)
    for hist in ((empty, empty, empty), (np.array([NONE]), np.array([0]), np.array([7])), (np.array([NONE]), np.array([3]), np.array([0]))):
        m = ev.surface_distance_metrics(hist)
        assert math.isnan(m['hd']) and math.isnan(m['hd95']) and math.isnan(m['assd'])
    m = ev.surface_distance_metrics((np.array([NONE]), np.array([0]), np.array([7])))
    assert (m['n_surface_prediction'], m['n_surface_target']) == (0, 7)
    m = ev.surface_distance_metrics((np.array([0]), np.array([5]), np.array([5])))
    assert (m['hd'], m['hd95'], m['assd']) == (0.0, 0.0, 0.0)
    m = ev.surface_distance_metrics((np.array([169]), np.array([1]), np.array([1])))
    assert (m['hd'], m['hd95'], m['assd']) == (13.0, 13.0, 13.0)
    # the percentile from the counts is numpy's on the expanded list, whatever the size
    rng = np.random.RandomState(5)
    for n in (2, 3, 20, 21, 40, 41, 1000):
        a, b = rng.randint(0, 30, size=n) ** 2, rng.randint(0, 30, size=rng.randint(1, n + 1)) ** 2
        m = ev.surface_distance_metrics(histogram_of(a, b))
        both = np.sqrt(np.concatenate([a, b]).astype(np.float64))
        assert m['hd95'] == float(np.percentile(both, 95)) and m['hd'] == both.max() and abs(m['assd'] - both.mean()) <= TOL


def test_boundary_metrics_match_numpy_on_the_fixture():
    from rcu_amd import evaluation as ev
    g = golden()
    for name in CASES:
        for bands in (3, 10):
            cells = g['{}_table_r{}'.format(name, bands)]
            m = ev.boundary_metrics(as_table(cells))
            vox, err, us, ues = (cells[..., i].astype(np.float64) for i in range(4))
            with np.errstate(invalid='ignore', divide='ignore'):
                expect = {'error_rate': err / vox, 'mean_uncertainty': us / (vox * ONE), 'mean_uncertainty_of_errors': ues / (err * ONE),
                          'mean_uncertainty_of_correct': (us - ues) / ((vox - err) * ONE)}
            for key in ev.BOUNDARY_BAND_KEYS:
                assert m[key].shape == (2, bands + 1)
                assert np.array_equal(np.isnan(m[key]), np.isnan(expect[key])), (name, bands, key)
                assert np.all(np.abs(m[key] - expect[key])[~np.isnan(expect[key])] <= TOL), (name, bands, key)
            assert m['n'] == g[name + '_target'].size and m['n_border'] == int(g[name + '_mask11'].sum())
            error = (g[name + '_prediction'] != 0) != (g[name + '_target'] != 0)
            assert m['errors'] == int(error.sum())
            assert abs(m['errors_border_share'] - (error & g[name + '_mask11']).sum() / error.sum()) <= TOL
            q = quantise(g[name + '_uncertainty'])
            assert abs(m['uncertainty_border_share'] - q[g[name + '_mask11']].sum() / q.sum()) <= TOL
    empty = ev.boundary_metrics(np.zeros((2, 4), dtype=ev.BOUNDARY_DTYPE))
    assert empty['n'] == 0 and math.isnan(empty['errors_border_share']) and np.all(np.isnan(empty['error_rate']))
    with pytest.raises(ValueError):
        ev.boundary_metrics(np.zeros((3, 4), dtype=ev.BOUNDARY_DTYPE))
    # tables add
    tables = [as_table(g[name + '_table_r3']) for name in CASES]
    total = ev.add_boundary_tables(tables)
    assert np.array_equal(as_cells(total), sum(g[name + '_table_r3'] for name in CASES))
    assert np.array_equal(as_cells(ev.add_boundary_tables(tables[::-1])), as_cells(total))


# ------------------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope='module')
def lib():
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    return _lib


def test_boundary_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, 'include', 'rcu.h')).read()
    declared = set(re.findall(r'\b(rcu_[a-z0-9_]+)\s*\(', header))
    so = lib.load()
    for name in NAMES:
        assert name in declared and name in lib.SIGNATURES and hasattr(so, name), name
    from rcu_amd import evaluation as ev
    assert ev.BOUNDARY_DTYPE.itemsize == 32 and 'rcu_boundary_cell' in header
    assert [ev.BOUNDARY_DTYPE.fields[k][1] for k in ('voxels', 'errors', 'unc_sum', 'unc_err_sum')] == [0, 8, 16, 24]
    assert lib.RCU_EDT_NONE == NONE == ev.EDT_NONE and '#define RCU_EDT_NONE 0xFFFFFFFFu' in header
    assert so.rcu_surface_distance_bins(155, 240, 240) == 154 ** 2 + 2 * 239 ** 2 + 2
    assert so.rcu_surface_distance_bins(1, 1, 1) == 2 and so.rcu_surface_distance_bins(0, 1, 1) == 0 and so.rcu_surface_distance_bins(1, 1, 16385) == 0


def test_boundary_argument_validation_without_gpu(lib):
    so = lib.load()
    mask, out, other, unc, d_in, d_out, table, ws = (ctypes.c_void_p(v << 20) for v in (1, 16, 32, 48, 64, 80, 96, 112))

    def refused(status, *words):
        assert status == -1        # RCU_ERR_INVALID
        msg = so.rcu_last_error()
        for w in words:
            assert w in msg, (w, msg)

    def edt(m=mask, d=4, h=5, w=6, v=2, zero=1, o=out):
        return so.rcu_edt_sq(m, d, h, w, v, zero, o, None)

    def surf(p=mask, t=other, d=4, h=5, w=6, v=2, hist=out, w_=ws):
        return so.rcu_surface_distance_hist(p, t, d, h, w, v, hist, w_, None)

    for fn, name in ((edt, b'rcu_edt_sq:'), (surf, b'rcu_surface_distance_hist:')):
        refused(fn(d=0), name, b'depth')
        refused(fn(d=16385, h=1, w=1), name, b'depth')
        refused(fn(h=0), name, b'height')
        refused(fn(h=16385, d=1, w=1), name, b'height')
        refused(fn(w=-1), name, b'width')
        refused(fn(w=16385, d=1, h=1), name, b'width')
        refused(fn(d=8192, h=16384, w=16), name, b'2^31')              # 2^31 voxels
        for v in (0, -1, 65536):
            refused(fn(v=v), name, b'n_volumes')
        refused(fn(d=1024, h=1024, w=1024, v=4), name, b'2^32')        # 2^32 voxels in the batch
    for zero in (-1, 2):
        refused(edt(zero=zero), b'rcu_edt_sq:', b'zero_is_feature')
    refused(edt(m=None), b'rcu_edt_sq:', b'null', b'mask_dev')
    refused(edt(o=None), b'rcu_edt_sq:', b'null', b'out_dev')
    refused(edt(m=None, zero=3), b'rcu_edt_sq:', b'zero_is_feature')   # judged first, nothing is dereferenced
    refused(surf(p=None), b'null', b'prediction_dev')
    refused(surf(t=None), b'null', b'target_dev')
    refused(surf(hist=None), b'null', b'hist_dev')
    refused(surf(w_=None), b'null', b'workspace_dev')
    assert so.rcu_surface_distance_workspace_bytes(155 * 240 * 240, 8) >= 6 * 8 * 155 * 240 * 240
    assert so.rcu_surface_distance_workspace_bytes(0, 1) == 0 and so.rcu_surface_distance_workspace_bytes(1000, 0) == 0
    assert so.rcu_surface_distance_workspace_bytes(1 << 30, 4) == 0

    def border(a=d_in, b=d_out, n=1000, din=1, dout=1, m=mask, dist=unc):
        return so.rcu_border_mask(a, b, n, din, dout, m, dist, None)

    refused(border(n=0), b'rcu_border_mask:', b'n must')
    refused(border(n=1 << 32), b'rcu_border_mask:', b'n must')
    refused(border(din=-1), b'rcu_border_mask:', b'distance_in')
    refused(border(din=65536), b'rcu_border_mask:', b'distance_in')
    refused(border(dout=-1), b'rcu_border_mask:', b'distance_out')
    refused(border(dout=65536), b'rcu_border_mask:', b'distance_out')
    refused(border(a=None), b'null', b'd_in_dev')
    refused(border(b=None), b'null', b'd_out_dev')
    refused(border(m=None, dist=None), b'rcu_border_mask:', b'both null')

    def tab(p=mask, t=other, a=d_in, b=d_out, u=unc, kind=2, n=1000, v=2, bands=10, tb=table):
        return so.rcu_boundary_table(p, t, a, b, u, kind, n, v, bands, tb, None)

    refused(tab(n=0), b'rcu_boundary_table:', b'n_per_volume')
    refused(tab(n=0x7fffffff), b'rcu_boundary_table:', b'n_per_volume')
    for v in (0, -3, 65536):
        refused(tab(v=v), b'rcu_boundary_table:', b'n_volumes')
    refused(tab(n=1 << 30, v=4), b'rcu_boundary_table:', b'2^32')
    for bands in (0, -1, 65):
        refused(tab(bands=bands), b'rcu_boundary_table:', b'bands')
    for kind in (-1, 4, 99):
        refused(tab(kind=kind), b'rcu_boundary_table:', b'unc_kind')
    refused(tab(u=None), b'rcu_boundary_table:', b'unc_dev')           # a kind without a map
    refused(tab(kind=0), b'rcu_boundary_table:', b'unc_dev')           # a map without a kind
    for kw, word in ((dict(p=None), b'prediction_dev'), (dict(t=None), b'target_dev'), (dict(a=None), b'd_in_dev'), (dict(b=None), b'd_out_dev'),
                     (dict(tb=None), b'table_dev')):
        refused(tab(**kw), b'rcu_boundary_table:', b'null', word)
    try:
        for width in (-1, 3, 48, 65, 128):
            refused(so.rcu_edt_set_slab_width(width), b'rcu_edt_set_slab_width:')
        for width in (1, 2, 4, 8, 16, 32, 64, 0):
            assert so.rcu_edt_set_slab_width(width) == 0
    finally:
        so.rcu_edt_set_slab_width(0)


# ------------------------------------------------------------------------------------------------------------ the action
def _rows(path):
    with open(path, newline='') as f:
        return list(csv.reader(f))


def test_action_is_registered_and_not_a_default(tmp_path):
    import inspect
    from rcu_amd import evalrun, scripts
    base = str(tmp_path / 'eval')
    mm = os.path.join(base, evalrun.MINMAX_NAME)
    actions = evalrun.get_actions(['boundary'], mm, base, 'foreground')
    assert len(actions) == 1 and isinstance(actions[0], evalrun.BoundaryAction)
    assert (actions[0].levels, actions[0].bands) == (1000, 10)
    assert (actions[0].rescale_confidence, actions[0].rescale_sigma) == ('subject', 'global')      # as UeCurvesAction / ComponentsAction prepare
    assert evalrun.metrics_wanted(actions) == (['minmax', 'boundary'], (0.5,), False)              # no brain mask
    actions = evalrun.get_actions(['minmax', 'ue_curves', 'components', 'boundary'], mm, base, '', levels=64, bands=3)
    assert [type(a).__name__ for a in actions] == ['SaveMinMaxAction', 'UeCurvesAction', 'ComponentsAction', 'BoundaryAction']
    assert evalrun.metrics_wanted(actions) == (['minmax', 'ue_hist', 'components', 'boundary'], (0.5,), False)
    assert evalrun._fusable(evalrun.EvalData('baseline', 'unused', 'probabilities'), actions)
    assert not evalrun._fusable(evalrun.EvalData('aleatoric', 'unused', 'sigma'), actions)
    # runs without it ask for exactly what they asked for before
    old = evalrun.get_actions(['minmax', 'ece_dice', 'calib', 'bnf_ue'], mm, base, 'foreground')
    assert evalrun.metrics_wanted(old)[0] == ['ece', 'minmax', 'ue']
    for bad in (dict(bands=0), dict(bands=65), dict(bands=-1), dict(levels=1)):
        with pytest.raises(ValueError):
            evalrun.get_actions(['boundary'], mm, base, '', **bad)
    for ok in (1, 64):
        assert evalrun.get_actions(['boundary'], mm, base, '', bands=ok)[0].bands == ok
    script = open(os.path.join(ROOT, 'bin-eval', 'eval_uncertainty.py')).read()
    assert "acts = args.act or ['minmax', 'ece_dice', 'calib', 'bnf_ue']" in script
    assert 'boundary' in script and "'--bands'" in script and 'bands=args.bands' in script
    assert inspect.signature(scripts.eval_uncertainty).parameters['bands'].default == 10
    assert inspect.signature(evalrun.evaluate_runs).parameters['bands'].default == 10


def test_loader_params_carry_the_border_flags():
    import inspect
    from rcu_amd import evalrun
    names = list(inspect.signature(evalrun.Loader.Params.__init__).parameters)
    assert names[-2:] == ['need_gt_dist_and_boarder', 'need_prediction_dist_and_boarder']          # keyword arguments at the end
    p = evalrun.Loader.Params()
    assert p.need_gt_dist_and_boarder is False and p.need_prediction_dist_and_boarder is False
    ahead = evalrun._LoaderAhead([], [evalrun.Loader.Params('probabilities'),
                                      evalrun.Loader.Params('probabilities', need_gt_dist_and_boarder=True)], depth=1)
    try:
        assert ahead.reader.params.need_gt_dist_and_boarder and not ahead.reader.params.need_prediction_dist_and_boarder
    finally:
        ahead.close()


def test_action_writes_its_three_files_from_hand_made_integers(tmp_path):
    from rcu_amd import evalrun, evaluation as ev
    g = golden()
    base = str(tmp_path / 'eval')
    (action,) = evalrun.get_actions(['boundary'], os.path.join(base, evalrun.MINMAX_NAME), base, '', levels=4, bands=3)
    action.setup_eval(evalrun.EvalData('baseline_mc', 'unused', 'probabilities'))
    subjects = []
    for name in ('box', 'face'):
        table = as_table(g[name + '_table_r3'])
        surface = histogram_of(g[name + '_sq_p_to_t'], g[name + '_sq_t_to_p'])
        hist = np.array([[5, 1, 0, 0], [90, 3, 1, 0], [1, 2, 1, 1], [0, 1, 2, 3]], dtype=np.uint64) * (2 if name == 'face' else 1)
        subjects.append((table, surface, hist))
        action.record_boundary(table, surface, hist, 'subject_' + name)
    action.finish_eval()
    out = os.path.join(base, evalrun.UNCERTAINTY_NAME)
    assert sorted(os.listdir(out)) == ['eval_boundary_bands_baseline_mc.csv', 'eval_boundary_baseline_mc.csv', 'eval_boundary_pooled_baseline_mc.csv']
    off = [k + '_off_border' for k in ev.UE_CURVE_KEYS]
    rows = _rows(os.path.join(out, 'eval_boundary_baseline_mc.csv'))
    assert rows[0] == ['test_id', 'subject_name'] + list(ev.BOUNDARY_TABLE_KEYS) + ['hd', 'hd95', 'assd'] + off and len(rows) == 3
    for row, name, (table, surface, hist) in zip(rows[1:], ('subject_box', 'subject_face'), subjects):
        bm, sm, cm = ev.boundary_metrics(table), ev.surface_distance_metrics(surface), ev.ue_curve_metrics(hist)
        assert row == ['baseline_mc', name] + [str(bm[k]) for k in ev.BOUNDARY_TABLE_KEYS] + [str(sm[k]) for k in ('hd', 'hd95', 'assd')] + \
            [str(cm[k]) for k in ev.UE_CURVE_KEYS]
    total = ev.add_boundary_tables([s[0] for s in subjects])
    bm, cm = ev.boundary_metrics(total), ev.ue_curve_metrics(subjects[0][2] + subjects[1][2])
    pooled = _rows(os.path.join(out, 'eval_boundary_pooled_baseline_mc.csv'))
    assert pooled == [['test_id'] + list(ev.BOUNDARY_TABLE_KEYS) + off,
                      ['baseline_mc'] + [str(bm[k]) for k in ev.BOUNDARY_TABLE_KEYS] + [str(cm[k]) for k in ev.UE_CURVE_KEYS]]
    bands = _rows(os.path.join(out, 'eval_boundary_bands_baseline_mc.csv'))
    assert bands[0] == ['side', 'band', 'voxels', 'errors', 'unc_sum', 'unc_err_sum'] + list(ev.BOUNDARY_BAND_KEYS) and len(bands) == 1 + 2 * 4
    cells = as_cells(total)
    for i, row in enumerate(bands[1:]):
        side, band = divmod(i, 4)
        assert row[:6] == [str(side), str(band)] + [str(int(v)) for v in cells[side, band]]
        assert row[6:] == [str(float(bm[k][side, band])) for k in ev.BOUNDARY_BAND_KEYS]
    # a second run of the same action object starts from nothing
    action.setup_eval(evalrun.EvalData('center', 'unused', 'probabilities'))
    action.record_boundary(*subjects[0], 'subject_box')
    action.finish_eval()
    assert _rows(os.path.join(out, 'eval_boundary_bands_center.csv'))[1][2] == str(int(cells[0, 0][0] - as_cells(subjects[1][0])[0, 0][0]))
