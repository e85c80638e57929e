"""Connected components, the per-component table and the component-level metrics without a GPU: the definitions restated in numpy and
pinned to scipy.ndimage's labels and sums (fixture G23), `component_metrics` against scikit-learn's stored values and a brute-force
filtered Dice, pooling, the C ABI's argument checks, the evaluation action's CSV files and its registration."""
import csv
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('rcu_cc_label', 'rcu_cc_workspace_bytes', 'rcu_cc_compact', 'rcu_cc_relabel', 'rcu_cc_table', 'rcu_cc_set_tile')
CASES = ('d10', 'd30', 'd60', 'img', 'diag')
ONE = 1 << 24
# Both sides of an AUROC / AUPRC comparison are one division of exact integers resp. a sum of at most a few hundred float64 terms in [0, 1]
# (scikit-learn sums them in another order): 1000 * 2^-53 < 1e-12 -- rounding, not slack.
TOL = 1e-12


# --------------------------------------------------------------------------------------- the definitions, in plain numpy
def backward_offsets(ndim, connectivity):
    """The neighbours that precede a voxel in raster order: 3 (6-connectivity) or 13 (26) in 3-D, 2 or 4 in 2-D."""
    out = []
    for off in np.ndindex(*([3] * ndim)):
        off = tuple(o - 1 for o in off)
        if off < (0,) * ndim and (connectivity == 26 or sum(o != 0 for o in off) == 1):
            out.append(off)
    return out


def numpy_labels(mask, connectivity):
    """Canonical labels: 0 for background, else 1 + the smallest linear index (C order) of the voxel's component.  Union-find over the
    list of adjacent foreground pairs: hook every pair's larger root to the smaller one, jump pointers until nothing moves."""
    fg = np.asarray(mask) != 0
    index = np.full(fg.shape, -1, dtype=np.int64)
    where = np.flatnonzero(fg.reshape(-1))
    index.reshape(-1)[where] = np.arange(where.size)              # compact ids in raster order: the smallest id is the smallest index
    a, b = [], []
    for off in backward_offsets(fg.ndim, connectivity):
        here = tuple(slice(max(0, -o), fg.shape[d] - max(0, o)) for d, o in enumerate(off))
        there = tuple(slice(max(0, o), fg.shape[d] - max(0, -o)) for d, o in enumerate(off))
        both = fg[here] & fg[there]
        a.append(index[here][both])
        b.append(index[there][both])
    a, b = np.concatenate(a), np.concatenate(b)
    parent = np.arange(where.size)
    while True:
        pa, pb = parent[a], parent[b]
        lo, hi = np.minimum(pa, pb), np.maximum(pa, pb)
        move = lo != hi
        if not move.any():
            break
        np.minimum.at(parent, hi[move], lo[move])
        while True:
            jumped = parent[parent]
            if np.array_equal(jumped, parent):
                break
            parent = jumped
    labels = np.zeros(fg.size, dtype=np.int32)
    labels[where] = where[parent] + 1
    return labels.reshape(fg.shape)


def flood_fill_labels(mask, connectivity):
    """The same labels by a plain flood fill from every unlabelled voxel in raster order (small volumes only)."""
    fg = np.asarray(mask) != 0
    offsets = backward_offsets(fg.ndim, connectivity)
    offsets = offsets + [tuple(-o for o in off) for off in offsets]
    labels = np.zeros(fg.shape, dtype=np.int32)
    for start in zip(*np.nonzero(fg)):                            # np.nonzero yields raster order
        if labels[start]:
            continue
        label = int(np.ravel_multi_index(start, fg.shape)) + 1
        labels[start] = label
        stack = [start]
        while stack:
            v = stack.pop()
            for off in offsets:
                u = tuple(c + o for c, o in zip(v, off))
                if all(0 <= c < s for c, s in zip(u, fg.shape)) and fg[u] and not labels[u]:
                    labels[u] = label
                    stack.append(u)
    return labels


def dense_of(labels):
    """Canonical labels -> (1..K in increasing order of the canonical label, K)."""
    values, inverse = np.unique(labels.reshape(-1), return_inverse=True)
    if values.size and values[0] == 0:
        return inverse.reshape(labels.shape).astype(np.int32), values.size - 1
    return (inverse.reshape(labels.shape) + 1).astype(np.int32), values.size


def quantise(u):
    """q(u) = rint(clamp(u, 0, 1) * 2^24) in float64, ties to even, NaN -> 0."""
    with np.errstate(invalid='ignore'):
        q = np.rint(np.clip(np.asarray(u, dtype=np.float64), 0.0, 1.0) * np.float64(ONE))
    return np.where(np.isnan(q), 0, q).astype(np.uint64)


def numpy_table(mask, other=None, uncertainty=None, connectivity=26, labels=None):
    """[K, 5] int64 rows root, voxels, other_voxels, unc_sum, unc_max in increasing order of the canonical label; integer arithmetic."""
    labels = numpy_labels(mask, connectivity) if labels is None else labels
    flat = labels.reshape(-1)
    where = np.flatnonzero(flat)
    roots, row = np.unique(flat[where], return_inverse=True)
    k = roots.size
    table = np.zeros((k, 5), dtype=np.uint64)
    table[:, 0] = roots - 1
    table[:, 1] = np.bincount(row, minlength=k)
    if other is not None:
        table[:, 2] = np.bincount(row[np.asarray(other).reshape(-1)[where] != 0], minlength=k)
    if uncertainty is not None:
        q = quantise(np.asarray(uncertainty).reshape(-1)[where])
        np.add.at(table[:, 3], row, q)
        np.maximum.at(table[:, 4], row, q)
    return table.astype(np.int64)


def as_rows(table):
    """A structured table of rcu_amd.evaluation.COMPONENT_DTYPE -> the [K, 5] int64 layout of the fixture."""
    return np.stack([table[k].astype(np.int64) for k in ('root', 'voxels', 'other_voxels', 'unc_sum', 'unc_max')], axis=1).reshape(-1, 5)


def as_table(rows):
    from rcu_amd import evaluation as ev
    out = np.zeros(len(rows), dtype=ev.COMPONENT_DTYPE)
    for i, k in enumerate(('root', 'voxels', 'other_voxels', 'unc_sum', 'unc_max')):
        out[k] = np.asarray(rows, dtype=np.int64).reshape(-1, 5)[:, i]
    return out


def fixture_cases():
    g = load_golden('g23_components')
    assert tuple(str(c) for c in g['cases']) == CASES
    for name in CASES:
        for conn in (6, 26):
            tag = '{}_c{}_'.format(name, conn)
            yield (name, conn, g[name + '_prediction'], g[name + '_target'], g[name + '_uncertainty'],
                   {k[len(tag):]: v for k, v in g.items() if k.startswith(tag)})


def same_metrics(a, b):
    return list(a) == list(b) and all((isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or
                                      (a[k] == b[k] and type(a[k]) is type(b[k])) for k in a)


# ------------------------------------------------------------------------------------- the restatement against the fixture
def test_restatement_reproduces_scipy_labels_and_tables():
    seen = 0
    for name, conn, pred, target, unc, ref in fixture_cases():
        for which, mask, other, u in (('pred', pred, target, unc), ('target', target, pred, None)):
            canonical = numpy_labels(mask, conn)
            assert np.array_equal(canonical, flood_fill_labels(mask, conn)), (name, conn, which)
            dense, k = dense_of(canonical)
            assert np.array_equal(dense, ref[which + '_labels']) and k == len(ref[which + '_table']), (name, conn, which)
            table = numpy_table(mask, other, u, conn)
            assert np.array_equal(table, ref[which + '_table']), (name, conn, which)
            # canonical label = 1 + the index of the component's first voxel, every voxel of the component carries it
            values, first = np.unique(dense.reshape(-1), return_index=True)
            assert np.array_equal(table[:, 0], first[values > 0])
            assert np.array_equal(canonical.reshape(-1)[table[:, 0]], table[:, 0] + 1)
            seen += 1
    assert seen == 20
    g = load_golden('g23_components')
    assert len(g['diag_c26_pred_table']) == 1 < len(g['diag_c6_pred_table'])          # the connectivities differ where only corners touch
    assert g['img_prediction'].ndim == 2


def test_quantisation_is_the_stated_rounding():
    u = np.array([0.0, -0.0, 1.0, 1.5, -3.0, np.nan, 0.5 / ONE, 1.5 / ONE, 2.5 / ONE, 0.5, np.inf, -np.inf, 1 - 2.0 ** -26])
    assert list(quantise(u)) == [0, 0, ONE, ONE, 0, 0, 0, 2, 2, ONE // 2, ONE, 0, ONE]
    # float32 maps are widened first: the value of the float32, not of its decimal
    f = np.float32(0.1)
    assert int(quantise(np.array([f]))[0]) == int(np.rint(np.float64(f) * ONE))


def test_quantisation_has_one_definition():
    """q(u) lives in one header that the component table and the boundary table both include."""
    csrc = os.path.join(ROOT, 'reliability-challenges-uncertainty_amd', 'csrc')
    shared = open(os.path.join(csrc, 'rcu_unc_source.h')).read()
    assert re.search(r'\bquantise\s*\(\s*double\b', shared) and '16777216' in shared and '#include "rcu_entropy.h"' in shared
    for name in ('rcu_cc.hip', 'rcu_edt.hip'):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "rcu_unc_source.h"' in text, name
        assert '16777216' not in text, name        # no second copy of the arithmetic


def test_host_metric_floats_are_the_stored_bits_g25():
    """Every float of the four host metric functions on the integers of G22, G23 and G24, as float.hex() (NaN as 'nan'): what the
    actions' CSV files print.  The generator's own ``compute`` is run again and compared entry by entry."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location('generate_metric_floats', os.path.join(ROOT, 'tests', 'golden', 'generate_metric_floats.py'))
    generator = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(generator)
    with open(generator.PATH) as f:
        stored = json.load(f)
    now = generator.compute()
    assert sorted(now) == sorted(stored) == ['boundary', 'components', 'surface', 'ue_curves']
    assert [len(stored[k]) for k in sorted(stored)] == [12, 22, 5, 7]
    for section in stored:
        assert sorted(now[section]) == sorted(stored[section]), section
        for table, expect in stored[section].items():
            assert now[section][table] == expect, (section, table)      # (hex strings and integers: NaN is the string 'nan')
    assert stored['ue_curves']['sum']['auroc'].startswith('0x1.') and stored['components']['diag_c26_l1000']['auroc_fp'] == 'nan'


# ------------------------------------------------------------------------------------------------------- component_metrics
def brute_force_filtered_dice(pred, target, unc, conn, levels):
    """Remove the components with mean uncertainty > k / levels from the MASK, count voxels, take the Dice: every k, no tables."""
    from rcu_amd import evaluation as ev
    dense, k = dense_of(numpy_labels(pred, conn))
    q = quantise(unc)
    tgt = target != 0
    mean = np.array([int(q[dense == c].sum()) / (int((dense == c).sum()) * ONE) for c in range(1, k + 1)])
    best = None
    for j in range(levels + 1):
        keep = np.concatenate([[False], ~(mean > j / levels)]) if k else np.array([False])
        kept = keep[dense]
        tp, fp, fn = int((kept & tgt).sum()), int((kept & ~tgt).sum()), int((~kept & tgt).sum())
        d = ev._dice(tp, fp, fn)
        if best is None or d > best[0]:
            best = (d, j / levels)
    return best


def test_metrics_match_scikit_learn_and_the_brute_force_dice():
    from rcu_amd import evaluation as ev
    for name, conn, pred, target, unc, ref in fixture_cases():
        pt, tt = as_table(ref['pred_table']), as_table(ref['target_table'])
        m = ev.component_metrics(pt, tt)
        assert list(m) == list(ev.COMPONENT_METRIC_KEYS)
        is_fp = ref['pred_table'][:, 2] == 0
        assert m['n_components'] == len(pt) and m['n_fp_components'] == int(is_fp.sum())
        assert m['fp_voxels'] == int(ref['pred_table'][is_fp, 1].sum())
        assert m['n_target_components'] == len(tt) and m['n_missed_target_components'] == int((ref['target_table'][:, 2] == 0).sum())
        print(name, conn, 'auroc', m['auroc_fp'], float(ref['auroc_fp']), 'auprc', m['auprc_fp'], float(ref['auprc_fp']))
        for key in ('auroc_fp', 'auprc_fp'):
            if math.isnan(float(ref[key])):
                assert math.isnan(m[key]), (name, conn, key)
            else:
                assert abs(m[key] - float(ref[key])) <= TOL, (name, conn, key)
        tp = int(((pred != 0) & (target != 0)).sum())
        assert m['dice'] == ev._dice(tp, int((pred != 0).sum()) - tp, int((target != 0).sum()) - tp)
        # TP is the same from either side
        assert int(ref['pred_table'][:, 2].sum()) == int(ref['target_table'][:, 2].sum()) == tp
        for levels in (1000, 7):
            m = ev.component_metrics(pt, tt, levels)
            assert (m['dice_filtered_max'], m['dice_filtered_max_threshold']) == brute_force_filtered_dice(pred, target, unc, conn, levels), (name, conn, levels)
            assert m['dice_filtered_max'] >= m['dice']                 # k = levels removes nothing (m_k <= 1)


def test_hand_made_tables():
    from rcu_amd import evaluation as ev
    # three predicted components: a large true positive (certain), a small false positive (uncertain), a false positive that ties with the tp
    pt = as_table([[0, 100, 80, 100 * (ONE // 10), ONE // 2], [500, 4, 0, 4 * (ONE // 2), ONE], [900, 10, 0, 10 * (ONE // 10), ONE // 8]])
    tt = as_table([[3, 90, 80, 0, 0], [700, 5, 0, 0, 0]])
    m = ev.component_metrics(pt, tt, 10)
    assert (m['n_components'], m['n_fp_components'], m['fp_voxels'], m['n_target_components'], m['n_missed_target_components']) == (3, 2, 14, 2, 1)
    assert m['auroc_fp'] == (1.0 + 0.5) / 2                            # one fp above the tp, one tied with it: ties count half
    assert abs(m['auprc_fp'] - (0.5 * 1.0 + 0.5 * (2 / 3))) <= TOL     # precision 1 at the first fp, 2 / 3 where the tie group ends
    assert m['dice'] == 2 * 80 / (114 + 95)
    # mean 0.1 = ONE // 10 / ONE is a hair under 1 / 10: the threshold 1 / 10 keeps both of those components, 0 removes everything
    assert (ONE // 10) / ONE <= 1 / 10
    assert m['dice_filtered_max'] == 2 * 80 / (110 + 95) and m['dice_filtered_max_threshold'] == 0.1
    empty = np.zeros(0, dtype=ev.COMPONENT_DTYPE)
    m = ev.component_metrics(empty, empty)
    assert m['n_components'] == 0 and math.isnan(m['auroc_fp']) and math.isnan(m['auprc_fp'])
    assert m['dice'] == 1.0 and m['dice_filtered_max'] == 1.0 and m['dice_filtered_max_threshold'] == 0.0       # ev._dice's 0 / 0
    m = ev.component_metrics(pt[1:], empty)                            # only false positives: removing them all is best
    assert math.isnan(m['auroc_fp']) and abs(m['auprc_fp'] - 1.0) <= TOL and m['dice'] == 0.0
    assert m['dice_filtered_max'] == 1.0 and m['dice_filtered_max_threshold'] == 0.0
    with pytest.raises(ValueError):
        ev.component_metrics(pt, tt, 0)


def test_pooled_metrics_do_not_depend_on_order_or_grouping():
    from rcu_amd import evaluation as ev
    subjects = [(as_table(ref['pred_table']), as_table(ref['target_table'])) for name, conn, *_, ref in fixture_cases() if conn == 6]
    assert len(subjects) == 5

    def pooled(order):
        return ev.component_metrics(np.concatenate([subjects[i][0] for i in order]), np.concatenate([subjects[i][1] for i in order]))

    base = pooled(range(5))
    assert base['n_components'] == sum(len(s[0]) for s in subjects) and not math.isnan(base['auroc_fp'])
    rng = np.random.RandomState(1)
    for _ in range(5):
        assert same_metrics(pooled(rng.permutation(5)), base)
    # rows shuffled inside the concatenation as well (a table is a multiset of rows)
    pt, tt = np.concatenate([s[0] for s in subjects]), np.concatenate([s[1] for s in subjects])
    assert same_metrics(ev.component_metrics(pt[rng.permutation(len(pt))], tt[rng.permutation(len(tt))]), base)
    # integer totals add
    for key in ('n_components', 'n_fp_components', 'fp_voxels', 'n_target_components', 'n_missed_target_components'):
        assert base[key] == sum(ev.component_metrics(*s)[key] for s in subjects)


# ------------------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope='module')
def lib():
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    return _lib


def test_component_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, 'include', 'rcu.h')).read()
    declared = set(re.findall(r'\b(rcu_[a-z0-9_]+)\s*\(', header))
    so = lib.load()
    for name in NAMES:
        assert name in declared and name in lib.SIGNATURES and hasattr(so, name), name
    from rcu_amd import evaluation as ev
    assert ev.COMPONENT_DTYPE.itemsize == 24 and 'rcu_cc_entry' in header
    assert [ev.COMPONENT_DTYPE.fields[k][1] for k in ('root', 'voxels', 'other_voxels', 'unc_max', 'unc_sum')] == [0, 4, 8, 12, 16]
    assert (lib.RCU_CC_UNC_NONE, lib.RCU_CC_UNC_F32, lib.RCU_CC_UNC_F64, lib.RCU_CC_UNC_P) == (0, 1, 2, 3)
    for k, v in (('NONE', 0), ('F32', 1), ('F64', 2), ('P', 3)):
        assert '#define RCU_CC_UNC_{} {}'.format(k, v) in header


def test_component_argument_validation_without_gpu(lib):
    so = lib.load()
    mask, labels, other, unc, counts, ws, table, dense = (ctypes.c_void_p(v << 20) for v in (1, 16, 32, 48, 64, 80, 96, 112))

    def refused(status, *words):
        assert status == -1        # RCU_ERR_INVALID
        msg = so.rcu_last_error()
        for w in words:
            assert w in msg, (w, msg)

    def label(m=mask, d=4, h=5, w=6, v=2, conn=26, out=labels):
        return so.rcu_cc_label(m, d, h, w, v, conn, out, None)

    for conn in (0, 4, 8, 18, 27, -6):
        refused(label(conn=conn), b'rcu_cc_label:', b'connectivity')
    for kw in (dict(d=0), dict(h=0), dict(w=-1)):
        refused(label(**kw), b'rcu_cc_label:', b'depth, height and width')
    refused(label(d=2048, h=1024, w=1024), b'rcu_cc_label:', b'2^31')             # 2^31 voxels
    refused(label(d=1, h=1, w=0x7fffffff), b'rcu_cc_label:', b'2^31')             # 2^31 - 1 voxels: one too many
    for v in (0, -1, 65536):
        refused(label(v=v), b'rcu_cc_label:', b'n_volumes')
    refused(label(m=None), b'rcu_cc_label:', b'null', b'mask_dev')
    refused(label(out=None), b'rcu_cc_label:', b'null', b'labels_dev')
    refused(label(m=None, conn=18), b'rcu_cc_label:', b'connectivity')            # judged first, nothing is dereferenced

    def compact(l=labels, n=1000, v=2, c=counts, w=ws):
        return so.rcu_cc_compact(l, n, v, c, w, None)

    def relabel(l=labels, n=1000, v=2, w=ws, out=dense):
        return so.rcu_cc_relabel(l, n, v, w, out, None)

    def tab(l=labels, o=other, u=unc, kind=2, n=1000, v=2, w=ws, t=table, k=10):
        return so.rcu_cc_table(l, o, u, kind, n, v, w, t, k, None)

    for fn, name in ((compact, b'rcu_cc_compact:'), (relabel, b'rcu_cc_relabel:'), (tab, b'rcu_cc_table:')):
        refused(fn(n=0), name, b'n_per_volume')
        refused(fn(n=0x7fffffff), name, b'n_per_volume')
        for v in (0, -3, 65536):
            refused(fn(v=v), name, b'n_volumes')
        refused(fn(n=1 << 30, v=4), name, b'2^32')
        refused(fn(l=None), name, b'null', b'labels_dev')
        refused(fn(w=None), name, b'null', b'workspace_dev')
    refused(compact(c=None), b'null', b'counts_dev')
    refused(relabel(out=None), b'null', b'dense_dev')
    for kind in (-1, 4, 99):
        refused(tab(kind=kind), b'rcu_cc_table:', b'unc_kind')
    refused(tab(u=None), b'rcu_cc_table:', b'unc_dev')                 # a kind without a map
    refused(tab(kind=0), b'rcu_cc_table:', b'unc_dev')                 # a map without a kind
    refused(tab(t=None), b'rcu_cc_table:', b'null', b'table_dev')
    assert tab(t=None, k=0) == 0                                       # an empty table: nothing to do, nothing touched
    assert so.rcu_cc_workspace_bytes(155 * 240 * 240, 8) >= 4 * 8 * 155 * 240 * 240
    assert so.rcu_cc_workspace_bytes(0, 1) == 0 and so.rcu_cc_workspace_bytes(1000, 0) == 0 and so.rcu_cc_workspace_bytes(1 << 30, 4) == 0
    try:
        for tile in ((0, 1, 1), (-1, 4, 4), (2, 2, 257), (1025, 1, 1), (1, 1, 0)):
            refused(so.rcu_cc_set_tile(*tile), b'rcu_cc_set_tile:')
        for tile in ((1, 1, 1), (4, 8, 32), (1, 1, 1024), (0, 0, 0)):
            assert so.rcu_cc_set_tile(*tile) == 0
    finally:
        so.rcu_cc_set_tile(0, 0, 0)


def test_python_wrappers_judge_shapes_before_the_device():
    from rcu_amd import evaluation as ev
    assert ev._volume_dims((24, 32)) == (1, 24, 32) and ev._volume_dims((7,)) == (1, 1, 7) and ev._volume_dims((2, 3, 4)) == (2, 3, 4)
    with pytest.raises(ValueError):
        ev._volume_dims((2, 3, 4, 5))
    assert ev._split_volumes((3, 4, 5, 6), 3) == (4, 5, 6) and ev._split_volumes((4, 5, 6), 1) == (4, 5, 6)
    with pytest.raises(ValueError):
        ev._split_volumes((4, 5, 6), 3)


# ------------------------------------------------------------------------------------------------------------ the action
def _rows(path):
    with open(path, newline='') as f:
        return list(csv.reader(f))


def test_action_writes_its_three_files_from_hand_made_tables(tmp_path):
    from rcu_amd import evalrun, evaluation as ev
    base = str(tmp_path / 'eval')
    (action,) = evalrun.get_actions(['components'], os.path.join(base, evalrun.MINMAX_NAME), base, 'foreground', levels=10, connectivity=6)
    assert isinstance(action, evalrun.ComponentsAction) and (action.levels, action.connectivity) == (10, 6)
    action.setup_eval(evalrun.EvalData('baseline_mc', 'unused', 'probabilities'))
    assert action.id_ == 'baseline_mc'
    pt_a = as_table([[0, 100, 80, 100 * (ONE // 10), ONE // 2], [500, 4, 0, 4 * (ONE // 2), ONE]])
    tt_a = as_table([[3, 90, 80, 0, 0], [700, 5, 0, 0, 0]])
    pt_b = as_table([[7, 10, 0, 10 * (ONE // 4), ONE // 4]])
    tt_b = np.zeros(0, dtype=ev.COMPONENT_DTYPE)
    action.record_tables(pt_a, tt_a, 'subject_a')
    action.record_tables(pt_b, tt_b, 'subject_b')
    action.finish_eval()
    out = os.path.join(base, evalrun.UNCERTAINTY_NAME)
    assert sorted(os.listdir(out)) == ['eval_component_list_baseline_mc.csv', 'eval_components_baseline_mc.csv', 'eval_components_pooled_baseline_mc.csv']
    rows = _rows(os.path.join(out, 'eval_components_baseline_mc.csv'))
    assert rows[0] == ['test_id', 'subject_name'] + list(ev.COMPONENT_METRIC_KEYS) and len(rows) == 3
    for row, name, tables in ((rows[1], 'subject_a', (pt_a, tt_a)), (rows[2], 'subject_b', (pt_b, tt_b))):
        expect = ev.component_metrics(*tables, levels=10)
        assert row == ['baseline_mc', name] + [str(expect[k]) for k in ev.COMPONENT_METRIC_KEYS]
    pooled = _rows(os.path.join(out, 'eval_components_pooled_baseline_mc.csv'))
    expect = ev.component_metrics(np.concatenate([pt_a, pt_b]), np.concatenate([tt_a, tt_b]), levels=10)
    assert pooled == [['test_id'] + list(ev.COMPONENT_METRIC_KEYS), ['baseline_mc'] + [str(expect[k]) for k in ev.COMPONENT_METRIC_KEYS]]
    assert expect['n_components'] == 3 and expect['n_fp_components'] == 2 and expect['auroc_fp'] == 1.0
    listed = _rows(os.path.join(out, 'eval_component_list_baseline_mc.csv'))
    assert listed[0] == ['subject', 'component', 'root_index', 'voxels', 'target_voxels', 'mean_uncertainty', 'max_uncertainty', 'is_fp']
    assert listed[1:] == [['subject_a', '1', '0', '100', '80', str((ONE // 10) / ONE), '0.5', '0'],
                          ['subject_a', '2', '500', '4', '0', '0.5', '1.0', '1'],
                          ['subject_b', '1', '7', '10', '0', '0.25', '0.25', '1']]
    # a second run of the same action object starts from nothing
    action.setup_eval(evalrun.EvalData('center', 'unused', 'probabilities'))
    action.record_tables(pt_b, tt_b, 'subject_b')
    action.finish_eval()
    assert len(_rows(os.path.join(out, 'eval_component_list_center.csv'))) == 2


def test_action_is_registered_and_not_a_default(tmp_path):
    from rcu_amd import evalrun
    base = str(tmp_path / 'eval')
    mm = os.path.join(base, evalrun.MINMAX_NAME)
    actions = evalrun.get_actions(['components'], mm, base, 'foreground')
    assert len(actions) == 1 and isinstance(actions[0], evalrun.ComponentsAction)
    assert (actions[0].levels, actions[0].connectivity) == (1000, 26)
    assert (actions[0].rescale_confidence, actions[0].rescale_sigma) == ('subject', 'global')      # as UeCurvesAction prepares
    assert evalrun.metrics_wanted(actions) == (['minmax', 'components'], (0.5,), False)
    actions = evalrun.get_actions(['minmax', 'ue_curves', 'components'], mm, base, '', levels=64, connectivity=6)
    assert [type(a).__name__ for a in actions] == ['SaveMinMaxAction', 'UeCurvesAction', 'ComponentsAction']
    assert evalrun.metrics_wanted(actions) == (['minmax', 'ue_hist', 'components'], (0.5,), False)
    # probability-map runs with the new action stay on the fused path; the other entries take the plain loop
    assert evalrun._fusable(evalrun.EvalData('baseline', 'unused', 'probabilities'), actions)
    assert not evalrun._fusable(evalrun.EvalData('aleatoric', 'unused', 'sigma'), actions)
    # runs without it ask for exactly what they asked for before
    old = evalrun.get_actions(['minmax', 'ece_dice', 'calib', 'bnf_ue'], mm, base, 'foreground')
    assert evalrun.metrics_wanted(old)[0] == ['ece', 'minmax', 'ue']
    for bad in (dict(connectivity=18), dict(connectivity=4), dict(levels=1), dict(levels=4097)):
        with pytest.raises(ValueError):
            evalrun.get_actions(['components'], mm, base, '', **bad)
    script = open(os.path.join(ROOT, 'bin-eval', 'eval_uncertainty.py')).read()
    assert "acts = args.act or ['minmax', 'ece_dice', 'calib', 'bnf_ue']" in script
    assert 'components' in script and "'--connectivity'" in script and 'choices=(6, 26)' in script
    import inspect
    from rcu_amd import scripts
    params = inspect.signature(scripts.eval_uncertainty).parameters
    assert params['actions'].default == ('minmax', 'ece_dice', 'calib', 'bnf_ue') and params['connectivity'].default == 26
    assert inspect.signature(evalrun.evaluate_runs).parameters['connectivity'].default == 26
