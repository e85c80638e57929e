"""The component-pair table and the lesion-wise metrics without a GPU: the C ABI's argument checks and struct layout, `lesion_metrics` /
`lesion_analysis` against the mask-based BraTS procedure of fixture G27 (scipy labels, scikit-learn scores; nothing of the table algebra),
pooling, the evaluation action's CSV files, its refusals and its registration."""
import csv
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('rcu_cc_pairs_bytes', 'rcu_cc_pairs', 'rcu_cc_pairs_set_hash_shift')
CASES = ('merge', 'bridge', 'small', 'half', 'notarget', 'nopred', 'noise', 'img', 'img2')
CONFIGS = tuple((conn, radius) for conn in (6, 26) for radius in (0, 2))
ONE = 1 << 24
# Both sides of a float comparison are one division of exact integers, or an exactly rounded sum of at most a few hundred such ratios in
# [0, 1] divided once (scikit-learn and numpy sum in another order): a few hundred * 2^-53 < 1e-12 -- rounding, not slack.
TOL = 1e-12


def as_components(rows):
    from rcu_amd import evaluation as ev
    out = np.zeros(len(rows), dtype=ev.COMPONENT_DTYPE)
    for i, k in enumerate(('root', 'voxels', 'other_voxels', 'unc_sum', 'unc_max')):
        out[k] = np.asarray(rows, dtype=np.int64).reshape(-1, 5)[:, i]
    return out


def as_pairs(rows):
    from rcu_amd import evaluation as ev
    out = np.zeros(len(rows), dtype=ev.PAIR_DTYPE)
    for i, k in enumerate(('a', 'b', 'voxels', 'inside_voxels')):
        out[k] = np.asarray(rows, dtype=np.int64).reshape(-1, 4)[:, i]
    return out


def pair_rows(table):
    """A structured table of PAIR_DTYPE -> the [M, 4] int64 layout of the fixture."""
    return np.stack([table[k].astype(np.int64) for k in ('a', 'b', 'voxels', 'inside_voxels')], axis=1).reshape(-1, 4)


def component_rows(table):
    return np.stack([table[k].astype(np.int64) for k in ('root', 'voxels', 'other_voxels', 'unc_sum', 'unc_max')], axis=1).reshape(-1, 5)


def fixture():
    g = load_golden('g27_lesions')
    assert tuple(str(c) for c in g['cases']) == CASES
    return g


def fixture_tables(g, name, conn, radius):
    tag = '{}_c{}_r{}_'.format(name, conn, radius)
    return as_components(g[tag + 'pred_table']), as_components(g[tag + 'lesion_table']), as_pairs(g[tag + 'pairs'])


def parameter_sets(g):
    return {str(n): (int(p[0]), float(p[1]), int(p[2])) for n, p in zip(g['parameter_names'], g['parameters'])}


def close(a, b):
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= TOL


def same_metrics(a, b):
    return list(a) == list(b) and all((isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or
                                      (a[k] == b[k] and type(a[k]) is type(b[k])) for k in a)


def numpy_pairs(a, b, inside=None):
    """np.unique over the stacked label pairs of one volume -> [M, 4] int64 sorted by (a, b)."""
    a, b = np.asarray(a).reshape(-1).astype(np.int64), np.asarray(b).reshape(-1).astype(np.int64)
    both = (a > 0) & (b > 0)
    if not both.any():
        return np.zeros((0, 4), dtype=np.int64)
    keys, inverse, counts = np.unique(np.stack([a[both], b[both]], axis=1), axis=0, return_inverse=True, return_counts=True)
    ins = np.zeros(len(keys), dtype=np.int64)
    if inside is not None:
        np.add.at(ins, inverse.reshape(-1), (np.asarray(inside).reshape(-1)[both] != 0).astype(np.int64))
    return np.concatenate([keys, counts[:, None], ins[:, None]], axis=1).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope='module')
def lib():
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    return _lib


def test_pair_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, 'include', 'rcu.h')).read()
    declared = set(re.findall(r'\b(rcu_[a-z0-9_]+)\s*\(', header))
    so = lib.load()
    for name in NAMES:
        assert name in declared and name in lib.SIGNATURES and hasattr(so, name), name
    assert 'rcu_cc_pairs.hip' in open(os.path.join(ROOT, 'reliability-challenges-uncertainty_amd', 'csrc', 'Makefile')).read()


def test_pair_struct_has_the_layout_of_the_header(tmp_path):
    """PAIR_DTYPE mirrors include/rcu.h's rcu_cc_pair by hand: compile the header with gcc as a C translation unit and compare the size and
    every field offset (as test_abi_cpu.py does for the ctypes structs)."""
    from rcu_amd import evaluation as ev
    fields = ('a', 'b', 'voxels', 'inside_voxels')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rcu.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(rcu_cc_pair));']
    lines += ['  printf("{0} %zu\\n", offsetof(rcu_cc_pair, {0}));'.format(f) for f in fields]
    lines += ['  printf("width %zu\\n", sizeof(((rcu_cc_pair*)0)->inside_voxels));', '  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines) + '\n')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    seen = dict((line.split()[0], int(line.split()[1])) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert seen['size'] == ev.PAIR_DTYPE.itemsize == 16 and seen['width'] == 4
    assert ev.PAIR_DTYPE.names == fields
    for f in fields:
        assert seen[f] == ev.PAIR_DTYPE.fields[f][1] and ev.PAIR_DTYPE.fields[f][0] == np.dtype('<u4'), f


def test_pair_argument_validation_without_gpu(lib):
    so = lib.load()
    a, b, inside, table = (ctypes.c_void_p(v << 20) for v in (1, 16, 32, 48))

    def refused(status, *words):
        assert status == -1        # RCU_ERR_INVALID
        msg = so.rcu_last_error()
        for w in words:
            assert w in msg, (w, msg)

    def pairs(a_=a, b_=b, i=inside, n=1000, v=2, cap=1024, t=table):
        return so.rcu_cc_pairs(a_, b_, i, n, v, cap, t, None)

    name = b'rcu_cc_pairs:'
    refused(pairs(n=0), name, b'n_per_volume')
    refused(pairs(n=0x7fffffff), name, b'n_per_volume')
    for v in (0, -3, 65536):
        refused(pairs(v=v), name, b'n_volumes')
    refused(pairs(n=1 << 30, v=4), name, b'2^32')
    for cap in (0, 1, 32, 63, 65, 96, 1000, (1 << 26) + 1, 1 << 27, (1 << 26) - 1):
        refused(pairs(cap=cap), name, b'capacity', b'power of two')
    refused(pairs(a_=None), name, b'null', b'a_dev')
    refused(pairs(b_=None), name, b'null', b'b_dev')
    refused(pairs(t=None), name, b'null', b'table_dev')
    refused(pairs(a_=None, cap=100), name, b'capacity')                 # the scalars are judged first, nothing is dereferenced
    refused(pairs(a_=None, v=0), name, b'n_volumes')
    # the size of the table: slots, then two counters per volume, both 256-byte aligned; 0 for arguments out of range
    assert so.rcu_cc_pairs_bytes(64, 1) == 64 * 16 + 256
    assert so.rcu_cc_pairs_bytes(1024, 3) == 3 * 1024 * 16 + 256
    assert so.rcu_cc_pairs_bytes(1 << 26, 8) == 8 * (1 << 30) + 256
    assert so.rcu_cc_pairs_bytes(64, 33) == 33 * 64 * 16 + 512
    for cap, v in ((0, 1), (63, 1), (100, 1), (1 << 27, 1), (64, 0), (64, -1), (64, 65536)):
        assert so.rcu_cc_pairs_bytes(cap, v) == 0, (cap, v)
    try:
        for shift in (-1, 64, 1000):
            refused(so.rcu_cc_pairs_set_hash_shift(shift), b'rcu_cc_pairs_set_hash_shift:', b'0..63')
        for shift in (63, 40, 0):
            assert so.rcu_cc_pairs_set_hash_shift(shift) == 0
    finally:
        so.rcu_cc_pairs_set_hash_shift(0)


def test_python_wrappers_judge_their_arguments_before_the_device():
    from rcu_amd import evaluation as ev
    assert ev.pair_capacity(0, 0) == 1024 and ev.pair_capacity(100, 153) == 1024 and ev.pair_capacity(200, 54) == 1024
    assert ev.pair_capacity(200, 55) == 2048 and ev.pair_capacity(70000, 3) == 1 << 19
    assert [ev._next_power_of_two(x) for x in (0, 1, 2, 3, 64, 65, 2940)] == [1, 1, 2, 4, 64, 128, 4096]
    for bad in (-1, 0.5, 46341):
        with pytest.raises(ValueError):
            ev._check_merge_radius(bad)
    assert ev._check_merge_radius(0) == 0 and ev._check_merge_radius(46340) == 46340 and ev._check_merge_radius(2.0) == 2
    empty = (np.zeros(0, dtype=ev.COMPONENT_DTYPE),) * 2 + (np.zeros(0, dtype=ev.PAIR_DTYPE),)
    for bad in (dict(match_iou=0.49), dict(match_iou=0.0), dict(match_iou=1.0), dict(match_iou=float('nan')), dict(levels=0), dict(min_lesion_voxels=-1)):
        with pytest.raises(ValueError) as info:
            ev.lesion_metrics(empty, **bad)
        if 'match_iou' in bad:
            assert 'one-to-one' in str(info.value)


# -------------------------------------------------------------------------------------------- lesion_metrics against G27
def test_fixture_holds_the_cases_it_is_there_for():
    g = fixture()
    assert tuple(str(k) for k in g['metric_keys']) == __import__('rcu_amd.evaluation', fromlist=['x']).LESION_METRIC_KEYS
    assert len(g['merge_c26_r0_lesion_table']) == 3 and len(g['merge_c26_r2_lesion_table']) == 2              # two blobs closer than r: one lesion
    pairs = g['bridge_c26_r0_pairs']
    assert max(np.bincount(pairs[:, 0])) == 2                                                                    # one component, two lesions
    keys = [str(k) for k in g['metric_keys']]
    small = dict(zip(keys, g['small_c26_r0_metrics_coarse'])), dict(zip(keys, g['small_c26_r0_metrics_default']))
    assert (small[0]['n_lesions'], small[0]['n_fp_components']) == (1, 1) and (small[1]['n_lesions'], small[1]['n_fp_components']) == (2, 0)
    half = g['half_c26_r0_lesions_default']
    assert list(half[:, 9]) == [0.5, 0.75] and list(half[:, 8]) == [0, 2]                                        # IoU exactly 0.5 is no match
    assert len(g['notarget_c6_r2_lesion_table']) == 0 and len(g['notarget_c6_r2_pairs']) == 0 and len(g['notarget_c6_r2_pred_table']) > 0
    assert len(g['nopred_c6_r0_pred_table']) == 0 and len(g['nopred_c6_r0_lesion_table']) > 0
    assert g['img_prediction'].ndim == 2 and g['img2_prediction'].ndim == 2 and max(g[c + '_prediction'].size for c in CASES) <= 24 * 40 * 48
    # the lesion tables' true sizes add up to the target, the pairs' inside voxels to the overlap
    for name in CASES:
        pred, target = g[name + '_prediction'] != 0, g[name + '_target'] != 0
        for conn, radius in CONFIGS:
            tag = '{}_c{}_r{}_'.format(name, conn, radius)
            assert int(g[tag + 'lesion_table'][:, 2].sum()) == int(target.sum()) and int(g[tag + 'pairs'][:, 3].sum()) == int((pred & target).sum())
            assert int(g[tag + 'pred_table'][:, 1].sum()) == int(pred.sum())


def test_lesion_metrics_match_the_mask_based_procedure_g27():
    from rcu_amd import evaluation as ev
    g = fixture()
    keys = [str(k) for k in g['metric_keys']]
    assert tuple(str(k) for k in g['curve_keys']) == ev.LESION_CURVE_KEYS and tuple(str(k) for k in g['list_keys']) == ev.LESION_LIST_KEYS
    seen = 0
    for name in CASES:
        for conn, radius in CONFIGS:
            tag = '{}_c{}_r{}_'.format(name, conn, radius)
            tables = fixture_tables(g, name, conn, radius)
            for pname, (levels, match_iou, min_voxels) in parameter_sets(g).items():
                metrics, curve, listed = ev.lesion_analysis(tables, levels, match_iou, min_voxels)
                assert list(metrics) == list(ev.LESION_METRIC_KEYS) and same_metrics(metrics, ev.lesion_metrics(tables, levels, match_iou, min_voxels))
                for key, expect in zip(keys, g[tag + 'metrics_' + pname]):
                    if key in ev.LESION_COUNT_KEYS:
                        assert isinstance(metrics[key], int) and metrics[key] == int(expect), (tag, pname, key)
                    else:
                        assert close(metrics[key], expect), (tag, pname, key, metrics[key], float(expect))
                if tag + 'curve_' + pname in g:
                    expect = g[tag + 'curve_' + pname]
                    assert len(curve) == levels + 1 == len(expect)
                    for row, ref in zip(curve, expect):
                        assert list(row) == list(ev.LESION_CURVE_KEYS)
                        assert row['n_predicted'] == int(ref[0]) and row['n_matched'] == int(ref[1]) and all(close(row[k], r) for k, r in zip(ev.LESION_CURVE_KEYS[2:], ref[2:]))
                (rows,) = listed
                expect = g[tag + 'lesions_' + pname]
                assert len(rows) == len(expect) == metrics['n_lesions']
                for row, ref in zip(rows, expect):
                    assert list(row) == list(ev.LESION_LIST_KEYS)
                    for key, r in zip(ev.LESION_LIST_KEYS, ref):
                        assert (close(row[key], r) if key in ('dice', 'iou') else (isinstance(row[key], int) and row[key] == int(r))), (tag, pname, key)
                seen += 1
    assert seen == 9 * 4 * 3


def test_pooled_metrics_match_the_fixture_and_do_not_depend_on_order_or_splitting():
    from rcu_amd import evaluation as ev
    g = fixture()
    keys = [str(k) for k in g['metric_keys']]
    pools = {str(n): str(m).split(',') for n, m in zip(g['pool_names'], g['pool_members'])}
    rng = np.random.RandomState(2)
    for pool, members in pools.items():
        for conn, radius in CONFIGS:
            subjects = [fixture_tables(g, m, conn, radius) for m in members]
            for pname, (levels, match_iou, min_voxels) in parameter_sets(g).items():
                tag = 'pooled_{}_c{}_r{}_'.format(pool, conn, radius)
                metrics, curve, listed = ev.lesion_analysis(subjects, levels, match_iou, min_voxels)
                for key, expect in zip(keys, g[tag + 'metrics_' + pname]):
                    assert close(metrics[key], expect), (tag, pname, key, metrics[key], float(expect))
                if tag + 'curve_' + pname in g:
                    assert all(close(row[k], r) for row, ref in zip(curve, g[tag + 'curve_' + pname]) for k, r in zip(ev.LESION_CURVE_KEYS, ref))
                # any order of the subjects and of the rows of the pair tables: the same bits
                for _ in range(3):
                    order = rng.permutation(len(subjects))
                    shuffled = [(subjects[i][0], subjects[i][1], subjects[i][2][rng.permutation(len(subjects[i][2]))]) for i in order]
                    again, curve_again, listed_again = ev.lesion_analysis(shuffled, levels, match_iou, min_voxels)
                    assert same_metrics(again, metrics) and len(curve_again) == len(curve) and all(same_metrics(a, b) for a, b in zip(curve_again, curve))
                    assert [listed_again[list(order).index(i)] for i in range(len(subjects))] == listed
                # the integer totals of the parts add up; the lesions' rows are the subjects' own
                parts = [ev.lesion_analysis(s, levels, match_iou, min_voxels) for s in subjects]
                for key in ev.LESION_COUNT_KEYS:
                    assert metrics[key] == sum(p[0][key] for p in parts), key
                assert listed == [p[2][0] for p in parts]
                half = len(subjects) // 2
                split = [ev.lesion_analysis(subjects[:half], levels, match_iou, min_voxels), ev.lesion_analysis(subjects[half:], levels, match_iou, min_voxels)]
                assert listed == split[0][2] + split[1][2]
                for k in range(levels + 1):
                    assert curve[k]['n_predicted'] == split[0][1][k]['n_predicted'] + split[1][1][k]['n_predicted']
                    assert curve[k]['n_matched'] == split[0][1][k]['n_matched'] + split[1][1][k]['n_matched']


def test_hand_made_tables():
    from rcu_amd import evaluation as ev
    # components: 1 = a good hit on lesion 1 (certain), 2 = a bridge over lesions 2 and 3 (uncertain), 3 = a false positive (most uncertain)
    comps = as_components([[0, 10, 8, 10 * (ONE // 10), ONE // 2], [50, 20, 9, 20 * (ONE // 2), ONE], [90, 4, 0, 4 * (3 * ONE // 4), ONE]])
    lesions = as_components([[1, 10, 10, 0, 0], [52, 6, 6, 0, 0], [60, 8, 8, 0, 0], [99, 2, 2, 0, 0]])
    pairs = as_pairs([[1, 1, 8, 8], [2, 2, 4, 4], [2, 3, 5, 5]])
    m, curve, (rows,) = ev.lesion_analysis((comps, lesions, pairs), levels=4)
    assert [m[k] for k in ev.LESION_COUNT_KEYS] == [4, 3, 1, 1, 1]
    d = [2 * 8 / (10 + 10), 2 * 4 / (6 + 20), 2 * 5 / (8 + 20), 0.0]
    assert m['lesion_dice'] == math.fsum(d) / (4 + 1)
    assert m['lesion_recall'] == 1 / 4 and m['lesion_precision'] == 1 / 3 and m['lesion_f1'] == 2 / 7
    assert m['sq'] == 8 / 12 and m['pq'] == (8 / 12) / (1 + 0.5 * 2 + 0.5 * 3)
    assert m['auroc_unmatched'] == 1.0 and abs(m['auprc_unmatched'] - 1.0) <= TOL           # both unmatched components are more uncertain than the match
    assert [r['matched_component'] for r in rows] == [1, 0, 0, 0] and [r['n_touching'] for r in rows] == [1, 1, 1, 0]
    assert [r['iou'] for r in rows] == [8 / 12, 4 / 22, 5 / 23, 0.0] and [r['dice'] for r in rows] == d
    # thresholds 0, 1/4, .., 1: the means are just under 0.1, 0.5 and 0.75 -> the components arrive at k = 1, 2, 3
    assert (ONE // 10) / ONE < 0.25 and [c['n_predicted'] for c in curve] == [0, 1, 2, 3, 3] and [c['n_matched'] for c in curve] == [0, 1, 1, 1, 1]
    assert [c['lesion_dice'] for c in curve] == [0.0, d[0] / 4, math.fsum(d) / 4, math.fsum(d) / 5, math.fsum(d) / 5]
    assert math.isnan(curve[0]['fdr']) and [c['fdr'] for c in curve[1:]] == [0.0, 1 / 2, 2 / 3, 2 / 3]
    assert (m['lesion_dice_filtered_max'], m['lesion_dice_filtered_max_threshold']) == (math.fsum(d) / 4, 0.5)
    assert (m['lesion_f1_filtered_max'], m['lesion_f1_filtered_max_threshold']) == (2 / 5, 0.25)
    # min_lesion_voxels drops lesion 4 (2 voxels) and lesion 2 (6): component 2 still touches lesion 3
    m7 = ev.lesion_metrics((comps, lesions, pairs), levels=4, min_lesion_voxels=7)
    assert [m7[k] for k in ev.LESION_COUNT_KEYS] == [2, 3, 1, 1, 0] and m7['lesion_dice'] == math.fsum([d[0], d[2]]) / 3
    m9 = ev.lesion_metrics((comps, lesions, pairs), levels=4, min_lesion_voxels=9)                   # ... and now it is a false positive
    assert [m9[k] for k in ev.LESION_COUNT_KEYS] == [1, 3, 1, 2, 0]
    # a stricter IoU: 8 / 12 is no match above 0.7
    assert ev.lesion_metrics((comps, lesions, pairs), levels=4, match_iou=0.7)['n_matched'] == 0
    # the exact running sum takes terms back without a trace
    total = ev._ExactSum()
    for x in (1e100, 1.0, -1e100, 0.1, -1.0):
        total.add(x)
    assert total.value() == 0.1


# ------------------------------------------------------------------------------------------------------------ the action
def _rows(path):
    with open(path, newline='') as f:
        return list(csv.reader(f))


def test_action_writes_its_four_files_from_fixture_tables(tmp_path):
    from rcu_amd import evalrun, evaluation as ev
    g = fixture()
    base = str(tmp_path / 'eval')
    (action,) = evalrun.get_actions(['lesions'], os.path.join(base, evalrun.MINMAX_NAME), base, 'foreground', levels=20, connectivity=6, merge_radius=2,
                                    min_lesion_voxels=0, match_iou=0.7)
    assert isinstance(action, evalrun.LesionsAction)
    assert (action.levels, action.connectivity, action.merge_radius, action.min_lesion_voxels, action.match_iou) == (20, 6, 2, 0, 0.7)
    action.setup_eval(evalrun.EvalData('baseline_mc', 'unused', 'probabilities'))
    members = ('noise', 'merge', 'notarget')
    subjects = {m: fixture_tables(g, m, 6, 2) for m in members}
    for m in members:
        action.record_tables(subjects[m], 'subject_' + m)
    action.finish_eval()
    out = os.path.join(base, evalrun.UNCERTAINTY_NAME)
    assert sorted(os.listdir(out)) == ['eval_lesion_curve_baseline_mc.csv', 'eval_lesion_list_baseline_mc.csv', 'eval_lesions_baseline_mc.csv',
                                       'eval_lesions_pooled_baseline_mc.csv']
    rows = _rows(os.path.join(out, 'eval_lesions_baseline_mc.csv'))
    assert rows[0] == ['test_id', 'subject_name'] + list(ev.LESION_METRIC_KEYS) and len(rows) == 4
    keys = [str(k) for k in g['metric_keys']]
    for row, m in zip(rows[1:], members):
        expect = ev.lesion_metrics(subjects[m], 20, 0.7, 0)
        assert row == ['baseline_mc', 'subject_' + m] + [str(expect[k]) for k in ev.LESION_METRIC_KEYS]
        for key, ref in zip(keys, g['{}_c6_r2_metrics_strict'.format(m)]):                             # ... which are the mask-based values
            assert close(float(row[2 + keys.index(key)]), ref), (m, key)
    pooled, curve, _ = ev.lesion_analysis([subjects[m] for m in members], 20, 0.7, 0)
    assert _rows(os.path.join(out, 'eval_lesions_pooled_baseline_mc.csv')) == [['test_id'] + list(ev.LESION_METRIC_KEYS),
                                                                               ['baseline_mc'] + [str(pooled[k]) for k in ev.LESION_METRIC_KEYS]]
    listed = _rows(os.path.join(out, 'eval_lesion_list_baseline_mc.csv'))
    assert listed[0] == ['subject', 'lesion', 'root_index', 'voxels', 'dilated_voxels', 'n_touching', 'touching_voxels', 'overlap', 'dice',
                         'matched_component', 'iou']
    expect = [['subject_' + m] + [str(r[k]) for k in ev.LESION_LIST_KEYS] for m in members for r in ev.lesion_analysis(subjects[m], 20, 0.7, 0)[2][0]]
    assert listed[1:] == expect and len(expect) == pooled['n_lesions'] > 2
    lines = _rows(os.path.join(out, 'eval_lesion_curve_baseline_mc.csv'))
    assert lines[0] == ['level', 'threshold'] + list(ev.LESION_CURVE_KEYS) and len(lines) == 22
    assert lines[1:] == [[str(k), str(k / 20)] + [str(row[c]) for c in ev.LESION_CURVE_KEYS] for k, row in enumerate(curve)]
    # the pooled files do not depend on the order in which the subjects arrived; a second run of the object starts from nothing
    action.setup_eval(evalrun.EvalData('center', 'unused', 'probabilities'))
    for m in members[::-1]:
        action.record_tables(subjects[m], 'subject_' + m)
    action.finish_eval()
    for name in ('eval_lesions_pooled_{}.csv', 'eval_lesion_curve_{}.csv'):
        a, b = _rows(os.path.join(out, name.format('baseline_mc'))), _rows(os.path.join(out, name.format('center')))
        assert [r[1:] if 'pooled' in name else r for r in a] == [r[1:] if 'pooled' in name else r for r in b]
    assert len(_rows(os.path.join(out, 'eval_lesions_center.csv'))) == 4


def test_action_is_registered_refuses_bad_arguments_and_is_not_a_default(tmp_path):
    from rcu_amd import evalrun
    base = str(tmp_path / 'eval')
    mm = os.path.join(base, evalrun.MINMAX_NAME)
    actions = evalrun.get_actions(['lesions'], mm, base, 'foreground')
    assert len(actions) == 1 and isinstance(actions[0], evalrun.LesionsAction)
    assert (actions[0].levels, actions[0].connectivity, actions[0].merge_radius, actions[0].min_lesion_voxels, actions[0].match_iou) == (1000, 26, 0, 0, 0.5)
    assert (actions[0].rescale_confidence, actions[0].rescale_sigma) == ('subject', 'global')      # as ComponentsAction prepares
    assert evalrun.metrics_wanted(actions) == (['minmax', 'lesions'], (0.5,), False)                # no brain mask
    actions = evalrun.get_actions(['minmax', 'components', 'lesions'], mm, base, '', levels=64, connectivity=6, merge_radius=3)
    assert [type(a).__name__ for a in actions] == ['SaveMinMaxAction', 'ComponentsAction', 'LesionsAction']
    assert evalrun.metrics_wanted(actions) == (['minmax', 'components', 'lesions'], (0.5,), False)
    assert evalrun._fusable(evalrun.EvalData('baseline', 'unused', 'probabilities'), actions)
    assert not evalrun._fusable(evalrun.EvalData('aleatoric', 'unused', 'sigma'), actions)
    # runs without it ask for exactly what they asked for before
    assert evalrun.metrics_wanted(evalrun.get_actions(['minmax', 'ece_dice', 'calib', 'bnf_ue'], mm, base, 'foreground'))[0] == ['ece', 'minmax', 'ue']
    assert evalrun.metrics_wanted(evalrun.get_actions(['components'], mm, base, ''))[0] == ['minmax', 'components']
    for bad in (dict(match_iou=0.49), dict(match_iou=0.3), dict(match_iou=1.0), dict(merge_radius=-1), dict(merge_radius=1.5), dict(min_lesion_voxels=-2),
                dict(connectivity=18), dict(levels=1)):
        with pytest.raises(ValueError) as info:
            evalrun.get_actions(['lesions'], mm, base, '', **bad)
        assert list(bad)[0] in str(info.value)
    script = open(os.path.join(ROOT, 'bin-eval', 'eval_uncertainty.py')).read()
    assert "acts = args.act or ['minmax', 'ece_dice', 'calib', 'bnf_ue']" in script
    for flag in ("'--merge_radius'", "'--min_lesion_voxels'", "'--match_iou'"):
        assert flag in script
    import inspect
    from rcu_amd import scripts
    for fn in (scripts.eval_uncertainty, evalrun.evaluate_runs, evalrun.get_actions):
        params = inspect.signature(fn).parameters
        assert (params['merge_radius'].default, params['min_lesion_voxels'].default, params['match_iou'].default) == (0, 0, 0.5)
    assert inspect.signature(scripts.eval_uncertainty).parameters['actions'].default == ('minmax', 'ece_dice', 'calib', 'bnf_ue')
