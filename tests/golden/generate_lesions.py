#!/usr/bin/env python3
"""G27: yardsticks of the component-pair table, the lesion tables and the lesion-wise metrics.

Nothing here goes through the table algebra of rcu_amd.evaluation.lesion_metrics: components are scipy.ndimage.label's, the dilation is
rint(distance_transform_edt(target == 0) ** 2) <= r * r, the pair table is np.unique over the stacked label pairs, and the metrics follow the
BraTS 2023 procedure written out on MASKS -- every lesion's mask, the union mask of the predicted components that touch its dilation, Dice
and IoU counted from those masks --, the two detection scores are scikit-learn's.  The filtering curve removes the components from the
prediction MASK, threshold by threshold, and runs the whole procedure again.

Cases (prediction mask, target mask, float64 uncertainty):
  merge     24 x 40 x 48: two target blobs closer than the dilation (one lesion at r = 2, two at r = 0), a far third one, predictions on each
  bridge    12 x 20 x 30: one predicted bar that bridges two lesions, a false positive, a missed lesion
  small     10 x 16 x 20: a 3-voxel lesion (dropped at min_lesion_voxels = 5; the component on it becomes a false positive) beside a large one
  half      6 x 8 x 10: a component and a lesion of 3 voxels each that share 2: an IoU of exactly 0.5 (not a match), and one of 3 / 4 (a match)
  notarget  8 x 9 x 10: an empty target;      nopred   8 x 9 x 10: an empty prediction
  noise     12 x 17 x 19: thresholded smooth noise, dozens of lesions and components
  img, img2 24 x 32 and 17 x 40 images (depth 1: the 4- / 8-neighbourhoods)
Per case, connectivity c in (6, 26) and merge radius r in (0, 2), under the tag <case>_c<c>_r<r>_:
  pred_table     int64 [K, 5]  root, voxels, target voxels, unc_sum, unc_max of the predicted components (G23's layout)
  lesion_table   int64 [L, 5]  root, dilated voxels, true voxels, 0, 0 of the lesions
  pairs          int64 [M, 4]  a, g, voxels, inside_voxels sorted by (a, g): labels 1..K / 1..L in table order
  metrics_<p>    float64 [len(metric_keys)] for the parameter sets p of `PARAMETERS` (levels, match_iou, min_lesion_voxels)
  curve_<p>      float64 [levels + 1, len(curve_keys)] (the parameter sets of at most 100 levels)
  lesions_<p>    float64 [kept lesions, len(list_keys)]
pooled_<group>_c<c>_r<r>_metrics_<p> / _curve_<p>: the same procedure over several subjects at once (`POOLS`).
Output: tests/golden/g27_lesions.npz (arrays, numbers and lists of names only).

    python tests/golden/generate_lesions.py
"""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ONE = 1 << 24
METRIC_KEYS = ('n_lesions', 'n_predicted', 'n_matched', 'n_fp_components', 'n_missed_lesions', 'lesion_dice', 'lesion_recall', 'lesion_precision',
               'lesion_f1', 'sq', 'pq', 'auroc_unmatched', 'auprc_unmatched', 'lesion_dice_filtered_max', 'lesion_dice_filtered_max_threshold',
               'lesion_f1_filtered_max', 'lesion_f1_filtered_max_threshold')
CURVE_KEYS = ('n_predicted', 'n_matched', 'lesion_recall', 'fdr', 'lesion_dice')
LIST_KEYS = ('lesion', 'root_index', 'voxels', 'dilated_voxels', 'n_touching', 'touching_voxels', 'overlap', 'dice', 'matched_component', 'iou')
PARAMETERS = {'default': (1000, 0.5, 0), 'coarse': (7, 0.5, 5), 'strict': (20, 0.7, 0)}
CASES = ('merge', 'bridge', 'small', 'half', 'notarget', 'nopred', 'noise', 'img', 'img2')
POOLS = {'all3d': ('merge', 'bridge', 'small', 'half', 'notarget', 'nopred', 'noise'), 'images': ('img', 'img2')}
NAN = float('nan')


def quantise(u):
    with np.errstate(invalid='ignore'):
        q = np.rint(np.clip(np.asarray(u, dtype=np.float64), 0.0, 1.0) * np.float64(ONE))
    return np.where(np.isnan(q), 0, q).astype(np.int64)


def structure(ndim, connectivity):
    from scipy import ndimage
    return ndimage.generate_binary_structure(ndim, 1 if connectivity == 6 else ndim)


def label(mask, connectivity):
    from scipy import ndimage
    return ndimage.label(mask, structure=structure(mask.ndim, connectivity))


def dilation(target, radius):
    from scipy import ndimage
    fg = target != 0
    if radius == 0 or not fg.any():
        return fg
    return np.rint(ndimage.distance_transform_edt(~fg) ** 2) <= radius * radius


def ratio(num, den):
    return num / den if den else NAN


def tables(pred, target, unc, connectivity, radius):
    """-> (pred labels, lesion labels, pred_table, lesion_table, pairs), everything from scipy.ndimage.label and numpy counting."""
    q = quantise(unc)
    tgt = target != 0
    p_labels, k = label(pred != 0, connectivity)
    l_labels, n_l = label(dilation(target, radius), connectivity)
    pred_table = np.zeros((k, 5), dtype=np.int64)
    for a in range(1, k + 1):
        m = p_labels == a
        pred_table[a - 1] = [np.flatnonzero(m.reshape(-1))[0], m.sum(), (m & tgt).sum(), q[m].sum(), q[m].max()]
    lesion_table = np.zeros((n_l, 5), dtype=np.int64)
    for g in range(1, n_l + 1):
        m = l_labels == g
        lesion_table[g - 1] = [np.flatnonzero(m.reshape(-1))[0], m.sum(), (m & tgt).sum(), 0, 0]
    both = (p_labels > 0) & (l_labels > 0)
    stacked = np.stack([p_labels[both], l_labels[both], tgt[both].astype(np.int64)], axis=1).astype(np.int64)
    keys, counts = np.unique(stacked[:, :2], axis=0, return_counts=True) if len(stacked) else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    inside = np.array([int(stacked[(stacked[:, 0] == a) & (stacked[:, 1] == g), 2].sum()) for a, g in keys], dtype=np.int64)
    pairs = np.concatenate([keys, counts[:, None], inside[:, None]], axis=1).astype(np.int64).reshape(-1, 4)
    return p_labels, l_labels, pred_table, lesion_table, pairs


def procedure(subjects, match_iou, min_lesion_voxels, kept_components=None):
    """The BraTS procedure on masks for a list of subjects (p_labels, l_labels, target mask, mean uncertainty per component); with
    ``kept_components`` (one boolean array per subject) the other components are erased from the prediction first.
    -> (counts and ratios, scores and flags of the components, the lesions' rows per subject)."""
    dices, ious, scores, unmatched, listed = [], [], [], [], []
    n_lesions = n_predicted = n_fp = n_missed = 0
    for s, (p_all, l_labels, tgt, mean) in enumerate(subjects):
        keep = np.ones(len(mean), dtype=bool) if kept_components is None else kept_components[s]
        p_labels = np.where(np.concatenate([[False], keep])[p_all], p_all, 0)
        present = [a for a in range(1, len(mean) + 1) if keep[a - 1]]
        lesions = [g for g in range(1, int(l_labels.max()) + 1) if int(((l_labels == g) & tgt).sum()) >= max(min_lesion_voxels, 1)]
        kept_dilation = np.isin(l_labels, lesions)
        matched, rows = set(), []
        for g in lesions:
            dil = l_labels == g
            lesion = dil & tgt
            touching = [a for a in np.unique(p_labels[dil]) if a > 0]
            union = np.isin(p_labels, touching)
            dice = 2 * int((union & lesion).sum()) / (int(lesion.sum()) + int(union.sum()))
            dices.append(dice)
            n_missed += not touching
            best, best_a = 0.0, 0
            for a in touching:
                comp = p_labels == a
                iou = int((comp & lesion).sum()) / int((comp | lesion).sum())
                if iou > best:
                    best, best_a = iou, int(a)
                if iou > match_iou:
                    matched.add(int(a))
                    ious.append(iou)
            rows.append([g, np.flatnonzero(dil.reshape(-1))[0], lesion.sum(), dil.sum(), len(touching), union.sum(), (union & lesion).sum(), dice,
                         best_a if best > match_iou else 0, best])
        listed.append(np.array(rows, dtype=np.float64).reshape(-1, len(LIST_KEYS)))
        n_lesions += len(lesions)
        n_predicted += len(present)
        n_fp += sum(1 for a in present if not (kept_dilation & (p_labels == a)).any())
        for a in present:
            scores.append(mean[a - 1])
            unmatched.append(a not in matched)
    tp = len(ious)
    out = {'n_lesions': n_lesions, 'n_predicted': n_predicted, 'n_matched': tp, 'n_fp_components': n_fp, 'n_missed_lesions': n_missed,
           'lesion_dice': ratio(math.fsum(dices), n_lesions + n_fp), 'lesion_recall': ratio(tp, n_lesions), 'lesion_precision': ratio(tp, n_predicted),
           'lesion_f1': ratio(2 * tp, n_lesions + n_predicted), 'sq': ratio(math.fsum(ious), tp),
           'pq': ratio(math.fsum(ious), tp + 0.5 * (n_predicted - tp) + 0.5 * (n_lesions - tp)),
           'fdr': ratio(n_predicted - tp, n_predicted)}
    return out, np.array(scores, dtype=np.float64), np.array(unmatched, dtype=bool), listed


def better(value, best):
    return best is None or value > best or (best != best and value == value)


def evaluate(subjects, levels, match_iou, min_lesion_voxels):
    from sklearn.metrics import average_precision_score, roc_auc_score
    base, scores, unmatched, listed = procedure(subjects, match_iou, min_lesion_voxels)
    metrics = {k: base[k] for k in METRIC_KEYS if k in base}
    both = 0 < int(unmatched.sum()) < unmatched.size
    metrics['auroc_unmatched'] = roc_auc_score(unmatched, scores) if both else NAN
    metrics['auprc_unmatched'] = average_precision_score(unmatched, scores) if unmatched.any() else NAN
    curve, seen, best_dice, best_f1 = [], {}, None, None
    for k in range(levels + 1):
        kept = [~(s[3] > k / levels) for s in subjects]
        key = b''.join(np.asarray(m).tobytes() for m in kept)
        if key not in seen:
            seen[key] = procedure(subjects, match_iou, min_lesion_voxels, kept)[0]
        row = seen[key]
        curve.append([row[c] for c in CURVE_KEYS])
        if better(row['lesion_dice'], None if best_dice is None else best_dice[0]):
            best_dice = (row['lesion_dice'], k / levels)
        if better(row['lesion_f1'], None if best_f1 is None else best_f1[0]):
            best_f1 = (row['lesion_f1'], k / levels)
    metrics.update(lesion_dice_filtered_max=best_dice[0], lesion_dice_filtered_max_threshold=best_dice[1], lesion_f1_filtered_max=best_f1[0],
                   lesion_f1_filtered_max_threshold=best_f1[1])
    return np.array([metrics[k] for k in METRIC_KEYS], dtype=np.float64), np.array(curve, dtype=np.float64), listed


def blob(shape, centre, radii):
    grids = np.ogrid[tuple(slice(0, e) for e in shape)]
    return sum(((g - c) / r) ** 2 for g, c, r in zip(grids, centre, radii)) <= 1.0


def make_cases():
    from scipy import ndimage
    rng = np.random.RandomState(27)
    cases = {}
    shape = (24, 40, 48)
    target = blob(shape, (8, 12, 12), (4, 5, 6)) | blob(shape, (8, 12, 23), (3, 4, 3)) | blob(shape, (17, 30, 38), (4, 6, 5))      # a gap of 2 voxels along x
    pred = blob(shape, (8, 13, 13), (4, 5, 5)) | blob(shape, (9, 12, 24), (2, 3, 3)) | blob(shape, (17, 29, 37), (5, 6, 6)) | blob(shape, (3, 33, 6), (2, 2, 3))
    cases['merge'] = (pred, target)
    shape = (12, 20, 30)
    target = blob(shape, (5, 6, 6), (3, 4, 4)) | blob(shape, (5, 6, 22), (3, 4, 4)) | blob(shape, (9, 16, 14), (2, 2, 3))
    pred = np.zeros(shape, dtype=bool)
    pred[4:7, 5:8, 4:25] = True                       # the bridge
    pred[1:3, 16:19, 25:29] = True                    # a false positive
    cases['bridge'] = (pred, target)
    shape = (10, 16, 20)
    target = blob(shape, (5, 8, 6), (3, 4, 4))
    target[2, 2, 15:18] = True                        # 3 voxels
    pred = blob(shape, (5, 8, 7), (3, 4, 4))
    pred[2, 2, 14:18] = True
    cases['small'] = (pred, target)
    shape = (6, 8, 10)
    target, pred = np.zeros(shape, dtype=bool), np.zeros(shape, dtype=bool)
    target[1, 1, 1:4], pred[1, 1, 2:5] = True, True                    # 3 and 3 share 2: IoU 2 / 4
    target[4, 5, 2:6], pred[4, 5, 2:5] = True, True                    # 4 and 3 share 3: IoU 3 / 4
    cases['half'] = (pred, target)
    shape = (8, 9, 10)
    cases['notarget'] = (rng.rand(*shape) < 0.05, np.zeros(shape, dtype=bool))
    cases['nopred'] = (np.zeros(shape, dtype=bool), blob(shape, (4, 4, 5), (2, 2, 3)) | (rng.rand(*shape) < 0.01))
    for name, shape, sigma in (('noise', (12, 17, 19), 1.0), ('img', (24, 32), 1.5), ('img2', (17, 40), 1.2)):
        field = ndimage.gaussian_filter(rng.randn(*shape), sigma)
        other = 0.7 * field + 0.3 * ndimage.gaussian_filter(rng.randn(*shape), sigma)
        cases[name] = (other > np.percentile(other, 88), field > np.percentile(field, 90))
    out = {}
    for name, (pred, target) in cases.items():
        unc = rng.rand(*pred.shape)
        if pred.any():      # component-wise different means: noisy inside some components, calm inside others
            labels, k = label(pred, 26)
            scale = np.concatenate([[1.0], rng.rand(k) ** 2])
            unc = unc * scale[labels]
        unc = np.floor(unc * 64) / 64                  # (six bits per voxel: the file stays small, equal values repeat)
        flat = unc.reshape(-1)
        flat[::13] = np.round(flat[::13], 2)
        flat[1:40:5] = (np.arange(8) + 0.5) / ONE
        flat[3], flat[7], flat[12] = -0.25, 1.5, np.nan
        out[name] = (pred.astype(np.uint8), target.astype(np.uint8) * 2, unc)
    return out


def main():
    import scipy
    import sklearn
    arrays = {'scipy_version': np.array(scipy.__version__), 'sklearn_version': np.array(sklearn.__version__), 'numpy_version': np.array(np.__version__),
              'cases': np.array(CASES), 'metric_keys': np.array(METRIC_KEYS), 'curve_keys': np.array(CURVE_KEYS), 'list_keys': np.array(LIST_KEYS),
              'parameter_names': np.array(list(PARAMETERS)), 'parameters': np.array([PARAMETERS[k] for k in PARAMETERS], dtype=np.float64),
              'pool_names': np.array(list(POOLS)), 'pool_members': np.array([','.join(POOLS[k]) for k in POOLS])}
    cases = make_cases()
    assert tuple(cases) == CASES
    for name, (pred, target, unc) in cases.items():
        arrays.update({name + '_prediction': pred, name + '_target': target, name + '_uncertainty': unc})
    for conn in (6, 26):
        for radius in (0, 2):
            subjects = {}
            for name, (pred, target, unc) in cases.items():
                tag = '{}_c{}_r{}_'.format(name, conn, radius)
                p_labels, l_labels, pred_table, lesion_table, pairs = tables(pred, target, unc, conn, radius)
                mean = pred_table[:, 3] / (pred_table[:, 1] * np.float64(ONE))
                subjects[name] = (p_labels, l_labels, target != 0, mean)
                arrays.update({tag + 'pred_table': pred_table, tag + 'lesion_table': lesion_table, tag + 'pairs': pairs})
                for pname, (levels, match_iou, min_voxels) in PARAMETERS.items():
                    metrics, curve, listed = evaluate([subjects[name]], levels, match_iou, min_voxels)
                    arrays.update({tag + 'metrics_' + pname: metrics, tag + 'lesions_' + pname: listed[0]})
                    if levels <= 100:      # (the 1001 rows of the default grid are judged through the two maxima)
                        arrays[tag + 'curve_' + pname] = curve
                m = dict(zip(METRIC_KEYS, arrays[tag + 'metrics_default']))
                print('{:9s} c{:<2d} r{} lesions {:3.0f} predicted {:3.0f} matched {:3.0f} fp {:3.0f} dice {:.4f} pq {:.4f} auroc {:.4f}'.format(
                    name, conn, radius, m['n_lesions'], m['n_predicted'], m['n_matched'], m['n_fp_components'], m['lesion_dice'], m['pq'], m['auroc_unmatched']))
            for pool, members in POOLS.items():
                for pname, (levels, match_iou, min_voxels) in PARAMETERS.items():
                    metrics, curve, _ = evaluate([subjects[m] for m in members], levels, match_iou, min_voxels)
                    arrays['pooled_{}_c{}_r{}_metrics_{}'.format(pool, conn, radius, pname)] = metrics
                    if levels <= 100:
                        arrays['pooled_{}_c{}_r{}_curve_{}'.format(pool, conn, radius, pname)] = curve
    # what the cases are there for
    assert len(arrays['merge_c26_r0_lesion_table']) == 3 and len(arrays['merge_c26_r2_lesion_table']) == 2
    assert any((arrays['bridge_c26_r0_pairs'][:, 0] == a).sum() == 2 for a in arrays['bridge_c26_r0_pairs'][:, 0])
    small = dict(zip(METRIC_KEYS, arrays['small_c26_r0_metrics_coarse']))
    assert small['n_lesions'] == 1 and small['n_fp_components'] == 1 and dict(zip(METRIC_KEYS, arrays['small_c26_r0_metrics_default']))['n_lesions'] == 2
    half = arrays['half_c26_r0_lesions_default']
    assert list(half[:, 9]) == [0.5, 0.75] and list(half[:, 8]) == [0.0, 2.0]
    assert len(arrays['notarget_c26_r2_lesion_table']) == 0 and len(arrays['nopred_c26_r2_pred_table']) == 0
    path = os.path.join(HERE, 'g27_lesions.npz')
    np.savez_compressed(path, **arrays)
    print('wrote {} ({:.1f} KiB)'.format(path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
