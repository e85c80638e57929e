#!/usr/bin/env python3
"""G23: yardsticks of the connected-component labelling, the per-component table and the component-level metrics.

The labelling (include/rcu.h, rcu_cc_label / rcu_cc_relabel) numbers the components of a binary mask in raster order of their first voxels,
which is scipy.ndimage.label's numbering; the table (rcu_cc_table) holds per component its first voxel, its size, its overlap with another
map and the sum / maximum of the quantised uncertainty q(u) = rint(clamp(u, 0, 1) * 2^24).  Here they come from scipy.ndimage (label,
sum_labels, maximum), the detection metrics of false-positive components (AUROC / average precision by mean uncertainty) from scikit-learn.

Cases (prediction mask, target mask, float64 uncertainty; both connectivities each):
  d10, d30, d60   random 12 x 17 x 9 volumes, prediction density 0.1 / 0.3 / 0.6, target = a shifted, thinned copy plus noise
  img             a 2-D 24 x 32 image (depth 1: the 4- / 8-neighbourhoods)
  diag            6 x 7 x 8: voxels that touch by edges and corners only -- one component under 26, many under 6 -- plus a few cubes
The uncertainty holds values outside [0, 1], exact ties of the rounding and a NaN.

Per case and connectivity c in (6, 26):
  <case>_c<c>_pred_labels / _target_labels   int32 dense labels
  <case>_c<c>_pred_table / _target_table     int64 [K, 5]: root, voxels, other_voxels, unc_sum, unc_max (the target's table: unc columns 0)
  <case>_c<c>_auroc_fp / _auprc_fp           scikit-learn on (other_voxels == 0, unc_sum / (voxels * 2^24)); NaN where a class is missing
Output: tests/golden/g23_components.npz (arrays and numbers only).

    python tests/golden/generate_components.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ONE = 1 << 24


def quantise(u):
    with np.errstate(invalid='ignore'):
        q = np.rint(np.clip(np.asarray(u, dtype=np.float64), 0.0, 1.0) * np.float64(ONE))
    return np.where(np.isnan(q), 0, q).astype(np.int64)


def structure(ndim, connectivity):
    from scipy import ndimage
    return ndimage.generate_binary_structure(ndim, 1 if connectivity == 6 else ndim)


def table_of(mask, other, q, connectivity):
    from scipy import ndimage
    labels, k = ndimage.label(mask != 0, structure=structure(mask.ndim, connectivity))
    index = np.arange(1, k + 1)
    values, first = np.unique(labels.reshape(-1), return_index=True)
    root = first[values > 0]
    assert np.array_equal(values[values > 0], index) and np.all(np.diff(root) > 0)      # raster order of first voxels
    cols = [root, ndimage.sum_labels(np.ones(mask.shape, dtype=np.int64), labels, index),
            ndimage.sum_labels((other != 0).astype(np.int64), labels, index)]
    if q is None:
        cols += [np.zeros(k), np.zeros(k)]
    else:
        cols += [ndimage.sum_labels(q, labels, index), ndimage.maximum(q, labels, index) if k else np.zeros(0)]
    table = np.stack([np.asarray(c, dtype=np.float64) for c in cols], axis=1) if k else np.zeros((0, 5))
    assert np.all(table == np.rint(table)) and np.all(table < 2.0 ** 53)
    return labels.astype(np.int32), table.astype(np.int64)


def main():
    import scipy
    import sklearn
    from sklearn.metrics import average_precision_score, roc_auc_score

    rng = np.random.RandomState(23)
    arrays = {'scipy_version': np.array(scipy.__version__), 'sklearn_version': np.array(sklearn.__version__),
              'numpy_version': np.array(np.__version__), 'cases': np.array(['d10', 'd30', 'd60', 'img', 'diag'])}

    def uncertainty_for(shape):
        u = rng.rand(*shape)
        flat = u.reshape(-1)
        flat[::11] = np.round(flat[::11], 2)                                  # repeated values
        flat[1:40:5] = (np.arange(8) + 0.5) / ONE                             # exact ties of the rounding: to even
        flat[3], flat[7], flat[12], flat[17] = -0.25, 1.5, np.nan, 1.0
        return u

    cases = {}
    for name, density in (('d10', 0.1), ('d30', 0.3), ('d60', 0.6)):
        shape = (12, 17, 9)
        pred = (rng.rand(*shape) < density).astype(np.uint8)
        target = (np.roll(pred, 1, axis=1) * (rng.rand(*shape) < 0.7) + (rng.rand(*shape) < 0.03)).astype(np.uint8) * 3
        cases[name] = (pred, target, uncertainty_for(shape))
    shape = (24, 32)
    pred = (rng.rand(*shape) < 0.35).astype(np.uint8)
    target = ((rng.rand(*shape) < 0.5) * pred + (rng.rand(*shape) < 0.05)).astype(np.uint8)
    cases['img'] = (pred, target, uncertainty_for(shape))
    shape = (6, 7, 8)
    z, y, x = np.indices(shape)
    pred = (((z + y + x) % 2 == 0) & (z % 2 == 0)).astype(np.uint8)           # a plane checkerboard on every other slice ...
    pred |= ((z % 2 == 1) & (y % 2 == 1) & (x % 2 == 0) & ((y + x) % 4 == 1)).astype(np.uint8)      # ... bridged by corners only
    pred[4:6, 4:6, 5:7] = 1
    target = np.zeros(shape, dtype=np.uint8)
    target[0:3, 0:4, 0:4] = 1
    target[4:6, 4:7, 5:8] = 2
    cases['diag'] = (pred, target, uncertainty_for(shape))

    for name, (pred, target, unc) in cases.items():
        arrays.update({name + '_prediction': pred, name + '_target': target, name + '_uncertainty': unc})
        q = quantise(unc)
        for conn in (6, 26):
            tag = '{}_c{}_'.format(name, conn)
            pred_labels, pred_table = table_of(pred, target, q, conn)
            target_labels, target_table = table_of(target, pred, None, conn)
            is_fp = pred_table[:, 2] == 0
            mean = pred_table[:, 3] / (pred_table[:, 1] * np.float64(ONE))
            both = 0 < int(is_fp.sum()) < is_fp.size
            arrays.update({tag + 'pred_labels': pred_labels, tag + 'pred_table': pred_table, tag + 'target_labels': target_labels,
                           tag + 'target_table': target_table,
                           tag + 'auroc_fp': np.array(roc_auc_score(is_fp, mean) if both else np.nan),
                           tag + 'auprc_fp': np.array(average_precision_score(is_fp, mean) if is_fp.any() else np.nan)})
            print('{:5s} c{:<2d} components {:4d} (fp {:4d})  target components {:4d}  auroc {:.6f}'.format(
                name, conn, len(pred_table), int(is_fp.sum()), len(target_table), float(arrays[tag + 'auroc_fp'])))
    assert len(arrays['diag_c6_pred_table']) > len(arrays['diag_c26_pred_table'])
    path = os.path.join(HERE, 'g23_components.npz')
    np.savez_compressed(path, **arrays)
    print('wrote {} ({:.1f} KiB)'.format(path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
