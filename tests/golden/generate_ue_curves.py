#!/usr/bin/env python3
"""G22: yardsticks of the uncertainty level histogram and of the threshold-free uncertainty-error metrics.

The level histogram hist[cell][level] (include/rcu.h, rcu_unc_hist; level(u) = #{k in 1..B-1 : u > k / B}) contains the counts the
REFERENCE derives at its 11 script thresholds: with B = 1000 every one of them is a level boundary, so the sums over the levels >= k must
equal common/evalutation/numpyfunctions.py:86-107 `uncertainty(prediction, target, unc > thr)` integer for integer.  The reference has no
threshold-free metric; AUROC and average precision of error detection by uncertainty level come from scikit-learn.

Three volumes:
  (a) 24 x 24 x 24 voxels of uniform random float32 p
  (b) the same size, peaked: about 97 % of the voxels with p < 1e-4 or p > 1 - 1e-4
      -- for both, uncertainty = ToEntropy(AddBackgroundProbabilities(p)) of the reference (float64), prediction = p > 0.5
  (c) 16 x 16 x 16 voxels whose uncertainty is GIVEN (float64): every boundary k / 1000, its two float64 neighbours, 0.0, -0.0, 1.0,
      1 + 1e-9, -1e-9 and one NaN, padded with uniform draws; prediction Bernoulli(0.5)
For all three: target Bernoulli(0.3), one random mask, and the reference's counts at the 11 thresholds with and without the mask.
For (a), (b): error = prediction != target, level by the plain-numpy definition, roc_auc_score(error, level) and
average_precision_score(error, level).

Output: tests/golden/g22_ue_curves.npz (arrays and numbers only).

    python tests/golden/generate_ue_curves.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

THRESHOLDS = [0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95]      # bin-eval/eval_uncertainty.py:239
LEVELS = 1000


def levels_of(u, levels):
    """level(u) = #{k in 1..levels-1 : u > k / levels}, float64 compares (NaN compares false: level 0)."""
    bounds = np.arange(1, levels, dtype=np.float64) / np.float64(levels)
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    with np.errstate(invalid='ignore'):
        return (u[:, None] > bounds[None, :]).sum(axis=1).astype(np.int64)


def main():
    import generate_golden as gg
    gg.install_reference()
    import common.evalutation.numpyfunctions as ref_np
    import rechun.eval.analysis as ref_an
    import sklearn
    from sklearn.metrics import average_precision_score, roc_auc_score

    rng = np.random.RandomState(22)
    arrays = {'thresholds': np.array(THRESHOLDS), 'levels': np.array(LEVELS), 'sklearn_version': np.array(sklearn.__version__),
              'numpy_version': np.array(np.__version__), 'metrics_source': np.array('scikit-learn roc_auc_score / average_precision_score')}

    def reference_entropy(p):
        to_eval = {'probabilities': p.copy()}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            to_eval = ref_an.ToEntropy()(ref_an.AddBackgroundProbabilities()(to_eval))
        assert to_eval['uncertainty'].dtype == np.float64
        return to_eval['uncertainty']

    def reference_counts(prediction, target, unc, mask):
        out = np.zeros((2, len(THRESHOLDS), 8), dtype=np.int64)
        with np.errstate(invalid='ignore'):
            for i, thr in enumerate(THRESHOLDS):
                out[0, i] = ref_np.uncertainty(prediction.astype(bool), target.astype(bool), unc > thr)
                out[1, i] = ref_np.uncertainty(prediction.astype(bool), target.astype(bool), unc > thr, mask=mask)
        return out

    shape = (24, 24, 24)
    p_a = rng.rand(*shape).astype(np.float32)
    p_b = rng.rand(*shape).astype(np.float32)
    certain = rng.rand(*shape) < 0.97
    tiny = (rng.rand(*shape) * 1e-4).astype(np.float32)
    p_b = np.where(certain, np.where(rng.rand(*shape) < 0.9, tiny, np.float32(1) - tiny), p_b).astype(np.float32)
    for tag, p in (('a', p_a), ('b', p_b)):
        unc = reference_entropy(p)
        target = (rng.rand(*shape) < 0.3).astype(np.uint8)
        prediction = (p > 0.5).astype(np.uint8)
        mask = rng.rand(*shape) > 0.5
        error = (prediction != target).reshape(-1)
        level = levels_of(unc, LEVELS)
        arrays.update({tag + '_p': p, tag + '_uncertainty': unc, tag + '_target': target, tag + '_prediction': prediction, tag + '_mask': mask,
                       tag + '_counts': reference_counts(prediction, target, unc, mask),
                       tag + '_auroc': np.array(roc_auc_score(error, level)), tag + '_auprc': np.array(average_precision_score(error, level))})
    frac = float(((p_b < 1e-4) | (p_b > 1 - 1e-4)).mean())
    assert 0.96 < frac < 0.98, frac

    # (c) the boundary probe
    shape = (16, 16, 16)
    t = np.arange(1, LEVELS, dtype=np.float64) / np.float64(LEVELS)
    assert all(float(repr(thr)) == t[int(round(thr * LEVELS)) - 1] for thr in THRESHOLDS)      # the script's literals ARE boundaries
    special = np.concatenate([t, np.nextafter(t, 0.0), np.nextafter(t, 1.0), [0.0, -0.0, 1.0, 1 + 1e-9, -1e-9, np.nan]])
    # level the definition gives each special value: t_k -> k-1, below -> k-1, above -> k; 0, -0 -> 0; 1, 1 + 1e-9 -> B-1; -1e-9, NaN -> 0
    k = np.arange(1, LEVELS)
    special_level = np.concatenate([k - 1, k - 1, k, [0, 0, LEVELS - 1, LEVELS - 1, 0, 0]]).astype(np.int64)
    n = int(np.prod(shape))
    unc_c = np.concatenate([special, rng.rand(n - special.size)])
    order = rng.permutation(n)
    unc_c = unc_c[order].reshape(shape)
    special_index = np.argsort(order)[:special.size]            # where special value i sits in the flattened volume
    assert np.array_equal(unc_c.reshape(-1)[special_index], special, equal_nan=True)
    target = (rng.rand(*shape) < 0.3).astype(np.uint8)
    prediction = (rng.rand(*shape) < 0.5).astype(np.uint8)
    mask = rng.rand(*shape) > 0.5
    arrays.update({'c_uncertainty': unc_c, 'c_target': target, 'c_prediction': prediction, 'c_mask': mask,
                   'c_counts': reference_counts(prediction, target, unc_c, mask), 'c_special_index': special_index.astype(np.int64),
                   'c_special_level': special_level})
    path = os.path.join(HERE, 'g22_ue_curves.npz')
    np.savez_compressed(path, **arrays)
    print('wrote {} ({:.1f} KiB); peaked fraction of (b) {:.4f}; auroc a / b {:.6f} / {:.6f}'.format(
        path, os.path.getsize(path) / 1024, frac, float(arrays['a_auroc']), float(arrays['b_auroc'])))


if __name__ == '__main__':
    main()
