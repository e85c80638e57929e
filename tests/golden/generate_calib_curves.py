#!/usr/bin/env python3
"""G26: yardsticks of the calibration level histogram and of the metrics derived from it.

The level histogram (include/rcu.h, rcu_calib_curve; level(p) = #{k in 1..B-1 : p >= t_k} on the float32 thresholds of rcu_ece_thresholds
extended to B levels) contains the REFERENCE's reliability histogram for every number of bins that divides B: merging B / n consecutive
levels must give common/evalutation/numpyfunctions.py `ece_binary(n_bins=n)`'s bins_count integer for integer and its ECE to the rounding of
the confidence sums.  The reference has no proper scoring rule and no recalibration; the Brier score and the isotonic fit come from
scikit-learn.

Three volumes of at most 4,096 voxels, each with a target and a mask:
  (a) G8's case (a): its map, target and mask reused
  (b) every threshold t_k of 10, 20 and 1000 levels with its float32 neighbours on both sides, plus 0, 1, 2^-30 and 1 - 2^-24;
      target Bernoulli(0.4), mask Bernoulli(0.6)
  (c) 4,096 voxels, peaked: about 97 % of the voxels with p < 1e-3, the rest uniform; target Bernoulli(p) on the uniform part and
      Bernoulli(0.002) on the rest, mask Bernoulli(0.5)
Stored per case and per selection (`nomask`, `masked`):
  the reference's ece_binary at 10 and 20 bins with its out_bins,
  sklearn.metrics.brier_score_loss(target, p),
  sklearn.isotonic.IsotonicRegression(y_min=0, y_max=1) fitted on (level index at B = 1000, target): its prediction at every level
  0..999 (`isotonic`), the levels that hold voxels (`isotonic_levels`) and brier_score_loss(target, prediction at the voxel's level).

Output: tests/golden/g26_calib_curves.npz (arrays and numbers only).

    python tests/golden/generate_calib_curves.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

LEVELS = 1000


def thresholds(levels):
    """t_k, k = 1..levels-1: the smallest float32 >= k * ((1 + 1e-8) / levels), the edges of np.linspace(0, 1 + 1e-8, levels + 1)."""
    edges = np.linspace(0., 1. + 1e-8, levels + 1)[1:-1]
    t = edges.astype(np.float32)
    low = t.astype(np.float64) < edges
    t[low] = np.nextafter(t[low], np.float32(2.0))
    return t


def levels_of(p, levels):
    """level(p) = #{k : p >= t_k} (NaN compares false: level 0)."""
    with np.errstate(invalid='ignore'):
        return np.searchsorted(thresholds(levels), np.asarray(p, dtype=np.float32).reshape(-1), side='right').astype(np.int64)


def main():
    import generate_golden as gg
    gg.install_reference()
    import common.evalutation.numpyfunctions as ref_np
    import sklearn
    from sklearn.isotonic import IsotonicRegression
    from sklearn.metrics import brier_score_loss

    rng = np.random.RandomState(26)
    arrays = {'levels': np.array(LEVELS), 'sklearn_version': np.array(sklearn.__version__), 'numpy_version': np.array(np.__version__)}
    g8 = np.load(os.path.join(HERE, 'g8_ece.npz'))
    cases = {'a': (g8['a_p'].reshape(-1), g8['a_target'].reshape(-1), g8['a_mask'].reshape(-1))}

    probes = []
    for b in (10, 20, LEVELS):
        t = thresholds(b)
        # the reference digitises against the float64 edges: t_k is the first float32 at or above edge k
        edges = np.linspace(0., 1. + 1e-8, b + 1)
        assert np.array_equal(np.digitize(t, edges) - 1, np.arange(1, b)) and np.array_equal(np.digitize(np.nextafter(t, np.float32(0)), edges) - 1,
                                                                                              np.arange(0, b - 1))
        probes.extend([t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(2))])
    p_b = np.concatenate(probes + [np.array([0.0, 1.0, 2.0 ** -30, 1 - 2.0 ** -24], dtype=np.float32)]).astype(np.float32)
    p_b = p_b[rng.permutation(p_b.size)]
    assert p_b.size <= 4096 and p_b.min() >= 0 and p_b.max() <= 1
    cases['b'] = (p_b, (rng.rand(p_b.size) < 0.4).astype(np.uint8), rng.rand(p_b.size) < 0.6)

    n = 4096
    uniform = rng.rand(n).astype(np.float32)
    certain = rng.rand(n) < 0.97
    p_c = np.where(certain, (rng.rand(n) * 1e-3).astype(np.float32), uniform).astype(np.float32)
    t_c = np.where(certain, rng.rand(n) < 0.002, rng.rand(n) < uniform).astype(np.uint8)
    cases['c'] = (p_c, t_c, rng.rand(n) < 0.5)
    frac = float((p_c < 1e-3).mean())
    assert 0.96 < frac < 0.98, frac

    for tag, (p, target, mask) in cases.items():
        assert p.dtype == np.float32 and p.size <= 4096
        arrays.update({tag + '_p': p, tag + '_target': target, tag + '_mask': mask})
        probs2 = np.stack([1 - p, p], axis=-1)
        for sel, m in (('nomask', None), ('masked', mask)):
            for n_bins in (10, 20):
                bins = {}
                ece = ref_np.ece_binary(probs2, target, n_bins=n_bins, mask=m, out_bins=bins)
                arrays['{}_ece{}_{}'.format(tag, n_bins, sel)] = np.array(ece)
                for k, v in bins.items():
                    arrays['{}_{}{}_{}'.format(tag, k, n_bins, sel)] = np.asarray(v)
            keep = np.ones(p.size, dtype=bool) if m is None else m
            y, q = target[keep].astype(np.float64), p[keep].astype(np.float64)
            arrays['{}_brier_{}'.format(tag, sel)] = np.array(brier_score_loss(y, q))
            level = levels_of(p[keep], LEVELS)
            iso = IsotonicRegression(y_min=0, y_max=1, out_of_bounds='clip').fit(level.astype(np.float64), y)
            arrays['{}_isotonic_{}'.format(tag, sel)] = iso.predict(np.arange(LEVELS, dtype=np.float64))
            arrays['{}_isotonic_levels_{}'.format(tag, sel)] = np.unique(level)
            arrays['{}_isotonic_brier_{}'.format(tag, sel)] = np.array(brier_score_loss(y, iso.predict(level.astype(np.float64))))
    path = os.path.join(HERE, 'g26_calib_curves.npz')
    np.savez_compressed(path, **arrays)
    print('wrote {} ({:.1f} KiB); peaked fraction of (c) {:.4f}; brier a / b / c {:.6f} / {:.6f} / {:.6f}'.format(
        path, os.path.getsize(path) / 1024, frac, *(float(arrays[t + '_brier_nomask']) for t in 'abc')))


if __name__ == '__main__':
    main()
