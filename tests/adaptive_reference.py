"""The adaptive MC schedule and criterion of include/rcu.h ("Adaptive MC") restated in float64 and integer numpy, with nothing from the
package: what tests/test_adaptive_cpu.py pins without a device and tests/test_gpu_adaptive.py compares the kernels with, integer for integer."""
from fractions import Fraction

import numpy as np

QUANTUM_BITS = 40                      # RCU_MC_EXACT: every statistics entry is a multiple of 2^-40
SCALE = 1 << QUANTUM_BITS
MI, VAR, EXACT = 1, 2, 8


def thr_q(eps, t):
    """ceil((1.0 - eps) * t * 2^40) in exact rational arithmetic on the float64 value of ``1.0 - eps``."""
    x = Fraction(1.0 - float(eps)) * int(t) * SCALE
    return -((-x.numerator) // x.denominator)


def plane_count(nb_classes, flags):
    return nb_classes + (nb_classes if flags & VAR else 0) + (1 if flags & MI else 0)


def leading_q(planes, nb_classes):
    """int64 ``[n, hw]``: (max_c S_c) * 2^40 of a float64 blob ``[planes, n, hw]`` whose entries are multiples of 2^-40."""
    lead = np.max(np.asarray(planes, dtype=np.float64)[:nb_classes], axis=0) * float(SCALE)
    q = lead.astype(np.int64)
    assert np.array_equal(q.astype(np.float64), lead), 'entries are not multiples of 2^-40'
    return q


def slice_scores(planes, nb_classes, threshold):
    """(unsettled uint32 ``[n]``, margin_q int64 ``[n]``) of rcu_mc_slice_scores."""
    q = leading_q(planes, nb_classes)
    return (q < int(threshold)).sum(axis=1).astype(np.uint32), q.min(axis=1).astype(np.int64)


def retired(unsettled, max_unsettled=0):
    return np.asarray(unsettled) <= int(max_unsettled)


def schedule(n, check_at, passes, decide):
    """The bookkeeping of a step over n slices: ``decide(k, t, active)`` -> bool per active slice (True = retired at checkpoint t, the k-th).
    -> (counts int32 ``[n]``, [active index list entering each span]): span 0 runs passes 1..t_1 on all slices, span k passes t_k + 1 .. t_{k+1}
    (the last: .. T) on the slices still active.  A checkpoint that leaves nothing active ends the step."""
    counts = np.zeros(n, dtype=np.int32)
    active = np.arange(n)
    spans = [active.copy()]
    ends = list(check_at) + [passes]
    for k, t in enumerate(check_at):
        gone = np.asarray(decide(k, t, active), dtype=bool)
        counts[active[gone]] = t
        active = active[~gone]
        if active.size == 0:
            return counts, spans
        spans.append(active.copy())
    counts[active] = ends[-1]
    return counts, spans


def merge_slices(dst, src, index):
    """rcu_mc_merge_slices on ``[planes, n, hw]`` / ``[planes, m, hw]`` arrays, in place; entries < 0 are skipped."""
    for i, to in enumerate(index):
        if to >= 0:
            dst[:, to] += src[:, i]
    return dst


def entropy(p):
    p = np.asarray(p, dtype=np.float64)
    return -np.sum(np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0), axis=1, keepdims=True)


def finalise_counts(planes, nb_classes, counts, flags):
    """rcu_mc_finalize_counts in float64 on ``[planes, n, hw]``: slice i divided by counts[i].  -> dict of ``[n, C or 1, hw]`` arrays."""
    planes = np.asarray(planes, dtype=np.float64)
    t = np.asarray(counts, dtype=np.float64)[None, :, None]
    c = nb_classes
    mean = np.moveaxis(planes[:c] / t, 0, 1)
    out = {'probabilities': mean, 'entropy': entropy(mean)}
    if flags & MI:
        out['mutual_info'] = out['entropy'] - (planes[-1] / t[0])[:, None, :]
    if flags & VAR:
        s, q = planes[:c], planes[c:2 * c]
        out['variance'] = np.maximum(((q - s * s / t) / (t - 1)).mean(axis=0), 0.0)[:, None, :]
    return out
