"""Float64 numpy reference of the step seam (include/rcu.h "Step seam", the reference's rechun/dl/customsteps.py:16-71 and
bin-dl/brats_test_aleatoric.py:63-73, :95-97) and the seeded input sets the tests of it share.  TEST INFRASTRUCTURE ONLY.

Written from the definitions, not from the kernels: every function takes the float32 arrays a kernel takes, converts them to float64 first
and does every step in float64.  Layouts are the library's: a volume is ``[n, C, ...]`` (class axis 1), a stack of passes ``[T, n, C, ...]``,
a statistics blob ``[planes, n, ...]`` with the planes in the blob's order ``[sum p_c (C)] [sum p_c^2 (C) if VAR] [sum H (1) if MI]``.

tests/test_step_seam_reference_cpu.py pins this module (against oracle/summary_oracle.py and fixture G6) and the properties of the input
sets; tests/test_gpu_step_seam.py compares the kernels with it."""
import numpy as np

# flags of include/rcu.h (repeated so that the module needs no built library)
MI, VAR, INPUT_PROBS, EXACT = 1, 2, 4, 8
FLAG_SETS = (0, MI, VAR, MI | VAR, EXACT, EXACT | MI, EXACT | MI | VAR)
GRID = 0.125            # every logit of grid_logits is a multiple of it


def _f64(x):
    return np.asarray(x, dtype=np.float64)


# ------------------------------------------------------------------------------------------ the definitions
def softmax(logits):
    """F.softmax(logits, 1) in float64 (customsteps.py:24, :33)."""
    x = _f64(logits)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def entropy(p, axis=1, keepdims=False):
    """Natural-log entropy with the p > 0 guard: 0 log 0 = 0 (common/utils/torchhelper.py:53-54)."""
    p = _f64(p)
    return -np.sum(np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0), axis=axis, keepdims=keepdims)


def quantise(x):
    """RCU_MC_EXACT: an addend enters as (x + 6144.0) - 6144.0 in float64, the nearest multiple of 2^-40."""
    return (_f64(x) + 6144.0) - 6144.0


def statistics_planes(probabilities, flags):
    """The blob ``[planes, n, ...]`` (float64) of a stack ``[T, n, C, ...]`` of per-pass probabilities, added in stack order; with
    RCU_MC_EXACT every addend (p, p * p, H) is quantised first."""
    p = _f64(probabilities)
    q = quantise if flags & EXACT else (lambda x: x)
    planes = [q(p).sum(0).swapaxes(0, 1)]                                 # [C, n, ...]
    if flags & VAR:
        planes.append(q(p * p).sum(0).swapaxes(0, 1))
    if flags & MI:
        planes.append(q(entropy(p, axis=2)).sum(0)[None])                 # [1, n, ...]
    return np.concatenate(planes, axis=0)


def finalise(planes, nb_classes, passes, flags):
    """rcu_mc_finalize of a blob: probabilities ``[n, C, ...]`` = sum p / T; entropy ``[n, 1, ...]`` of that mean; mutual_info = entropy -
    (sum H) / T (MI); variance = mean over classes of the unbiased variance over the passes, from the two sums, clamped at 0 (VAR)."""
    planes, C, T = _f64(planes), int(nb_classes), float(passes)
    mean = planes[:C].swapaxes(0, 1) / T
    out = {'probabilities': mean, 'entropy': entropy(mean, axis=1, keepdims=True)}
    if flags & MI:
        out['mutual_info'] = out['entropy'] - (planes[2 * C if flags & VAR else C] / T)[:, None]
    if flags & VAR:
        s, sq = planes[:C], planes[C:2 * C]
        out['variance'] = np.maximum(((sq - s * s / T) / (T - 1.0)).mean(axis=0), 0.0)[:, None]
    return out


def summary(probabilities, do_mi=True, do_var=True):
    """MultiPredictionSummary (customsteps.py:57-71) straight from the stack ``[T, n, C, ...]``: what ``finalise(statistics_planes(...))``
    must equal to float64 rounding."""
    p = _f64(probabilities)
    mean = p.mean(0)
    out = {'probabilities': mean, 'entropy': entropy(mean, axis=1, keepdims=True)}
    if do_mi:
        out['mutual_info'] = out['entropy'] - entropy(p, axis=2, keepdims=True).mean(0)
    if do_var:
        out['variance'] = np.maximum(p.var(axis=0, ddof=1).mean(axis=1, keepdims=True), 0.0)
    return out


def sigma_of(raw, is_log_sigma=False):
    """sigma = exp(raw) or |raw| (brats_test_aleatoric.py:66-69)."""
    raw = _f64(raw)
    return np.exp(raw) if is_log_sigma else np.abs(raw)


def first_argmax(x):
    """Arg-max over axis 1, the FIRST maximum on ties (np.argmax's rule) -> uint8 ``[n, ...]``."""
    return np.argmax(_f64(x), axis=1).astype(np.uint8)


def foreground(probabilities):
    """The foreground-class probability map: p[1] (brats_test_default.py:99), p[0] for a single class."""
    p = _f64(probabilities)
    return p[:, 1 if p.shape[1] > 1 else 0]


def sigma_of_prediction(logits, raw, is_log_sigma=False):
    """(prediction, sigma of the predicted class) (brats_test_aleatoric.py:95-97)."""
    pred = first_argmax(logits)
    return pred, np.take_along_axis(sigma_of(raw, is_log_sigma), pred[:, None].astype(np.int64), axis=1)[:, 0]


def votes(x):
    """The vote of a pass per voxel: 1 where the first-maximum arg-max of ``[n, C, ...]`` is not class 0."""
    return (first_argmax(x) != 0).astype(np.uint32)


def vote_plane(stack, bits, n_words):
    """uint32 ``[n_words, n, ...]``: bit b % 32 of word b // 32 set where volume t of ``stack`` (with b = bits[t]) votes."""
    plane = np.zeros((n_words,) + tuple(np.shape(stack[0])[:1]) + tuple(np.shape(stack[0])[2:]), dtype=np.uint32)
    for volume, b in zip(stack, bits):
        plane[b // 32] |= votes(volume) << np.uint32(b % 32)
    return plane


# ------------------------------------------------------------------------------------------ the input sets
PASSES = 5                      # T of every statistics test
SHAPES = {'one_voxel': (3, 9, 31),      # HW = 279 (odd), V = 837: three whole workgroups of 256 and a partial fourth
          'four_wide': (5, 6, 52)}      # HW = 312 = 4 * 78 (78 is no power of two), V / 4 = 390: one whole, one partial workgroup
PLANTED = ('equal', 'tie_1_2', 'tie_0', 'saturated', 'shifted')


def planted_rows(n, hw):
    """{kind: [(sample, pixel), ...]}: the rows every pass of grid_logits plants -- at the start of the first sample and at the end of the
    last one (the partial workgroup)."""
    return {kind: [(0, k), (n - 1, hw - len(PLANTED) + k)] for k, kind in enumerate(PLANTED)}


def grid_logits(seed, nb_classes, n, h, w, passes=PASSES):
    """float32 ``[passes, n, C, h, w]``: random multiples of 1/8 in [-6, 6] -- every difference is 0 or >= 0.125, so a float32 softmax
    keeps the order and exact ties stay exact -- with the rows of ``planted_rows``:
      equal      all classes equal
      tie_1_2    classes 1 and 2 share the maximum (C >= 3; left random below)
      tie_0      class 0 and the last class share the maximum (C >= 2)
      saturated  class t % C at +60, the rest at -60: float32 p is exactly 1 and 0
      shifted    every logit + 10000 (the max-subtraction)"""
    C = int(nb_classes)
    rng = np.random.RandomState(seed)
    x = rng.randint(-48, 49, size=(passes, n, C, h * w)).astype(np.float64) * GRID
    for kind, places in planted_rows(n, h * w).items():
        for i, px in places:
            for t in range(passes):
                row = x[t, i, :, px]
                if kind == 'equal':
                    row[:] = row[0]
                elif kind == 'tie_1_2' and C >= 3:
                    row[1] = row[2] = row.max() + 0.5
                elif kind == 'tie_0' and C >= 2:
                    row[0] = row[C - 1] = row.max() + 0.5
                elif kind == 'saturated':
                    row[:] = -60.0
                    row[t % C] = 60.0
                elif kind == 'shifted':
                    row += 10000.0
    out = x.reshape(passes, n, C, h, w).astype(np.float32)
    assert np.array_equal(out.astype(np.float64).reshape(x.shape), x)          # every value is a float32
    return out


def grid_probabilities(logits):
    """The float64 softmax of ``[T, n, C, ...]`` logits, cast to float32: the RCU_MC_INPUT_PROBS input."""
    return np.stack([softmax(v) for v in logits]).astype(np.float32)


def raw_sigma(seed, nb_classes, n, h, w):
    """float32 ``[n, C, h, w]`` raw sigma-head outputs: normal x 2, with planted 0, -0, negative and large values at the first pixels."""
    rng = np.random.RandomState(seed)
    r = (rng.randn(n, int(nb_classes), h * w) * 2.0).astype(np.float32)
    r[0, :, 0] = 0.0
    r[0, :, 1] = -0.0
    r[0, :, 2] = -3.5
    r[0, :, 3] = 7.25
    r[n - 1, :, h * w - 1] = -1e-3
    return r.reshape(n, int(nb_classes), h, w)


def min_gap(logits):
    """Smallest non-zero difference between two classes' logits of one voxel (class axis 2 of ``[T, n, C, ...]``); inf if none."""
    s = np.sort(_f64(logits), axis=2)
    d = np.diff(s, axis=2)
    d = d[d > 0]
    return float(d.min()) if d.size else float('inf')
