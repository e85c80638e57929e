"""A float64 numpy restatement of include/rcu_warp.h ("Affine test-time augmentation"): the taps and weights of the bilinear warp, the warp itself
and the warped statistics.  numpy rounds every float64 product and sum on its own (no fused operation), which is the header's definition.

The fixture tests/golden/g38_warp.npz (tests/golden/generate_warp.py) is witnessed by torch's affine_grid / grid_sample in float64."""
import numpy as np

U = 2.0 ** -24
WARP_BOUND_ULPS = 12          # three lerps, each a rounded difference and a rounded fmaf: |out_dev - out| <= 12 u max|tap| (include/rcu_warp.h)
IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
# D4 element code (include/rcu.h RCU_TTA_*) -> the integer-tap matrix of the same gather (codes 4-7 on square planes)
D4 = np.array([((1, 0, 0), (0, 1, 0)), ((1, 0, 0), (0, -1, 0)), ((-1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, -1, 0)),
               ((0, 1, 0), (1, 0, 0)), ((0, 1, 0), (-1, 0, 0)), ((0, -1, 0), (1, 0, 0)), ((0, -1, 0), (-1, 0, 0))], dtype=np.float64)


def matrix(rotation_deg=0.0, scale=1.0, shift_y=0.0, shift_x=0.0, flip=False):
    """R(rotation) / scale, the second column negated for flip, the shifts in the last column (rcu_amd.steps.affine_matrix)."""
    a = np.deg2rad(np.float64(rotation_deg))
    c, s = np.cos(a) / np.float64(scale), np.sin(a) / np.float64(scale)
    sign = -1.0 if flip else 1.0
    return np.array([[c, -s * sign, shift_y], [s, c * sign, shift_x]], dtype=np.float64)


def inverse(M):
    M = np.asarray(M, dtype=np.float64)
    lin = np.linalg.inv(M[:, :2])
    return np.concatenate([lin, -(lin @ M[:, 2:])], axis=1)


def theta(M, H, W):
    """The affine_grid matrix of M for H x W planes at align_corners=False."""
    M = np.asarray(M, dtype=np.float64)
    return np.array([[M[1, 1], M[1, 0] * H / W, 2.0 * M[1, 2] / W], [M[0, 1] * W / H, M[0, 0], 2.0 * M[0, 2] / H]], dtype=np.float64)


def _axis(a, b, t, yc, xc, centre, extent):
    s = (a * yc + b * xc) + (t + centre)          # each operation rounded once
    s = np.minimum(np.maximum(s, 0.0), np.float64(extent - 1))
    lo = np.floor(s)
    lo_i = lo.astype(np.int64)
    return lo_i, np.minimum(lo_i + 1, extent - 1), s - lo


def taps(M, H, W):
    """-> dict: i0, i1, j0, j1 (int64 [H, W]), fy64, fx64 (the exact float64 weights) and fy, fx (the definition's float32 weights)."""
    M = np.asarray(M, dtype=np.float64)
    assert M.shape == (2, 3) and np.isfinite(M).all()
    cy, cx = np.float64(H - 1) / 2.0, np.float64(W - 1) / 2.0
    yc = (np.arange(H, dtype=np.float64) - cy)[:, None] + np.zeros((1, W))
    xc = (np.arange(W, dtype=np.float64) - cx)[None, :] + np.zeros((H, 1))
    i0, i1, fy = _axis(M[0, 0], M[0, 1], M[0, 2], yc, xc, cy, H)
    j0, j1, fx = _axis(M[1, 0], M[1, 1], M[1, 2], yc, xc, cx, W)
    return dict(i0=i0, i1=i1, j0=j0, j1=j1, fy64=fy, fx64=fx, fy=fy.astype(np.float32), fx=fx.astype(np.float32))


def _lerp(a, b, t):
    return t * (b - a) + a


def warp(x, M, weights='float32', return_max_tap=False):
    """x [..., H, W] -> its warp with M, evaluated in float64 from the definition's taps and its float32 weights (``weights='float64'``: the
    unrounded weights, what grid_sample in float64 computes).  ``return_max_tap``: also max |tap| per output pixel (the scale of the bound)."""
    x = np.asarray(x)
    H, W = x.shape[-2:]
    t = taps(M, H, W)
    fy, fx = (t['fy64'], t['fx64']) if weights == 'float64' else (t['fy'].astype(np.float64), t['fx'].astype(np.float64))
    xd = x.astype(np.float64)
    v00, v01 = xd[..., t['i0'], t['j0']], xd[..., t['i0'], t['j1']]
    v10, v11 = xd[..., t['i1'], t['j0']], xd[..., t['i1'], t['j1']]
    out = _lerp(_lerp(v00, v01, fx), _lerp(v10, v11, fx), fy)
    if return_max_tap:
        return out, np.maximum(np.maximum(np.abs(v00), np.abs(v01)), np.maximum(np.abs(v10), np.abs(v11)))
    return out


def _fmaf(t, d, a):
    # float32 operands: the product is exact in float64, the sum is rounded to float64 and then to float32 (a double rounding differs from fmaf
    # in rare ties only; this emulation sizes the bound, it is not compared bit for bit)
    return (t.astype(np.float64) * d.astype(np.float64) + a.astype(np.float64)).astype(np.float32)


def warp_float32(x, M):
    """The device's float32 chain emulated on the CPU: lerp(a, b, t) = fmaf(t, b - a, a)."""
    x = np.asarray(x, dtype=np.float32)
    H, W = x.shape[-2:]
    t = taps(M, H, W)
    v00, v01 = x[..., t['i0'], t['j0']], x[..., t['i0'], t['j1']]
    v10, v11 = x[..., t['i1'], t['j0']], x[..., t['i1'], t['j1']]
    fx, fy = np.broadcast_to(t['fx'], v00.shape), np.broadcast_to(t['fy'], v00.shape)
    top = _fmaf(fx, (v01 - v00).astype(np.float32), v00)
    bot = _fmaf(fx, (v11 - v10).astype(np.float32), v10)
    return _fmaf(fy, (bot - top).astype(np.float32), top)


def quantise(x):
    """RCU_MC_EXACT: an addend rounded to the nearest multiple of 2^-40 (ties to even), as (x + 6144.0) - 6144.0 does in float64."""
    return (np.asarray(x, dtype=np.float64) + 6144.0) - 6144.0


def entropy(p, axis):
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return -np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0).sum(axis)


def accumulate_warped(probs, mats):
    """probs [G, n, C, H, W] probabilities, mats [G, 2, 3] -> float64 sums over the groups of the warped probabilities: (sum p [n, C, H, W],
    sum p^2 [n, C, H, W], sum H [n, H, W]), unquantised (the device's RCU_MC_EXACT addends are within 2^-41 of theirs)."""
    probs = np.asarray(probs)
    s1 = np.zeros(probs.shape[1:], dtype=np.float64)
    s2 = np.zeros_like(s1)
    sh = np.zeros(probs.shape[1:2] + probs.shape[3:], dtype=np.float64)
    for g in range(probs.shape[0]):
        p = warp(probs[g], mats[g])
        s1 += p
        s2 += p * p
        sh += entropy(p, 1)
    return s1, s2, sh
