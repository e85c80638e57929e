"""Float64 numpy restatement of include/rcu.h "Last-layer Laplace": the curvature weights, the per-slice moments, the fit, the probit predictive and
the error bounds the GPU tests assert.  Nothing here imports the package: it is the yardstick of rcu_amd.laplace and of csrc/rcu_laplace.hip."""
import math

import numpy as np

CHUNK = 1024      # RCU_DENSITY_CHUNK
U = 2.0 ** -24    # unit roundoff of float32
PI_8 = float(np.float32(math.pi / 8.0))      # the device's constant
GRID = [2.0 ** (k / 4.0) for k in range(-80, 81)]


def pairs(C):
    return [(a, b) for a in range(C) for b in range(a, C)]


def omega(p):
    """p [..., C] -> omega [..., P] in the dtype of p: float32 in gives the device's weights bit for bit (one subtraction and one multiplication,
    or one multiplication and a sign), float64 in the exact ones."""
    p = np.asarray(p)
    one = p.dtype.type(1)
    cols = [p[..., a] * (one - p[..., a]) if a == b else -(p[..., a] * p[..., b]) for a, b in pairs(p.shape[-1])]
    out = np.stack(cols, -1)
    assert out.dtype == p.dtype
    return out


def moments(psi, p):
    """psi [n, hw, F], p [n, hw, C] (float32: the device's omega; float64: the exact one) -> w [n, P], S [n, P, F], G [n, P, F, F] in float64."""
    psi = np.asarray(psi, dtype=np.float64)
    om = omega(p).astype(np.float64)
    return om.sum(1), np.einsum('svq,svi->sqi', om, psi), np.einsum('svq,svi,svj->sqij', om, psi, psi, optimize=True)


def moment_bounds(psi, p, chunk=CHUNK):
    """(bound of w, of S, of G): (m + 2) 2^-24 times sum_v |omega|, |omega psi_i|, |omega psi_i psi_j|."""
    psi = np.abs(np.asarray(psi, dtype=np.float64))
    om = np.abs(omega(p).astype(np.float64))
    k = (chunk + 2) * U
    return k * om.sum(1), k * np.einsum('svq,svi->sqi', om, psi), k * np.einsum('svq,svi,svj->sqij', om, psi, psi, optimize=True)


def hessian(w, S, G):
    """Moments summed over the slices, w [P], S [P, F], G [P, F, F] -> H [C D, C D]."""
    P, F = S.shape
    C = {3: 2, 6: 3, 10: 4}[P]
    D = F + 1
    H = np.zeros((C * D, C * D))
    for q, (a, b) in enumerate(pairs(C)):
        M = np.block([[G[q], S[q][:, None]], [S[q][None, :], np.array([[w[q]]])]])
        H[a * D:(a + 1) * D, b * D:(b + 1) * D] = M
        H[b * D:(b + 1) * D, a * D:(a + 1) * D] = M.T
    return H


def fsum_slices(a):
    a = np.asarray(a, dtype=np.float64)
    flat = a.reshape(a.shape[0], -1)
    return np.array([math.fsum(flat[:, k]) for k in range(flat.shape[1])]).reshape(a.shape[1:])


def evidence(lam, theta_sq, n_params, tau):
    return -0.5 * tau * theta_sq + 0.5 * n_params * math.log(tau) - 0.5 * float(np.sum(np.log(np.maximum(lam, 0.0) + tau)))


def evidence_tau(H_eff, theta):
    lam = np.linalg.eigvalsh(H_eff)
    scores = [evidence(lam, float(np.sum(np.square(theta))), H_eff.shape[0], t) for t in GRID]
    return GRID[int(np.argmax(scores))], scores


def fit(w, S, G, theta, hessian_scale=1.0, prior_precision=1.0):
    """Per-slice moments and theta [C, D] -> dict(H, Sigma, A, b, kappa, tau)."""
    H = hessian(fsum_slices(w), fsum_slices(S), fsum_slices(G))
    H_eff = hessian_scale * H
    tau = evidence_tau(H_eff, theta)[0] if prior_precision == 'evidence' else float(prior_precision)
    L = np.linalg.cholesky(H_eff + tau * np.eye(H.shape[0]))
    Li = np.linalg.solve(L, np.eye(H.shape[0]))
    Sigma = Li.T @ Li
    Sigma = 0.5 * (Sigma + Sigma.T)
    C, D = theta.shape
    F = D - 1
    A, b, kappa = np.zeros((C, F, F)), np.zeros((C, F)), np.zeros(C)
    for c in range(C):
        LT = np.linalg.cholesky(Sigma[c * D:(c + 1) * D, c * D:(c + 1) * D]).T
        A[c], b[c], kappa[c] = LT[:F, :F], -LT[:F, F], LT[F, F] ** 2
    return dict(H=H, Sigma=Sigma, A=A, b=b, kappa=kappa, tau=tau)


def softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def predictive(A, b, kappa, psi, z):
    """float64 on the GIVEN parameters (pass the float32-rounded ones to get the device's yardstick).  psi [V, F], z [V, C] ->
    dict(s2, std, t, zt, p), each [V, C]."""
    A, b, kappa, psi, z = (np.asarray(v, dtype=np.float64) for v in (A, b, kappa, psi, z))
    y = np.einsum('cij,vj->vci', A, psi, optimize=True) - b[None]
    s2 = (y * y).sum(-1) + kappa[None]
    t = 1.0 + PI_8 * s2
    zt = z / np.sqrt(t)
    return dict(s2=s2, std=np.sqrt(s2), t=t, zt=zt, p=softmax(zt))


def s2_bounds(A, b, kappa, psi):
    """(3 F + 8) 2^-24 sum_i s_i^2 with s_i = sum_j |A_ij psi_j| + |b_i|, plus 2^-23 kappa_c -> [V, C]."""
    A, b, kappa, psi = (np.abs(np.asarray(v, dtype=np.float64)) for v in (A, b, kappa, psi))
    F = psi.shape[1]
    s = np.einsum('cij,vj->vci', A, psi, optimize=True) + b[None]
    return (3 * F + 8) * U * (s * s).sum(-1) + 2.0 ** -23 * kappa[None]


def std_bounds(bound_s2, s2):
    """The device's std is the correctly rounded root of ITS s2, which is within bound_s2 = B of the reference's: |sqrt(a) - sqrt(b)| =
    |a - b| / (sqrt(a) + sqrt(b)) with a >= b - B, plus the one rounding of the root, 2^-24 relative on a value of at most sqrt(b + B):
    B / (sqrt(max(b - B, 0)) + sqrt(b)) + 2^-24 sqrt(b + B) -- to first order B / (2 sqrt(s2)) + 2^-24 sqrt(s2)."""
    return bound_s2 / (np.sqrt(np.maximum(s2 - bound_s2, 0.0)) + np.sqrt(s2)) + U * np.sqrt(s2 + bound_s2)


def s2_through_std_bounds(bound_s2, s2):
    """s2 is not an output; std^2 stands for it.  std = sqrt(s2_dev) (1 + d), |d| <= 2^-24, so |std^2 - s2_ref| <= B + (2 d + d^2)(s2_ref + B):
    the issue's bound B plus the one rounding of the root, 2^-23 s2 to first order."""
    return bound_s2 + (2.0 * U + U * U) * (s2 + bound_s2)


def zt_bounds(bound_s2, pred, z):
    """The bound of s2 propagated through zt = z / sqrt(t), t = fma(pi/8, s2, 1): t carries (pi/8) bound_s2 and one rounding, the square root
    halves the relative error and adds a rounding, the division adds another: |zt| ((pi/8) bound_s2 / (2 t) + 4 * 2^-24) to first order (three
    roundings; the fourth unit covers the second-order terms, all below 2^-40)."""
    return np.abs(pred['zt']) * (PI_8 * bound_s2 / (2.0 * pred['t']) + 4.0 * U)


def p_tolerance(bound_zt, softmax_tol):
    """dp_c / dzt_k = p_c (delta_ck - p_k), so |dp_c| <= 2 p_c (1 - p_c) max_k |dzt_k| <= max_k |dzt_k| / 2; plus the tolerance of the float32
    softmax itself (tests/test_gpu_step_seam.py, P_TOL)."""
    return 0.5 * bound_zt.max(-1, keepdims=True) + softmax_tol
