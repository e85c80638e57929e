"""Float64 numpy restatement of include/rcu.h "Feature-space density": per-slice class moments, the fit, the energy and the error bounds the GPU
tests assert.  Nothing here imports the package: it is the yardstick of rcu_amd.density and of csrc/rcu_density.hip."""
import math

import numpy as np

CHUNK = 1024      # RCU_DENSITY_CHUNK
U = 2.0 ** -24    # unit roundoff of float32


def moments(phi, labels, K):
    """phi [n, hw, F], labels [n, hw] -> n int64 [n, K], S float64 [n, K, F], G float64 [n, K, F, F]."""
    phi = np.asarray(phi, dtype=np.float64)
    labels = np.asarray(labels)
    n, hw, F = phi.shape
    counts = np.zeros((n, K), np.int64)
    S = np.zeros((n, K, F))
    G = np.zeros((n, K, F, F))
    for s in range(n):
        for c in range(K):
            x = phi[s][labels[s] == c]
            counts[s, c] = x.shape[0]
            S[s, c] = x.sum(0)
            G[s, c] = x.T @ x
    return counts, S, G


def moment_bounds(phi, labels, K, chunk=CHUNK):
    """(bound of S, bound of G): (m + 1) 2^-24 sum_v |phi_i| and (m + 1) 2^-24 sum_v |phi_i phi_j|, the bound of a float32 accumulation of m terms."""
    _, s_abs, g_abs = moments(np.abs(np.asarray(phi, dtype=np.float64)), labels, K)
    return (chunk + 1) * U * s_abs, (chunk + 1) * U * g_abs


def fit(counts, S, G, ridge=1e-6, shared_covariance=False):
    """Per-slice moments -> dict(n, mu, cov, A, b, k); exactly rounded sums over the slices (math.fsum), then float64."""
    counts, S, G = np.asarray(counts), np.asarray(S, dtype=np.float64), np.asarray(G, dtype=np.float64)
    K, F = S.shape[1:]
    n = np.array([sum(int(v) for v in counts[:, c]) for c in range(K)], dtype=np.int64)
    for c in range(K):
        if n[c] <= F:
            raise ValueError('class {} has {} voxels, F = {}'.format(c, int(n[c]), F))
    s_sum = np.array([[math.fsum(S[:, c, i]) for i in range(F)] for c in range(K)])
    g_sum = np.array([[[math.fsum(G[:, c, i, j]) for j in range(F)] for i in range(F)] for c in range(K)])
    total = int(n.sum())
    mu = s_sum / n[:, None]
    cov = g_sum / n[:, None, None] - np.einsum('ci,cj->cij', mu, mu)
    if shared_covariance:
        pooled = sum(float(n[c]) * cov[c] for c in range(K)) / float(total)
        cov = np.stack([pooled] * K)
    cov = np.stack([cov[c] + ridge * (np.trace(cov[c]) / F) * np.eye(F) for c in range(K)])
    A, b, k = np.zeros_like(cov), np.zeros_like(mu), np.zeros(K)
    for c in range(K):
        L = np.linalg.cholesky(cov[c])
        inv = np.zeros_like(L)
        for i in range(F):      # forward substitution, row by row
            e = np.zeros(F)
            e[i] = 1.0
            inv[i] = (e - L[i, :i] @ inv[:i]) / L[i, i]
        A[c] = inv
        b[c] = inv @ mu[c]
        k[c] = math.log(int(n[c]) / total) - float(np.log(np.diag(L)).sum()) - 0.5 * F * math.log(2.0 * math.pi)
    return dict(n=n, mu=mu, cov=cov, A=A, b=b, k=k)


def energy(A, b, k, phi):
    """e = -log sum_c exp(k_c - d2_c / 2), d2_c = |A_c phi - b_c|^2 in float64 on the GIVEN parameters (pass the float32-rounded ones to get the
    device's yardstick).  phi [V, F] -> (e [V], d2 [V, K])."""
    A, b, k, phi = (np.asarray(v, dtype=np.float64) for v in (A, b, k, phi))
    y = np.einsum('cij,vj->vci', A, phi) - b[None]
    d2 = (y * y).sum(-1)
    t = k[None] - 0.5 * d2
    m = t.max(1)
    return -(m + np.log(np.exp(t - m[:, None]).sum(1))), d2


def energy_bounds(A, b, phi):
    """Per voxel and class (3 F + 8) 2^-24 sum_i s_i^2 with s_i = sum_j |A_ij phi_j| + |b_i| -> [V, K]."""
    A, b, phi = (np.abs(np.asarray(v, dtype=np.float64)) for v in (A, b, phi))
    F = phi.shape[1]
    s = np.einsum('cij,vj->vci', A, phi) + b[None]
    return (3 * F + 8) * U * (s * s).sum(-1)


def energy_tolerance(bound_d2, e):
    """The energy's tolerance: half the largest class bound plus 2^-22 max(1, |e|) for the logsumexp."""
    return 0.5 * bound_d2.max(1) + 2.0 ** -22 * np.maximum(1.0, np.abs(e))
