#!/usr/bin/env python3
"""G32: yardsticks of the feature-space density (include/rcu.h "Feature-space density"): class moments, the Gaussian fit and the energies, made
with numpy and scipy alone -- scipy.stats.multivariate_normal.logpdf and scipy.special.logsumexp are the witnesses of the energy, independent of
the Cholesky / triangular-inverse route the package and tests/density_reference.py take.

Inputs, seeded: for F in 8, 32, 64 three slices of 312 voxels of float32 features (`phi_<F>` [3, 312, F]): class-dependent means, a random
correlated covariance per class, and ONE DEAD CHANNEL (channel 3 is the constant 0.25 everywhere: its variance is exactly zero, only the ridge lets
the Cholesky factorisation through, and A gets entries of the order 1 / sqrt(ridge)).  Labels `labels3` [3, 312] in {0, 1, 2} and `labels2` =
labels3 > 0; slice 2 is all background, so it lacks classes 1 and 2.
Per F, for K = 2 (labels2): the per-slice moments `n_<F>`, `S_<F>`, `G_<F>` (float64; sums of exactly representable products accumulated in
float64 by numpy), the fit at ridge 1e-6 `mu_<F>`, `A_<F>`, `b_<F>`, `k_<F>` and the witness energies `e_<F>` [3, 312] of the float64 fit.
For K = 1 (one class: every label 0) and K = 3 (labels3) the witness energies alone, `e1_<F>`, `e3_<F>`: their fits follow from the moments.

Output: tests/golden/g32_density.npz (arrays and numbers only).

    python tests/golden/generate_density.py
"""
import os

import numpy as np
from scipy.special import logsumexp
from scipy.stats import multivariate_normal

HERE = os.path.dirname(os.path.abspath(__file__))
RIDGE = 1e-6
SLICES, HW, DEAD = 3, 312, 3


def make_features(rng, F, labels3):
    phi = np.zeros((SLICES, HW, F), np.float32)
    for c in range(3):
        mean = rng.normal(0.0, 1.0, F) + 0.5 * c
        mix = rng.normal(0.0, 1.0, (F, F)) / np.sqrt(F) + np.diag(rng.uniform(0.3, 1.2, F))
        where = labels3 == c
        phi[where] = (mean + rng.normal(0.0, 1.0, (int(where.sum()), F)) @ mix.T).astype(np.float32)
    phi[..., DEAD] = 0.25
    return phi


def class_gaussians(phi, labels, K):
    """(log prior, mean, covariance with the ridge) per class from the pooled voxels: plain numpy in float64."""
    x = phi.reshape(-1, phi.shape[-1]).astype(np.float64)
    y = labels.reshape(-1)
    F = x.shape[1]
    out = []
    for c in range(K):
        xc = x[y == c]
        mu = xc.sum(0) / xc.shape[0]
        cov = xc.T @ xc / xc.shape[0] - np.outer(mu, mu)
        cov = cov + RIDGE * (np.trace(cov) / F) * np.eye(F)
        out.append((np.log(xc.shape[0] / x.shape[0]), mu, cov))
    return out


def witness_energy(phi, gaussians):
    x = phi.reshape(-1, phi.shape[-1]).astype(np.float64)
    terms = np.stack([lp + multivariate_normal.logpdf(x, mean=mu, cov=cov, allow_singular=False) for lp, mu, cov in gaussians], axis=1)
    return -logsumexp(terms, axis=1).reshape(phi.shape[:2])


def main():
    rng = np.random.default_rng(20320)
    labels3 = rng.choice(3, size=(SLICES, HW), p=(0.4, 0.3, 0.3)).astype(np.uint8)
    labels3[2] = 0
    labels2 = (labels3 > 0).astype(np.uint8)
    out = dict(labels3=labels3, labels2=labels2, ridge=np.float64(RIDGE), dead_channel=np.int64(DEAD))
    for F in (8, 32, 64):
        phi = make_features(rng, F, labels3)
        out['phi_{}'.format(F)] = phi
        x = phi.astype(np.float64)
        n = np.zeros((SLICES, 2), np.int64)
        S = np.zeros((SLICES, 2, F))
        G = np.zeros((SLICES, 2, F, F))
        for s in range(SLICES):
            for c in range(2):
                xc = x[s][labels2[s] == c]
                n[s, c], S[s, c], G[s, c] = xc.shape[0], xc.sum(0), xc.T @ xc
        g2 = class_gaussians(phi, labels2, 2)
        A, b, k = [], [], []
        for lp, mu, cov in g2:
            L = np.linalg.cholesky(cov)
            inv = np.linalg.solve(L, np.eye(F))
            inv = np.tril(inv)
            A.append(inv)
            b.append(inv @ mu)
            k.append(lp - np.log(np.diag(L)).sum() - 0.5 * F * np.log(2.0 * np.pi))
        out.update({'n_{}'.format(F): n, 'S_{}'.format(F): S, 'G_{}'.format(F): G, 'mu_{}'.format(F): np.stack([g[1] for g in g2]),
                    'A_{}'.format(F): np.stack(A), 'b_{}'.format(F): np.stack(b), 'k_{}'.format(F): np.array(k),
                    'e_{}'.format(F): witness_energy(phi, g2),
                    'e1_{}'.format(F): witness_energy(phi, class_gaussians(phi, np.zeros_like(labels2), 1)),
                    'e3_{}'.format(F): witness_energy(phi, class_gaussians(phi, labels3, 3))})
    path = os.path.join(HERE, 'g32_density.npz')
    np.savez(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
