#!/usr/bin/env python3
"""G35: yardsticks of the last-layer Laplace approximation (include/rcu.h "Last-layer Laplace"), made with torch autograd and numpy alone, by
routes the package and tests/laplace_reference.py do not take:

  H_<tag>       the Hessian of the summed cross-entropy in theta = (W, w0), class-major, by torch.autograd.functional.hessian in float64 on the
                CPU.  For a softmax on a linear layer it equals the generalised Gauss-Newton matrix, whatever the labels.
  s2_<tag>      psi~^T inv(scale_<tag> * H + tau_<tag> I)_cc psi~ per voxel and class, by numpy.linalg.inv of the whole matrix (no Cholesky,
                no triangular factors).
  evtau_<tag>   the first maximiser over tau_k = 2^(k/4), k = -80..80, of -(tau/2) |theta|^2 + (C D / 2) log tau - (1/2) log det(scale H + tau I)
                by numpy.linalg.slogdet (no eigenvalues).

Cases <tag> = <F>_<C>: 24_3, 32_2, 40_4, 64_2.  Inputs, seeded: three slices of 64 voxels of float32 features `psi_<tag>` [3, 64, F], non-negative
as a ReLU leaves them, correlated, with ONE DEAD CHANNEL (channel 5 is zero everywhere: H has C exactly zero rows and only the prior lets the
factorisation through) and ONE SATURATED VOXEL (slice 0, voxel 7: its logits are more than 104 apart, so the float32 softmax `p32_<tag>` [3, 64, C]
holds exactly 1 and 0 there and its curvature weights are exactly zero).  `W_<tag>` [C, F], `w0_<tag>` [C] float32; the logits are `z_<tag>` =
W psi + w0 in float64.

Output: tests/golden/g35_laplace.npz (arrays and numbers only).

    python tests/golden/generate_laplace.py
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ((24, 3), (32, 2), (40, 4), (64, 2))
SLICES, HW, DEAD, SATURATED = 3, 64, 5, (0, 7)
GRID = [2.0 ** (k / 4.0) for k in range(-80, 81)]


def make_case(rng, F, C):
    mix = rng.normal(0.0, 1.0, (F, F)) / np.sqrt(F) + np.diag(rng.uniform(0.3, 1.2, F))
    psi = np.maximum(rng.normal(0.2, 1.0, (SLICES, HW, F)) @ mix.T, 0.0).astype(np.float32)
    W = (rng.normal(0.0, 1.5, (C, F)) / np.sqrt(F)).astype(np.float32)
    w0 = rng.normal(0.0, 0.5, C).astype(np.float32)
    direction = np.maximum(W[0] - W[1:].mean(0), 0.0).astype(np.float64)
    direction[DEAD] = 0.0
    gaps = (W[0].astype(np.float64) - W[1:].astype(np.float64)) @ direction
    assert (gaps > 0).all(), gaps
    psi[SATURATED] = (direction * (160.0 / gaps.min())).astype(np.float32)
    psi[..., DEAD] = 0.0
    return psi, W, w0


def float32_softmax(z64):
    z = z64.astype(np.float32)
    e = np.exp(z - z.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    assert p.dtype == np.float32
    return p


def autograd_hessian(psi, W, w0, labels):
    C, F = W.shape
    x = torch.from_numpy(psi.reshape(-1, F).astype(np.float64))
    y = torch.from_numpy(labels.reshape(-1).astype(np.int64))
    theta = torch.from_numpy(np.concatenate([W, w0[:, None]], 1).astype(np.float64))

    def loss(t):
        return torch.nn.functional.cross_entropy(x @ t[:, :F].T + t[:, F], y, reduction='sum')
    H = torch.autograd.functional.hessian(loss, theta)
    return H.reshape(C * (F + 1), C * (F + 1)).numpy()


def main():
    rng = np.random.default_rng(20350)
    out = dict(dead_channel=np.int64(DEAD), saturated=np.array(SATURATED, np.int64))
    for F, C in CASES:
        tag = '{}_{}'.format(F, C)
        psi, W, w0 = make_case(rng, F, C)
        z = psi.astype(np.float64) @ W.astype(np.float64).T + w0.astype(np.float64)
        p32 = float32_softmax(z)
        sat = p32[SATURATED]
        assert sorted(sat.tolist()) == [0.0] * (C - 1) + [1.0], sat
        H = autograd_hessian(psi, W, w0, rng.integers(0, C, (SLICES, HW)))
        H = 0.5 * (H + H.T)
        scale, tau = float(rng.choice([0.25, 1.0, 2.0])), float(rng.choice([0.5, 1.0, 4.0]))
        D = F + 1
        Sigma = np.linalg.inv(scale * H + tau * np.eye(C * D))
        ext = np.concatenate([psi.reshape(-1, F).astype(np.float64), np.ones((SLICES * HW, 1))], 1)
        s2 = np.stack([np.einsum('vi,ij,vj->v', ext, Sigma[c * D:(c + 1) * D, c * D:(c + 1) * D], ext) for c in range(C)], 1)
        theta_sq = float((W.astype(np.float64) ** 2).sum() + (w0.astype(np.float64) ** 2).sum())
        scores = [-0.5 * t * theta_sq + 0.5 * C * D * np.log(t) - 0.5 * np.linalg.slogdet(scale * H + t * np.eye(C * D))[1] for t in GRID]
        out.update({'psi_' + tag: psi, 'W_' + tag: W, 'w0_' + tag: w0, 'z_' + tag: z, 'p32_' + tag: p32, 'H_' + tag: H,
                    'scale_' + tag: np.float64(scale), 'tau_' + tag: np.float64(tau), 's2_' + tag: s2.reshape(SLICES, HW, C),
                    'evtau_' + tag: np.float64(GRID[int(np.argmax(scores))]), 'evscores_' + tag: np.array(scores)})
    path = os.path.join(HERE, 'g35_laplace.npz')
    np.savez(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
