#!/usr/bin/env python3
"""G38: yardsticks of the affine test-time augmentation warp (include/rcu_warp.h), witnessed by torch's F.affine_grid / F.grid_sample in
float64 (mode='bilinear', padding_mode='border', align_corners=False) -- independent of tests/warp_reference.py, which forms the taps and the
weights itself from the pixel-unit matrix.

Inputs, seeded: five planes `x_<k>` [2, H, W] float32 (standard normal) for (H, W) in SHAPES and four output-to-source matrices `mats` [4, 2, 3]
float64 (10 degrees / 1.1 / shift (1.5, -2.25); -25 degrees / 0.85 / mirrored; 45 degrees / 1.3, where most of the border is clamped; a pure
half-pixel shift).  Per shape k and matrix m: `torch_<k>_<m>` float64, grid_sample of the float64 image under
theta = [[m11, m10 H/W, 2 m12/W], [m01 W/H, m00, 2 m02/H]], and `ref_<k>_<m>` float64, warp_reference.warp with the definition's float32 weights
(a pin of the restatement: with its float64 weights it must agree with torch to 1e-12 max|x|).

Output: tests/golden/g38_warp.npz (arrays only).

    python tests/golden/generate_warp.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import warp_reference as ref  # noqa: E402

SHAPES = ((15, 17), (32, 48), (1, 1), (33, 33), (24, 40))


def matrices():
    return np.stack([ref.matrix(10.0, 1.1, 1.5, -2.25), ref.matrix(-25.0, 0.85, flip=True), ref.matrix(45.0, 1.3), ref.matrix(0.0, 1.0, 0.5, -0.5)])


def torch_warp(x, M):
    h, w = x.shape[-2:]
    th = torch.tensor([[M[1, 1], M[1, 0] * h / w, 2.0 * M[1, 2] / w], [M[0, 1] * w / h, M[0, 0], 2.0 * M[0, 2] / h]], dtype=torch.float64)
    xt = torch.from_numpy(x.astype(np.float64))[None]
    grid = F.affine_grid(th[None], list(xt.shape), align_corners=False)
    return F.grid_sample(xt, grid, mode='bilinear', padding_mode='border', align_corners=False)[0].numpy()


def main():
    rng = np.random.default_rng(20380)
    mats = matrices()
    out = {'mats': mats, 'shapes': np.array(SHAPES, dtype=np.int64)}
    worst = 0.0
    for k, (h, w) in enumerate(SHAPES):
        x = rng.standard_normal((2, h, w)).astype(np.float32)
        out['x_{}'.format(k)] = x
        for m, M in enumerate(mats):
            witness = torch_warp(x, M)
            out['torch_{}_{}'.format(k, m)] = witness
            out['ref_{}_{}'.format(k, m)] = ref.warp(x, M)
            worst = max(worst, float(np.abs(ref.warp(x, M, weights='float64') - witness).max() / np.abs(x).max()))
    print('float64 weights against torch: {:.3g} of max|x|'.format(worst))
    path = os.path.join(HERE, 'g38_warp.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
