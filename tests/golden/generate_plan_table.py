#!/usr/bin/env python3
"""G30: what the planner decides, case by case (no GPU: rcu_unet_plan + rcu_unet_layer_info through tests/plan_rows.py).

Which kernel runs a layer, on which grid, in which layout family and what it reports as executed work follow from tables and rules in
csrc/rcu_plan.hip and the kernels' ConvConfigInfo rows; this fixture pins their outcome so that a change of how those facts are written down
can be told from a change of the facts.  Cases:
  explicit  the shipped shapes 192x128, 240x240, 192x256, 256x256 (depth 4, 32 start filters) x 4 and 3 input channels x max_batch 8, 160, 320,
            448, 480, 640 x {default options, every single non-default option value}
  sweep     600 seeded draws: depth 2..5, start filters 4..64, input channels {1, 3, 4, 5, 32}, residual / sigma_out / provide_features on and
            off, a list of sizes with odd and non-tile ones, batch sizes and options at random
Per case the fixture keeps the case itself, a 64-bit hash over every exact field of every rcu_layer_info row (names, kernel, cin, cout, height,
width, grid, flags, flops_per_slice) and the rows' mfma_flops_per_slice as numbers (compared at rel 1e-12 by tests/test_plan_table_cpu.py).
The generator refuses to write unless every case plans and every kernel that can be a plan entry occurs (KERNELS: the 30 ConvConfigInfo rows
without the two '+head' ones, which forward_impl substitutes at run time).

Run once against a library of the commit whose planner is to be pinned:
    RCU_HIP_LIBRARY=/path/to/librcu_hip.so python tests/golden/generate_plan_table.py
Output: tests/golden/g30_plan_table.npz.
"""
import hashlib
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for path in (os.path.dirname(TESTS), TESTS):
    if path not in sys.path:
        sys.path.insert(0, path)
PATH = os.path.join(HERE, 'g30_plan_table.npz')

OPTION_VALUES = [('conv_winograd', 0), ('conv_winograd4', 0), ('conv_winograd4', 2), ('conv_winograd4', 3), ('conv_first', 0), ('act_layout', 1),
                 ('fuse_head', 0), ('head_winograd4', 0), ('pad_levels', 0), ('upconv_winograd4', 0), ('upconv_winograd4', 2)]
KERNELS = sorted(
    ['conv3x3_igemm<{}>'.format(t) for t in ('T8x16,N64,K8,db', 'T8x16,N32,K8,db', 'T8x16,N32,K8', 'S2T12x8,N64,K8,db', 'T16x16,N32,K8,db', 'T16x16,N64,K8,db',
                                             'S2T8x16,N64,K8,db')] +
    ['upconv_subpixel_igemm<{}>'.format(t) for t in ('T8x16,N64,K8,db', 'T8x16,N32,K8,db', 'S2T12x8,N64,K8,db', 'T16x16,N32,K8,db')] +
    ['{}<{},K8>'.format(f, t) for f in ('conv3x3_winograd', 'upconv_winograd') for t in ('T16x16,N64', 'T16x32,N32', 'S2T8x16,N64', 'S8T4x8,N64')] +
    ['conv3x3_first<T8x32,K36>'] +
    ['conv3x3_winograd4<{},N32,K8>'.format(t) for t in ('T32x32', 'S2T16x32', 'S8T8x16', 'S8T12x8', 'S4T8x32')] +
    ['upconv_winograd4<{},N32,K8>'.format(t) for t in ('T32x32', 'S2T16x32', 'S8T8x16')])
SIZES = [(48, 32), (16, 16), (128, 512), (100, 76), (33, 47), (192, 128), (240, 240), (192, 256), (256, 256), (64, 64), (96, 64), (32, 96), (155, 120),
         (24, 16), (64, 256), (72, 40)]


def cases():
    """[(height, width, max_batch, desc fields, options)]"""
    out = []
    for h, w in ((192, 128), (240, 240), (192, 256), (256, 256)):
        for cin in (4, 3):
            for n in (8, 160, 320, 448, 480, 640):
                for options in [{}] + [{k: v} for k, v in OPTION_VALUES]:
                    out.append((h, w, n, dict(in_channels=cin), options))
    rng = random.Random(30)
    for _ in range(600):
        h, w = rng.choice(SIZES)
        depth = rng.randint(2, 5)
        while (1 << depth) > min(h, w):
            depth -= 1
        desc = dict(depth=depth, start_filters=rng.choice([4, 8, 16, 32, 64, rng.randint(4, 64)]), in_channels=rng.choice([1, 3, 4, 5, 32]),
                    residual=int(rng.random() < 0.25), sigma_out=int(rng.random() < 0.3), provide_features=int(rng.random() < 0.2))
        n = rng.choice([1, 2, 3, 8, 10, 16, 160, 480, 640])
        options = dict(rng.sample(OPTION_VALUES, rng.choice([0, 0, 1, 1, 2])))
        out.append((h, w, n, desc, options))
    return out


def row_hash(rows):
    """64 bits of SHA-256 over the exact fields of a plan's rows (flops_per_slice as float.hex: the sum it comes from is exact in double)."""
    text = repr([(r['name'], r['kernel'], r['cin'], r['cout'], r['height'], r['width'], r['grid'], r['upsample'], r['pooled'], r['dual_source'],
                  r['head_fusable'], float(r['flops']).hex()) for r in rows])
    return int.from_bytes(hashlib.sha256(text.encode()).digest()[:8], 'little')


def compute(case_list):
    """(hash per case, rows per case, mfma_flops_per_slice of all rows back to back, kernels seen)"""
    from plan_rows import plan_rows
    hashes, counts, mfma, seen = [], [], [], set()
    for h, w, n, desc, options in case_list:
        rows = plan_rows(h, w, n, options, **desc)
        hashes.append(row_hash(rows))
        counts.append(len(rows))
        mfma.extend(r['mfma_flops'] for r in rows)
        seen.update(r['kernel'] for r in rows)
    return np.array(hashes, dtype=np.uint64), np.array(counts, dtype=np.int32), np.array(mfma, dtype=np.float64), seen


def main():
    case_list = cases()
    hashes, counts, mfma, seen = compute(case_list)      # (a case that does not plan raises)
    assert sorted(seen) == KERNELS, (sorted(set(KERNELS) - seen), sorted(seen - set(KERNELS)))
    np.savez_compressed(PATH, cases=np.array(json.dumps(case_list)), hashes=hashes, counts=counts, mfma=mfma, kernels=np.array(KERNELS))
    print('{}: {} cases, {} rows, {} kernels, {} bytes'.format(PATH, len(case_list), int(counts.sum()), len(seen), os.path.getsize(PATH)))


if __name__ == '__main__':
    main()
