#!/usr/bin/env python3
"""G37: yardsticks of the nearest-neighbour feature uncertainty (include/rcu_knn.h): sorted squared distances to the k = 8 nearest bank rows made
with sklearn.neighbors.NearestNeighbors(algorithm='brute') in float64 -- independent of tests/knn_reference.py, which sums (xhat - b)^2 directly
-- a table of sampling keys and one tiny bank selection made by sorting triples.

Inputs, seeded: for F in 1, 5, 32 a set of 257 query voxels `phi_<F>` [257, F] and 100 tapped bank vectors `bank_<F>` [100, F], float32,
post-ReLU-like (max(N(0.3, 1), 0), so about 38 % exact zeros) with a log-normal scale per channel.  Voxels 0 and 1 and bank row 0 are zero
vectors; bank rows 1..5 are planted equal to voxels 2..6; bank rows 6 and 7 are duplicates of row 8.
Per F and normalize in 0, 1: `rows_<F>_<normalize>` (the float32 rows the device holds: divided by max(|row|, 2^-40) in float64 and rounded
once when normalize is on), `sq_<F>_<normalize>` (float32 |row|^2 from the rounded rows) and `d2_<F>_<normalize>` [257, 8] (float64, the witness).
Keys: `key_seed`, `key_g`, `key_v` -> `key63` under knn_seed(key_seed), with g beyond 2^32 (oracle.mask_oracle.philox4x32_10, pinned to the
published Philox vectors).  Selection: `sel_labels` [3, 40] and per_class (5, 4) under seed 7 -> `sel_label`, `sel_key63`, `sel_g`, `sel_v`.

Output: tests/golden/g37_knn.npz (arrays and numbers only).

    python tests/golden/generate_knn.py
"""
import os
import sys

import numpy as np
from sklearn.neighbors import NearestNeighbors

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import mask_oracle as mo  # noqa: E402

N, M, K = 257, 100, 8
M63 = 2 ** 63 - 1


def features(rng, n, F):
    scale = rng.lognormal(0.0, 1.0, (1, F))
    return (np.maximum(rng.normal(0.3, 1.0, (n, F)), 0.0) * scale).astype(np.float32)


def unit(x):
    x = x.astype(np.float64)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 2.0 ** -40)


def key63(seed, g, v):
    key = ((seed * 1000003) % M63 + 32 * (1 << 40)) % M63
    counter = np.array([[v & 0xFFFFFFFF, g & 0xFFFFFFFF, g >> 32, 0x6b6e6e]], dtype=np.uint32)
    r = mo.philox4x32_10(counter, (key & 0xFFFFFFFF, key >> 32))[0]
    return ((int(r[0]) << 32) | int(r[1])) >> 1


def main():
    rng = np.random.default_rng(20370)
    out = {}
    for F in (1, 5, 32):
        phi, bank = features(rng, N, F), features(rng, M, F)
        phi[:2], bank[0] = 0.0, 0.0
        phi[2:7] += np.float32(0.125)      # (no planted voxel is a zero vector)
        bank[1:6] = phi[2:7]
        bank[6], bank[7] = bank[8], bank[8]
        out['phi_{}'.format(F)], out['bank_{}'.format(F)] = phi, bank
        for normalize in (0, 1):
            rows = (unit(bank) if normalize else bank).astype(np.float32)
            x = unit(phi) if normalize else phi.astype(np.float64)
            wide = rows.astype(np.float64)
            dist, _ = NearestNeighbors(n_neighbors=K, algorithm='brute', metric='euclidean').fit(wide).kneighbors(x)
            tag = '{}_{}'.format(F, normalize)
            out['rows_' + tag], out['sq_' + tag], out['d2_' + tag] = rows, (wide * wide).sum(1).astype(np.float32), dist ** 2
    probes = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (7, 154, 57599), (7, 2 ** 32 - 1, 3), (7, 2 ** 32, 3), (7, 2 ** 32 + 5, 0), (12345, 2 ** 40 + 9, 2 ** 31 - 1),
              (2 ** 31 - 1, 3, 17)]
    out['key_seed'], out['key_g'], out['key_v'] = (np.array(col, dtype=np.int64) for col in zip(*probes))
    out['key63'] = np.array([key63(*p) for p in probes], dtype=np.int64)
    labels = (rng.random((3, 40)) < 0.3).astype(np.uint8)
    keys = np.array([[key63(7, g, v) for v in range(40)] for g in range(3)], dtype=np.int64)
    chosen = []
    for c, m in enumerate((5, 4)):
        triples = sorted((int(keys[g, v]), g, v) for g in range(3) for v in range(40) if labels[g, v] == c)[:m]
        chosen += [(c,) + t for t in triples]
    chosen = np.array(chosen, dtype=np.int64)
    out.update(sel_labels=labels, sel_seed=np.int64(7), sel_per_class=np.array((5, 4), dtype=np.int64), sel_label=chosen[:, 0], sel_key63=chosen[:, 1],
               sel_g=chosen[:, 2], sel_v=chosen[:, 3])
    path = os.path.join(HERE, 'g37_knn.npz')
    np.savez(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
