#!/usr/bin/env python3
"""G33: yardsticks of the quantile rescale (include/rcu.h "Quantile rescale"), made with numpy alone: np.sort on the keys and np.searchsorted
(tests/quantile_reference.py), with np.quantile(x, k / Q, method='inverted_cdf') as the independent witness of every boundary.

Cases, seeded (`<case>_maps` float32 [subjects, n], `<case>_mask` uint8 of the same shape where the case has one, `<case>_Q`):
  normal     1 x 1439 standard normal values, Q = 1000 (N is no multiple of Q; about a fifth of the levels hold two voxels)
  lognormal  3 x 1920 (4 x 24 x 20) log-normal values with one outlier at 1e6, a mask that keeps about 70 %, one subject's mask EMPTY, Q = 1000
  ties       2 x 12480 (5 x 48 x 52) values, 85 % of them the one value 0.125 at random places, the rest log-normal, Q = 1000
  special    1 x 64: +0, -0, the smallest and largest denormals of both signs, -1, 1, the largest finite values, -inf, +inf, Q = 7 and a mask
  small      1 x 5 values, Q = 7 (N < Q: boundaries coincide)
  equal      1 x 63 times the value -2.5, Q = 16 (every boundary the same key)
Per case: `<case>_N`, `<case>_ranks` int64 [Q-1], `<case>_keys` uint32 [Q-1], `<case>_levels` int64 [subjects, n] (of EVERY voxel) and
`<case>_rescaled` float32 [subjects, n].

Output: tests/golden/g33_quantiles.npz (arrays and numbers only).

    python tests/golden/generate_quantiles.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import quantile_reference as qr  # noqa: E402

OUT = os.path.join(HERE, 'g33_quantiles.npz')


def distinct(a):
    """The same float32 values with every repeated one moved up to a neighbouring value that is still free ('normal' and 'lognormal' promise
    distinct values: the level counts r_{l+1} - r_l hold for those only)."""
    flat = a.reshape(-1)
    while True:
        _, first = np.unique(flat, return_index=True)
        repeated = np.setdiff1d(np.arange(flat.size), first)
        if repeated.size == 0:
            return a
        flat[repeated] = np.nextafter(flat[repeated], np.float32(np.inf))


def cases():
    rng = np.random.RandomState(33)
    out = {}
    out['normal'] = (distinct(rng.standard_normal((1, 1439)).astype(np.float32)), None, 1000)
    energy = distinct(np.exp(rng.normal(2.0, 1.5, (3, 1920))).astype(np.float32))
    energy[1, 777] = 1e6
    mask = (rng.rand(3, 1920) < 0.7).astype(np.uint8)
    mask[2] = 0
    mask[1, 777] = 1
    out['lognormal'] = (energy, mask, 1000)
    ties = np.exp(rng.normal(0.0, 1.0, (2, 12480))).astype(np.float32)
    ties[rng.rand(2, 12480) < 0.85] = 0.125
    out['ties'] = (ties, None, 1000)
    tiny, huge = np.float32(1e-45), np.finfo(np.float32).max
    big_denormal = np.array([0x007fffff], np.uint32).view(np.float32)[0]
    values = np.array([0.0, -0.0, tiny, -tiny, big_denormal, -big_denormal, -1.0, 1.0, huge, -huge, -np.inf, np.inf, 0.5, -0.5, 3.0, -3.0], np.float32)
    special = np.tile(values, 4)[None, :]
    special_mask = np.ones((1, 64), np.uint8)
    special_mask[0, 48:] = 0
    special_mask[0, 59] = 1       # (one +inf more than -inf inside the population)
    out['special'] = (special, special_mask, 7)
    out['small'] = (np.array([[3.5, -1.25, 0.0, 8.0, 2.0]], np.float32), None, 7)
    out['equal'] = (np.full((1, 63), -2.5, np.float32), None, 16)
    return out


def witness(maps, mask, q):
    """np.quantile(..., method='inverted_cdf') of the population values at k / Q -> the keys of the values it returns."""
    x = maps.reshape(-1) if mask is None else maps.reshape(-1)[mask.reshape(-1) != 0]
    with np.errstate(invalid='ignore'):
        return qr.key(np.quantile(x.astype(np.float32), np.arange(1, q) / q, method='inverted_cdf').astype(np.float32))


def build():
    arrays = {}
    for name, (maps, mask, q) in cases().items():
        pop = qr.population_keys(maps, mask)
        n, ranks, keys = qr.table(pop, q)
        # -0.0 and +0.0 share a key but not a bit pattern: the witness is compared through the key
        assert np.array_equal(witness(maps, mask, q), keys), name
        for plan in ((16, 16), (12, 10, 10), (8, 8, 8, 8)):
            assert np.array_equal(qr.select(pop, q, plan)[0], keys), (name, plan)
        levels = qr.levels(qr.key(maps.reshape(-1)), keys).reshape(maps.shape)
        arrays[name + '_maps'] = maps
        if mask is not None:
            arrays[name + '_mask'] = mask
        arrays[name + '_Q'] = np.int64(q)
        arrays[name + '_N'] = np.int64(n)
        arrays[name + '_ranks'] = ranks
        arrays[name + '_keys'] = keys
        arrays[name + '_levels'] = levels
        arrays[name + '_rescaled'] = qr.rescaled(levels, q)
    return arrays


if __name__ == '__main__':
    np.savez_compressed(OUT, **build())
    print('wrote {} ({} bytes)'.format(OUT, os.path.getsize(OUT)))
