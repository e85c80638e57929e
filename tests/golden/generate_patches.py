#!/usr/bin/env python3
"""G28: yardsticks of the patch table, the patch level histogram and the patch accuracy vs. patch uncertainty metrics (Mukhoti & Gal, 2018).

A volume [depth, height, width] is cut into non-overlapping windows of pd x ph x pw voxels anchored at the origin (partial at the far
edges), numbered in raster order.  Per patch, over its voxels whose mask byte is not 0: n, errors ((prediction != 0) != (target != 0)),
foreground (prediction != 0 or target != 0) and sum_q, the sum of q(u) = rint(clamp(u, 0, 1) * 2^24) in float64, NaN -> 0 (include/rcu.h,
rcu_patch_table).  Everything here is restated in plain numpy, patch by patch; AUROC and average precision come from scikit-learn.

Inputs, all seeded:
  three volumes of 5 x 13 x 71 voxels (an odd voxel count, a width that no patch edge divides and that crosses a 64-lane row) and one image
  of 1 x 24 x 40; blob-like target and prediction; uncertainty maps high near the blobs' boundaries, quantised to 2^-8 but for one region of
  full-precision draws
  volume 0   float64 map with NaN, +-inf, values below 0 and above 1, -0.0, ties of the rounding ((m + 1/2) / 2^24, m even and odd), values no
             float32 holds, an all-zero region and constant 0.5 / 0.25 blocks aligned to the patches (means exactly ON a level boundary);
             one mask (bytes 0, 1, 2, 255) that empties whole patches
  volumes 1, 2 and the image   maps a float32 holds exactly (so the float32 and the float64 form give one table); volume 2 has the blocks too
Sets: 'v0' (float64 map, no mask), 'v0_mask', 'v0_f32' (the map rounded to float32, no mask), 'v1', 'v2', 'img'.
Per set and patch size in PATCHES:
  the table, made by looping over the patches (columns n_<set>, errors_<set>, foreground_<set>, sum_q_<set>: the tables of all patch sizes
  one after the other, table_offsets says where each starts)
  the histograms at B in LEVELS and accuracy_per_mille in PER_MILLE (hist_<B> uint16 [case, 3, B], the rows of hist_cases_<B> naming set,
  patch and per mille of each case): cell 0 accurate with foreground, 1 inaccurate, 2 accurate pure background, accurate := 1000 (n -
  errors) > per_mille n, patches with n = 0 skipped; the level from the COUNTING definition #{k in 1..B-1 : sum_q B > k n 2^24}, in
  integers.  (To keep the file small the two grids of thousands of patches, (1,1,1) and (3,1,1), have histograms for set 'v0' at 500 per
  mille only.)
  the metrics at B in METRIC_LEVELS, accuracy 500 per mille (`metrics` [set, patch, B, key], keys in `metric_keys`): PAvPU, p(accurate |
  certain), p(uncertain | inaccurate) by brute force over the thresholds k / B (uncertain := level >= k) on per-patch arrays,
  roc_auc_score / average_precision_score(inaccurate, level); once over all patches, once (suffix _fg) over those that hold foreground

Output: tests/golden/g28_patches.npz (arrays, numbers and names only).

    python tests/golden/generate_patches.py
"""
import math
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

PATCHES = [(1, 1, 1), (1, 4, 4), (2, 4, 4), (1, 3, 5), (4, 4, 4), (1, 1, 16), (3, 1, 1), (1, 16, 16), (16, 16, 16)]
LEVELS = [2, 10, 1000, 4096]
PER_MILLE = [0, 500, 999]
METRIC_LEVELS = [10, 1000]
SETS = ['v0', 'v0_mask', 'v0_f32', 'v1', 'v2', 'img']
BASE_KEYS = ['n_patches', 'n_inaccurate', 'pavpu_max', 'pavpu_max_threshold', 'p_ac_at_max', 'p_ui_at_max', 'pavpu_mean', 'auroc', 'auprc']
KEYS = BASE_KEYS + [k + '_fg' for k in BASE_KEYS]
ONE = 1 << 24


def blobs(rng, shape, count):
    """A smooth field: a sum of Gaussian bumps."""
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing='ij')
    field = np.zeros(shape)
    for _ in range(count):
        c = [rng.uniform(0, s) for s in shape]
        r = rng.uniform(2.0, 7.0)
        field += np.exp(-(((z - c[0]) * 2) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * r * r))
    return field


def make_case(rng, shape, count):
    field = blobs(rng, shape, count)
    cut = np.quantile(field, 0.8)
    target = (field > cut).astype(np.uint8)
    prediction = ((field + 0.15 * blobs(rng, shape, count) - 0.05) > cut).astype(np.uint8) * rng.choice([1, 3, 255], size=shape).astype(np.uint8)
    unc = np.clip(1.0 - np.abs(field - cut) * 4.0, 0.0, 1.0)
    unc = np.round(unc * 256) / 256                     # coarse: multiples of 2^-8
    fine = rng.random(shape)                            # one region of full-precision draws
    unc[-1] = np.where(rng.random(shape[1:]) < 0.7, fine[-1], unc[-1])
    return prediction, target, unc


def blocks(unc):
    unc[0:4, 0:8, 0:16] = 0.5                           # whole (1,4,4), (2,4,4), (4,4,4), (1,1,16) patches with a mean ON k / B
    unc[0:4, 8:12, 0:16] = 0.25


def quantise(u):
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        q = np.rint(np.clip(u, 0.0, 1.0) * float(ONE))  # ties to even
    return np.where(np.isnan(u), 0.0, q).astype(np.uint64)


def table_of(prediction, target, unc, mask, patch):
    """[patches, 4] uint64 by looping over the patch masks."""
    d, h, w = target.shape
    pd, ph, pw = patch
    q = quantise(unc)
    rows = []
    for z0 in range(0, d, pd):
        for y0 in range(0, h, ph):
            for x0 in range(0, w, pw):
                inside = np.zeros(target.shape, dtype=bool)
                inside[z0:z0 + pd, y0:y0 + ph, x0:x0 + pw] = True
                if mask is not None:
                    inside &= mask != 0
                p, t = prediction[inside] != 0, target[inside] != 0
                rows.append((int(inside.sum()), int((p != t).sum()), int((p | t).sum()), int(q[inside].sum(dtype=np.uint64))))
    return np.array(rows, dtype=np.uint64).reshape(-1, 4)


def levels_by_counting(n, sum_q, levels):
    """#{k in 1..B-1 : sum_q B > k n 2^24} per row, in uint64 (every product below 2^49)."""
    k = np.arange(1, levels, dtype=np.uint64)[None, :]
    out = np.zeros(len(n), dtype=np.int64)
    for a in range(0, len(n), 512):
        lhs = (sum_q[a:a + 512] * np.uint64(levels))[:, None]
        rhs = k * (n[a:a + 512] * np.uint64(ONE))[:, None]
        out[a:a + 512] = (lhs > rhs).sum(axis=1)
    return out


def cells_of(table, per_mille):
    n, errors, fg = table[:, 0], table[:, 1], table[:, 2]
    accurate = np.uint64(1000) * (n - errors) > np.uint64(per_mille) * n
    return np.where(accurate, np.where(fg > 0, 0, 2), 1)


def brute_force(inaccurate, level, levels):
    """BASE_KEYS of per-patch arrays (inaccurate: bool, level: int), thresholds k / B with uncertain := level >= k."""
    from sklearn.metrics import average_precision_score, roc_auc_score
    nan = float('nan')
    n, n_in = len(level), int(inaccurate.sum())
    if n == 0:
        return [0, 0] + [nan] * 7
    curve = []
    for k in range(1, levels):
        uncertain = level >= k
        n_ac, n_au = int((~inaccurate & ~uncertain).sum()), int((~inaccurate & uncertain).sum())
        n_ic, n_iu = int((inaccurate & ~uncertain).sum()), int((inaccurate & uncertain).sum())
        curve.append(((n_ac + n_iu) / (n_ac + n_au + n_ic + n_iu), n_ac / (n_ac + n_ic) if n_ac + n_ic else nan, n_iu / (n_ic + n_iu) if n_ic + n_iu else nan))
    best = 0
    for i, c in enumerate(curve):
        if c[0] > curve[best][0]:
            best = i                                    # the smallest threshold that attains the maximum
    mean = math.fsum(c[0] for c in curve) / (levels - 1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        auroc = roc_auc_score(inaccurate, level) if 0 < n_in < n else nan
        auprc = average_precision_score(inaccurate, level) if n_in else nan
    return [n, n_in, curve[best][0], (best + 1) / levels, curve[best][1], curve[best][2], mean, auroc, auprc]


def main():
    rng = np.random.default_rng(28)
    out = {'patches': np.array(PATCHES, dtype=np.int64), 'levels': np.array(LEVELS, dtype=np.int64), 'per_mille': np.array(PER_MILLE, dtype=np.int64),
           'metric_levels': np.array(METRIC_LEVELS, dtype=np.int64), 'sets': np.array(SETS), 'metric_keys': np.array(KEYS)}
    shape = (5, 13, 71)
    cases = [make_case(rng, shape, 6) for _ in range(3)] + [make_case(rng, (1, 24, 40), 4)]
    # volume 0: float64 with everything a map can hold
    u0 = cases[0][2]
    blocks(u0)
    u0[0:2, :, 48:] = 0.0                               # an all-zero region
    specials = [np.nan, np.inf, -np.inf, -0.25, 1.5, -0.0, 1.0, 1.0 + 2.0 ** -40, 1.0 - 2.0 ** -30, 2.0 ** -26, 2.0 ** -25, 3 * 2.0 ** -26,
                (1000 + 0.5) / ONE, (1001 + 0.5) / ONE, (ONE - 2 + 0.5) / ONE, (ONE - 1 + 0.5) / ONE, 0.1, 1 / 3, 0.5 + 2.0 ** -40, 0.25 - 2.0 ** -50]
    spots = rng.choice(np.flatnonzero(np.ones(shape, dtype=bool).reshape(-1)), size=8 * len(specials), replace=False)
    flat = u0.reshape(-1)
    block = np.zeros(shape, dtype=bool)
    block[0:4, 0:12, 0:16] = True
    for i, e in enumerate(spots):
        if not block.reshape(-1)[e]:                    # (the constant blocks stay constant)
            flat[e] = specials[i % len(specials)]
    mask0 = rng.choice([0, 1, 2, 255], size=shape, p=[0.2, 0.5, 0.2, 0.1]).astype(np.uint8)
    mask0[:, 0:8, 16:40] = 0                            # whole patches empty
    mask0[3] = 0
    # volumes 1, 2 and the image: what a float32 holds
    for c in (1, 2, 3):
        cases[c] = (cases[c][0], cases[c][1], cases[c][2].astype(np.float32).astype(np.float64))
    blocks(cases[2][2])
    for c, (prediction, target, unc) in enumerate(cases):
        out['prediction_{}'.format(c)], out['target_{}'.format(c)] = prediction, target
        out['uncertainty_{}'.format(c)] = unc if c == 0 else unc.astype(np.float32)
    out['mask_0'] = mask0
    with np.errstate(over='ignore', invalid='ignore'):
        u0_f32 = u0.astype(np.float32).astype(np.float64)
    inputs = {'v0': (*cases[0][:2], u0, None), 'v0_mask': (*cases[0][:2], u0, mask0), 'v0_f32': (*cases[0][:2], u0_f32, None),
              'v1': (*cases[1], None), 'v2': (*cases[2], None), 'img': (*cases[3], None)}
    hists, hist_cases = {b: [] for b in LEVELS}, {b: [] for b in LEVELS}
    metrics = np.full((len(SETS), len(PATCHES), len(METRIC_LEVELS), len(KEYS)), np.nan)
    offsets = np.zeros((len(SETS), len(PATCHES) + 1), dtype=np.int64)
    for s, name in enumerate(SETS):
        prediction, target, unc, mask = inputs[name]
        tables = []
        for p, patch in enumerate(PATCHES):
            table = table_of(prediction, target, unc, mask, patch)
            tables.append(table)
            offsets[s, p + 1] = offsets[s, p] + len(table)
            used = table[table[:, 0] != 0]
            for levels in LEVELS:
                level = levels_by_counting(used[:, 0], used[:, 3], levels)
                for per_mille in PER_MILLE:
                    if len(table) > 1000 and not (name == 'v0' and per_mille == 500):
                        continue
                    hist = np.bincount(cells_of(used, per_mille) * levels + level, minlength=3 * levels)
                    assert hist.max() < 65536
                    hists[levels].append(hist.astype(np.uint16).reshape(3, levels))
                    hist_cases[levels].append((s, p, per_mille))
                if levels in METRIC_LEVELS:
                    cell = cells_of(used, 500)
                    holds = cell != 2
                    metrics[s, p, METRIC_LEVELS.index(levels)] = (brute_force(cell == 1, level, levels) +
                                                                   brute_force(cell[holds] == 1, level[holds], levels))
        table = np.concatenate(tables)
        out['n_' + name], out['errors_' + name], out['foreground_' + name] = (table[:, k].astype(np.uint16) for k in range(3))
        out['sum_q_' + name] = table[:, 3]
    out['table_offsets'], out['metrics'] = offsets, metrics
    for b in LEVELS:
        out['hist_{}'.format(b)], out['hist_cases_{}'.format(b)] = np.stack(hists[b]), np.array(hist_cases[b], dtype=np.int64)
    path = os.path.join(HERE, 'g28_patches.npz')
    np.savez_compressed(path, **out)
    print('{}: {} bytes, {} histograms per B'.format(path, os.path.getsize(path), len(hists[LEVELS[0]])))


if __name__ == '__main__':
    main()
