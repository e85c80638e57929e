"""The definitions of include/rcu.h, "Quantile rescale", restated in integer numpy (no GPU, nothing of the package): the key, the population, the
table, the level, the rescaled value, and one radix pass of the selection."""
import numpy as np


def key(values):
    """uint32, order-preserving over all of float32 (NaN has none): -0.0 as +0.0; ``~b`` where the sign bit is set, else ``b | 0x80000000``."""
    b = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    negative = (b >> 31) != 0
    return np.where(negative, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def population_keys(maps, masks=None):
    """The keys of the population over all maps of a run, in one array: inside the masks where there are any, every voxel otherwise."""
    parts = []
    for i, m in enumerate(maps):
        k = key(np.asarray(m).reshape(-1))
        if masks is not None:
            k = k[np.asarray(masks[i]).reshape(-1) != 0]
        parts.append(k)
    return np.concatenate(parts)


def ranks(n, q):
    """r_k = ceil(k n / Q), k = 1 .. Q-1, in Python integers."""
    return [(k * int(n) + int(q) - 1) // int(q) for k in range(1, int(q))]


def table(keys, q):
    """(N, ranks, boundary keys b_k = the key of the r_k-th smallest population value)."""
    ordered = np.sort(np.asarray(keys, dtype=np.uint32))
    r = ranks(ordered.size, q)
    return int(ordered.size), np.array(r, dtype=np.int64), ordered[np.array(r, dtype=np.int64) - 1]


def levels(keys, bounds):
    """l = #{k : key > b_k}."""
    return np.searchsorted(np.asarray(bounds, dtype=np.uint32), np.asarray(keys, dtype=np.uint32), side='left').astype(np.int64)


def rescaled(level, q):
    """(l + 0.5) / Q in float64, stored as float32."""
    return ((np.asarray(level, dtype=np.float64) + 0.5) / float(q)).astype(np.float32)


def grid_level(u, b):
    """The rule every evaluation action reads an uncertainty through: #{k in 1..B-1 : u > k / B}, compared in float64."""
    thresholds = np.arange(1, int(b), dtype=np.float64) / float(b)
    return np.searchsorted(thresholds, np.asarray(u, dtype=np.float64), side='left').astype(np.int64)


def key_hist(keys, prefixes, shift, bits):
    """One radix pass over population keys: int64 [max(len(prefixes), 1), 2^bits]; no prefixes: everything is slot 0."""
    keys = np.asarray(keys, dtype=np.uint64)
    hi = keys >> np.uint64(shift + bits)
    digit = ((keys >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.int64)
    out = np.zeros((max(len(prefixes), 1), 1 << bits), dtype=np.int64)
    if len(prefixes) == 0:
        np.add.at(out[0], digit, 1)
        return out
    table_ = np.asarray(prefixes, dtype=np.uint64)
    slot = np.searchsorted(table_, hi)
    listed = (slot < table_.size) & (table_[np.minimum(slot, table_.size - 1)] == hi)
    np.add.at(out, (slot[listed], digit[listed]), 1)
    return out


def select(keys, q, plan):
    """The table by the radix passes of ``plan`` (digit widths from the top, adding up to 32), each pass a ``key_hist`` and a host step written
    out here on its own -- a second route to ``table`` that shares nothing with the package's ``quantile_refine``.  -> (boundary keys, the
    (prefixes, shift, bits, hist) of every pass)."""
    keys = np.asarray(keys, dtype=np.uint32)
    r = ranks(keys.size, q)
    prefix = [0] * len(r)
    passes, shift, prefixes = [], 32, []
    for bits in plan:
        shift -= bits
        hist = key_hist(keys, prefixes, shift, bits)
        passes.append((list(prefixes), shift, bits, hist))
        row_of = {p: i for i, p in enumerate(prefixes)} if prefixes else None
        below_or_at = np.cumsum(hist, axis=1)       # [row][d] = the row's voxels with a digit <= d
        for k in range(len(r)):
            row = below_or_at[row_of[prefix[k]] if row_of else 0]
            d = int(np.argmax(row >= r[k]))          # the first digit at which the count reaches the rank
            assert row[d] >= r[k]
            r[k] -= int(row[d - 1]) if d else 0
            prefix[k] = (prefix[k] << bits) | d
        prefixes = sorted(set(prefix))
    return np.array(prefix, dtype=np.uint32), passes
