"""Float64 numpy restatement of include/rcu_knn.h "Nearest-neighbour feature uncertainty": the bank's float32 parameters, the distances and their k
smallest, the error bound the device is held to, the sampling keys (on oracle.mask_oracle.philox4x32_10, which is pinned to the published vectors)
and the bank selection by sorting triples.  Nothing here imports the package."""
import numpy as np

from oracle import mask_oracle as mo

MIN_NORM = 2.0 ** -40
U = 2.0 ** -24
COUNTER_TAG = 0x6b6e6e
M63 = 2 ** 63 - 1


def knn_seed(seed):
    """pass_seed(seed, 0) + 32 * 2^40 mod 2^63 - 1, pass_seed(seed, 0) = seed * 1000003 mod 2^63 - 1."""
    return ((int(seed) * 1000003) % M63 + 32 * (1 << 40)) % M63


def key63(key, g, v):
    """key63 of the voxels (global slice index g, pixel v) -- arrays of one shape -- under the 64-bit ``key``: int64."""
    g = np.asarray(g, dtype=np.uint64)
    v = np.asarray(v, dtype=np.uint64)
    g, v = np.broadcast_arrays(g, v)
    counter = np.zeros(g.shape + (4,), dtype=np.uint32)
    counter[..., 0] = (v & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    counter[..., 1] = (g & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    counter[..., 2] = (g >> np.uint64(32)).astype(np.uint32)
    counter[..., 3] = np.uint32(COUNTER_TAG)
    key = int(key)
    r = mo.philox4x32_10(counter, (key & 0xFFFFFFFF, key >> 32))
    word = (r[..., 0].astype(np.uint64) << np.uint64(32)) | r[..., 1].astype(np.uint64)
    return (word >> np.uint64(1)).astype(np.int64)


def slice_keys(seed, slice_index, hw):
    """int64 [n, hw]: what rcu_amd.knn.sample_keys(n, hw, slice_index, seed) returns."""
    g = np.asarray(slice_index, dtype=np.uint64).reshape(-1, 1)
    return key63(knn_seed(seed), g, np.arange(hw, dtype=np.uint64)[None, :])


def normalised(phi):
    """xhat = phi / max(|phi|, 2^-40) in float64 from the float32 (or any) values of ``phi`` [n, F]."""
    phi = np.asarray(phi, dtype=np.float64)
    return phi / np.maximum(np.sqrt((phi * phi).sum(-1, keepdims=True)), MIN_NORM)


def bank_parameters(features, normalize):
    """(rows float32 [M, F], bank_sq float32 [M]) of the tapped float32 ``features``: rows normalised in float64 and rounded once when ``normalize``;
    bank_sq summed in float64 from the rounded rows and rounded once."""
    rows = np.asarray(features, dtype=np.float32).astype(np.float64)
    if normalize:
        rows = normalised(rows)
    rows = rows.astype(np.float32)
    wide = rows.astype(np.float64)
    return rows, (wide * wide).sum(1).astype(np.float32)


def queries(phi, normalize):
    phi = np.asarray(phi, dtype=np.float32).astype(np.float64)
    return normalised(phi) if normalize else phi


def squared_distances(phi, rows, normalize):
    """d2(v, m) float64 [n, M] of the float32 features ``phi`` [n, F] against the float32 bank ``rows`` (``bank_parameters``): in exact arithmetic
    |xhat|^2 + |b|^2 - 2 xhat . b is sum_c (xhat_c - b_c)^2, which float64 evaluates without cancellation."""
    x = queries(phi, normalize)
    b = np.asarray(rows, dtype=np.float64)
    out = np.empty((x.shape[0], b.shape[0]))
    for i in range(0, x.shape[0], 4096):
        diff = x[i:i + 4096, None, :] - b[None, :, :]
        out[i:i + 4096] = (diff * diff).sum(-1)
    return out


def neighbours(phi, rows, k, normalize):
    """The k smallest of d2(v, .) as a sorted multiset: float64 [n, k]."""
    return np.sort(squared_distances(phi, rows, normalize), axis=1)[:, :k]


def score(phi, rows, k, normalize):
    return np.sqrt(neighbours(phi, rows, k, normalize)[:, k - 1])


def error_bound(phi, rows, normalize):
    """max_m E(v, m), E = (2 F + 8) 2^-24 (|xhat_v| + |b_m|)^2: float64 [n] -- what every one of the k sorted device distances is held to."""
    x = queries(phi, normalize)
    b = np.asarray(rows, dtype=np.float64)
    f = x.shape[1]
    nx, nb = np.sqrt((x * x).sum(1)), np.sqrt((b * b).sum(1))
    return (2 * f + 8) * U * (nx + nb.max()) ** 2


def select_bank(labels, keys, per_class):
    """The bank's triples by sorting: ``labels`` [slices, hw] and ``keys`` [slices, hw] of the slices with global indices 0 .. slices - 1 ->
    (label, key63, g, v) int64 arrays in the order class, then ascending (key63, g, v), per class c the first ``per_class[c]``."""
    labels, keys = np.asarray(labels), np.asarray(keys)
    rows = []
    for c, m in enumerate(per_class):
        g, v = np.nonzero(labels == c)
        triples = sorted(zip(keys[g, v].tolist(), g.tolist(), v.tolist()))[:m]
        rows += [(c,) + t for t in triples]
    out = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    return out[:, 0], out[:, 1], out[:, 2], out[:, 3]
