"""EXTENSION -- nearest-neighbour feature uncertainty (include/rcu_knn.h "Nearest-neighbour feature uncertainty"; Sun et al., ICML 2022, deep
nearest neighbours).  A bank of held-out feature vectors is sampled from the U-Net's penultimate features; at test time a voxel is uncertain when
its (L2-normalised) feature vector is far from its k-th nearest bank row: one eval-mode forward pass, any trained checkpoint, no retraining and
no distributional assumption.  The two kernels are HIP (csrc/rcu_knn.hip): ``sample_keys`` -- the Philox key of every voxel -- and ``distances``
-- the voxels x bank distance product with its k-smallest selection.  The bank of a class is the voxels with the smallest (key, slice, pixel)
triples, so it is a function of the set of slices alone: it cannot depend on batching or slice order."""
import ctypes
import os
import zipfile

import numpy as np
import torch

from . import _lib
from .density import _feature_channels, _nhwc, eval_features

MAX_FEATURES = _lib.RCU_KNN_MAX_FEATURES
MAX_BANK = _lib.RCU_KNN_MAX_BANK
MAX_K = _lib.RCU_KNN_MAX_K
MIN_NORM = 2.0 ** -40
_FIELDS = ('features', 'labels', 'key63', 'g', 'v')
_DTYPES = dict(features=np.float32, labels=np.uint8, key63=np.int64, g=np.int64, v=np.int64)


def knn_seed(seed):
    """Key of the bank's sampling draw for a run seeded with ``seed``: ``pass_seed(seed, 0)`` + 32 * 2^40.  The mask, augmentation and logit keys
    lie within 2048 + 7 * 2^40 of ``pass_seed(seed, 0)`` and the corruption keys end at 23 * 2^40 above it (``corruption.corruption_seed``): nothing of
    the same seed reaches this key."""
    from . import steps
    return (steps.pass_seed(seed, 0) + 32 * (1 << 40)) % (2 ** 63 - 1)


def check_model(model):
    """The model's feature channels; a model that is no ``model.UNet`` or has more than 32 of them is refused by name."""
    channels = _feature_channels(model)
    if channels > MAX_FEATURES:
        raise ValueError('the k-NN uncertainty takes U-Nets of up to {} feature channels (start_filters), got {}'.format(MAX_FEATURES, channels))
    return channels


def sample_keys(n, hw, slice_index, seed, device=None):
    """The sampling keys of ``n`` slices of ``hw`` pixels: int64 ``[n, hw]`` on the device, entry (i, v) being key63 of (global slice index
    ``slice_index[i]``, pixel v) under ``knn_seed(seed)`` (include/rcu_knn.h "Sampling keys")."""
    n, hw = int(n), int(hw)
    if torch.is_tensor(slice_index):
        device = slice_index.device if device is None and slice_index.is_cuda else device
        index = slice_index.detach().to('cpu', torch.int64).reshape(-1)
    else:
        index = torch.as_tensor([int(g) for g in slice_index], dtype=torch.int64)
    if index.numel() != n or (n and int(index.min()) < 0):
        raise ValueError('sample_keys: slice_index must hold {} indices >= 0'.format(n))
    device = torch.device('cuda' if device is None else device)
    if device.type != 'cuda':
        raise RuntimeError('rcu_amd.knn only runs on the GPU (librcu_hip); got the device {}'.format(device))
    index = index.to(device)
    keys = torch.empty((n, hw), device=device, dtype=torch.int64)
    if n * hw:
        _lib.check(_lib.load().rcu_knn_sample_keys(n, hw, _lib.ptr(index), knn_seed(seed), _lib.ptr(keys), _lib.current_stream()))
    return keys


class KnnBank:
    """The sampled bank: ``features`` float32 ``[M, F]`` as tapped, ``labels`` uint8 ``[M]``, and the triples that chose the rows -- ``key63``, ``g``
    (global slice index) and ``v`` (pixel) int64 ``[M]`` -- in the order class, then ascending triple; ``normalize``, ``per_class`` (the M_c asked
    for) and the ``seed`` of the draw."""

    def __init__(self, features, labels, key63, g, v, normalize=True, per_class=(), seed=0):
        given = dict(features=features, labels=labels, key63=key63, g=g, v=v)
        for name in _FIELDS:
            a = np.asarray(given[name])
            if a.dtype != _DTYPES[name]:
                raise ValueError('KnnBank: {} must be {}, got {}'.format(name, np.dtype(_DTYPES[name]).name, a.dtype))
            setattr(self, name, np.ascontiguousarray(a))
        if self.features.ndim != 2:
            raise ValueError('KnnBank: features must be [M, F]')
        self.M, self.F = (int(s) for s in self.features.shape)
        if not 1 <= self.F <= MAX_FEATURES:
            raise ValueError('KnnBank: F must be in 1..{}, got {}'.format(MAX_FEATURES, self.F))
        if not 1 <= self.M <= MAX_BANK:
            raise ValueError('KnnBank: M must be in 1..{}, got {}'.format(MAX_BANK, self.M))
        if any(getattr(self, name).shape != (self.M,) for name in _FIELDS[1:]):
            raise ValueError('KnnBank: labels, key63, g and v must have the bank\'s M = {} entries'.format(self.M))
        if not np.isfinite(self.features).all():
            raise ValueError('KnnBank: the features are not finite')
        order = np.lexsort((self.v, self.g, self.key63, self.labels))
        if not np.array_equal(order, np.arange(self.M)):
            raise ValueError('KnnBank: the rows are not in the order class, then ascending (key63, g, v)')
        self.normalize = bool(normalize)
        self.per_class = tuple(int(m) for m in np.asarray(per_class).reshape(-1))
        self.seed = int(seed)
        self._device = {}

    def counts(self):
        k = max(len(self.per_class), int(self.labels.max()) + 1)
        return [int(c) for c in np.bincount(self.labels, minlength=k)]

    def as_dict(self):
        return {'F': self.F, 'M': self.M, 'counts': self.counts(), 'per_class': list(self.per_class), 'normalize': self.normalize, 'seed': self.seed}

    def float32_parameters(self):
        """(rows, bank_sq): what the device evaluates, and what a reference has to evaluate in float64.  With ``normalize`` the rows are the
        features divided by max(|row|, 2^-40) in float64 and rounded once to float32; bank_sq = |row|^2 summed in float64 from the rounded rows and
        rounded once."""
        rows = self.features.astype(np.float64)
        if self.normalize:
            rows = rows / np.maximum(np.sqrt((rows * rows).sum(1, keepdims=True)), MIN_NORM)
        rows = rows.astype(np.float32)
        wide = rows.astype(np.float64)
        return rows, (wide * wide).sum(1).astype(np.float32)

    def device_parameters(self, device):
        """The float32 parameters on ``device``, uploaded once."""
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(a).to(device).contiguous() for a in self.float32_parameters())
        return self._device[key]


def _per_class(per_class, nb_classes):
    k = int(nb_classes)
    sizes = [per_class] * k if isinstance(per_class, (int, np.integer)) and not isinstance(per_class, bool) else list(per_class)
    if len(sizes) != k or any(isinstance(m, bool) or int(m) != m or int(m) < 1 for m in sizes):
        raise ValueError('per_class must be an integer >= 1 or one per class ({} classes), got {!r}'.format(k, per_class))
    sizes = [int(m) for m in sizes]
    if sum(sizes) > MAX_BANK:
        raise ValueError('the bank takes up to {} rows, per_class asks for {}'.format(MAX_BANK, sum(sizes)))
    return sizes


def merge_candidates(kept, candidates, per_class):
    """The candidates so far (``kept``: a dict of the five bank arrays, or None) and a batch's (``candidates``, likewise) -> per class c the
    ``per_class[c]`` rows with the smallest triples (key63, g, v) of both, in the order class, then ascending triple.  Keeping the smallest of a
    union is associative and commutative: any partition of the slices into batches, in any order, ends with the same rows."""
    parts = [p for p in (kept, candidates) if p is not None]
    both = {name: np.concatenate([np.asarray(p[name], dtype=_DTYPES[name]) for p in parts]) for name in _FIELDS}
    order = np.lexsort((both['v'], both['g'], both['key63'], both['labels']))
    labels = both['labels'][order]
    keep = []
    for c, m in enumerate(per_class):
        first = int(np.searchsorted(labels, c, side='left'))
        last = int(np.searchsorted(labels, c, side='right'))
        keep.append(order[first:min(last, first + int(m))])
    keep = np.concatenate(keep) if keep else order[:0]
    return {name: both[name][keep] for name in _FIELDS}


def _slice_indices(batch, n, counted):
    if len(batch) < 3 or batch[2] is None:
        return list(range(counted, counted + n))
    g = batch[2]
    if torch.is_tensor(g) or isinstance(g, (list, tuple, np.ndarray)):
        g = [int(i) for i in (g.tolist() if torch.is_tensor(g) else g)]
        if len(g) != n:
            raise ValueError('fit_knn: a batch of {} slices came with {} slice indices'.format(n, len(g)))
        return g
    return list(range(int(g), int(g) + n))


def fit_knn(model, batches, per_class, seed, normalize=True, nb_classes=None):
    """Sample the bank on ``batches``: an iterable of ``(images [n, C_in, H, W], target [n, H, W])`` or ``(images, target, g)`` with integer
    targets in 0..nb_classes-1 (``nb_classes``: the model's by default) and ``g`` the global index of the batch's first slice (or one index per
    slice); without it the slices are counted in the order they come, as the test scripts count theirs.  One eval-mode forward per batch with the
    feature tap; per class the ``per_class`` voxels with the smallest (key63, g, v) over all slices seen are kept -- all of them when the class
    has fewer -- so the same slices in other batches or another order give the same arrays.  A class without a voxel raises ValueError.
    -> KnnBank."""
    check_model(model)
    k = int(model.nb_classes if nb_classes is None else nb_classes)
    sizes = _per_class(per_class, k)
    seed = 0 if seed is None else int(seed)
    kept, counted = None, 0
    never = torch.iinfo(torch.int64).max
    with eval_features(model):
        for batch in batches:
            images, target = batch[0], batch[1]
            n, _, h, w = images.shape
            g = _slice_indices(batch, n, counted)
            counted += n
            if not torch.is_tensor(target) or target.numel() != n * h * w or target.is_floating_point():
                raise ValueError('fit_knn: the target must be an integer tensor of {} x {} x {} entries'.format(n, h, w))
            model(images)
            features = model.features
            f = features.shape[1]
            flat = features.permute(0, 2, 3, 1).reshape(n * h * w, f)
            target = target.to(features.device).reshape(-1)
            if n and (int(target.min()) < 0 or int(target.max()) >= k):
                raise ValueError('fit_knn: the target must lie in 0..{} (nb_classes = {})'.format(k - 1, k))
            keys = sample_keys(n, h * w, g, seed, device=features.device).reshape(-1)
            chosen, labels = [], []
            for c in range(k):
                member = target == c
                count = int(member.sum())
                if not count:
                    continue
                keys_c = torch.where(member, keys, torch.full_like(keys, never))
                bound = torch.topk(keys_c, min(sizes[c], count), largest=False).values.max()
                # every voxel of the class at or below the bound: voxels that tie with it are all candidates, the triple decides on the host
                index = torch.nonzero(member & (keys <= bound)).reshape(-1)
                chosen.append(index)
                labels.append(torch.full_like(index, c, dtype=torch.uint8))
            if not chosen:
                continue
            index = torch.cat(chosen)
            g_of = torch.as_tensor(g, dtype=torch.int64, device=index.device)
            candidates = dict(features=flat[index].to(torch.float32).cpu().numpy(), labels=torch.cat(labels).cpu().numpy(),
                              key63=keys[index].cpu().numpy(), g=g_of[index // (h * w)].cpu().numpy(), v=(index % (h * w)).cpu().numpy())
            kept = merge_candidates(kept, candidates, sizes)
    if kept is None:
        raise ValueError('fit_knn: no batches')
    for c in range(k):
        if not (kept['labels'] == c).any():
            raise ValueError('class {} has no voxel in the slices seen: the bank needs at least one per class'.format(c))
    return KnnBank(normalize=normalize, per_class=sizes, seed=seed, **kept)


def save_knn(bank, path):
    """``bank`` -> an .npz of its arrays (no pickle) with normalize, per_class and seed."""
    with open(os.fspath(path), 'wb') as f:
        np.savez(f, normalize=np.bool_(bank.normalize), per_class=np.asarray(bank.per_class, dtype=np.int64), seed=np.int64(bank.seed),
                 **{name: getattr(bank, name) for name in _FIELDS})


def load_knn(path):
    """The KnnBank ``save_knn`` wrote; anything else raises a ValueError that names the file."""
    path = os.fspath(path)
    try:
        with np.load(path, allow_pickle=False) as doc:
            missing = [name for name in _FIELDS + ('normalize', 'per_class', 'seed') if name not in doc.files]
            if missing:
                raise ValueError('no {} array'.format(', '.join(missing)))
            if doc['normalize'].shape != () or doc['seed'].shape != () or doc['per_class'].ndim != 1:
                raise ValueError('normalize and seed must be scalars, per_class a vector')
            return KnnBank(*(doc[name] for name in _FIELDS), normalize=bool(doc['normalize']), per_class=doc['per_class'], seed=int(doc['seed']))
    except (OSError, ValueError, KeyError, EOFError, zipfile.BadZipFile) as e:      # (BadZipFile: a file that is no .npz)
        raise ValueError('k-NN bank file {!r} cannot be read: {}'.format(path, e)) from None


def check_k(bank, k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_K:
        raise ValueError('k must be an integer in 1..{}, got {!r}'.format(MAX_K, k))
    if int(k) > bank.M:
        raise ValueError('k = {} exceeds the bank\'s M = {} rows'.format(int(k), bank.M))
    return int(k)


def distances(bank, features, k, with_neighbours=False):
    """The distance of every voxel of the ``[N, F, H, W]`` features to its k-th nearest row of ``bank``: float32 ``[N, 1, H, W]``; with
    ``with_neighbours`` also the k sorted squared distances ``[N, H, W, k]``.  A voxel's values depend on its feature values and the bank alone."""
    k = check_k(bank, k)
    if isinstance(features, torch.Tensor) and features.dim() == 4 and features.shape[1] > MAX_FEATURES:
        raise ValueError('the k-NN kernel takes 1..{} feature channels, got {}'.format(MAX_FEATURES, features.shape[1]))
    nhwc, pitch = _nhwc(features)
    n, f, h, w = features.shape
    if f != bank.F:
        raise ValueError('the bank has F = {} feature channels, the features have {}'.format(bank.F, f))
    rows, rows_sq = bank.device_parameters(features.device)
    out = torch.empty((n, 1, h, w), device=features.device, dtype=torch.float32)
    d2 = torch.empty((n, h, w, k), device=features.device, dtype=torch.float32) if with_neighbours else None
    if n * h * w:
        _lib.check(_lib.load().rcu_knn_distances(ctypes.c_void_p(nhwc.data_ptr()), pitch, f, n * h * w, _lib.ptr(rows), _lib.ptr(rows_sq), bank.M, k,
                                                 int(bank.normalize), _lib.ptr(out), _lib.ptr(d2), _lib.current_stream()))
    return (out, d2) if with_neighbours else out
