"""EXTENSION -- feature-space density uncertainty (include/rcu.h "Feature-space density"; Mukhoti et al. 2021, Deep Deterministic Uncertainty;
Lee et al. 2018 for the shared covariance).  One Gaussian per target class is fitted to the U-Net's penultimate features on held-out data; at
test time a voxel is uncertain when its feature vector is improbable under that mixture: one eval-mode forward pass, any trained checkpoint, no
retraining.  The two hot paths are HIP kernels (csrc/rcu_density.hip): ``feature_moments`` -- per-slice class-conditioned counts, sums and Gram
matrices -- and ``energy`` -- the negative log density per voxel.  The fit between them is host arithmetic in float64 with exactly rounded sums,
so it cannot depend on batching or slice order."""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib

MAX_FEATURES = 64
MAX_CLASSES = 8
CHUNK = 1024      # RCU_DENSITY_CHUNK: voxels a float32 accumulator covers before it is promoted


def _nhwc(features):
    """The ``[N, F, H, W]`` feature tensor -> (tensor that owns the memory, pitch): in place when it is the permuted view ``UNet.features``
    returns (channels-last at a pitch, as ``PostNet.forward`` recovers it), else a channels-last copy at a pitch of F rounded up to 4."""
    if not isinstance(features, torch.Tensor) or features.dim() != 4:
        raise ValueError('expected a [N, F, H, W] feature tensor')
    if not features.is_cuda:
        raise RuntimeError('rcu_amd.density only runs on the GPU (librcu_hip); got a {} tensor'.format(features.device))
    n, f, h, w = features.shape
    if not 1 <= f <= MAX_FEATURES:
        raise ValueError('the density kernels take 1..{} feature channels, got {}'.format(MAX_FEATURES, f))
    nhwc = features.permute(0, 2, 3, 1)
    pitch = nhwc.stride(2)
    in_place = (features.dtype == torch.float32 and nhwc.stride(3) == 1 and pitch >= f and pitch % 4 == 0 and nhwc.stride(1) == w * pitch and
                nhwc.stride(0) == h * w * pitch and features.data_ptr() % 16 == 0)
    if in_place:
        return nhwc, pitch
    pitch = (f + 3) // 4 * 4
    buf = torch.zeros((n, h, w, pitch), device=features.device, dtype=torch.float32)
    buf[..., :f] = nhwc
    return buf, pitch


def feature_moments(features, labels, nb_classes):
    """Per slice and class: ``n`` int64 ``[N, K]``, ``S`` = sum phi float64 ``[N, K, F]``, ``G`` = sum phi phi^T float64 ``[N, K, F, F]`` (both
    triangles) of the ``[N, F, H, W]`` features under the integer ``labels`` ``[N, H, W]`` (or ``[N, 1, H, W]``) in 0..K-1, on the device.  The rows
    of a slice are bit for bit a function of that slice alone.  A label outside 0..K-1 raises ValueError."""
    k = int(nb_classes)
    if not 1 <= k <= MAX_CLASSES:
        raise ValueError('nb_classes must be in 1..{}, got {}'.format(MAX_CLASSES, nb_classes))
    nhwc, pitch = _nhwc(features)
    n, f, h, w = features.shape
    if not torch.is_tensor(labels) or labels.numel() != n * h * w or labels.is_floating_point():
        raise ValueError('labels must be an integer tensor of {} x {} x {} entries'.format(n, h, w))
    labels = labels.to(features.device).reshape(n, h * w)
    if n and (int(labels.min()) < 0 or int(labels.max()) >= k):
        raise ValueError('labels must lie in 0..{} (nb_classes = {}), got {}..{}'.format(k - 1, k, int(labels.min()), int(labels.max())))
    labels = labels.to(torch.uint8).contiguous()
    lib = _lib.load()
    counts = torch.empty((n, k), device=features.device, dtype=torch.int64)
    s = torch.empty((n, k, f), device=features.device, dtype=torch.float64)
    g = torch.empty((n, k, f, f), device=features.device, dtype=torch.float64)
    ws = torch.empty(max(int(lib.rcu_density_moments_workspace_bytes(n, h * w, f, k)), 8) // 8, device=features.device, dtype=torch.float64)
    _lib.check(lib.rcu_density_moments(ctypes.c_void_p(nhwc.data_ptr()), pitch, f, _lib.ptr(labels), n, h * w, k, _lib.ptr(counts), _lib.ptr(s),
                                       _lib.ptr(g), _lib.ptr(ws), _lib.current_stream()))
    return counts, s, g


class DensityFit:
    """The class Gaussians: ``F`` channels, ``K`` classes, ``n`` int64 ``[K]``, ``mu`` ``[K, F]``, ``cov`` ``[K, F, F]`` (with the ridge), ``A`` =
    chol(cov)^-1 ``[K, F, F]`` lower triangular, ``b`` = A mu ``[K, F]``, ``k`` ``[K]`` (float64 all), ``ridge``, ``shared_covariance`` and the
    ``voxels`` the fit saw."""

    def __init__(self, n, mu, cov, A, b, k, ridge, shared_covariance=False):
        self.n = np.ascontiguousarray(n, dtype=np.int64)
        self.mu, self.cov, self.A, self.b, self.k = (np.ascontiguousarray(v, dtype=np.float64) for v in (mu, cov, A, b, k))
        self.K, self.F = (int(v) for v in self.mu.shape)
        if self.n.shape != (self.K,) or self.cov.shape != (self.K, self.F, self.F) or self.A.shape != self.cov.shape or \
                self.b.shape != self.mu.shape or self.k.shape != (self.K,):
            raise ValueError('DensityFit: the arrays do not have the shapes of K = {} classes, F = {} channels'.format(self.K, self.F))
        self.ridge, self.shared_covariance = float(ridge), bool(shared_covariance)
        self.voxels = int(self.n.sum())
        self._device = {}

    def as_dict(self):
        return {'F': self.F, 'K': self.K, 'counts': [int(v) for v in self.n], 'ridge': self.ridge, 'voxels': self.voxels,
                'shared_covariance': self.shared_covariance}

    def float32_parameters(self):
        """(A, b, k) rounded once to float32: what the device evaluates, and what a reference has to evaluate in float64."""
        return self.A.astype(np.float32), self.b.astype(np.float32), self.k.astype(np.float32)

    def device_parameters(self, device):
        """The float32 parameters on ``device``, uploaded once."""
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(v).to(device).contiguous() for v in self.float32_parameters())
        return self._device[key]


def _fsum_over_slices(a):
    """Every entry of ``a[slice, ...]`` summed over the slices with an exactly rounded sum."""
    a = np.asarray(a, dtype=np.float64)
    flat = a.reshape(a.shape[0], -1)
    return np.array([math.fsum(col) for col in flat.T.tolist()], dtype=np.float64).reshape(a.shape[1:])


def _inverse_lower(L):
    """L^-1 of a lower-triangular L by forward substitution, row by row: lower triangular by construction."""
    f = L.shape[0]
    inv = np.zeros_like(L)
    eye = np.eye(f)
    for i in range(f):
        inv[i] = (eye[i] - L[i, :i] @ inv[:i]) / L[i, i]
    return inv


def fit_from_moments(n, S, G, ridge=1e-6, shared_covariance=False):
    """The fit of include/rcu.h from per-slice moments ``n [slices, K]``, ``S [slices, K, F]``, ``G [slices, K, F, F]`` (numpy or tensors):
    exactly rounded sums over the slices, then float64.  A class with n_c <= F raises ValueError."""
    n, S, G = (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v) for v in (n, S, G))
    if n.ndim != 2 or S.ndim != 3 or G.ndim != 4 or S.shape[:2] != n.shape or G.shape != S.shape + S.shape[2:]:
        raise ValueError('fit_from_moments: expected n [slices, K], S [slices, K, F], G [slices, K, F, F]')
    if not (np.isfinite(ridge) and ridge >= 0):
        raise ValueError('ridge must be a finite number >= 0, got {!r}'.format(ridge))
    K, F = S.shape[1:]
    counts = np.array([sum(int(v) for v in n[:, c]) for c in range(K)], dtype=np.int64)
    for c in range(K):
        if counts[c] <= F:
            raise ValueError('class {} has {} voxels: the fit needs more than F = {} per class'.format(c, int(counts[c]), F))
    s_sum, g_sum = _fsum_over_slices(S), _fsum_over_slices(G)
    total = int(counts.sum())
    mu = s_sum / counts[:, None].astype(np.float64)
    cov = g_sum / counts[:, None, None].astype(np.float64) - mu[:, :, None] * mu[:, None, :]
    if shared_covariance:
        pooled = sum(float(counts[c]) * cov[c] for c in range(K)) / float(total)
        cov = np.repeat(pooled[None], K, axis=0)
    cov = cov + ridge * (np.trace(cov, axis1=1, axis2=2) / F)[:, None, None] * np.eye(F)[None]
    A, b, k = np.zeros_like(cov), np.zeros_like(mu), np.zeros(K)
    for c in range(K):
        try:
            L = np.linalg.cholesky(cov[c])
        except np.linalg.LinAlgError:
            raise ValueError('class {}: the covariance of the features is not positive definite (ridge = {!r}); a larger ridge lets dead '
                             'channels through'.format(c, ridge)) from None
        A[c] = _inverse_lower(L)
        b[c] = A[c] @ mu[c]
        k[c] = math.log(int(counts[c]) / total) - float(np.log(np.diag(L)).sum()) - 0.5 * F * math.log(2.0 * math.pi)
    return DensityFit(counts, mu, cov, A, b, k, ridge, shared_covariance)


def _feature_channels(model):
    from . import model as model_mod
    if not isinstance(model, model_mod.UNet):
        raise ValueError('the density uncertainty needs a rcu_amd.model.UNet (its feature tap), got {}'.format(type(model).__name__))
    return int(model.start_filters)


class eval_features:
    """Context: ``model`` in eval mode (no dropout site active) with ``provide_features`` set; the flag is restored on the way out."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        from . import steps
        self.before = self.model.provide_features
        steps.set_dropout_mode(self.model, False)
        self.model.provide_features = True
        return self.model

    def __exit__(self, *exc):
        self.model.provide_features = self.before
        return False


def fit_density(model, batches, ridge=1e-6, shared_covariance=False, nb_classes=None):
    """Fit the class Gaussians on ``batches``: an iterable of ``(images [n, C_in, H, W], target [n, H, W])`` with integer targets in
    0..nb_classes-1 (``nb_classes``: the model's by default).  One eval-mode forward per batch with the feature tap; per-slice moments are kept and
    combined at the end with exactly rounded sums -- the same slices in other batches or another order give the same bits.  -> DensityFit."""
    _feature_channels(model)
    k = int(model.nb_classes if nb_classes is None else nb_classes)
    rows = []
    with eval_features(model):
        for batch in batches:
            images, target = batch[0], batch[1]
            model(images)
            counts, s, g = feature_moments(model.features, target, k)
            rows.append((counts.cpu().numpy(), s.cpu().numpy(), g.cpu().numpy()))
    if not rows:
        raise ValueError('fit_density: no batches')
    return fit_from_moments(*(np.concatenate([r[i] for r in rows]) for i in range(3)), ridge=ridge, shared_covariance=shared_covariance)


_ARRAYS = ('n', 'mu', 'cov', 'A', 'b', 'k')


def save_density(fit, path):
    """``fit`` -> an .npz of its arrays (float64 / int64 as they are) with ridge and shared_covariance."""
    with open(os.fspath(path), 'wb') as f:
        np.savez(f, ridge=np.float64(fit.ridge), shared_covariance=np.bool_(fit.shared_covariance), **{name: getattr(fit, name) for name in _ARRAYS})


def load_density(path):
    """The DensityFit ``save_density`` wrote; anything else raises ValueError."""
    path = os.fspath(path)
    try:
        with np.load(path, allow_pickle=False) as doc:
            missing = [name for name in _ARRAYS + ('ridge',) if name not in doc.files]
            if missing:
                raise ValueError('no {} array'.format(', '.join(missing)))
            return DensityFit(*(doc[name] for name in _ARRAYS), ridge=float(doc['ridge']),
                              shared_covariance=bool(doc['shared_covariance']) if 'shared_covariance' in doc.files else False)
    except (OSError, ValueError) as e:
        raise ValueError('density file {!r} cannot be read: {}'.format(path, e)) from None


def energy(fit, features, with_d2=False):
    """The negative log density of every voxel of the ``[N, F, H, W]`` features under ``fit``: float32 ``[N, 1, H, W]``; with ``with_d2`` also the
    squared Mahalanobis distances ``[N, H, W, K]``.  A voxel's energy depends on its feature values and the parameters alone."""
    nhwc, pitch = _nhwc(features)
    n, f, h, w = features.shape
    if f != fit.F:
        raise ValueError('the fit has F = {} feature channels, the features have {}'.format(fit.F, f))
    a, b, k = fit.device_parameters(features.device)
    out = torch.empty((n, 1, h, w), device=features.device, dtype=torch.float32)
    d2 = torch.empty((n, h, w, fit.K), device=features.device, dtype=torch.float32) if with_d2 else None
    if n * h * w:
        _lib.check(_lib.load().rcu_density_energy(ctypes.c_void_p(nhwc.data_ptr()), pitch, f, n * h * w, fit.K, _lib.ptr(a), _lib.ptr(b), _lib.ptr(k),
                                                  _lib.ptr(out), _lib.ptr(d2), _lib.current_stream()))
    return (out, d2) if with_d2 else out
