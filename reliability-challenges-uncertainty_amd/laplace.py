"""EXTENSION -- last-layer Laplace uncertainty (include/rcu.h "Last-layer Laplace"; Daxberger et al. 2021, Laplace Redux; MacKay 1992 for the
probit predictive).  A Gaussian posterior over the weights of the 1x1 classifier conv_cls.1 alone, centred on the trained weights, its precision the
generalised Gauss-Newton matrix of the cross-entropy plus an isotropic prior: no retraining, any trained checkpoint, one eval-mode pass.  Unlike
the feature-space density it changes the probabilities themselves.  The two hot paths are HIP kernels (csrc/rcu_laplace.hip):
``hessian_moments`` -- per-slice curvature-weighted sums, sums of features and Gram matrices -- and ``predict`` -- the per-voxel logit variances,
the probit-corrected softmax and the prediction in one read of the features.  The fit between them is host arithmetic in float64 with exactly
rounded sums, so it cannot depend on batching or slice order.  Voxels of one image are not independent observations: ``hessian_scale`` tempers the
curvature and is the user's to choose."""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from .density import _fsum_over_slices, _inverse_lower, _nhwc

MAX_FEATURES = 64
MIN_CLASSES, MAX_CLASSES = 2, 4      # RCU_LAPLACE_MAX_CLASSES
EVIDENCE = 'evidence'
EVIDENCE_GRID = tuple(2.0 ** (k / 4.0) for k in range(-80, 81))


def check_classes(nb_classes):
    c = int(nb_classes)
    if not MIN_CLASSES <= c <= MAX_CLASSES:
        raise ValueError('the last-layer Laplace takes {}..{} classes, got {}'.format(MIN_CLASSES, MAX_CLASSES, nb_classes))
    return c


def pairs(nb_classes):
    """The class pairs (c, c'), c <= c', in the row-major order of include/rcu.h."""
    c = check_classes(nb_classes)
    return [(a, b) for a in range(c) for b in range(a, c)]


def _nchw(name, t, like):
    n, _, h, w = like.shape
    if not torch.is_tensor(t) or t.dim() != 4 or t.shape[0] != n or tuple(t.shape[2:]) != (h, w) or t.device != like.device:
        raise ValueError('{} must be a [N, C, H, W] tensor of the features\' N, H, W and device'.format(name))
    check_classes(t.shape[1])
    return t.to(torch.float32).contiguous()


def hessian_moments(head_features, probabilities):
    """Per slice and class pair (``pairs``): ``w`` = sum omega float64 ``[N, P]``, ``S`` = sum omega psi ``[N, P, F]``, ``G`` = sum omega psi psi^T
    ``[N, P, F, F]`` (both triangles, bitwise symmetric) of the ``[N, F, H, W]`` classifier input ``UNet.head_features`` under the float32 softmax
    ``probabilities`` ``[N, C, H, W]``, on the device.  The rows of a slice are bit for bit a function of that slice alone."""
    nhwc, pitch = _nhwc(head_features)
    n, f, h, w = head_features.shape
    probabilities = _nchw('probabilities', probabilities, head_features)
    c = probabilities.shape[1]
    p = len(pairs(c))
    dev = head_features.device
    w_out = torch.empty((n, p), device=dev, dtype=torch.float64)
    s_out = torch.empty((n, p, f), device=dev, dtype=torch.float64)
    g_out = torch.empty((n, p, f, f), device=dev, dtype=torch.float64)
    if n * h * w == 0:
        raise ValueError('hessian_moments: an empty batch')
    lib = _lib.load()
    ws = torch.empty(max(int(lib.rcu_laplace_moments_workspace_bytes(n, h * w, f, c)), 16) // 8, device=dev, dtype=torch.float64)
    _lib.check(lib.rcu_laplace_moments(ctypes.c_void_p(nhwc.data_ptr()), pitch, f, _lib.ptr(probabilities), n, h * w, c, _lib.ptr(w_out),
                                       _lib.ptr(s_out), _lib.ptr(g_out), _lib.ptr(ws), _lib.current_stream()))
    return w_out, s_out, g_out


class LaplaceFit:
    """The last-layer posterior: ``C`` classes, ``F`` features, D = F + 1.  ``H`` ``[C D, C D]`` the summed GGN (before ``hessian_scale``),
    ``Sigma`` = (hessian_scale H + tau I)^-1, per class ``A`` ``[C, F, F]`` (upper triangular), ``b`` ``[C, F]``, ``kappa`` ``[C]`` with
    s2_c = |A_c psi - b_c|^2 + kappa_c (float64 all); the scalars ``tau``, ``hessian_scale``, ``temperature`` (the model's when it was fitted)
    and the ``voxels`` the fit saw."""

    def __init__(self, H, Sigma, A, b, kappa, tau, hessian_scale, temperature, voxels):
        self.H, self.Sigma, self.A, self.b, self.kappa = (np.ascontiguousarray(v, dtype=np.float64) for v in (H, Sigma, A, b, kappa))
        if self.A.ndim != 3 or self.A.shape[1] != self.A.shape[2]:
            raise ValueError('LaplaceFit: A must be [C, F, F]')
        self.C, self.F = (int(v) for v in self.A.shape[:2])
        check_classes(self.C)
        full = self.C * (self.F + 1)
        if not 1 <= self.F <= MAX_FEATURES or self.H.shape != (full, full) or self.Sigma.shape != (full, full) or \
                self.b.shape != (self.C, self.F) or self.kappa.shape != (self.C,):
            raise ValueError('LaplaceFit: the arrays do not have the shapes of C = {} classes, F = {} features'.format(self.C, self.F))
        self.tau, self.hessian_scale, self.temperature, self.voxels = float(tau), float(hessian_scale), float(temperature), int(voxels)
        self._device = {}

    def as_dict(self):
        return {'F': self.F, 'C': self.C, 'tau': self.tau, 'hessian_scale': self.hessian_scale, 'temperature': self.temperature,
                'voxels': self.voxels}

    def float32_parameters(self):
        """(A, b, kappa) rounded once to float32: what the device evaluates, and what a reference has to evaluate in float64."""
        return self.A.astype(np.float32), self.b.astype(np.float32), self.kappa.astype(np.float32)

    def device_parameters(self, device):
        """The float32 parameters on ``device``, uploaded once."""
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(v).to(device).contiguous() for v in self.float32_parameters())
        return self._device[key]


def assemble_hessian(w, S, G):
    """Summed moments ``w [P]``, ``S [P, F]``, ``G [P, F, F]`` -> H ``[C D, C D]``: block (c, c') is M_q = [[G_q, S_q], [S_q^T, w_q]]."""
    P, F = S.shape
    C = next((c for c in range(MIN_CLASSES, MAX_CLASSES + 1) if c * (c + 1) // 2 == P), None)
    if C is None:
        raise ValueError('the moments have {} pairs: not C (C + 1) / 2 for C in {}..{}'.format(P, MIN_CLASSES, MAX_CLASSES))
    D = F + 1
    H = np.zeros((C * D, C * D))
    for q, (c, d) in enumerate(pairs(C)):
        M = np.empty((D, D))
        M[:F, :F], M[:F, F], M[F, :F], M[F, F] = G[q], S[q], S[q], w[q]
        H[c * D:(c + 1) * D, d * D:(d + 1) * D] = M
        H[d * D:(d + 1) * D, c * D:(c + 1) * D] = M.T
    return H


def evidence_objective(eigenvalues, theta_sq, n_params, tau):
    """The tau-dependent part of the Laplace log evidence (include/rcu.h)."""
    return -0.5 * tau * theta_sq + 0.5 * n_params * math.log(tau) - 0.5 * float(np.log(np.maximum(eigenvalues, 0.0) + tau).sum())


def _prior_precision(value):
    if isinstance(value, str):
        if value != EVIDENCE:
            raise ValueError('prior_precision must be a number > 0 or {!r}, got {!r}'.format(EVIDENCE, value))
        return value
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or value <= 0:
        raise ValueError('prior_precision must be a number > 0 or {!r}, got {!r}'.format(EVIDENCE, value))
    return float(value)


def _positive(name, value):
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or value <= 0:
        raise ValueError('{} must be a finite number > 0, got {!r}'.format(name, value))
    return float(value)


def fit_from_moments(w, S, G, theta, hessian_scale=1.0, prior_precision=1.0, temperature=1.0, voxels=0):
    """The fit of include/rcu.h from per-slice moments ``w [slices, P]``, ``S [slices, P, F]``, ``G [slices, P, F, F]`` (numpy or tensors) and
    ``theta`` ``[C, F + 1]``, the classifier as the model applies it (class-major: F weights, then the bias): exactly rounded sums over the slices,
    then float64.  ``prior_precision``: a number > 0 or ``'evidence'``.  -> LaplaceFit."""
    w, S, G = (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64) for v in (w, S, G))
    if w.ndim != 2 or S.ndim != 3 or G.ndim != 4 or S.shape[:2] != w.shape or G.shape != S.shape + S.shape[2:] or w.shape[0] < 1:
        raise ValueError('fit_from_moments: expected w [slices, P], S [slices, P, F], G [slices, P, F, F]')
    scale = _positive('hessian_scale', hessian_scale)
    prior = _prior_precision(prior_precision)
    temperature = _positive('temperature', temperature)
    H = assemble_hessian(_fsum_over_slices(w), _fsum_over_slices(S), _fsum_over_slices(G))
    F = S.shape[2]
    D = F + 1
    C = H.shape[0] // D
    theta = np.asarray(theta, dtype=np.float64)
    if theta.shape != (C, D):
        raise ValueError('theta must be [C, F + 1] = [{}, {}], got {}'.format(C, D, list(theta.shape)))
    if not np.isfinite(H).all():
        raise ValueError('the moments are not finite')
    H_eff = scale * H
    if prior == EVIDENCE:
        lam = np.linalg.eigvalsh(H_eff)
        theta_sq = float((theta * theta).sum())
        scores = [evidence_objective(lam, theta_sq, C * D, t) for t in EVIDENCE_GRID]
        tau = EVIDENCE_GRID[int(np.argmax(scores))]      # the first maximiser
    else:
        tau = prior
    try:
        Linv = _inverse_lower(np.linalg.cholesky(H_eff + tau * np.eye(C * D)))
    except np.linalg.LinAlgError:
        raise ValueError('hessian_scale * H + tau I is not positive definite (tau = {!r})'.format(tau)) from None
    Sigma = Linv.T @ Linv
    Sigma = 0.5 * (Sigma + Sigma.T)
    A, b, kappa = np.zeros((C, F, F)), np.zeros((C, F)), np.zeros(C)
    for c in range(C):
        try:
            LT = np.linalg.cholesky(Sigma[c * D:(c + 1) * D, c * D:(c + 1) * D]).T
        except np.linalg.LinAlgError:
            raise ValueError('class {}: the posterior covariance block is not positive definite in float64 (tau = {!r}); a larger '
                             'prior_precision conditions it'.format(c, tau)) from None
        A[c], b[c], kappa[c] = LT[:F, :F], -LT[:F, F], LT[F, F] ** 2
    return LaplaceFit(H, Sigma, A, b, kappa, tau, scale, temperature, voxels)


def check_model(model, fit=None):
    """The refusals of include/rcu.h for ``model`` (and ``fit``), each a ValueError that names the cause.  -> (F, C)."""
    from . import model as model_mod
    if not isinstance(model, model_mod.UNet):
        raise ValueError('the last-layer Laplace needs a rcu_amd.model.UNet (its classifier tap), got {}'.format(type(model).__name__))
    if model.sigma_out:
        raise ValueError('the last-layer Laplace is not defined for a sigma_out model (a second head shares the features)')
    c = check_classes(model.nb_classes)
    f = int(model.start_filters)
    if not 1 <= f <= MAX_FEATURES:
        raise ValueError('the Laplace kernels take 1..{} features, the model has start_filters = {}'.format(MAX_FEATURES, f))
    if fit is not None:
        if (fit.F, fit.C) != (f, c):
            raise ValueError('the Laplace fit has F = {}, C = {}; the model has start_filters = {}, nb_classes = {}'.format(fit.F, fit.C, f, c))
        if fit.temperature != float(model.temperature):
            raise ValueError('the Laplace fit was made at temperature {!r}, the model runs at {!r}: the curvature is that of other '
                             'probabilities'.format(fit.temperature, float(model.temperature)))
    return f, c


def classifier_parameters(model):
    """theta* ``[C, F + 1]`` float64: conv_cls.1's weights and bias divided by the model's temperature, as the model applies them."""
    f, c = check_model(model)
    state = model.state_dict()
    weight = state['conv_cls.1.weight'].detach().cpu().numpy().astype(np.float64).reshape(c, f)
    bias = state['conv_cls.1.bias'].detach().cpu().numpy().astype(np.float64).reshape(c, 1)
    return np.concatenate([weight, bias], axis=1) / float(model.temperature)


class eval_head_features:
    """Context: ``model`` in eval mode (no dropout site active) with ``provide_head_features`` set; the flag is restored on the way out."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        from . import steps
        self.before = self.model.provide_head_features
        steps.set_dropout_mode(self.model, False)
        self.model.provide_head_features = True
        return self.model

    def __exit__(self, *exc):
        self.model.provide_head_features = self.before
        return False


def fit_laplace(model, batches, hessian_scale=1.0, prior_precision=1.0):
    """Fit on ``batches``: an iterable of image tensors ``[n, C_in, H, W]`` (or tuples / lists whose first entry is one; no labels are needed --
    the GGN of the cross-entropy does not depend on them).  One eval-mode forward per batch with the classifier tap; per-slice moments are kept
    and combined at the end with exactly rounded sums -- the same slices in other batches or another order give the same bits.  -> LaplaceFit."""
    from . import steps
    check_model(model)
    _positive('hessian_scale', hessian_scale)
    _prior_precision(prior_precision)
    rows, voxels = [], 0
    with eval_head_features(model):
        for batch in batches:
            images = batch[0] if isinstance(batch, (tuple, list)) else batch
            logits = model(images)
            w, s, g = hessian_moments(model.head_features, steps.softmax(logits))
            rows.append((w.cpu().numpy(), s.cpu().numpy(), g.cpu().numpy()))
            voxels += logits.shape[0] * logits.shape[2] * logits.shape[3]
    if not rows:
        raise ValueError('fit_laplace: no batches')
    return fit_from_moments(*(np.concatenate([r[i] for r in rows]) for i in range(3)), theta=classifier_parameters(model),
                            hessian_scale=hessian_scale, prior_precision=prior_precision, temperature=float(model.temperature), voxels=voxels)


_ARRAYS = ('H', 'Sigma', 'A', 'b', 'kappa')
_SCALARS = ('tau', 'hessian_scale', 'temperature', 'voxels')


def save_laplace(fit, path):
    """``fit`` -> an .npz of its float64 arrays and its scalars."""
    with open(os.fspath(path), 'wb') as f:
        np.savez(f, tau=np.float64(fit.tau), hessian_scale=np.float64(fit.hessian_scale), temperature=np.float64(fit.temperature),
                 voxels=np.int64(fit.voxels), **{name: getattr(fit, name) for name in _ARRAYS})


def load_laplace(path):
    """The LaplaceFit ``save_laplace`` wrote; anything else raises ValueError."""
    path = os.fspath(path)
    try:
        with np.load(path, allow_pickle=False) as doc:
            missing = [name for name in _ARRAYS + _SCALARS if name not in doc.files]
            if missing:
                raise ValueError('no {} array'.format(', '.join(missing)))
            return LaplaceFit(*(doc[name] for name in _ARRAYS), tau=float(doc['tau']), hessian_scale=float(doc['hessian_scale']),
                              temperature=float(doc['temperature']), voxels=int(doc['voxels']))
    except (OSError, ValueError) as e:
        raise ValueError('Laplace file {!r} cannot be read: {}'.format(path, e)) from None


def predict(fit, head_features, logits, std=True, std_pred=True, prediction=True):
    """The probit predictive of ``fit`` for the ``[N, F, H, W]`` classifier input and the ``[N, C, H, W]`` logits of one forward, in one read of
    the features -> dict: ``probabilities`` float32 ``[N, C, H, W]``; ``std`` ``[N, C, H, W]``, the standard deviation of every logit;
    ``prediction`` uint8 ``[N, H, W]``, the first maximum of the probabilities; ``std_pred`` ``[N, 1, H, W]``, the std of that class.  The three
    optional outputs can be switched off; that changes no bit of the others.  A voxel's outputs depend on its features, its logits and the
    parameters alone."""
    nhwc, pitch = _nhwc(head_features)
    n, f, h, w = head_features.shape
    logits = _nchw('logits', logits, head_features)
    c = logits.shape[1]
    if (f, c) != (fit.F, fit.C):
        raise ValueError('the fit has F = {}, C = {}; the features have {} channels, the logits {} classes'.format(fit.F, fit.C, f, c))
    a, b, kappa = fit.device_parameters(head_features.device)
    dev = head_features.device
    out = {'probabilities': torch.empty_like(logits)}
    if std:
        out['std'] = torch.empty_like(logits)
    if std_pred:
        out['std_pred'] = torch.empty((n, 1, h, w), device=dev, dtype=torch.float32)
    if prediction:
        out['prediction'] = torch.empty((n, h, w), device=dev, dtype=torch.uint8)
    if n * h * w:
        _lib.check(_lib.load().rcu_laplace_predict(ctypes.c_void_p(nhwc.data_ptr()), pitch, f, _lib.ptr(logits), n, h * w, c, _lib.ptr(a),
                                                   _lib.ptr(b), _lib.ptr(kappa), _lib.ptr(out['probabilities']), _lib.ptr(out.get('std')),
                                                   _lib.ptr(out.get('std_pred')), _lib.ptr(out.get('prediction')), _lib.current_stream()))
    return out
