"""Float64 numpy restatement of PostNet (include/rcu.h "PostNet"): nb_convs x [Conv2d 1x1 -> Dropout2d factor -> BatchNorm2d (eval, NOT
folded) -> ReLU] + Conv2d 1x1, with the error bound the GPU tests assert entry by entry.  Nothing here imports the package or torch's
convolutions: it is the yardstick of csrc/rcu_postnet.hip and of oracle/unet_oracle.py::postnet_forward.

The bound.  The kernel evaluates every layer on FOLDED float32 weights (rcu_postnet_finalize_weights): alpha = fl(gamma / sqrt(var + eps)),
W' = fl(alpha W), and

  eval    a' = relu(W' a + b_all),                     b_all = fl(alpha (b - mean) + beta)
  masked  a' = relu(m (W' a + b_conv) + b_shift),      b_conv = fl(alpha b), b_shift = fl(beta - alpha mean), m = the Dropout2d factor

each output channel as one chain of fused multiply-adds over the C input channels that starts from the constant (the fp32 matrix cores).  With
e_l >= |kernel's a_l - reference's a_l| per entry, e_0 = 0 (both read the same float32 features), ReLU 1-Lipschitz and m >= 0:

  eval    e_{l+1} = |W'| e_l + g (|W'| |a_l| + |b_all|)
  masked  e_{l+1} = m (|W'| e_l + g (|W'| |a_l| + |b_conv|)) + g |b_shift|

(the mask factor multiplies both terms; what is added behind it has its own, unmultiplied, term), the last conv as a layer without ReLU, and

  g = (C + 3) 2^-24:  C roundings of the fma chain of length C (padding channels add exact zeros), 2 of the fold (alpha's own rounding and
      the product alpha W, both relative to |W'|), 1 of the mask's fmaf (eval mode does not spend it).

|a_l| is the reference's activation, so the bound is first order in 2^-24, as such bounds are.  The roundings inside the folded constants are
relative to the constants' parts and are covered by the same g wherever b_all does not cancel to less than a tenth of its parts; the float32
oracle is held to the same bound on every case without a device (tests/test_capped_launches_cpu.py)."""
import numpy as np

BN_EPS = 1e-5
U = 2.0 ** -24    # unit roundoff of float32
K_EXTRA = 3       # the fold's two roundings and the mask's fmaf


def gamma(channels):
    return (channels + K_EXTRA) * U


def _np(state, key, dtype=np.float64):
    v = state[key]
    return (v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)).astype(dtype)


def folded(state, layer, channels, bn=True):
    """(W', b_all, b_conv, b_shift) of hidden conv ``layer`` in float32, operation by operation as rcu_postnet_finalize_weights folds them."""
    pre = 'convs.{}.conv2d_batch_relu'.format(layer)
    w = _np(state, pre + '.conv.weight', np.float32).reshape(channels, channels)
    b = _np(state, pre + '.conv.bias', np.float32)
    if bn:
        alpha = (_np(state, pre + '.bn.weight') / np.sqrt(_np(state, pre + '.bn.running_var') + BN_EPS)).astype(np.float32)
        beta, mean = _np(state, pre + '.bn.bias', np.float32), _np(state, pre + '.bn.running_mean', np.float32)
    else:
        alpha, beta, mean = np.ones(channels, np.float32), np.zeros(channels, np.float32), np.zeros(channels, np.float32)
    return alpha[:, None] * w, alpha * (b - mean) + beta, alpha * b, beta - alpha * mean


def forward(state, x, nb_convs=3, masks=None, bn=True):
    """x [n, C, h, w] float32, masks None or nb_convs arrays [n, C] -> (logits, bound), both float64 [n, classes, h, w]."""
    x = np.asarray(x, dtype=np.float32)
    n, c, h, w = x.shape
    g = gamma(c)
    a = np.ascontiguousarray(x.transpose(0, 2, 3, 1)).reshape(n, h * w, c).astype(np.float64)
    e = np.zeros_like(a)
    for l in range(nb_convs):
        pre = 'convs.{}.conv2d_batch_relu'.format(l)
        wt = _np(state, pre + '.conv.weight').reshape(c, c)
        y = a @ wt.T + _np(state, pre + '.conv.bias')
        wf, b_all, b_conv, b_shift = (np.abs(v.astype(np.float64)) for v in folded(state, l, c, bn))
        if masks is not None:
            m = np.asarray(masks[l], dtype=np.float32).astype(np.float64).reshape(n, 1, c)
            assert (m >= 0).all()
            y = y * m
            e = m * (e @ wf.T + g * (np.abs(a) @ wf.T + b_conv)) + g * b_shift
        else:
            e = e @ wf.T + g * (np.abs(a) @ wf.T + b_all)
        if bn:
            y = (y - _np(state, pre + '.bn.running_mean')) / np.sqrt(_np(state, pre + '.bn.running_var') + BN_EPS) \
                * _np(state, pre + '.bn.weight') + _np(state, pre + '.bn.bias')
        a = np.maximum(y, 0.0)
    wl = _np(state, 'conv_logits.weight')
    classes = wl.shape[0]
    wl = wl.reshape(classes, c)
    bl = _np(state, 'conv_logits.bias')
    wa = np.abs(wl.astype(np.float32).astype(np.float64))
    logits = a @ wl.T + bl
    e = e @ wa.T + g * (np.abs(a) @ wa.T + np.abs(bl))

    def nchw(t):
        return np.ascontiguousarray(t.reshape(n, h, w, classes).transpose(0, 3, 1, 2))
    return nchw(logits), nchw(e)


def fraction_used(got, logits, bound):
    """The largest |got - logits| / bound; where the bound is zero the entry must be exact (-> inf otherwise)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - logits)
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(frac.max())


def draw_masks(n, channels, nb_convs, p, generator):
    """Dropout2d factors per image and hidden conv, drawn as oracle.unet_oracle.sample_masks draws them: a list of nb_convs float32 [n, C]."""
    import torch
    keep = 1.0 - p
    return [((torch.rand(n, channels, generator=generator) < keep).float() / keep).numpy() for _ in range(nb_convs)]


def features(n, channels, h, w, seed):
    import torch
    return torch.randn(n, channels, h, w, generator=torch.Generator().manual_seed(seed)).numpy()


# ---------------------------------------------------------------------------------------------- the cases of tests/test_gpu_postnet.py
SEAM_SHAPES = ((3, 5, 7), (2, 9, 14))       # hw = 35: every wave of 32 voxels holds two or three images; hw = 126
SEAM_CHANNELS = (32, 40, 48, 64, 96)
SEAM_CLASSES = (1, 2, 3, 32)
SEAM_CONVS = (0, 1, 3)


def seam_masks(n, channels, nb_convs, seed):
    """p = 0.3 draws with an all-zero row (what p = 1 gives: image 0 at the first conv), an all-ones row and, from two convs on, an all-ones site."""
    import torch
    masks = draw_masks(n, channels, nb_convs, 0.3, torch.Generator().manual_seed(seed))
    masks[0][0] = 0.0
    masks[-1][-1] = 1.0
    if nb_convs > 1:
        masks[1][:] = 1.0
    return masks


def seam_case(shape, channels, classes, nb_convs):
    """(state, x [n, C, h, w] float32, masks or None when there is no hidden conv) of one small case; seeded by the case alone."""
    from oracle import unet_oracle as uo
    n, h, w = shape
    seed = 1000 * channels + 10 * classes + nb_convs + h
    state = uo.postnet_synthetic_state(seed, channels, classes, nb_convs)
    x = features(n, channels, h, w, seed + 1)
    return state, x, (seam_masks(n, channels, nb_convs, seed + 2) if nb_convs else None)
