"""Synthetic inputs of the auxiliary-fit tests (include/rcu_fit.h) and the raw call of rcu_postnet_loss_grad on device buffers the test lays out
itself: any channel pitch, garbage in the padding channels, every pointer one element off its allocation, any stream."""
import ctypes

import numpy as np

import auxfit_reference as ref


def make_inputs(seed, n, hw, F, L, zero_channel=None, all_zero_labels=False):
    """-> (phi, labels, params, expected): float32 phi [n * hw, F] -- continuous features, every voxel its own draw, nothing rejected: per channel a
    normal distribution of width 0.5 .. 1.5 about a mean that is far from zero in every third channel (|mu| up to tens of sigma: what the variance
    and the first layer's products have to survive), a quarter of the channels non-negative -- uint8 labels correlated with phi, a PostNet's raw
    parameters (torch's default initialisation ranges, some negative BatchNorm weights) as float32 arrays by state_dict name, and the float64
    reference of that batch.  A function of the arguments alone."""
    N = n * hw
    rng = np.random.default_rng([seed, N, F, L])
    offsets = rng.standard_normal(F) * np.where(np.arange(F) % 3 == 0, 30.0, 1.0)
    phi = (rng.standard_normal((N, F)) * (0.5 + rng.random(F)) + offsets).astype(np.float32)
    phi[:, ::4] = np.abs(phi[:, ::4])
    if zero_channel is not None:
        phi[:, zero_channel] = 0.0
    score = phi[:, 1] - phi[:, 1].mean() + rng.standard_normal(N)
    labels = np.zeros(N, np.uint8) if all_zero_labels else (score > 0.7).astype(np.uint8)
    params = {}
    bound = 1.0 / np.sqrt(F)
    for name, shape in ref.packing(F, L):
        if name.endswith('bn.weight'):
            value = 0.5 + rng.random(shape)
            value[::5] *= -1.0
        elif name.endswith('bn.bias'):
            value = 0.2 * rng.standard_normal(shape)
        else:
            value = rng.uniform(-bound, bound, shape)
        params[name] = value.astype(np.float32)
    return phi, labels, params, ref.loss_and_grad(phi, labels, params, L)


def device_call(phi, labels, flat_params, n, hw, F, L, pitch=32, off=0, garbage=True, stream=None, poison=float('nan')):
    """rcu_postnet_loss_grad on cuda:0 -> dict(loss float, grads, mean, var float32 numpy, flag int).  ``off``: 0 or 1, every buffer starts that
    many elements into its allocation.  The padding channels hold NaN when ``garbage``; the outputs are poisoned before the call."""
    import torch
    from rcu_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda')
    N = n * hw
    count = ref.param_count(F, L)

    def alloc(numel, dtype, fill):
        whole = torch.full((numel + off,), fill, device=dev, dtype=dtype)
        return whole, whole[off:]

    keep = []
    xw, x = alloc(N * pitch, torch.float32, float('nan') if garbage else 0.0)
    x.view(N, pitch)[:, :F] = torch.from_numpy(np.ascontiguousarray(phi)).to(dev)
    lw, lab = alloc(N, torch.uint8, 0)
    lab.copy_(torch.from_numpy(np.ascontiguousarray(labels)).to(dev))
    pw, par = alloc(count, torch.float32, 0.0)
    par.copy_(torch.from_numpy(np.ascontiguousarray(flat_params, dtype=np.float32)).to(dev))
    gw, grads = alloc(count, torch.float32, poison)
    ow, loss = alloc(1, torch.float64, poison)
    mw, mean = alloc(L * F, torch.float32, poison)
    vw, var = alloc(L * F, torch.float32, poison)
    fw, flag = alloc(1, torch.int32, 0)
    nbytes = int(lib.rcu_postnet_fit_workspace_bytes(F, L, n, hw))
    assert nbytes > 0
    ww, ws = alloc((nbytes + 7) // 8, torch.float64, poison)
    keep += [xw, lw, pw, gw, ow, mw, vw, fw, ww]
    handle = ctypes.c_void_p(stream.cuda_stream) if stream is not None else _lib.current_stream()
    _lib.check(lib.rcu_postnet_loss_grad(_lib.ptr(x), pitch, F, n, hw, _lib.ptr(lab), L, _lib.ptr(par), _lib.ptr(grads), _lib.ptr(loss), _lib.ptr(mean),
                                         _lib.ptr(var), _lib.ptr(flag), _lib.ptr(ws), handle))
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    return dict(loss=float(loss.cpu()[0]), grads=grads.cpu().numpy(), mean=mean.cpu().numpy().reshape(L, F), var=var.cpu().numpy().reshape(L, F),
                flag=int(flag.cpu()[0]))
