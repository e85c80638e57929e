"""EXTENSION -- fit the auxiliary feature network on the device (include/rcu_fit.h "Auxiliary fit"): the reference's
bin-dl/*_train_auxiliary_feat.py as a post-hoc fit on a FROZEN U-Net.  The U-Net runs in eval mode with its feature tap, the target is "the
segmentation's arg-max is wrong here", and the only thing that learns is the PostNet: a per-voxel MLP under cross-entropy with BatchNorm in train
mode.  Its loss and the gradient of every parameter come from one call of the HIP kernels of csrc/rcu_postnet_fit.hip; ``torch.optim.Adam`` makes
the step on the ~3,400 numbers (plumbing).  There is no CPU or autograd fallback."""
import ctypes

import torch

from . import _lib

MAX_CONVS = 4      # RCU_POSTNET_FIT_MAX_CONVS
MAX_FEATURES = 32


def packing(in_channels, nb_convs):
    """[(state_dict name, shape)] in the order of the flat parameter / gradient array (include/rcu_fit.h "Packing")."""
    f = int(in_channels)
    rows = []
    for k in range(int(nb_convs)):
        base = 'convs.{}.conv2d_batch_relu.'.format(k)
        rows += [(base + 'conv.weight', (f, f, 1, 1)), (base + 'conv.bias', (f,)), (base + 'bn.weight', (f,)), (base + 'bn.bias', (f,))]
    return rows + [('conv_logits.weight', (2, f, 1, 1)), ('conv_logits.bias', (2,))]


def _check_postnet(postnet):
    from . import model as model_mod
    if not isinstance(postnet, model_mod.PostNet):
        raise ValueError('the auxiliary fit needs a rcu_amd.model.PostNet, got {}'.format(type(postnet).__name__))
    if postnet._dropouts:
        raise ValueError('the auxiliary fit does not take a PostNet built with dropout (the reference\'s configuration has none); build it with '
                         'dropout=None')
    if postnet.nb_classes != 2:
        raise ValueError('the auxiliary fit is binary (nb_classes = 2: right / wrong), got {}'.format(postnet.nb_classes))
    if not 1 <= postnet.in_channels <= MAX_FEATURES:
        raise ValueError('the auxiliary fit kernels take 1..{} feature channels, got {}'.format(MAX_FEATURES, postnet.in_channels))
    if not 1 <= postnet.nb_convs <= MAX_CONVS:
        raise ValueError('the auxiliary fit kernels take nb_convs in 1..{}, got {}'.format(MAX_CONVS, postnet.nb_convs))


def _ordered_parameters(postnet):
    named = dict(postnet.named_parameters())
    rows = packing(postnet.in_channels, postnet.nb_convs)
    if sorted(named) != sorted(name for name, _ in rows):
        raise ValueError('the PostNet\'s parameters are not those of the packing table')
    return [(name, named[name]) for name, _ in rows]


def _batch_norms(postnet):
    modules = dict(postnet.named_modules())
    return [modules['convs.{}.conv2d_batch_relu.bn'.format(k)] for k in range(postnet.nb_convs)]


def _nhwc(features):
    """The ``[N, F, H, W]`` features -> (tensor that owns the memory, pitch): in place when it is the channels-last view ``UNet.features`` returns
    at a pitch >= 32, else a channels-last copy at pitch 32."""
    if not isinstance(features, torch.Tensor) or features.dim() != 4:
        raise ValueError('expected a [N, F, H, W] feature tensor')
    if not features.is_cuda:
        raise RuntimeError('rcu_amd.auxiliary only runs on the GPU (librcu_hip); got a {} tensor'.format(features.device))
    n, f, h, w = features.shape
    nhwc = features.permute(0, 2, 3, 1)
    pitch = nhwc.stride(2)
    if (features.dtype == torch.float32 and nhwc.stride(3) == 1 and pitch >= 32 and pitch % 4 == 0 and nhwc.stride(1) == w * pitch and
            nhwc.stride(0) == h * w * pitch):
        return nhwc, pitch
    buf = torch.zeros((n, h, w, 32), device=features.device, dtype=torch.float32)
    buf[..., :f] = nhwc
    return buf, 32


def error_target(logits, target):
    """uint8 ``[N, H, W]``: 1 where the first maximum of the eval-mode ``logits`` ``[N, C, H, W]`` differs from ``target > 0``."""
    n, _, h, w = logits.shape
    return (torch.argmax(logits, dim=1) != (target.reshape(n, h, w) > 0).to(torch.int64)).to(torch.uint8)


class _Call:
    """The buffers of rcu_postnet_loss_grad for one PostNet geometry on one device; ``run`` enqueues a call on the current stream."""

    def __init__(self, in_channels, nb_convs, device):
        self.F, self.L, self.device = int(in_channels), int(nb_convs), device
        self.lib = _lib.load()
        self.count = int(self.lib.rcu_postnet_fit_param_count(self.F, self.L))
        if not self.count:
            raise ValueError('the auxiliary fit kernels take 1..{} channels and 1..{} convs'.format(MAX_FEATURES, MAX_CONVS))
        self.params = torch.zeros(self.count, device=device, dtype=torch.float32)
        self.grads = torch.zeros(self.count, device=device, dtype=torch.float32)
        self.mean = torch.zeros((self.L, self.F), device=device, dtype=torch.float32)
        self.var = torch.zeros((self.L, self.F), device=device, dtype=torch.float32)
        self.flags = torch.zeros(1, device=device, dtype=torch.int32)
        self.workspace = None

    def run(self, features, labels, loss_out):
        """``loss_out``: a float64 device tensor whose first element receives the loss.  -> N"""
        nhwc, pitch = _nhwc(features)
        n, f, h, w = features.shape
        if f != self.F:
            raise ValueError('the PostNet takes {} feature channels, the features have {}'.format(self.F, f))
        if not torch.is_tensor(labels) or labels.numel() != n * h * w or labels.is_floating_point():
            raise ValueError('labels must be an integer tensor of {} x {} x {} entries'.format(n, h, w))
        if n * h * w < 2:
            raise ValueError('train-mode BatchNorm needs at least two voxels')
        labels = labels.to(device=features.device, dtype=torch.uint8).reshape(n, h * w).contiguous()
        need = int(self.lib.rcu_postnet_fit_workspace_bytes(self.F, self.L, n, h * w))
        if self.workspace is None or self.workspace.numel() * 8 < need:
            self.workspace = torch.empty((need + 7) // 8, device=features.device, dtype=torch.float64)
        _lib.check(self.lib.rcu_postnet_loss_grad(ctypes.c_void_p(nhwc.data_ptr()), pitch, f, n, h * w, _lib.ptr(labels), self.L,
                                                  _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(loss_out), _lib.ptr(self.mean),
                                                  _lib.ptr(self.var), _lib.ptr(self.flags), _lib.ptr(self.workspace), _lib.current_stream()))
        self._keep = (nhwc, labels)      # the call is asynchronous: its inputs live until the next one
        return n * h * w

    def views(self, flat):
        """name -> the view of ``flat`` that is the tensor of that name."""
        out, at = {}, 0
        for name, shape in packing(self.F, self.L):
            size = 1
            for s in shape:
                size *= s
            out[name] = flat[at:at + size].view(shape)
            at += size
        return out


def _bad_label():
    return ValueError('the auxiliary fit takes labels in {0, 1}: a label >= 2 was seen (include/rcu_fit.h)')


def loss_and_grad(postnet, features, labels):
    """The train-mode cross-entropy of ``postnet`` on the ``[N, F, H, W]`` ``features`` under the uint8 / integer ``labels`` in {0, 1} and its
    gradient: -> (loss float, {state_dict name: float32 gradient tensor}, (batch mean, biased batch variance) float32 ``[nb_convs, F]``).  The
    module is not changed (no running-statistics update); a label >= 2 raises ValueError."""
    _check_postnet(postnet)
    call = _Call(postnet.in_channels, postnet.nb_convs, features.device)
    call.params.copy_(torch.cat([p.detach().to(features.device, torch.float32).reshape(-1) for _, p in _ordered_parameters(postnet)]))
    out = torch.zeros(2, device=features.device, dtype=torch.float64)
    call.run(features, labels, out)
    out[1] = call.flags[0].to(torch.float64)
    loss, flag = out.cpu().tolist()      # the flag comes back with the loss: one read
    if flag:
        raise _bad_label()
    return loss, call.views(call.grads), (call.mean, call.var)


class Fitter:
    """``postnet`` bound to the kernels for a fit: its parameters become views of the flat parameter array, their ``.grad`` views of the gradient
    array, ``torch.optim.Adam(lr)`` steps them.  ``step`` enqueues one optimisation step; ``close`` hands the module back ready for inference."""

    def __init__(self, postnet, lr, device):
        _check_postnet(postnet)
        postnet.to(device)
        self.postnet, self.call = postnet, _Call(postnet.in_channels, postnet.nb_convs, device)
        self.ordered = _ordered_parameters(postnet)
        self.call.params.copy_(torch.cat([p.detach().to(device, torch.float32).reshape(-1) for _, p in self.ordered]))
        p_views, g_views = self.call.views(self.call.params), self.call.views(self.call.grads)
        for name, p in self.ordered:
            p.data = p_views[name]
            p.requires_grad_(True)
            p.grad = g_views[name]
        self.optimizer = torch.optim.Adam([p for _, p in self.ordered], lr=float(lr))
        self.norms = _batch_norms(postnet)

    def step(self, features, labels, loss_out):
        """Loss and gradients of the batch (the loss goes to ``loss_out[0]``, float64 on the device), torch's running-statistics update, one Adam
        step: all enqueued on the current stream.  -> the voxels of the batch."""
        with torch.no_grad():
            n_vox = self.call.run(features, labels, loss_out)
            for k, bn in enumerate(self.norms):
                bn.running_mean.mul_(1 - bn.momentum).add_(self.call.mean[k], alpha=bn.momentum)
                bn.running_var.mul_(1 - bn.momentum).add_(self.call.var[k], alpha=bn.momentum * n_vox / (n_vox - 1))
                bn.num_batches_tracked += 1
        self.optimizer.step()
        return n_vox

    def close(self):
        for _, p in self.ordered:
            p.grad = None
            p.requires_grad_(False)
            p.data = p.data.clone()
        self.postnet.eval()
        self.postnet.weights_changed()


def fit_auxiliary_feat(model, postnet, batches, epochs, lr=1e-4, seed=None, skip_black=True, on_epoch=None):
    """Fit ``postnet`` to predict where the frozen U-Net ``model`` is wrong.  ``batches``: an iterable of ``(images [n, C_in, H, W], target
    [n, H, W])`` that can be walked once per epoch, or a callable that returns one for each epoch.  Per batch: one eval-mode forward of ``model``
    with its feature tap, ``error_target``, one rcu_postnet_loss_grad call, torch's running-statistics update, one ``torch.optim.Adam(lr)``
    step -- all enqueued, no host synchronisation; the losses are read back once per epoch.  ``seed``: re-initialise the PostNet under
    ``torch.manual_seed(seed)`` first (None: start from the weights it has).  ``skip_black`` drops the slices whose images are all zero (the
    reference's none-black selection); host tensors are filtered before the upload, device tensors with one read-back.
    ``on_epoch(epoch, postnet, row)`` is called after every epoch with the module ready for inference.
    -> [{'epoch', 'steps', 'voxels', 'error_fraction', 'mean_loss', 'losses'}] per epoch."""
    from . import density as density_mod
    _check_postnet(postnet)
    density_mod._feature_channels(model)
    if int(model.start_filters) != postnet.in_channels:
        raise ValueError('the U-Net has {} feature channels, the PostNet takes {}'.format(int(model.start_filters), postnet.in_channels))
    epochs = int(epochs)
    if epochs < 1:
        raise ValueError('epochs must be at least 1, got {}'.format(epochs))
    device = next(model.parameters()).device
    if seed is not None:
        torch.manual_seed(int(seed))
        for module in postnet.modules():
            if hasattr(module, 'reset_parameters'):
                module.reset_parameters()
    fitter = Fitter(postnet, lr, device)
    flags = fitter.call.flags
    rows = []
    try:
        with density_mod.eval_features(model):
            for epoch in range(1, epochs + 1):
                losses = torch.zeros(64, device=device, dtype=torch.float64)
                errors = torch.zeros((), device=device, dtype=torch.int64)
                flags.zero_()
                steps = voxels = 0
                for batch in (batches() if callable(batches) else batches):
                    images, target = batch[0], batch[1]
                    if skip_black:
                        keep = images.reshape(images.shape[0], -1).ne(0).any(dim=1)
                        if not bool(keep.all()):
                            images, target = images[keep], target[keep.to(target.device)]
                    if images.shape[0] == 0:
                        continue
                    images = images.float().to(device).contiguous()
                    with torch.no_grad():
                        labels = error_target(model(images), target.to(device))
                        if steps == losses.numel():
                            losses = torch.cat([losses, torch.zeros_like(losses)])
                        errors += labels.sum(dtype=torch.int64)
                    voxels += fitter.step(model.features, labels, losses[steps:])
                    steps += 1
                if not steps:
                    raise ValueError('fit_auxiliary_feat: no batches' + (' (every slice is black)' if skip_black else ''))
                host = torch.cat([losses[:steps], errors.to(torch.float64).reshape(1), flags.to(torch.float64)]).cpu()
                if host[-1]:
                    raise _bad_label()
                row = dict(epoch=epoch, steps=steps, voxels=voxels, error_fraction=float(host[-2]) / voxels, mean_loss=float(host[:steps].mean()),
                           losses=[float(v) for v in host[:steps]])
                rows.append(row)
                postnet.weights_changed()
                if on_epoch is not None:
                    on_epoch(epoch, postnet, row)
    finally:
        fitter.close()
    return rows
