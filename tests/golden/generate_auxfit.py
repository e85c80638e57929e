#!/usr/bin/env python3
"""Fixture G36 (tests/golden/g36_auxfit.npz): what the REFERENCE's own modules give for one batch of the auxiliary fit -- its PostNet
(common/model/postnet.py) in train mode, nn.CrossEntropyLoss and torch.optim.Adam(1e-4), as bin-dl/*_train_auxiliary_feat.py uses them -- in
float64 on the CPU, and the same module in float32.  Run where the reference is (see generate_golden.py):

    python tests/golden/generate_auxfit.py

Contents: the inputs (phi [N, F] with a dead last channel, labels, the initial state_dict as ``sd0::``); of the first step in float64 the loss,
the gradients ``g64::``, the batch statistics mu / var [L, F] and the condition sums ``cond::`` (sum_v |du_i| |a_j| with du the gradient autograd
leaves at the conv outputs and a the conv inputs; bias: sum |du|; bn.bias / bn.weight: sum |dy|, sum |dy| |xhat|); the float32 run's gradients
``g32::``; the float64 state_dict after three Adam steps ``sd3::`` (running statistics and num_batches_tracked included) and the three losses."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import generate_golden as gg  # noqa: E402
import auxfit_cases as cases  # noqa: E402

N_SLICES, H, W, F, L, STEPS, LR = 2, 15, 20, 32, 3, 3, 1e-4


def build(dtype, params):
    from common.model.postnet import PostNet
    net = PostNet(F, 2, nb_convs=L).to(dtype)
    state = net.state_dict()
    for name, value in params.items():
        state[name] = torch.from_numpy(value.reshape(tuple(state[name].shape))).to(dtype)
    net.load_state_dict(state)
    return net.train()


def run(dtype, phi, labels, params, steps):
    net = build(dtype, params)
    x = torch.from_numpy(phi).to(dtype).reshape(N_SLICES, H, W, F).permute(0, 3, 1, 2).contiguous()
    target = torch.from_numpy(labels.astype(np.int64)).reshape(N_SLICES, H, W)
    optimizer = torch.optim.Adam(net.parameters(), lr=LR)
    criterion = nn.CrossEntropyLoss()
    taps = {}

    def tap(kind, k):
        def hook(module, inputs, output):
            if kind == 'conv':
                output.retain_grad()
                taps['a', k], taps['u', k] = inputs[0].detach(), output
            else:
                output.retain_grad()
                taps['y', k] = output
        return hook

    handles = []
    for k in range(L):
        unit = net.convs[k].conv2d_batch_relu
        handles += [unit.conv.register_forward_hook(tap('conv', k)), unit.bn.register_forward_hook(tap('bn', k))]

    def tap_logits(module, inputs, output):
        output.retain_grad()
        taps['a', L], taps['z', 0] = inputs[0].detach(), output

    final = net.conv_logits.register_forward_hook(tap_logits)
    first, losses = None, []
    for step in range(steps):
        optimizer.zero_grad()
        loss = criterion(net(x), target)
        loss.backward()
        losses.append(float(loss.detach()))
        if step == 0:
            flat = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double().numpy()      # noqa: E731
            first = dict(loss=float(loss), grads={name: p.grad.detach().clone().numpy() for name, p in net.named_parameters()}, cond={})
            mu, var = [], []
            for k in range(L):
                base = 'convs.{}.conv2d_batch_relu.'.format(k)
                u, a, du = flat(taps['u', k]), flat(taps['a', k]), flat(taps['u', k].grad)
                # ReLU(inplace) rewrote BatchNorm's output, so the gradient retained on it may be that of a; masked by a > 0 it is dy either way
                dy = np.where(flat(taps['a', k + 1]) > 0, flat(taps['y', k].grad), 0.0)
                m, v = u.mean(0), ((u - u.mean(0)) ** 2).mean(0)
                xhat = (u - m) / np.sqrt(v + 1e-5)
                mu.append(m), var.append(v)
                first['cond'][base + 'conv.weight'] = np.abs(du).T @ np.abs(a)
                first['cond'][base + 'conv.bias'] = np.abs(du).sum(0)
                first['cond'][base + 'bn.weight'] = (np.abs(dy) * np.abs(xhat)).sum(0)
                first['cond'][base + 'bn.bias'] = np.abs(dy).sum(0)
            dz, a_last = flat(taps['z', 0].grad), flat(taps['a', L])
            first['cond']['conv_logits.weight'] = np.abs(dz).T @ np.abs(a_last)
            first['cond']['conv_logits.bias'] = np.abs(dz).sum(0)
            first['mu'], first['var'] = np.stack(mu), np.stack(var)
            for h in handles + [final]:
                h.remove()
        optimizer.step()
    return first, losses, {k: v.detach().numpy() for k, v in net.state_dict().items()}


def main():
    gg.install_reference()
    torch.manual_seed(36)
    phi, labels, params, _ = cases.make_inputs(36, N_SLICES, H * W, F, L, zero_channel=F - 1)
    first64, losses, final = run(torch.float64, phi, labels, params, STEPS)
    first32, _, _ = run(torch.float32, phi, labels, params, 1)
    assert all(np.isfinite(v).all() for v in first64['grads'].values()) and all(np.isfinite(v).all() for v in first32['grads'].values())
    initial = {k: v.detach().numpy() for k, v in build(torch.float32, params).state_dict().items()}
    arrays = dict(phi=phi, labels=labels, shape=np.array([N_SLICES, H, W, F, L, STEPS]), lr=np.float64(LR), loss=np.float64(first64['loss']),
                  losses=np.array(losses), mu=first64['mu'], var=first64['var'])
    arrays.update({'sd0::' + k: v for k, v in initial.items()})
    arrays.update({'g64::' + k: v for k, v in first64['grads'].items()})
    arrays.update({'g32::' + k: v for k, v in first32['grads'].items()})
    arrays.update({'cond::' + k: v for k, v in first64['cond'].items()})
    arrays.update({'sd3::' + k: v for k, v in final.items()})
    gg.save('g36_auxfit', **arrays)


if __name__ == '__main__':
    main()
