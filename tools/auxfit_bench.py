#!/usr/bin/env python3
"""Time of one step of the auxiliary fit (rcu_postnet_loss_grad, include/rcu_fit.h "Auxiliary fit") on one batch of 32 x 240 x 240 voxels of
F = 32 features at pitch 32, L = 3 hidden convs.

loss_grad   rcu_postnet_loss_grad through the C entry point on preallocated buffers against THE YARDSTICK: loss, backward and BatchNorm update of
            the same module (torch.nn: 3 x [Conv2d 1x1, BatchNorm2d, ReLU] + Conv2d 1x1, CrossEntropyLoss) by torch autograd on the same device
            and the same features (channels-last), which is what the reference runs.  The new path must not be slower; no further ratio is fixed.
unet        the eval-mode U-Net forward with the feature tap on the same batch (bench.py's model): the other half of a fit step; the ratio.
rates       achieved TB/s over the (2 L + 1) x 128 bytes per voxel the passes read, and the fp32 MFMA rate of the passes (16 steps of 32 x 32 x 2
            per layer product and 32 voxels) against the chip's peak -- which of the two roofs is the nearer one.
All paths alternated launch by launch in ONE process, every path warmed up first, each launch between two events on the launch stream, medians.
Prints one JSON line; ``--out`` also writes it.

    python tools/auxfit_bench.py [--reps 15] [--out profiles/auxfit_bench.json]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from density_bench import C, PARAMS, alternated      # noqa: E402  (the same model and timing loop)

SLICES, H, W, F, L = 32, 240, 240, 32, 3
PEAK_TBS = 8.0            # HBM3E peak of the MI355X
MFMA_F32_CLOCK = 64.0     # cycles of a v_mfma_f32_32x32x2_f32 per SIMD
SIMDS, GHZ = 1024, 2.4


def layer_products(L):
    """32 x 32 layer products per 32 voxels over the 2 L + 1 passes: forward chains, the W^T products of the walk down and the gradient products."""
    stats = sum(range(1, L + 1))
    down = sum(L + (L - t) + (1 if t > 1 else 0) + 1 for t in range(1, L + 1))
    return stats + L + down


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    from oracle import unet_oracle as uo
    from rcu_amd import _lib, auxiliary, density
    from rcu_amd.model import PostNet, UNet
    lib = _lib.load()
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(5)
    nhwc = torch.randn(SLICES, H, W, F, device=dev, generator=gen).abs_()
    feats = nhwc.permute(0, 3, 1, 2)      # the channels-last view UNet.features hands out
    labels = (torch.rand(SLICES, H, W, device=dev, generator=gen) < 0.1).to(torch.uint8)
    target = labels.long()

    net = PostNet(F, 2, nb_convs=L)
    call = auxiliary._Call(F, L, dev)
    call.params.copy_(torch.cat([p.detach().reshape(-1) for _, p in auxiliary._ordered_parameters(net)]).to(dev))
    loss = torch.zeros(1, device=dev, dtype=torch.float64)

    layers = []
    for _ in range(L):
        layers += [torch.nn.Conv2d(F, F, 1), torch.nn.BatchNorm2d(F), torch.nn.ReLU(inplace=True)]
    twin = torch.nn.Sequential(*layers, torch.nn.Conv2d(F, 2, 1)).to(dev).to(memory_format=torch.channels_last).train()
    criterion = torch.nn.CrossEntropyLoss()

    def autograd():
        for p in twin.parameters():
            p.grad = None
        criterion(twin(feats), target).backward()

    unet = UNet(**PARAMS)
    unet.load_state_dict(uo.synthetic_state(20, **PARAMS))
    unet = unet.to(dev).eval()
    images = torch.randn(SLICES, C, H, W, device=dev, generator=gen)

    def forward():
        with density.eval_features(unet), torch.no_grad():
            unet(images)

    times = alternated(torch, {'loss_grad': lambda: call.run(feats, labels, loss), 'torch_autograd': autograd, 'unet_forward_features': forward},
                       args.reps)
    voxels = SLICES * H * W
    ms = times['loss_grad']['ms_median']
    read_bytes = (2 * L + 1) * 128 * voxels
    mfma_cycles = layer_products(L) * 16 * MFMA_F32_CLOCK * (voxels / 32) / SIMDS
    rec = {'batch': [SLICES, H, W], 'F': F, 'L': L, 'voxels': voxels, 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
           'librcu': lib.rcu_version().decode(), 'times': times,
           'ratio_loss_grad_over_torch_autograd': round(ms / times['torch_autograd']['ms_median'], 4),
           'not_slower_than_torch_autograd': ms <= times['torch_autograd']['ms_median'],
           'ratio_loss_grad_over_unet_forward': round(ms / times['unet_forward_features']['ms_median'], 4),
           'read_TBs': round(read_bytes / (ms * 1e-3) / 1e12, 4), 'read_fraction_of_peak': round(read_bytes / (ms * 1e-3) / 1e12 / PEAK_TBS, 4),
           'layer_products_per_32_voxels': layer_products(L), 'mfma_ms_at_peak': round(mfma_cycles / (GHZ * 1e6), 4),
           'mfma_fraction_of_peak': round(mfma_cycles / (GHZ * 1e6) / ms, 4)}
    rec['nearer_roof'] = 'mfma' if rec['mfma_fraction_of_peak'] > rec['read_fraction_of_peak'] else 'hbm'      # (near neither: see DESIGN.md)
    line = json.dumps(rec, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
