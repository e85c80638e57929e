#!/usr/bin/env python3
"""Per-layer gate of the 25-product up-convolutions (csrc/rcu_wino4_up.hip): the BraTS-shaped forward of tools/layer_report.py under
upconv_winograd4=0 and =2 in ONE process, old - new - old per plan size, HIP events between the kernels.

    python tools/upconv4_gate.py [forwards per leg, default 10] [samples per launch ..., default 640 480 320 160]

A layer passes at a plan size where the new kernel is faster by more than the spread between the two legs of the old one."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402


def leg(model, x, n, reps):
    for _ in range(2):
        model(x)
    model.profile_begin(bench.HEIGHT, bench.WIDTH, n, reps)
    for _ in range(reps):
        model(x)
    torch.cuda.synchronize()
    cnt, ms = model.profile_collect(bench.HEIGHT, bench.WIDTH, n)
    layers = model.layer_table(bench.HEIGHT, bench.WIDTH, n)
    return layers, [t / cnt for t in ms[1:1 + len(layers)]]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    sizes = [int(v) for v in sys.argv[2:]] or [640, 480, 320, 160]
    dev = torch.device('cuda')
    from rcu_amd import steps
    volume = bench.make_volume(20)[0]
    for n in sizes:
        models = {}
        for mode in (0, 2):
            m = bench.make_model(20, dev)
            m.plan_options = dict(upconv_winograd4=mode)
            steps.set_dropout_mode(m, True)
            models[mode] = m
        x = volume.repeat((n + volume.shape[0] - 1) // volume.shape[0], 1, 1, 1)[:n].to(dev)
        old1 = leg(models[0], x, n, reps)
        new = leg(models[2], x, n, reps)
        old2 = leg(models[0], x, n, reps)
        print('{} samples per launch, {} forwards per leg'.format(n, reps))
        print('{:<24} {:>4}->{:<4} {:>3}x{:<3} {:<36} {:>8} {:>8} {:>8} {:>8} {:>7}  {}'.format(
            'layer', 'cin', 'cout', 'H', 'W', 'new kernel', 'old ms', 'old ms', 'spread', 'new ms', 'gain %', 'verdict'))
        for i, L in enumerate(new[0]):
            if not L['upsample']:
                continue
            a, b, c = old1[1][i], old2[1][i], new[1][i]
            spread, best_old = abs(a - b), min(a, b)
            print('{:<24} {:>4}->{:<4} {:>3}x{:<3} {:<36} {:>8.3f} {:>8.3f} {:>8.3f} {:>8.3f} {:>7.1f}  {}'.format(
                L['name'][:24], L['cin'], L['cout'], L['height'], L['width'], L['kernel'], a, b, spread, c, 100.0 * (best_old - c) / best_old,
                'faster' if best_old - c > spread else 'not faster'))
        print('conv stack: old {:.3f} / {:.3f} ms, new {:.3f} ms'.format(sum(old1[1]), sum(old2[1]), sum(new[1])))
        del models, x
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
