#!/usr/bin/env python3
"""Time of the feature-space density (rcu_density_energy, rcu_density_moments; include/rcu.h "Feature-space density") on one native BraTS batch,
155 x 240 x 240 voxels of F = 32 features at pitch 32, K = 2 classes.

kernels   the energy kernel and the moments kernel against rcu_postnet_forward of a PostNet(in_channels 32, nb_convs 2, nb_classes 2) on the same
          feature tensor -- THE YARDSTICK: it reads the same 128 bytes per voxel through the same fp32 MFMA -- in ONE process, alternated launch by
          launch, every path warmed up first, each launch between two events on the launch stream, medians reported.  Target for the energy kernel:
          at most 1.5 x the yardstick.  The moments kernel, the energy with the d2 output, and F = 64, K = 3 (on a pitch-64 tensor, against the same
          PostNet at 64 channels) are reported with their ratio, no target.
step      the eval-mode default step (SegmentationPredictStep(do_probs=True)) on that volume (bench.py's model) against DensityPredictStep, and
          against the default step with the feature tap alone (what provide_features pays regardless: the compact copy of the padded level 0),
          alternated.  ``--parent DIR``: the default step of another checkout (the parent commit, built) measured by this tool in a child process of
          its own, before and after this checkout's.
Every measurement runs in a child process under a time limit of its own.  Prints one JSON line; ``--out`` also writes it.

    python tools/density_bench.py [--reps 15] [--parent ../parent] [--out profiles/density_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
SLICES, C, H, W = 155, 4, 240, 240
PARAMS = dict(nb_classes=2, in_channels=4, depth=4, start_filters=32, dropout=0.05)     # bench.py's MODEL_PARAMS
TARGET_RATIO = 1.5


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ts):
    return {'ms_median': round(statistics.median(ts), 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4)}


def alternated(torch, paths, reps):
    for fn in paths.values():          # warm-up of every path
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(reps):              # one launch of each path per round
        for k, fn in paths.items():
            times[k].append(event_ms(torch, fn))
    return {k: summary(ts) for k, ts in times.items()}


def volume_and_model(torch):
    from oracle import unet_oracle as uo
    from rcu_amd.model import UNet
    dev = torch.device('cuda:0')
    model = UNet(**PARAMS)
    model.load_state_dict(uo.synthetic_state(20, **PARAMS))
    images = torch.randn(SLICES, C, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    return images, model.to(dev).eval()


def default_step(steps, images, ctx):
    bc = steps.BatchContext({'images': images}, 0, sample_offset=0)
    steps.SegmentationPredictStep(do_probs=True)(bc, None, ctx)
    return bc


def measure_step_only(args):
    """The eval-mode default step of the checkout this process imports (``--root``)."""
    import torch
    from rcu_amd import _lib, steps
    images, model = volume_and_model(torch)
    ctx = steps.TorchTestContext('cuda:0', model)
    rec = alternated(torch, {'default_step': lambda: default_step(steps, images, ctx)}, args.reps)['default_step']
    return dict(rec, librcu=_lib.load().rcu_version().decode(), root=os.path.basename(args.root.rstrip('/')))


def synthetic_fit(torch, density, F, K, seed):
    """A well-conditioned fit of the right shape: the kernels' time does not depend on the parameters' values."""
    import numpy as np
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((1, 4096, F)) @ (rng.standard_normal((F, F)) / F ** 0.5 + np.eye(F)) + rng.standard_normal(F)
    y = rng.integers(0, K, (1, 4096))
    n = np.stack([[(y[0] == c).sum() for c in range(K)]])
    S = np.stack([[x[0][y[0] == c].sum(0) for c in range(K)]])
    G = np.stack([[x[0][y[0] == c].T @ x[0][y[0] == c] for c in range(K)]])
    return density.fit_from_moments(n, S, G)


def measure(args):
    import torch
    from rcu_amd import _lib, density, steps
    from rcu_amd.model import PostNet
    lib = _lib.load()
    dev = torch.device('cuda:0')
    voxels = SLICES * H * W
    rec = {'batch': [SLICES, H, W], 'voxels': voxels, 'reps': args.reps, 'target_ratio_energy': TARGET_RATIO, 'device': torch.cuda.get_device_name(0),
           'librcu': lib.rcu_version().decode(), 'kernels': {}}
    gen = torch.Generator(device=dev).manual_seed(5)
    for F, K in ((32, 2), (64, 3)):
        nhwc = torch.randn(SLICES, H, W, F, device=dev, generator=gen)
        feats = nhwc.permute(0, 3, 1, 2)                       # the view UNet.features hands out: read in place
        labels = torch.randint(0, K, (SLICES, H, W), device=dev, generator=gen, dtype=torch.int64).to(torch.uint8)
        fit = synthetic_fit(torch, density, F, K, F)
        post = PostNet(F, 2, nb_convs=2).to(dev).eval()
        # the moments through the C entry point on preallocated outputs: the wrapper's label check and allocations are host time, not the kernel's
        counts = torch.empty((SLICES, K), device=dev, dtype=torch.int64)
        s_out = torch.empty((SLICES, K, F), device=dev, dtype=torch.float64)
        g_out = torch.empty((SLICES, K, F, F), device=dev, dtype=torch.float64)
        ws = torch.empty(lib.rcu_density_moments_workspace_bytes(SLICES, H * W, F, K) // 8, device=dev, dtype=torch.float64)

        def moments():
            _lib.check(lib.rcu_density_moments(_lib.ptr(nhwc), F, F, _lib.ptr(labels), SLICES, H * W, K, _lib.ptr(counts), _lib.ptr(s_out),
                                               _lib.ptr(g_out), _lib.ptr(ws), _lib.current_stream()))

        paths = {'postnet_forward': lambda: post(feats), 'energy': lambda: density.energy(fit, feats),
                 'energy_with_d2': lambda: density.energy(fit, feats, with_d2=True), 'moments': moments}
        got = alternated(torch, paths, args.reps)
        yard = got['postnet_forward']['ms_median']
        for k, entry in got.items():
            entry['feature_bytes_per_s'] = voxels * F * 4 / (entry['ms_median'] * 1e-3)
            entry['ratio_to_yardstick'] = round(entry['ms_median'] / yard, 3)
        if (F, K) == (32, 2):
            got['energy']['within_target'] = got['energy']['ratio_to_yardstick'] <= TARGET_RATIO
        rec['kernels']['F{}_K{}'.format(F, K)] = got
        rec['kernels']['F{}_K{}'.format(F, K)]['moments_workspace_bytes'] = ws.numel() * 8
        del nhwc, feats, labels, post, counts, s_out, g_out, ws
        torch.cuda.empty_cache()
    # the step
    images, model = volume_and_model(torch)
    ctx = steps.TorchTestContext('cuda:0', model)
    fit = synthetic_fit(torch, density, 32, 2, 1)
    dstep = steps.DensityPredictStep(fit)

    def density_step():
        bc = steps.BatchContext({'images': images}, 0, sample_offset=0)
        dstep(bc, None, ctx)
        return bc

    def tap_step():
        with density.eval_features(model):
            return default_step(steps, images, ctx)

    step = alternated(torch, {'default_step': lambda: default_step(steps, images, ctx), 'default_step_with_feature_tap': tap_step,
                              'density_step': density_step}, args.reps)
    base, tap, full = (step[k]['ms_median'] for k in ('default_step', 'default_step_with_feature_tap', 'density_step'))
    step.update({'added_ms': round(full - base, 4), 'added_share': round((full - base) / base, 5), 'added_ms_feature_tap': round(tap - base, 4),
                 'added_ms_energy_kernel': round(full - tap, 4)})
    rec['step'] = step
    return rec


def child(root, extra, timeout):
    """This tool's measurement from the checkout ``root``, in a process of its own under a time limit -> its JSON record."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--root', root] + extra
    done = subprocess.run(cmd, timeout=timeout, stdout=subprocess.PIPE, check=True, cwd=root)
    return json.loads(done.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: its default step is measured too')
    ap.add_argument('--timeout', type=int, default=420, help='seconds each measuring child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--root', default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--step-only', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, os.path.abspath(args.root))
        print(json.dumps(measure_step_only(args) if args.step_only else measure(args)))
        return 0
    t0 = time.time()
    reps = ['--reps', str(args.reps)]
    try:
        parent = [child(os.path.abspath(args.parent), reps + ['--step-only'], args.timeout)] if args.parent else []
        rec = child(os.path.abspath(args.root), reps, args.timeout)
        if args.parent:
            parent.append(child(os.path.abspath(args.parent), reps + ['--step-only'], args.timeout))
            rec['step']['parent_commit_default_step'] = parent
            rec['step']['this_checkout_default_step_only'] = child(os.path.abspath(args.root), reps + ['--step-only'], args.timeout)
    except subprocess.TimeoutExpired:
        print('density_bench: a measurement did not finish within {} s'.format(args.timeout), file=sys.stderr)
        return 124
    except subprocess.CalledProcessError as e:
        print('density_bench: a measuring process failed with status {}'.format(e.returncode), file=sys.stderr)
        return 1      # (nothing more is started on the GPU after a failed measurement)
    rec['wall_s'] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
