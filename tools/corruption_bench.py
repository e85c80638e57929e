#!/usr/bin/env python3
"""Time of the input corruptions (rcu_corrupt, include/rcu.h "Input corruptions") on one native BraTS batch, 155 x 4 x 240 x 240 float32.

kernels   every kind against rcu_tta_transform(flip_h) on the same tensor -- THE YARDSTICK: it reads and writes the same 8 bytes per element --
          in ONE process, alternated launch by launch, every path warmed up first, each launch between two events on the launch stream,
          medians reported.  Target for the pointwise kinds (gaussian_noise, intensity_shift, bias_field, ghosting, channel_drop): at most
          1.5 x the yardstick.  gaussian_blur at sigma 1 and 3, downsample and contrast are reported with their ratio, no target.
step      CorruptInputStep([gaussian_blur severity 2, gaussian_noise severity 3]) followed by McPredictStep(T = 20, seeded) and
          MultiPredictionSummary on that volume (bench.py's model) against the MC step alone, alternated; target: the corruption adds less
          than 3 % (what the logit-sampling extension was held to).  ``--parent DIR``: the plain MC step of another checkout (the parent
          commit, built) measured by this tool in a child process of its own, before and after this checkout's.
Every measurement runs in a child process under a time limit of its own.  Prints one JSON line; ``--out`` also writes it.

    python tools/corruption_bench.py [--reps 15] [--parent ../parent] [--out profiles/corruption_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
SLICES, C, H, W, T = 155, 4, 240, 240, 20
PARAMS = dict(nb_classes=2, in_channels=4, depth=4, start_filters=32, dropout=0.05)     # bench.py's MODEL_PARAMS
TARGET_RATIO, TARGET_STEP_SHARE = 1.5, 0.03
POINTWISE = ('gaussian_noise', 'intensity_shift', 'bias_field', 'ghosting', 'channel_drop')
KERNEL_CASES = (('gaussian_noise', {'kind': 'gaussian_noise', 'severity': 3}), ('gaussian_blur_sigma1', {'kind': 'gaussian_blur', 'amount': 1.0}),
                ('gaussian_blur_sigma3', {'kind': 'gaussian_blur', 'amount': 3.0}), ('downsample', {'kind': 'downsample', 'severity': 3}),
                ('contrast', {'kind': 'contrast', 'severity': 3}), ('intensity_shift', {'kind': 'intensity_shift', 'severity': 3}),
                ('bias_field', {'kind': 'bias_field', 'severity': 3}), ('ghosting', {'kind': 'ghosting', 'severity': 3}),
                ('channel_drop', {'kind': 'channel_drop', 'channels': [1]}))
STEP_SPEC = [{'kind': 'gaussian_blur', 'severity': 2}, {'kind': 'gaussian_noise', 'severity': 3}]


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ts):
    return {'ms_median': round(statistics.median(ts), 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4)}


def volume_and_model(torch):
    from oracle import unet_oracle as uo
    from rcu_amd.model import UNet
    dev = torch.device('cuda:0')
    model = UNet(**PARAMS)
    model.load_state_dict(uo.synthetic_state(20, **PARAMS))
    images = torch.randn(SLICES, C, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    return images, model.to(dev).eval()


def mc_step(steps, images, ctx, before=()):
    bc = steps.BatchContext({'images': images}, 0, sample_offset=0)
    for step in before:
        step(bc, None, ctx)
    steps.McPredictStep(T, seed=20)(bc, None, ctx)
    steps.MultiPredictionSummary()(bc, None, ctx)
    return bc


def measure_mc_only(args):
    """The plain MC step of the checkout this process imports (``--root``)."""
    import torch
    from rcu_amd import _lib, steps
    images, model = volume_and_model(torch)
    ctx = steps.TorchTestContext('cuda:0', model)
    for _ in range(2):
        mc_step(steps, images, ctx)
    torch.cuda.synchronize()
    ts = [event_ms(torch, lambda: mc_step(steps, images, ctx)) for _ in range(args.reps)]
    return dict(summary(ts), librcu=_lib.load().rcu_version().decode(), root=os.path.basename(args.root.rstrip('/')))


def measure(args):
    import torch
    from rcu_amd import _lib
    from rcu_amd import corruption as co
    from rcu_amd import steps
    lib = _lib.load()
    images, model = volume_and_model(torch)
    rec = {'batch': [SLICES, C, H, W], 'bytes_read_and_written': 2 * images.numel() * 4, 'reps': args.reps, 'target_ratio_pointwise': TARGET_RATIO,
           'target_step_share': TARGET_STEP_SHARE, 'device': torch.cuda.get_device_name(0), 'librcu': lib.rcu_version().decode(), 'kernels': {}}
    out = torch.empty_like(images)
    paths = {'tta_flip_h': lambda: steps.tta_transform(images, 'flip_h', out=out)}
    for name, spec in KERNEL_CASES:
        (stage,) = co.parse(spec)
        paths[name] = (lambda stage=stage: co.corrupt_stage(images, stage, co.corruption_seed(20, 0), 0, out))
    for fn in paths.values():          # warm-up of every path
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(args.reps):          # alternated: one launch of each path per round
        for k, fn in paths.items():
            times[k].append(event_ms(torch, fn))
    yard = statistics.median(times['tta_flip_h'])
    for k, ts in times.items():
        entry = summary(ts)
        entry['bytes_per_s'] = rec['bytes_read_and_written'] / (entry['ms_median'] * 1e-3)
        entry['ratio_to_yardstick'] = round(entry['ms_median'] / yard, 3)
        if k in POINTWISE:
            entry['within_target'] = entry['ratio_to_yardstick'] <= TARGET_RATIO
        rec['kernels'][k] = entry
    rec['pointwise_within_target'] = all(rec['kernels'][k]['within_target'] for k in POINTWISE)
    del out
    # the step in front of the T = 20 MC step
    ctx = steps.TorchTestContext('cuda:0', model)
    corrupt_step = steps.CorruptInputStep(co.parse(STEP_SPEC), 20)
    both = {'mc_step': lambda: mc_step(steps, images, ctx), 'corrupt_and_mc_step': lambda: mc_step(steps, images, ctx, before=(corrupt_step,))}
    for fn in both.values():
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in both}
    for _ in range(args.reps):
        for k, fn in both.items():
            times[k].append(event_ms(torch, fn))
    step = {k: summary(ts) for k, ts in times.items()}
    added = step['corrupt_and_mc_step']['ms_median'] - step['mc_step']['ms_median']
    step.update({'stages': STEP_SPEC, 'mc_steps': T, 'added_ms': round(added, 4), 'added_share': round(added / step['mc_step']['ms_median'], 5),
                 'within_target': added / step['mc_step']['ms_median'] < TARGET_STEP_SHARE})
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
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: its plain MC step is measured too')
    ap.add_argument('--timeout', type=int, default=420, help='seconds each measuring child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--root', default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--mc-only', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, os.path.abspath(args.root))
        print(json.dumps(measure_mc_only(args) if args.mc_only else measure(args)))
        return 0
    t0 = time.time()
    reps = ['--reps', str(args.reps)]
    try:
        parent = [child(os.path.abspath(args.parent), reps + ['--mc-only'], args.timeout)] if args.parent else []
        rec = child(os.path.abspath(args.root), reps, args.timeout)
        if args.parent:
            parent.append(child(os.path.abspath(args.parent), reps + ['--mc-only'], args.timeout))
            rec['step']['parent_commit_mc_step'] = parent
            rec['step']['this_checkout_mc_step_only'] = child(os.path.abspath(args.root), reps + ['--mc-only'], args.timeout)
    except subprocess.TimeoutExpired:
        print('corruption_bench: a measurement did not finish within {} s'.format(args.timeout), file=sys.stderr)
        return 124
    except subprocess.CalledProcessError as e:
        print('corruption_bench: a measuring process failed with status {}'.format(e.returncode), file=sys.stderr)
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
