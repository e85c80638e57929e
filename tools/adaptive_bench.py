#!/usr/bin/env python3
"""Cost and gain of adaptive MC dropout (include/rcu.h "Adaptive MC") on one MI355X.  Two measurements, each alternated launch by launch after
a warm-up, medians reported:
  (a) scores   rcu_mc_slice_scores on the exact statistics of one native BraTS batch (155 slices of 240 x 240, C = 2, five passes of bench.py's
               model) against THE YARDSTICK rcu_mc_finalize with the mean and entropy outputs on the same blob: it reads the same 16 bytes per
               voxel and writes 12 more.  Device events; bytes per second of both.
  (b) step     McPredictStep(T = 20, seeded masks, adaptive check_at = [5]) + MultiPredictionSummary on that volume against the plain step,
               at tolerances chosen from the measured margins so that a fraction f in {0, 0.25, 0.5, 0.75, 1} of the slices retires (synthetic
               volumes have no empty slices: the margin quantile is the only way to reach a given f).  Ratio to the plain step beside the
               pass-count model (1 + 5 + (1 - f) * 15) / 21; at f = 0 the overhead is held to 3 %.  ``--baseline-only`` times the plain leg
               alone through calls that exist without the extension: run from a checkout of the parent commit it shows that the leg has not
               moved, and ``--parent FILE`` folds that record in.
``--profile-fraction F`` runs the adaptive step at fraction F three times and nothing else: the program of a kernel-trace run.
The measurement runs in a child process under a time limit of its own.  Prints one JSON line; ``--out`` also writes it.

    python tools/adaptive_bench.py [--reps 7] [--out profiles/adaptive_bench.json] [--parent parent.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PARAMS = dict(nb_classes=2, in_channels=4, depth=4, start_filters=32, dropout=0.05)      # bench.py's MODEL_PARAMS
SLICES, H, W, T = 155, 240, 240, 20
CHECK_AT = [5]
FRACTIONS = (0.0, 0.25, 0.5, 0.75, 1.0)
TARGET_SHARE = 0.03


def summary(ts):
    return {'ms_median': round(statistics.median(ts), 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4)}


def pass_model(f):
    return (1 + CHECK_AT[0] + (1 - f) * (T - CHECK_AT[0])) / (T + 1.0)


def setup():
    import torch
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    from rcu_amd.model import UNet
    dev = torch.device('cuda:0')
    model = UNet(**PARAMS)
    model.load_state_dict(uo.synthetic_state(20, **PARAMS))
    model = model.to(dev).eval()
    images = torch.randn(SLICES, 4, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    return torch, steps, dev, images, steps.TorchTestContext('cuda:0', model)


def run_step(steps, images, ctx, mc_steps=T, **kw):
    bc = steps.BatchContext({'images': images}, 0)
    steps.McPredictStep(mc_steps, seed=20, **kw)(bc, None, ctx)
    stats = bc.output['multi_probabilities']
    steps.MultiPredictionSummary()(bc, None, ctx)
    return stats, bc


def tolerances(torch, steps, images, ctx):
    """{f: (tolerance, slices that retire)} from the margins of the plain five-pass statistics."""
    stats, _ = run_step(steps, images, ctx, mc_steps=CHECK_AT[0])
    _, margin_q = steps.split_scores(steps.slice_scores(stats, 0))
    scale = CHECK_AT[0] * float(1 << 40)
    ratios = sorted((q / scale for q in margin_q), reverse=True)
    out = {}
    for f in FRACTIONS:
        k = int(round(f * SLICES))
        if k == 0:
            bar = (1.0 + ratios[0]) / 2
        elif k == SLICES:
            bar = ratios[-1] / 2
        else:
            bar = (ratios[k - 1] + ratios[k]) / 2
        out[f] = (1.0 - bar, sum(r >= bar for r in ratios))
    return out, ratios


def measure_step(args, rec):
    torch, steps, dev, images, ctx = setup()

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    legs = {'plain': lambda: run_step(steps, images, ctx)}
    chosen = {}
    if not args.baseline_only:
        chosen, ratios = tolerances(torch, steps, images, ctx)
        for f, (tol, _) in chosen.items():
            legs['f={}'.format(f)] = lambda tol=tol: run_step(steps, images, ctx, adaptive=dict(check_at=CHECK_AT, tolerance=tol))
        rec['margins'] = {'min': ratios[-1], 'median': ratios[len(ratios) // 2], 'max': ratios[0],
                          'note': 'min over the voxels of a slice of the leading class mean probability after 5 passes; synthetic weights'}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    times = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            times[k].append(wall_ms(fn))
    step = {k: summary(ts) for k, ts in times.items()}
    plain = step['plain']['ms_median']
    for f, (tol, expected) in chosen.items():
        leg = step['f={}'.format(f)]
        stats, _ = legs['f={}'.format(f)]()
        retired = sum(1 for c in stats.counts.tolist() if c < T)
        leg.update(tolerance=tol, retired=retired, expected_retired=expected, passes_run=stats.passes_run, passes_plain=SLICES * T,
                   ratio_to_plain=round(leg['ms_median'] / plain, 4), pass_count_model=round(pass_model(retired / float(SLICES)), 4))
    if chosen:
        step['f=0_added_share'] = round(step['f=0.0']['ms_median'] / plain - 1.0, 5)
        step['target_share'] = TARGET_SHARE
        step['within_target'] = step['f=0_added_share'] <= TARGET_SHARE
    rec['step'] = dict(step, volume=[SLICES, H, W], mc_steps=T, check_at=CHECK_AT, reps=args.reps, warmup=args.warmup,
                       clock='host wall clock around a synchronised step')


def measure_scores(args, rec):
    torch, steps, dev, images, ctx = setup()
    from rcu_amd import _lib
    lib, stream = _lib.load(), _lib.current_stream()
    stats, _ = run_step(steps, images, ctx, mc_steps=CHECK_AT[0])
    n, hw, c = stats.n, stats.hw, stats.nb_classes
    thr = steps.adaptive_threshold(0.01, CHECK_AT[0])
    scores = torch.empty(2 * n, device=dev, dtype=torch.int64)
    mean = torch.empty((n, c, H, W), device=dev)
    entropy = torch.empty((n, 1, H, W), device=dev)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def finalize():
        _lib.check(lib.rcu_mc_finalize(_lib.ptr(stats.blob), n, hw, c, CHECK_AT[0], stats.flags, _lib.ptr(mean), _lib.ptr(entropy), None, None, stream))

    paths = {'slice_scores': lambda: steps.slice_scores(stats, thr, out=scores), 'finalize_mean_entropy': finalize}
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(max(args.reps, 21)):
        for k, fn in paths.items():
            times[k].append(event_ms(fn))
    out = {k: summary(ts) for k, ts in times.items()}
    voxels = n * hw
    out['slice_scores']['gb_per_s'] = round(8.0 * c * voxels / (out['slice_scores']['ms_median'] * 1e-3) / 1e9, 1)
    out['finalize_mean_entropy']['gb_per_s'] = round((8.0 * c + 4.0 * (c + 1)) * voxels / (out['finalize_mean_entropy']['ms_median'] * 1e-3) / 1e9, 1)
    out['ratio_to_finalize'] = round(out['slice_scores']['ms_median'] / out['finalize_mean_entropy']['ms_median'], 3)
    out['not_slower'] = out['ratio_to_finalize'] <= 1.0
    rec['scores'] = dict(out, batch=[n, H, W], nb_classes=c, bytes_per_voxel={'slice_scores': 8 * c, 'finalize_mean_entropy': 8 * c + 4 * (c + 1)},
                         clock='device events around one call (the scores call is two launches: the reset of the outputs and the kernel)')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--timeout', type=int, default=540, help='seconds the measuring child process may take')
    ap.add_argument('--baseline-only', action='store_true', help='time the plain leg alone (runs on a checkout without the extension)')
    ap.add_argument('--parent', default=None, help='a --baseline-only record made from a checkout of the parent commit: folded in as step.parent_commit')
    ap.add_argument('--profile-fraction', type=float, default=None, help='run the adaptive step at this retired fraction three times, nothing else')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.child:      # the GPU step in a process of its own, under its own time limit
        try:
            return subprocess.run([sys.executable, os.path.abspath(__file__), '--child'] + sys.argv[1:], timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print('adaptive_bench: the measurement did not finish within {} s'.format(args.timeout), file=sys.stderr)
            return 124
    import torch
    from rcu_amd import _lib
    if args.profile_fraction is not None:
        _, steps, _, images, ctx = setup()
        chosen, _ = tolerances(torch, steps, images, ctx)
        tol, expected = chosen[args.profile_fraction]
        for _ in range(3):
            stats, _ = run_step(steps, images, ctx, adaptive=dict(check_at=CHECK_AT, tolerance=tol))
        torch.cuda.synchronize()
        print(json.dumps({'profiled_fraction': args.profile_fraction, 'tolerance': tol, 'expected_retired': expected, 'passes_run': stats.passes_run}))
        return 0
    t0 = time.time()
    rec = {'device': torch.cuda.get_device_name(0), 'librcu': _lib.load().rcu_version().decode()}
    measure_step(args, rec)
    if not args.baseline_only:
        measure_scores(args, rec)
    if args.parent:
        with open(args.parent) as f:
            parent = json.load(f)['step']['plain']
        rec['step']['parent_commit'] = dict(parent, note='the plain step timed by this tool (--baseline-only) from a checkout of the parent commit')
        rec['step']['plain_vs_parent'] = round(rec['step']['plain']['ms_median'] / parent['ms_median'], 4)
        for f in FRACTIONS:
            leg = rec['step'].get('f={}'.format(f))
            if leg:
                leg['ratio_to_parent_plain'] = round(leg['ms_median'] / parent['ms_median'], 4)
    rec['wall_s'] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
