#!/usr/bin/env python3
"""Cost of the MC sample-agreement extension on one MI355X.  Two measurements, each alternated launch by launch after a warm-up, medians
reported:
  (a) step     McPredictStep(T = 20, seeded masks) + MultiPredictionSummary on one native BraTS volume (155 slices of 240 x 240, bench.py's
               model) with ``agreement=True`` (the voting head, the vote plane's read-modify-write, the OR merge of the lanes, and
               SampleAgreementStep's table kernel) against ``agreement=False`` of the same build: ms per volume and the added share, against
               the 3 % the logit-sampling extension was held to.  ``--baseline-only`` times the ``agreement=False`` leg alone through calls
               that exist without the extension: run from a checkout of the parent commit it shows that the leg has not moved, and
               ``--parent FILE`` folds that record in.
  (b) tables   rcu_agreement_tables on 8 x 155 x 240 x 240 voxels, one image (240 x 240) per volume, T = 20, on a blob-like plane (about 2 % of
               the voxels voted by all passes, a shell of partial agreement around them: most waves skip) and on a uniformly random plane (no
               wave skips: the worst case), against THE YARDSTICK of a one-pass kernel, rcu_unc_hist_from_p at B = 1000 on the same voxels
               (6 bytes per voxel against the plane's 4).
The measurement runs in a child process under a time limit of its own.  Prints one JSON line; ``--out`` also writes it.

    python tools/agreement_bench.py [--reps 7] [--out profiles/agreement_bench.json] [--parent parent.json]
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
VOLUMES = 8
TARGET_SHARE = 0.03


def summary(ts):
    return {'ms_median': round(statistics.median(ts), 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4)}


def measure_step(args, rec):
    import torch
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    from rcu_amd.model import UNet
    dev = torch.device('cuda:0')
    model = UNet(**PARAMS)
    model.load_state_dict(uo.synthetic_state(20, **PARAMS))
    model = model.to(dev).eval()
    images = torch.randn(SLICES, 4, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    ctx = steps.TorchTestContext('cuda:0', model)

    def run(agreement):
        bc = steps.BatchContext({'images': images}, 0)
        kw = {'agreement': True} if agreement else {}
        steps.McPredictStep(T, seed=20, **kw)(bc, None, ctx)
        steps.MultiPredictionSummary()(bc, None, ctx)
        if agreement:
            steps.SampleAgreementStep()(bc, None, ctx)
        return bc

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    legs = {'agreement_off': lambda: run(False)}
    if not args.baseline_only:
        legs['agreement_on'] = lambda: run(True)
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    times = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            times[k].append(wall_ms(fn))
    step = {k: summary(ts) for k, ts in times.items()}
    if 'agreement_on' in step:
        off, on = step['agreement_off']['ms_median'], step['agreement_on']['ms_median']
        step['added_ms'] = round(on - off, 4)
        step['added_share'] = round((on - off) / off, 5)
        step['target_share'] = TARGET_SHARE
        step['within_target'] = (on - off) / off <= TARGET_SHARE
    rec['step'] = dict(step, volume=[SLICES, H, W], mc_steps=T, reps=args.reps, warmup=args.warmup, clock='host wall clock around a synchronised step')


def blob_plane(torch, dev):
    """[1, VOLUMES * SLICES, H, W] int32: an ellipsoid all T passes vote for (about 2 % of the voxels), a shell of random votes around it."""
    z = torch.arange(SLICES, device=dev).view(SLICES, 1, 1).float()
    y = torch.arange(H, device=dev).view(1, H, 1).float()
    x = torch.arange(W, device=dev).view(1, 1, W).float()
    g = torch.Generator(device=dev).manual_seed(5)
    plane = torch.zeros((1, VOLUMES, SLICES, H, W), device=dev, dtype=torch.int32)
    for v in range(VOLUMES):
        r = ((z - 70 - 3 * v) / 28.0) ** 2 + ((y - 110 + 5 * v) / 40.0) ** 2 + ((x - 128) / (33.0 + v)) ** 2
        shell = torch.randint(0, 1 << T, (SLICES, H, W), device=dev, generator=g, dtype=torch.int32)
        plane[0, v] = torch.where(r <= 0.8, torch.full_like(shell, (1 << T) - 1), torch.where(r <= 1.0, shell, torch.zeros_like(shell)))
    return plane.view(1, VOLUMES * SLICES, H, W)


def measure_tables(args, rec):
    import torch
    from rcu_amd import _lib, evaluation as ev
    lib = _lib.load()
    dev = torch.device('cuda:0')
    stream = _lib.current_stream()
    images, hw = VOLUMES * SLICES, H * W
    n = images * hw
    g = torch.Generator(device=dev).manual_seed(1)
    planes = {'blob': blob_plane(torch, dev),
              'random': torch.randint(-2 ** 31, 2 ** 31, (1, images, H, W), device=dev, generator=g, dtype=torch.int64).to(torch.int32)}
    p = torch.rand((VOLUMES, n // VOLUMES), device=dev, generator=g)
    prediction = (p > 0.5).to(torch.uint8)
    target = torch.roll(prediction, 4, dims=1).contiguous()
    hist_ue = torch.empty((VOLUMES, 4, 1000), device=dev, dtype=torch.int64)
    ws = torch.empty(lib.rcu_unc_hist_workspace_bytes(n // VOLUMES, VOLUMES, 1000), device=dev, dtype=torch.uint8)
    hist = torch.empty((images, T + 1), device=dev, dtype=torch.int64)
    pairs = torch.empty((images, T * (T + 1) // 2), device=dev, dtype=torch.int64)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def tables(plane):
        _lib.check(lib.rcu_agreement_tables(_lib.ptr(plane), 1, hw, images, T, _lib.ptr(hist), _lib.ptr(pairs), stream))

    def hist_from_p():
        _lib.check(lib.rcu_unc_hist_from_p(_lib.ptr(p), _lib.ptr(prediction), _lib.ptr(target), None, n // VOLUMES, VOLUMES, 1000, _lib.ptr(hist_ue),
                                           _lib.ptr(ws), stream))

    paths = {'tables_blob': lambda: tables(planes['blob']), 'tables_random': lambda: tables(planes['random']), 'unc_hist_from_p': hist_from_p}
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(max(args.reps, 11)):
        for k, fn in paths.items():
            times[k].append(event_ms(fn))
    out = {k: summary(ts) for k, ts in times.items()}
    yard = out['unc_hist_from_p']['ms_median']
    for k in ('tables_blob', 'tables_random'):
        out[k]['ratio_to_unc_hist_from_p'] = round(out[k]['ms_median'] / yard, 3)
        out[k]['plane_gb_per_s'] = round(4.0 * n / (out[k]['ms_median'] * 1e-3) / 1e9, 1)
    out['unc_hist_from_p']['gb_per_s'] = round(6.0 * n / (yard * 1e-3) / 1e9, 1)
    tables(planes['blob'])
    whole = ev.agreement_metrics(hist.sum(0).cpu().numpy(), pairs.sum(0).cpu().numpy())
    out['blob_plane'] = {'voted_by_all_share': round(whole['intersection'] / n, 5), 'union_share': round(whole['union'] / n, 5),
                         'mean_pairwise_dice': round(whole['mean_pairwise_dice'], 5)}
    rec['tables'] = dict(out, batch=[VOLUMES, SLICES, H, W], volumes=images, voxels_per_volume=hw, passes=T, bytes_per_voxel={'plane': 4, 'unc_hist_from_p': 6})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--timeout', type=int, default=540, help='seconds the measuring child process may take')
    ap.add_argument('--baseline-only', action='store_true', help='time the agreement=False leg alone (runs on a checkout without the extension)')
    ap.add_argument('--parent', default=None, help='a --baseline-only record made from a checkout of the parent commit: folded in as step.parent_commit')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.child:      # the GPU step in a process of its own, under its own time limit
        try:
            return subprocess.run([sys.executable, os.path.abspath(__file__), '--child'] + sys.argv[1:], timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print('agreement_bench: the measurement did not finish within {} s'.format(args.timeout), file=sys.stderr)
            return 124
    import torch
    from rcu_amd import _lib
    t0 = time.time()
    rec = {'device': torch.cuda.get_device_name(0), 'librcu': _lib.load().rcu_version().decode()}
    measure_step(args, rec)
    if not args.baseline_only:
        measure_tables(args, rec)
    if args.parent:
        with open(args.parent) as f:
            parent = json.load(f)['step']['agreement_off']
        rec['step']['parent_commit'] = dict(parent, note='agreement_off timed by this tool (--baseline-only) from a checkout of the parent commit')
        rec['step']['agreement_off_vs_parent'] = round(rec['step']['agreement_off']['ms_median'] / parent['ms_median'], 4)
    rec['wall_s'] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
