#!/usr/bin/env python3
"""Time of the calibration level histogram (rcu_calib_curve) against the 10-bin reliability histogram it sits next to.

On 8 and on 160 benchmark volumes (160 x 192 x 128 voxels, bench.py's shape) and two input distributions -- uniform p, and a peaked one with
about 97 % of the voxels at p < 1e-3 (level 0 of 1000) -- three paths are timed in ONE process, alternated launch by launch, every shape warmed
up first, each launch between two events on the launch stream, medians reported:
    ece_hist_10           rcu_ece_hist with 10 bins: THE YARDSTICK (6 bytes read per voxel: p, target, mask)
    calib_curve_1000      rcu_calib_curve, B = 1000 (the same 6 bytes per voxel)
    calib_curve_4096      rcu_calib_curve, B = 4096
The levels merged into 10 bins are compared with the yardstick's counts at every timed size (they must be equal, integer for integer).
Target: calib_curve_1000 at most 1.5 x the yardstick's time on both distributions.
The measurement runs in a child process under a time limit of its own.  Prints one JSON line; ``--out`` also writes it.

    python tools/calib_curve_bench.py [--reps 15] [--volumes 8,160] [--sweep-blocks 1,2,4,8] [--out profiles/calib_curve_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SLICES, HEIGHT, WIDTH = 160, 192, 128      # bench.py
TARGET_RATIO = 1.5
BYTES_PER_VOXEL = 6


def make_input(torch, dev, volumes, n, dist, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    p = torch.rand((volumes, n), device=dev, generator=g)
    if dist == 'peaked':
        tiny = torch.rand((volumes, n), device=dev, generator=g) * 1e-3
        certain = torch.rand((volumes, n), device=dev, generator=g) < 0.97
        p = torch.where(certain, tiny, p)
        del tiny, certain
    target = (torch.rand((volumes, n), device=dev, generator=g) < 0.3).to(torch.uint8)
    mask = (torch.rand((volumes, n), device=dev, generator=g) < 0.8).to(torch.uint8)
    return p.contiguous(), target, mask


def measure(args):
    import torch
    from rcu_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda:0')
    n = SLICES * HEIGHT * WIDTH
    stream = _lib.current_stream()
    thr10 = _lib.ece_thresholds(10)
    rec = {'volume': [SLICES, HEIGHT, WIDTH], 'voxels_per_volume': n, 'reps': args.reps, 'target_ratio': TARGET_RATIO,
           'device': torch.cuda.get_device_name(0), 'librcu': lib.rcu_version().decode(), 'cases': {}}

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for volumes in args.volumes:
        for dist in ('uniform', 'peaked'):
            p, target, mask = make_input(torch, dev, volumes, n, dist, seed=volumes + (1 if dist == 'peaked' else 0))
            ece_raw = torch.empty(volumes * ctypes.sizeof(_lib.EceResult), device=dev, dtype=torch.uint8)
            ws_ece = torch.empty(max(lib.rcu_ece_workspace_bytes(n, volumes), 8), device=dev, dtype=torch.uint8)
            levels = {b: torch.empty((volumes, 3, b), device=dev, dtype=torch.int64) for b in (1000, 4096)}
            totals = torch.empty((volumes, 2, 4), device=dev, dtype=torch.int64)
            ws = torch.empty(lib.rcu_calib_curve_workspace_bytes(n, volumes, 4096), device=dev, dtype=torch.uint8)

            def ece_hist():
                _lib.check(lib.rcu_ece_hist(_lib.ptr(p), _lib.ptr(target), _lib.ptr(mask), n, volumes, thr10, 10, _lib.ptr(ece_raw), _lib.ptr(ws_ece), stream))

            def calib_curve(b):
                _lib.check(lib.rcu_calib_curve(_lib.ptr(p), _lib.ptr(target), _lib.ptr(mask), n, volumes, b, _lib.ptr(levels[b]), _lib.ptr(totals),
                                               _lib.ptr(ws), stream))

            paths = {'ece_hist_10': ece_hist, 'calib_curve_1000': lambda: calib_curve(1000), 'calib_curve_4096': lambda: calib_curve(4096)}
            for fn in paths.values():          # warm-up of every shape
                fn()
                fn()
            torch.cuda.synchronize()
            ece_counts = ece_raw.view(torch.int64).reshape(volumes, 3, _lib.RCU_MAX_BINS)[:, 0, :10]
            merged = levels[1000][:, :2].sum(dim=1).reshape(volumes, 10, 100).sum(dim=2)
            equal = bool(torch.equal(merged, ece_counts)) and bool(torch.equal(levels[4096][:, :2].sum(dim=(1, 2)), merged.sum(dim=1)))
            times = {k: [] for k in paths}
            for _ in range(args.reps):          # alternated: one launch of each path per round
                for k, fn in paths.items():
                    times[k].append(event_ms(fn))
            case = {'volumes': volumes, 'distribution': dist, 'merged_levels_equal_ece_hist': equal,
                    'share_in_level_0': float(levels[1000][:, :2, 0].sum()) / max(float(merged.sum()), 1.0)}
            nbytes = volumes * n * BYTES_PER_VOXEL
            for k, ts in times.items():
                ms = statistics.median(ts)
                case[k] = {'ms_median': round(ms, 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4), 'bytes': nbytes,
                           'gb_per_s': round(nbytes / (ms * 1e-3) / 1e9, 1)}
            yard = case['ece_hist_10']['ms_median']
            for k in ('calib_curve_1000', 'calib_curve_4096'):
                case[k]['ratio_to_yardstick'] = round(case[k]['ms_median'] / yard, 3)
            if args.sweep_blocks:               # tuning aid: blocks per workgroup of the level histogram, B = 1000
                sweep = {}
                for blocks in args.sweep_blocks:
                    _lib.check(lib.rcu_calib_curve_set_blocks_per_workgroup(blocks))
                    calib_curve(1000)
                    sweep[str(blocks)] = round(statistics.median(event_ms(lambda: calib_curve(1000)) for _ in range(args.reps)), 4)
                _lib.check(lib.rcu_calib_curve_set_blocks_per_workgroup(0))
                case['sweep_blocks_per_workgroup_ms'] = sweep
            rec['cases']['{}_{}'.format(volumes, dist)] = case
            del p, target, mask
            torch.cuda.empty_cache()
    verdict = {}
    for volumes in args.volumes:
        uni, peak = rec['cases']['{}_uniform'.format(volumes)], rec['cases']['{}_peaked'.format(volumes)]
        verdict[str(volumes)] = {
            'ratio_uniform': uni['calib_curve_1000']['ratio_to_yardstick'], 'ratio_peaked': peak['calib_curve_1000']['ratio_to_yardstick'],
            'ratio_uniform_4096': uni['calib_curve_4096']['ratio_to_yardstick'], 'ratio_peaked_4096': peak['calib_curve_4096']['ratio_to_yardstick'],
            'within_target': max(uni['calib_curve_1000']['ratio_to_yardstick'], peak['calib_curve_1000']['ratio_to_yardstick']) <= TARGET_RATIO}
    rec['verdict'] = verdict
    rec['all_histograms_equal'] = all(c['merged_levels_equal_ece_hist'] for c in rec['cases'].values())
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--volumes', type=lambda s: [int(v) for v in s.split(',')], default=[8, 160])
    ap.add_argument('--sweep-blocks', type=lambda s: [int(v) for v in s.split(',')], default=[])
    ap.add_argument('--timeout', type=int, default=540, help='seconds the measuring child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.child:      # the GPU step in a process of its own, under its own time limit
        try:
            return subprocess.run([sys.executable, os.path.abspath(__file__), '--child'] + sys.argv[1:], timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print('calib_curve_bench: the measurement did not finish within {} s'.format(args.timeout), file=sys.stderr)
            return 124
    t0 = time.time()
    rec = measure(args)
    rec['wall_s'] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')
    return 0 if rec['all_histograms_equal'] else 1


if __name__ == '__main__':
    sys.exit(main())
