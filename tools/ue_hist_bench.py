#!/usr/bin/env python3
"""Time of the uncertainty level histogram (rcu_unc_hist_from_p / rcu_unc_hist) against the 11-threshold counts kernel it sits next to.

On 8 and on 160 benchmark volumes (160 x 192 x 128 voxels, bench.py's shape) and two input distributions -- uniform p, and the peaked one of
fixture G22 (b): about 97 % of the voxels with p < 1e-4 or p > 1 - 1e-4 -- four paths are timed in ONE process, alternated launch by launch,
every shape warmed up first, each launch between two events on the launch stream, medians reported:
    unc_counts_from_p     rcu_unc_counts_from_p with the 11 script thresholds: THE YARDSTICK (6 bytes read per voxel)
    hist_from_p_1000      rcu_unc_hist_from_p, B = 1000 (the same 6 bytes per voxel)
    hist_from_p_4096      rcu_unc_hist_from_p, B = 4096
    entropy_then_hist     rcu_normalised_entropy (4 read + 8 written) + rcu_unc_hist at B = 1000 (10 read): what the from-p kernel replaces
The histograms of the from-p and of the map path are compared at every timed size (they must be equal, integer for integer).
Target: hist_from_p_1000 at most 1.5 x the yardstick's time on both distributions, and the peaked input at most 1.5 x the uniform one.
The measurement runs in a child process under a time limit of its own.  Prints one JSON line; ``--out`` also writes it.

    python tools/ue_hist_bench.py [--reps 15] [--volumes 8,160] [--sweep-blocks 1,2,4,8] [--out profiles/ue_hist_bench.json]
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

SLICES, HEIGHT, WIDTH = 160, 192, 128      # bench.py
TARGET_RATIO = 1.5


def make_input(torch, dev, volumes, n, dist, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    p = torch.rand((volumes, n), device=dev, generator=g)
    if dist == 'peaked':
        tiny = torch.rand((volumes, n), device=dev, generator=g) * 1e-4
        low = torch.rand((volumes, n), device=dev, generator=g) < 0.9
        certain = torch.rand((volumes, n), device=dev, generator=g) < 0.97
        p = torch.where(certain, torch.where(low, tiny, 1 - tiny), p)
        del tiny, low, certain
    target = (torch.rand((volumes, n), device=dev, generator=g) < 0.3).to(torch.uint8)
    return p.contiguous(), (p > 0.5).to(torch.uint8), target


def measure(args):
    import ctypes
    import torch
    from rcu_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda:0')
    n = SLICES * HEIGHT * WIDTH
    stream = _lib.current_stream()
    thr = (ctypes.c_double * 11)(*[lib.rcu_unc_from_p_threshold(i) for i in range(11)])
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
            p, pred, target = make_input(torch, dev, volumes, n, dist, seed=volumes + (1 if dist == 'peaked' else 0))
            counts = torch.empty((volumes, 11, 8), device=dev, dtype=torch.int64)
            ws_counts = torch.empty(lib.rcu_unc_from_p_workspace_bytes(n, volumes), device=dev, dtype=torch.uint8)
            hist = {b: torch.empty((volumes, 4, b), device=dev, dtype=torch.int64) for b in (1000, 4096)}
            hist_map = torch.empty((volumes, 4, 1000), device=dev, dtype=torch.int64)
            ws_hist = torch.empty(lib.rcu_unc_hist_workspace_bytes(n, volumes, 4096), device=dev, dtype=torch.uint8)
            entropy = torch.empty((volumes, n), device=dev, dtype=torch.float64)

            def counts_from_p():
                _lib.check(lib.rcu_unc_counts_from_p(_lib.ptr(p), _lib.ptr(pred), _lib.ptr(target), None, n, volumes, thr, 11, _lib.ptr(counts),
                                                     _lib.ptr(ws_counts), stream))

            def hist_from_p(levels):
                _lib.check(lib.rcu_unc_hist_from_p(_lib.ptr(p), _lib.ptr(pred), _lib.ptr(target), None, n, volumes, levels, _lib.ptr(hist[levels]),
                                                   _lib.ptr(ws_hist), stream))

            def entropy_then_hist():
                _lib.check(lib.rcu_normalised_entropy(_lib.ptr(p), volumes * n, _lib.ptr(entropy), None, stream))
                _lib.check(lib.rcu_unc_hist(_lib.ptr(entropy), 1, _lib.ptr(pred), _lib.ptr(target), None, n, volumes, 1000, _lib.ptr(hist_map),
                                            _lib.ptr(ws_hist), stream))

            paths = {'unc_counts_from_p': counts_from_p, 'hist_from_p_1000': lambda: hist_from_p(1000),
                     'hist_from_p_4096': lambda: hist_from_p(4096), 'entropy_then_hist': entropy_then_hist}
            for fn in paths.values():          # warm-up of every shape
                fn()
                fn()
            torch.cuda.synchronize()
            equal = bool(torch.equal(hist[1000], hist_map))
            base_counts = counts[:, 0, :4].sum(dim=0).tolist()
            cells_equal = hist[1000].sum(dim=2).sum(dim=0).tolist() == base_counts
            times = {k: [] for k in paths}
            for _ in range(args.reps):          # alternated: one launch of each path per round
                for k, fn in paths.items():
                    times[k].append(event_ms(fn))
            case = {'volumes': volumes, 'distribution': dist, 'hist_from_p_equals_map_path': equal, 'cell_totals_equal_counts_kernel': cells_equal,
                    'share_in_level_0': float(hist[1000][:, :, 0].sum()) / (volumes * n)}
            for k, ts in times.items():
                ms = statistics.median(ts)
                nbytes = volumes * n * (22 if k == 'entropy_then_hist' else 6)
                case[k] = {'ms_median': round(ms, 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4),
                           'bytes': nbytes, 'bytes_per_s': nbytes / (ms * 1e-3)}
            yard = case['unc_counts_from_p']['ms_median']
            for k in ('hist_from_p_1000', 'hist_from_p_4096', 'entropy_then_hist'):
                case[k]['ratio_to_yardstick'] = round(case[k]['ms_median'] / yard, 3)
            if args.sweep_blocks:               # tuning aid: blocks per workgroup of the histogram kernel, B = 1000
                sweep = {}
                for blocks in args.sweep_blocks:
                    _lib.check(lib.rcu_unc_hist_set_blocks_per_workgroup(blocks))
                    hist_from_p(1000)
                    sweep[str(blocks)] = round(statistics.median(event_ms(lambda: hist_from_p(1000)) for _ in range(args.reps)), 4)
                _lib.check(lib.rcu_unc_hist_set_blocks_per_workgroup(0))
                case['sweep_blocks_per_workgroup_ms'] = sweep
            rec['cases']['{}_{}'.format(volumes, dist)] = case
            del p, pred, target, entropy
            torch.cuda.empty_cache()
    verdict = {}
    for volumes in args.volumes:
        uni, peak = rec['cases']['{}_uniform'.format(volumes)], rec['cases']['{}_peaked'.format(volumes)]
        verdict[str(volumes)] = {
            'ratio_uniform': uni['hist_from_p_1000']['ratio_to_yardstick'], 'ratio_peaked': peak['hist_from_p_1000']['ratio_to_yardstick'],
            'peaked_over_uniform': round(peak['hist_from_p_1000']['ms_median'] / uni['hist_from_p_1000']['ms_median'], 3),
            'within_target': max(uni['hist_from_p_1000']['ratio_to_yardstick'], peak['hist_from_p_1000']['ratio_to_yardstick']) <= TARGET_RATIO}
    rec['verdict'] = verdict
    rec['all_histograms_equal'] = all(c['hist_from_p_equals_map_path'] and c['cell_totals_equal_counts_kernel'] for c in rec['cases'].values())
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
            print('ue_hist_bench: the measurement did not finish within {} s'.format(args.timeout), file=sys.stderr)
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
