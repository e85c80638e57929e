#!/usr/bin/env python3
"""Time of the exact squared distance transform (rcu_edt_sq) and of the device work of the 'boundary' evaluation action on the native BraTS
batch, 8 x 155 x 240 x 240 voxels, on the blob-plus-islands mask of tools/components_bench.py (the target: the mask rolled by 4 voxels).
Paths, timed in ONE process, alternated launch by launch after a warm-up, each launch between two events on the launch stream, medians
reported (per batch and per volume):
    edt_sq            ONE rcu_edt_sq of the target (zero_is_feature = 1); edt_sq_inverted the other one (zero_is_feature = 0)
    boundary_table    rcu_boundary_table with the in-register entropy of a float32 probability map, 10 bands
    off_border_hist   rcu_border_mask (1, 1), its inversion, and rcu_unc_hist_from_p at B = 1000 inside that mask
    surface_hist      rcu_surface_distance_hist: two surfaces, two transforms, two histograms
    unc_hist_from_p   rcu_unc_hist_from_p at B = 1000 on the same voxels: THE YARDSTICK of a one-pass kernel
The action's device path is edt_sq + edt_sq_inverted + boundary_table + off_border_hist + surface_hist; `action_wall_ms` is the whole of
evaluation._boundary_on_device (allocations, the compaction of the histograms and the copies to the host included) by the wall clock.
`single_feature` is the transform's worst case for the pruning, one volume with one feature voxel in a corner.  The oracle,
scipy.ndimage.distance_transform_edt on one volume of the same mask, is timed on this host when scipy is importable.
The measurement runs in a child process under a time limit of its own.  Prints one JSON line; ``--out`` also writes it.

    python tools/boundary_bench.py [--reps 11] [--out profiles/boundary_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _path not in sys.path:
        sys.path.insert(0, _path)

from components_bench import SHAPE, VOLUMES, blob_mask      # noqa: E402  (the mask of that tool)

WAIT_FOR_FILES_MS = 38.0       # what the evaluation loop already waits for a subject's .nii.gz files (README, components paragraph)


def measure(args):
    import torch
    from rcu_amd import _lib, evaluation as ev
    lib = _lib.load()
    dev = torch.device('cuda:0')
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    v = VOLUMES
    d, h, w = SHAPE
    stream = _lib.current_stream()
    rec = {'batch': [v] + list(SHAPE), 'voxels_per_volume': n, 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
           'librcu': lib.rcu_version().decode(), 'bands': 10, 'levels': 1000}

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    g = torch.Generator(device=dev).manual_seed(1)
    p = torch.rand((v, n), device=dev, generator=g)
    prediction = blob_mask(torch, dev, 7)
    target = torch.roll(prediction, 4, dims=3).contiguous().reshape(v, n)
    prediction = prediction.reshape(v, n)
    d_in = torch.empty((v, n), device=dev, dtype=torch.int32)
    d_out = torch.empty((v, n), device=dev, dtype=torch.int32)
    table = torch.empty(v * 2 * 11 * ev.BOUNDARY_DTYPE.itemsize, device=dev, dtype=torch.uint8)
    shell = torch.empty((v, n), device=dev, dtype=torch.uint8)
    hist = torch.empty((v, 4, 1000), device=dev, dtype=torch.int64)
    ws_hist = torch.empty(lib.rcu_unc_hist_workspace_bytes(n, v, 1000), device=dev, dtype=torch.uint8)
    bins = int(lib.rcu_surface_distance_bins(d, h, w))
    surface = torch.empty((v, 2, bins), device=dev, dtype=torch.int32)
    ws_surface = torch.empty(lib.rcu_surface_distance_workspace_bytes(n, v), device=dev, dtype=torch.uint8)

    def edt(zero, out):
        _lib.check(lib.rcu_edt_sq(_lib.ptr(target), d, h, w, v, zero, _lib.ptr(out), stream))

    def boundary_table():
        _lib.check(lib.rcu_boundary_table(_lib.ptr(prediction), _lib.ptr(target), _lib.ptr(d_in), _lib.ptr(d_out), _lib.ptr(p), _lib.RCU_CC_UNC_P, n, v, 10,
                                          _lib.ptr(table), stream))

    def off_border_hist():
        _lib.check(lib.rcu_border_mask(_lib.ptr(d_in), _lib.ptr(d_out), v * n, 1, 1, _lib.ptr(shell), None, stream))
        off = (shell == 0).to(torch.uint8)
        _lib.check(lib.rcu_unc_hist_from_p(_lib.ptr(p), _lib.ptr(prediction), _lib.ptr(target), _lib.ptr(off), n, v, 1000, _lib.ptr(hist), _lib.ptr(ws_hist), stream))

    def surface_hist():
        _lib.check(lib.rcu_surface_distance_hist(_lib.ptr(prediction), _lib.ptr(target), d, h, w, v, _lib.ptr(surface), _lib.ptr(ws_surface), stream))

    def hist_from_p():
        _lib.check(lib.rcu_unc_hist_from_p(_lib.ptr(p), _lib.ptr(prediction), _lib.ptr(target), None, n, v, 1000, _lib.ptr(hist), _lib.ptr(ws_hist), stream))

    paths = {'edt_sq': lambda: edt(1, d_in), 'edt_sq_inverted': lambda: edt(0, d_out), 'boundary_table': boundary_table,
             'off_border_hist': off_border_hist, 'surface_hist': surface_hist, 'unc_hist_from_p': hist_from_p}
    first_ms = event_ms(paths['edt_sq'])
    print('boundary_bench: first rcu_edt_sq launch {:.2f} ms'.format(first_ms), file=sys.stderr, flush=True)
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(args.reps):                     # alternated: one launch of each path per round (the transforms first: the others read them)
        for k, fn in paths.items():
            times[k].append(event_ms(fn))
    rec['foreground_share'] = float(target.float().mean())
    rec['first_edt_launch_ms'] = round(first_ms, 3)
    for k, ts in times.items():
        ms = statistics.median(ts)
        rec[k] = {'ms_median': round(ms, 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4), 'ms_per_volume': round(ms / v, 4)}
    action = ('edt_sq', 'edt_sq_inverted', 'boundary_table', 'off_border_hist', 'surface_hist')
    device_ms = sum(rec[k]['ms_median'] for k in action)
    rec['action_device_path'] = list(action)
    rec['action_device_ms_per_volume'] = round(device_ms / v, 4)
    rec['action_ratio_to_unc_hist_from_p'] = round(device_ms / rec['unc_hist_from_p']['ms_median'], 2)
    rec['edt_ratio_to_unc_hist_from_p'] = round(rec['edt_sq']['ms_median'] / rec['unc_hist_from_p']['ms_median'], 2)
    rec['wait_for_files_ms_per_subject'] = WAIT_FOR_FILES_MS
    rec['action_device_path_under_wait_for_files'] = device_ms / v < WAIT_FOR_FILES_MS
    del d_in, d_out, shell, surface, ws_surface
    torch.cuda.empty_cache()
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev._boundary_on_device(p, prediction, target, SHAPE, 10, 1000)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    rec['action_wall_ms'] = {'ms_median': round(statistics.median(walls), 3), 'ms_per_volume': round(statistics.median(walls) / v, 3), 'runs': 3,
                             'note': 'evaluation._boundary_on_device: allocations, compaction and copies to the host included; the first run warms the allocator'}
    # the worst case of the pruning: one volume, one feature voxel in a corner (every walk runs the whole line)
    one = torch.ones((1, n), device=dev, dtype=torch.uint8)
    one[0, n - 1] = 0
    out = torch.empty((1, n), device=dev, dtype=torch.int32)

    def worst():
        _lib.check(lib.rcu_edt_sq(_lib.ptr(one), d, h, w, 1, 1, _lib.ptr(out), stream))
    first_worst = event_ms(worst)
    print('boundary_bench: single-feature volume, first launch {:.2f} ms'.format(first_worst), file=sys.stderr, flush=True)
    ts = [event_ms(worst) for _ in range(3)]
    rec['single_feature'] = {'volumes': 1, 'ms_median': round(statistics.median(ts), 4), 'first_launch_ms': round(first_worst, 3),
                             'far_corner_sq': int(out[0, 0].item()), 'expected_far_corner_sq': (d - 1) ** 2 + (h - 1) ** 2 + (w - 1) ** 2}
    try:
        import scipy
        from scipy import ndimage
        host = target[0].reshape(SHAPE).cpu().numpy() != 0
        t0 = time.perf_counter()
        ref = ndimage.distance_transform_edt(host)
        cpu_s = time.perf_counter() - t0
        import numpy as np
        out_all = torch.empty((v, n), device=dev, dtype=torch.int32)
        edt(1, out_all)
        same = bool(np.array_equal(np.rint(ref ** 2).astype(np.uint32).reshape(-1), out_all[0].cpu().numpy().view(np.uint32)))
        rec['cpu_oracle'] = {'distance_transform_edt_s': round(cpu_s, 4), 'scipy': scipy.__version__, 'equal_to_device': same,
                             'note': 'scipy.ndimage on this host, one volume, one run'}
        rec['edt_speedup_over_cpu_oracle'] = round(cpu_s / (rec['edt_sq']['ms_per_volume'] * 1e-3), 1)
    except ImportError:
        rec['cpu_oracle'] = {'note': 'scipy is not importable on this host: not measured'}
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--timeout', type=int, default=420, help='seconds the measuring child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.child:      # the GPU step in a process of its own, under its own time limit
        try:
            return subprocess.run([sys.executable, os.path.abspath(__file__), '--child'] + sys.argv[1:], timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print('boundary_bench: the measurement did not finish within {} s'.format(args.timeout), file=sys.stderr)
            return 124
    t0 = time.time()
    rec = measure(args)
    rec['wall_s'] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
