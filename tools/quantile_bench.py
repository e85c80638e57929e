#!/usr/bin/env python3
"""Time of the quantile rescale's kernels (rcu_key_hist, rcu_quantile_apply) against the level histogram and against a sort.

On 8 x 155 x 240 x 240 float32 voxels (eight native BraTS volumes) and two inputs -- a log-normal map, and the tie-heavy one: 85 % of the
voxels on one value at random places -- these paths are timed in ONE process, alternated launch by launch, every path warmed up first, each
launch between two events on the launch stream, medians reported:
    key_hist_pass1    rcu_key_hist, shift 16, bits 16, no prefixes: the first pass of the default plan (4 bytes read per voxel)
    key_hist_pass2    rcu_key_hist, shift 0, bits 16, with the prefixes the host selects from pass 1 at Q = 1000 (4 bytes per voxel)
    quantile_apply    rcu_quantile_apply at Q = 1000 (4 read + 4 written)
    unc_hist_1000     rcu_unc_hist in its map form at B = 1000 on the same tensor: THE YARDSTICK, the one-pass kernel closest in bytes (6 per voxel)
    torch_sort        torch.sort of the same tensor: what a torch.quantile route would cost
The table the two passes give is compared with the sort's (the keys at the ranks r_k must be equal); the level histogram of the rescaled
map says how many levels are in use and what the largest holds.  ``--eval-loop K``: also the wall time per subject of `--act quantiles`
next to `--act minmax` on K synthetic native-size subjects written to a temporary directory (both wait for the .nii.gz files; quantiles
reads them twice).
The measurement runs in a child process under a time limit of its own.  Prints one JSON line; ``--out`` also writes it.

    python tools/quantile_bench.py [--reps 15] [--volumes 8] [--eval-loop 4] [--out profiles/quantile_bench.json]
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

SLICES, HEIGHT, WIDTH = 155, 240, 240      # a native BraTS volume
Q = 1000


def make_input(torch, dev, volumes, n, dist, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.exp(torch.randn((volumes, n), device=dev, generator=g) * 1.5 + 2.0)
    if dist == 'ties':
        x = torch.where(torch.rand((volumes, n), device=dev, generator=g) < 0.85, torch.full_like(x, 0.125), x)
    return x.contiguous()


def measure(args):
    import ctypes
    import numpy as np
    import torch
    from rcu_amd import _lib
    from rcu_amd import evaluation as ev
    lib = _lib.load()
    dev = torch.device('cuda:0')
    n, volumes = SLICES * HEIGHT * WIDTH, args.volumes
    stream = _lib.current_stream()
    rec = {'volume': [SLICES, HEIGHT, WIDTH], 'volumes': volumes, 'voxels': volumes * n, 'quantiles': Q, 'reps': args.reps,
           'device': torch.cuda.get_device_name(0), 'librcu': lib.rcu_version().decode(), 'cases': {}}

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for dist in ('lognormal', 'ties'):
        x = make_input(torch, dev, volumes, n, dist, seed=3 if dist == 'ties' else 2)
        zeros = torch.zeros((volumes, n), device=dev, dtype=torch.uint8)
        counts = torch.zeros(2, device=dev, dtype=torch.int64)
        hist1 = torch.zeros((1, 1 << 16), device=dev, dtype=torch.int64)
        ws1 = torch.empty(lib.rcu_key_hist_workspace_bytes(0), device=dev, dtype=torch.uint8)
        _lib.check(lib.rcu_key_hist(_lib.ptr(x), None, n, volumes, None, 0, 16, 16, _lib.ptr(hist1), _lib.ptr(counts), _lib.ptr(ws1), stream))
        total = int(counts.cpu()[1])
        ranks = ev.quantile_ranks(total, Q)
        _, inside, prefixes, slots = ev.quantile_refine(hist1.cpu().numpy(), ranks)
        table2 = (ctypes.c_uint32 * len(prefixes))(*prefixes)
        hist2 = torch.zeros((len(prefixes), 1 << 16), device=dev, dtype=torch.int64)
        ws2 = torch.empty(lib.rcu_key_hist_workspace_bytes(len(prefixes)), device=dev, dtype=torch.uint8)
        _lib.check(lib.rcu_key_hist(_lib.ptr(x), None, n, volumes, table2, len(prefixes), 0, 16, _lib.ptr(hist2), _lib.ptr(counts), _lib.ptr(ws2), stream))
        _, _, keys, at = ev.quantile_refine(hist2.cpu().numpy(), inside, slots, prefixes)
        keys = np.array([keys[s] for s in at], dtype=np.uint32)
        bounds = (ctypes.c_uint32 * (Q - 1))(*[int(k) for k in keys])
        out = torch.empty_like(x)
        ws_apply = torch.empty(lib.rcu_quantile_apply_workspace_bytes(Q), device=dev, dtype=torch.uint8)
        level_hist = torch.empty((volumes, 4, Q), device=dev, dtype=torch.int64)
        ws_hist = torch.empty(lib.rcu_unc_hist_workspace_bytes(n, volumes, Q), device=dev, dtype=torch.uint8)
        unit = torch.rand((volumes, n), device=dev)       # the yardstick's own input: a map in [0, 1] whose levels are all in use

        def pass1():
            _lib.check(lib.rcu_key_hist(_lib.ptr(x), None, n, volumes, None, 0, 16, 16, _lib.ptr(hist1), _lib.ptr(counts), _lib.ptr(ws1), stream))

        def pass2():
            _lib.check(lib.rcu_key_hist(_lib.ptr(x), None, n, volumes, table2, len(prefixes), 0, 16, _lib.ptr(hist2), _lib.ptr(counts), _lib.ptr(ws2),
                                        stream))

        def apply():
            _lib.check(lib.rcu_quantile_apply(_lib.ptr(x), volumes * n, bounds, Q, _lib.ptr(out), None, _lib.ptr(ws_apply), stream))

        def unc_hist(source):
            _lib.check(lib.rcu_unc_hist(_lib.ptr(source), 0, _lib.ptr(zeros), _lib.ptr(zeros), None, n, volumes, Q, _lib.ptr(level_hist), _lib.ptr(ws_hist),
                                        stream))

        # checks, before anything is timed: the table against the sort, and what the rescaled map's level histogram looks like
        ordered = torch.sort(x.reshape(-1)).values
        picked = ordered[torch.tensor([r - 1 for r in ranks], device=dev)].cpu().numpy()
        table_equals_sort = bool(np.array_equal(ev.float_key(picked), keys))
        del ordered
        apply()
        unc_hist(out)
        per_level = level_hist.sum(dim=(0, 1)).cpu().numpy()
        levels_used = int((per_level > 0).sum())
        largest_level_share = float(per_level.max()) / total      # (1 / Q where the values are distinct; float32 repeats values at this size)
        paths = {'key_hist_pass1': pass1, 'key_hist_pass2': pass2, 'quantile_apply': apply, 'unc_hist_1000': lambda: unc_hist(unit),
                 'torch_sort': lambda: torch.sort(x.reshape(-1))}
        for fn in paths.values():
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(args.reps):          # alternated: one launch of each path per round
            for k, fn in paths.items():
                times[k].append(event_ms(fn))
        per_voxel = {'key_hist_pass1': 4, 'key_hist_pass2': 4, 'quantile_apply': 8, 'unc_hist_1000': 6, 'torch_sort': None}
        case = {'distribution': dist, 'population': total, 'prefixes_of_pass2': len(prefixes), 'table_equals_sort': table_equals_sort,
                'levels_in_use_after_rescale': levels_used, 'largest_level_share': largest_level_share, 'all_voxels_in_a_level': int(per_level.sum()) == total,
                'share_on_the_most_common_value': float((x == x.reshape(-1)[:1024].mode().values).float().mean())}
        for k, ts in times.items():
            ms = statistics.median(ts)
            case[k] = {'ms_median': round(ms, 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4)}
            if per_voxel[k]:
                case[k].update(bytes=volumes * n * per_voxel[k], bytes_per_s=volumes * n * per_voxel[k] / (ms * 1e-3))
        for k in ('key_hist_pass1', 'key_hist_pass2', 'quantile_apply'):
            case[k]['ratio_to_unc_hist'] = round(case[k]['ms_median'] / case['unc_hist_1000']['ms_median'], 3)
            case[k]['ratio_to_sort'] = round(case[k]['ms_median'] / case['torch_sort']['ms_median'], 3)
        case['table_ms'] = round(case['key_hist_pass1']['ms_median'] + case['key_hist_pass2']['ms_median'], 4)
        case['table_ratio_to_sort'] = round(case['table_ms'] / case['torch_sort']['ms_median'], 3)
        rec['cases'][dist] = case
        del x, zeros, out, unit, hist2, level_hist
        torch.cuda.empty_cache()
    rec['all_tables_equal_the_sort'] = all(c['table_equals_sort'] and c['all_voxels_in_a_level'] for c in rec['cases'].values())
    if args.eval_loop:
        rec['eval_loop'] = eval_loop(args.eval_loop)
    return rec


def eval_loop(subjects):
    """Wall seconds per subject of `--act minmax` and of `--act quantiles` on synthetic native-size subjects (a density run in a temporary tree)."""
    import tempfile
    import numpy as np
    from rcu_amd import nifti, scripts
    rng = np.random.RandomState(4)
    shape = (SLICES, HEIGHT, WIDTH)
    out = {'subjects': subjects}
    with tempfile.TemporaryDirectory() as root:
        run_dir = os.path.join(root, 'pred')
        os.makedirs(run_dir)
        brain = np.zeros(shape, np.float32)
        brain[20:130, 40:200, 50:190] = 1.0       # about 28 % of the volume, as a skull-stripped head
        for i in range(subjects):
            sub = 'Brats18_bench_{}'.format(i)
            os.makedirs(os.path.join(root, 'gt', 'HGG', sub))
            energy = np.exp(rng.normal(2.0, 1.5, shape)).astype(np.float32) * brain
            for mod, arr in (('flair', brain), ('t1', brain), ('t2', brain), ('t1ce', brain), ('seg', (brain > 0).astype(np.uint8))):
                nifti.write(os.path.join(root, 'gt', 'HGG', sub, '{}_{}.nii.gz'.format(sub, mod)), arr)
            nifti.write(os.path.join(run_dir, '{}_density.nii.gz'.format(sub)), energy)
            nifti.write(os.path.join(run_dir, '{}_prediction.nii.gz'.format(sub)), (energy > 20).astype(np.uint8))
        for action in ('minmax', 'quantiles', 'minmax', 'quantiles'):        # alternated; the second round is reported (files in the page cache)
            t0 = time.perf_counter()
            scripts.eval_uncertainty('brats', {'density': run_dir}, os.path.join(root, 'gt'), os.path.join(root, 'eval'), actions=(action,))
            out[action + '_s_per_subject'] = round((time.perf_counter() - t0) / subjects, 3)
    out['quantiles_over_minmax'] = round(out['quantiles_s_per_subject'] / out['minmax_s_per_subject'], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--volumes', type=int, default=8)
    ap.add_argument('--eval-loop', type=int, default=0, help='subjects of the evaluation-loop measurement (0: skip it)')
    ap.add_argument('--timeout', type=int, default=540, help='seconds the measuring child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.child:      # the GPU step in a process of its own, under its own time limit
        try:
            return subprocess.run([sys.executable, os.path.abspath(__file__), '--child'] + sys.argv[1:], timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print('quantile_bench: the measurement did not finish within {} s'.format(args.timeout), file=sys.stderr)
            return 124
    t0 = time.time()
    rec = measure(args)
    rec['wall_s'] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')
    return 0 if rec['all_tables_equal_the_sort'] else 1


if __name__ == '__main__':
    sys.exit(main())
