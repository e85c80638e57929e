#!/usr/bin/env python3
"""Time of the patch table and the patch level histogram (rcu_patch_table / rcu_patch_hist) against the voxel level histogram they sit next to.

On 8 native BraTS volumes (155 x 240 x 240) of the blob-plus-islands input of tools/components_bench.py -- the prediction an ellipsoid plus
sparse islands, the target the same mask shifted by four voxels, p = 0.7..1 inside the prediction and below 0.01 outside, so nearly every
patch is pure background at one of a few dozen low levels -- the paths are timed in ONE process, alternated launch by launch, every shape warmed up first,
each launch between two events on the launch stream, medians reported:
    unc_hist_from_p_1000   rcu_unc_hist_from_p, B = 1000: THE YARDSTICK (the same 6 bytes read per voxel)
    table_1x4x4            rcu_patch_table from p, patches of 1 x 4 x 4 (6 bytes read per voxel, 32 written per patch)
    hist_1000              rcu_patch_hist of that table, B = 1000 (32 bytes read per patch)
    table_and_hist         the two together: what the 'patches' action runs per batch
and, without a target: table_4x4x4, table_16x16x16 (about 2,200 lanes per volume), hist_4096, and table_1x4x4 / hist_1000 on a uniformly
random p (no hot key).  The device histogram is compared with the host rule on the device's table at every timed input.
Target: table_and_hist at most 1.5 x the yardstick's time.  With ``--eval-subjects N`` (default 4; 0 skips it) the wall time per subject of
the evaluation loop for 'patches' beside 'ue_curves' on N native-size subjects.
The measurement runs in a child process under a time limit of its own.  Prints one JSON line; ``--out`` also writes it.

    python tools/patches_bench.py [--reps 15] [--eval-subjects 4] [--out profiles/patches_bench.json]
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if path not in sys.path:
        sys.path.insert(0, path)

from components_bench import SHAPE, VOLUMES, blob_mask      # noqa: E402  (the mask is that tool's)

TARGET_RATIO = 1.5


def measure(args):
    import numpy as np
    import torch
    from rcu_amd import _lib
    from rcu_amd import evaluation as ev
    lib = _lib.load()
    dev = torch.device('cuda:0')
    d, h, w = SHAPE
    n = d * h * w
    stream = _lib.current_stream()
    rec = {'volume': list(SHAPE), 'volumes': VOLUMES, 'voxels_per_volume': n, 'reps': args.reps, 'target_ratio': TARGET_RATIO,
           'device': torch.cuda.get_device_name(0), 'librcu': lib.rcu_version().decode(), 'cases': {}}

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    prediction = blob_mask(torch, dev, 7)
    target = torch.roll(prediction, 4, dims=3).contiguous()
    g = torch.Generator(device=dev).manual_seed(11)
    noise = torch.rand((VOLUMES,) + SHAPE, device=dev, generator=g)
    inputs = {'blob': torch.where(prediction != 0, 0.7 + 0.3 * noise, 0.01 * noise).contiguous(), 'uniform': noise}
    ws = torch.empty(lib.rcu_unc_hist_workspace_bytes(n, VOLUMES, 4096), device=dev, dtype=torch.uint8)
    ue_hist = torch.empty((VOLUMES, 4, 1000), device=dev, dtype=torch.int64)
    patches = {patch: lib.rcu_patch_count(d, h, w, *patch) for patch in ((1, 4, 4), (4, 4, 4), (16, 16, 16))}
    tables = {patch: torch.empty((VOLUMES, count, 4), device=dev, dtype=torch.int64) for patch, count in patches.items()}
    hists = {b: torch.empty((VOLUMES, 3, b), device=dev, dtype=torch.int64) for b in (1000, 4096)}

    for name, p in inputs.items():
        def yardstick():
            _lib.check(lib.rcu_unc_hist_from_p(_lib.ptr(p), _lib.ptr(prediction), _lib.ptr(target), None, n, VOLUMES, 1000, _lib.ptr(ue_hist),
                                               _lib.ptr(ws), stream))

        def table(patch):
            _lib.check(lib.rcu_patch_table(_lib.ptr(prediction), _lib.ptr(target), None, _lib.ptr(p), _lib.RCU_CC_UNC_P, d, h, w, VOLUMES, *patch,
                                           _lib.ptr(tables[patch]), stream))

        def hist(levels):
            _lib.check(lib.rcu_patch_hist(_lib.ptr(tables[(1, 4, 4)]), patches[(1, 4, 4)], VOLUMES, levels, 500, _lib.ptr(hists[levels]), stream))

        def both():
            table((1, 4, 4))
            hist(1000)

        paths = {'unc_hist_from_p_1000': yardstick, 'table_1x4x4': lambda: table((1, 4, 4)), 'hist_1000': lambda: hist(1000), 'table_and_hist': both}
        if name == 'blob':
            paths.update({'table_4x4x4': lambda: table((4, 4, 4)), 'table_16x16x16': lambda: table((16, 16, 16)), 'hist_4096': lambda: hist(4096)})
        for fn in paths.values():          # warm-up of every shape
            fn()
            fn()
        torch.cuda.synchronize()
        host_table = [t.view(ev.PATCH_DTYPE).reshape(-1) for t in tables[(1, 4, 4)].cpu().numpy().view(np.uint64)]
        equal = bool(np.array_equal(hists[1000].cpu().numpy().view(np.uint64), ev.patch_histogram_of_table(host_table, 1000, 500)))
        voxels_equal = int(tables[(1, 4, 4)][:, :, 0].sum()) == VOLUMES * n
        times = {k: [] for k in paths}
        for _ in range(args.reps):          # alternated: one launch of each path per round
            for k, fn in paths.items():
                times[k].append(event_ms(fn))
        case = {'input': name, 'device_histogram_equals_host_rule': equal, 'table_counts_every_voxel': voxels_equal,
                'share_of_patches_pure_background': float(hists[1000][:, 2, :].sum()) / (VOLUMES * patches[(1, 4, 4)]),
                'share_of_patches_in_the_fullest_key': float(hists[1000].sum(dim=0).max()) / (VOLUMES * patches[(1, 4, 4)])}
        for k, ts in times.items():
            ms = statistics.median(ts)
            case[k] = {'ms_median': round(ms, 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4)}
            if k != 'hist_1000' and k != 'hist_4096':
                case[k]['voxel_bytes_per_s'] = VOLUMES * n * 6 / (ms * 1e-3)
        yard = case['unc_hist_from_p_1000']['ms_median']
        for k in paths:
            case[k]['ratio_to_yardstick'] = round(case[k]['ms_median'] / yard, 3)
        rec['cases'][name] = case
    rec['verdict'] = {'ratio_table_and_hist': rec['cases']['blob']['table_and_hist']['ratio_to_yardstick'],
                      'within_target': rec['cases']['blob']['table_and_hist']['ratio_to_yardstick'] <= TARGET_RATIO}
    rec['all_histograms_equal'] = all(c['device_histogram_equals_host_rule'] and c['table_counts_every_voxel'] for c in rec['cases'].values())
    del inputs, noise, tables
    torch.cuda.empty_cache()
    if args.eval_subjects:
        rec['evaluation_loop'] = eval_loop(args.eval_subjects)
    return rec


def eval_loop(subjects):
    """Wall time per subject of evalrun.evaluate_runs (fused loop) for ue_curves alone, patches alone and both, on one tree."""
    import numpy as np
    from rcu_amd import evalrun, nifti
    rng = np.random.RandomState(3)
    tmp = tempfile.mkdtemp(prefix='patches_bench_')
    try:
        gt_root, run_dir = os.path.join(tmp, 'gt', 'HGG'), os.path.join(tmp, 'pred')
        os.makedirs(run_dir)
        names = ['Brats18_bench_{}_1'.format(i) for i in range(subjects)]
        z, y, x = np.ogrid[:SHAPE[0], :SHAPE[1], :SHAPE[2]]
        for i, sub in enumerate(names):
            os.makedirs(os.path.join(gt_root, sub))
            blob = ((z - 70 - 3 * i) / 28.0) ** 2 + ((y - 110 + 5 * i) / 40.0) ** 2 + ((x - 128) / 33.0) ** 2 <= 1.0
            islands = rng.rand(*SHAPE) < 0.002
            conf = np.where(blob, 0.7 + 0.3 * rng.rand(*SHAPE), np.where(islands, 0.6, 0.01 * rng.rand(*SHAPE))).astype(np.float32)
            seg = np.roll(blob | islands, 4, axis=2).astype(np.uint8)
            for mod in ('flair', 't1', 't2', 't1ce'):
                nifti.write(os.path.join(gt_root, sub, '{}_{}.nii.gz'.format(sub, mod)), blob.astype(np.float32))
            nifti.write(os.path.join(gt_root, sub, '{}_seg.nii.gz'.format(sub)), seg)
            nifti.write(os.path.join(run_dir, '{}_probabilities.nii.gz'.format(sub)), conf)
            nifti.write(os.path.join(run_dir, '{}_prediction.nii.gz'.format(sub)), (conf > 0.5).astype(np.uint8))
        entry = evalrun.get_eval_data('baseline', run_dir, evalrun.collect_brats_ground_truth(os.path.join(tmp, 'gt')), expected_subjects=names)
        out = {'subjects': subjects, 'shape': list(SHAPE)}
        for tag, acts in (('warm_up', ['ue_curves', 'patches']), ('ue_curves', ['ue_curves']), ('patches', ['patches']),
                          ('ue_curves_and_patches', ['ue_curves', 'patches'])):
            timing = {}
            t0 = time.perf_counter()
            evalrun.evaluate_runs([entry], acts, os.path.join(tmp, 'eval_' + tag), 'foreground', timing=timing)
            wall = time.perf_counter() - t0
            if tag != 'warm_up':
                out[tag] = {'wall_s_per_subject': round(wall / subjects, 4), 'upload_and_kernels_s_per_subject': round(timing['upload_and_kernels_s'] / subjects, 4),
                            'wait_for_files_s_per_subject': round(timing['wait_for_files_s'] / subjects, 4), 'csv_rows_s_per_subject': round(timing['csv_rows_s'] / subjects, 4)}
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--eval-subjects', type=int, default=4, help='subjects of the synthetic run tree of the evaluation-loop comparison (0: skip it)')
    ap.add_argument('--timeout', type=int, default=540, help='seconds the measuring child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.child:      # the GPU step in a process of its own, under its own time limit
        try:
            return subprocess.run([sys.executable, os.path.abspath(__file__), '--child'] + sys.argv[1:], timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print('patches_bench: the measurement did not finish within {} s'.format(args.timeout), file=sys.stderr)
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
