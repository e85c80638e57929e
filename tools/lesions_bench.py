#!/usr/bin/env python3
"""Time of the component-pair table (rcu_cc_pairs) and of the device path of the 'lesions' action on the native BraTS batch, 8 x 155 x 240 x
240 voxels, for the two masks of tools/components_bench.py:
    blob         an ellipsoid plus sparse islands as the prediction, the same mask shifted by four voxels as the target
    serpentine   the one-voxel-wide band as the prediction against an all-ones target: ONE pair, every active wave on one slot
and on a 64^3 checkerboard under 6-connectivity paired with itself (131,072 one-voxel pairs, 64 distinct keys in every active wave).
Paths, timed in ONE process, alternated launch by launch after a warm-up, each launch between two events on the launch stream, medians:
    pairs             rcu_cc_pairs over the dense labels of prediction and target, inside = the target (9 bytes read per voxel)
    table_yardstick   rcu_cc_table with RCU_CC_UNC_NONE and other = target on the SAME predicted labels (5 bytes per voxel): THE YARDSTICK,
                      the existing pass closest in kind.  The target on the blob mask: pairs <= 1.8 x table_yardstick, the ratio of the bytes
Next to them: the whole device path of the action per volume (evaluation._lesion_tables_on_device: labelling of prediction and lesions, the
two tables, the relabelling, the pairs; merge radius 0 and 2) beside the 'components' action's (two labellings, two tables), host
synchronisations included; np.unique over one volume's stacked label pairs on this host, for scale; and, with --eval-subjects N, the wall
time per subject of the evaluation loop with `--act lesions` beside `--act components` on one synthetic tree of N native-size subjects.
The measurement runs in a child process under a time limit of its own.  Prints one JSON line; ``--out`` also writes it.

    python tools/lesions_bench.py [--reps 11] [--eval-subjects 4] [--out profiles/lesions_bench.json]
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

from components_bench import SHAPE, VOLUMES, blob_mask, serpentine_mask      # noqa: E402  (the two masks are that tool's)

BYTE_RATIO = 9 / 5


def summary(ts, v):
    ms = statistics.median(ts)
    return {'ms_median': round(ms, 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4), 'ms_per_volume': round(ms / v, 4)}


def measure(args):
    import numpy as np
    import torch
    from rcu_amd import _lib, evaluation as ev
    lib = _lib.load()
    dev = torch.device('cuda:0')
    n, v = SHAPE[0] * SHAPE[1] * SHAPE[2], VOLUMES
    stream = _lib.current_stream()
    rec = {'batch': [v] + list(SHAPE), 'voxels_per_volume': n, 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
           'librcu': lib.rcu_version().decode(), 'byte_ratio_target': BYTE_RATIO, 'masks': {}}

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def pair_paths(labels_p, ws_p, dense_p, dense_t, target, volumes, n_vox, capacity):
        table = torch.empty(lib.rcu_cc_pairs_bytes(capacity, volumes), device=dev, dtype=torch.uint8)
        counts = torch.empty(volumes, device=dev, dtype=torch.int32)
        _lib.check(lib.rcu_cc_compact(_lib.ptr(labels_p), n_vox, volumes, _lib.ptr(counts), _lib.ptr(ws_p), stream))
        total = int(counts.cpu().numpy().view('uint32').sum())
        rows = torch.empty(max(total, 1) * ev.COMPONENT_DTYPE.itemsize, device=dev, dtype=torch.uint8)

        def pairs():
            _lib.check(lib.rcu_cc_pairs(_lib.ptr(dense_p), _lib.ptr(dense_t), _lib.ptr(target), n_vox, volumes, capacity, _lib.ptr(table), stream))

        def yardstick():
            _lib.check(lib.rcu_cc_table(_lib.ptr(labels_p), _lib.ptr(target), None, _lib.RCU_CC_UNC_NONE, n_vox, volumes, _lib.ptr(ws_p), _lib.ptr(rows),
                                        total, stream))
        return {'pairs': pairs, 'table_yardstick': yardstick}, table

    def timed(paths, reps, volumes):
        for fn in paths.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(reps):
            for k, fn in paths.items():
                times[k].append(event_ms(fn))
        return {k: summary(ts, volumes) for k, ts in times.items()}

    g = torch.Generator(device=dev).manual_seed(1)
    p = torch.rand((v, n), device=dev, generator=g)
    for name in ('blob', 'serpentine'):
        if name == 'blob':
            prediction = blob_mask(torch, dev, 7)
            target = torch.roll(prediction, 4, dims=3).contiguous().reshape(v, n)
        else:
            prediction = serpentine_mask(torch, dev)
            target = torch.ones((v, n), device=dev, dtype=torch.uint8)
        prediction = prediction.reshape(v, n)
        labelling_p = ev._labelling_on_device(prediction, SHAPE, 26)
        labelling_t = ev._labelling_on_device(target, SHAPE, 26)
        dense_p, dense_t = ev._dense_of_labelling(labelling_p[0], labelling_p[2]), ev._dense_of_labelling(labelling_t[0], labelling_t[2])
        capacity = ev.pair_capacity(labelling_p[1].max(), labelling_t[1].max())
        paths, table = pair_paths(labelling_p[0], labelling_p[2], dense_p, dense_t, target, v, n, capacity)
        case = {'foreground_share': float(prediction.float().mean()), 'predicted_components_in_batch': int(labelling_p[1].sum()),
                'target_components_in_batch': int(labelling_t[1].sum()), 'capacity': capacity}
        case.update(timed(paths, args.reps, v))
        counters, tables = ev._pairs_unpack(table, capacity, v)
        case['pairs_in_batch'], case['dropped'] = int(sum(len(t) for t in tables)), int(counters[:, 1].sum())
        case['ratio_to_table_yardstick'] = round(case['pairs']['ms_median'] / case['table_yardstick']['ms_median'], 3)
        if name == 'blob':
            case['meets_byte_ratio_target'] = case['ratio_to_table_yardstick'] <= BYTE_RATIO
        # the whole device path of the two actions, host synchronisations included, alternated
        whole = {'lesions_r0': lambda: ev._lesion_tables_on_device(prediction, target, SHAPE, _lib.RCU_CC_UNC_P, p, 26, 0),
                 'lesions_r2': lambda: ev._lesion_tables_on_device(prediction, target, SHAPE, _lib.RCU_CC_UNC_P, p, 26, 2),
                 'components': lambda: (ev._component_tables_on_device(prediction, SHAPE, target, _lib.RCU_CC_UNC_P, p, 26),
                                        ev._component_tables_on_device(target, SHAPE, prediction, _lib.RCU_CC_UNC_NONE, None, 26))}
        for fn in whole.values():
            fn()
        reps = max(3, min(args.reps, 5))
        times = {k: [] for k in whole}
        for _ in range(reps):
            for k, fn in whole.items():
                times[k].append(wall_ms(fn))
        case['device_path_wall'] = {k: summary(ts, v) for k, ts in times.items()}
        # np.unique over one volume's stacked label pairs on this host
        a, b = dense_p[0].cpu().numpy().astype(np.int64), dense_t[0].cpu().numpy().astype(np.int64)
        t0 = time.perf_counter()
        both = (a > 0) & (b > 0)
        np.unique((a[both] << 32) | b[both], return_counts=True)
        case['numpy_unique_one_volume_s'] = round(time.perf_counter() - t0, 4)
        rec['masks'][name] = case
        del prediction, target, labelling_p, labelling_t, dense_p, dense_t, table, paths, whole
        torch.cuda.empty_cache()
    # the checkerboard: one 64^3 volume, 6-connectivity, paired with its own canonical labels
    z, y, x = torch.meshgrid(*(torch.arange(64, device=dev),) * 3, indexing='ij')
    board = ((z + y + x) % 2 == 0).to(torch.uint8).reshape(1, -1)
    labelling = ev._labelling_on_device(board, (64, 64, 64), 6)
    dense = ev._dense_of_labelling(labelling[0], labelling[2])
    capacity = ev.pair_capacity(labelling[1].max(), labelling[1].max())
    paths, table = pair_paths(labelling[0], labelling[2], dense, labelling[0], board, 1, 64 ** 3, capacity)
    case = {'pairs_expected': 64 ** 3 // 2, 'capacity': capacity}
    case.update(timed(paths, args.reps, 1))
    counters, tables = ev._pairs_unpack(table, capacity, 1)
    case['pairs_found'], case['dropped'] = len(tables[0]), int(counters[0, 1])
    rec['checkerboard_64'] = case
    del p
    torch.cuda.empty_cache()
    if args.eval_subjects > 0:
        rec['evaluation_loop'] = eval_loop(args.eval_subjects)
    return rec


def eval_loop(subjects):
    """Wall time per subject of evalrun.evaluate_runs (fused loop) for components alone, lesions alone and both, on one tree."""
    import numpy as np
    from rcu_amd import evalrun, nifti
    rng = np.random.RandomState(3)
    tmp = tempfile.mkdtemp(prefix='lesions_bench_')
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
        for tag, acts in (('warm_up', ['components', 'lesions']), ('components', ['components']), ('lesions', ['lesions']),
                          ('components_and_lesions', ['components', 'lesions'])):
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
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--eval-subjects', type=int, default=4, help='subjects of the synthetic run tree of the evaluation-loop comparison (0: skip it)')
    ap.add_argument('--timeout', type=int, default=540, help='seconds the measuring child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.child:      # the GPU step in a process of its own, under its own time limit
        try:
            return subprocess.run([sys.executable, os.path.abspath(__file__), '--child'] + sys.argv[1:], timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            print('lesions_bench: the measurement did not finish within {} s'.format(args.timeout), file=sys.stderr)
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
