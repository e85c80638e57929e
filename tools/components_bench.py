#!/usr/bin/env python3
"""Time of the connected-component labelling and of the per-component table (rcu_cc_label, rcu_cc_compact, rcu_cc_table) on the native BraTS
batch, 8 x 155 x 240 x 240 voxels, for two masks:
    blob         an ellipsoid of about 1.7e5 voxels per volume plus sparse islands (0.2 % of the voxels): a whole-tumour prediction
    serpentine   a one-voxel-wide band through the whole volume (every other row of every other plane, joined at alternating ends): the
                 longest union chains a volume of this size can hold
Paths, timed in ONE process, alternated launch by launch after a warm-up of every shape, each launch between two events on the launch
stream, medians reported (per batch and per volume):
    label             rcu_cc_label, 26-connectivity (and 6, once)
    compact           rcu_cc_compact: the ranks of the roots
    table             rcu_cc_table with the other map and the in-register entropy of a float32 probability map
    unc_hist_from_p   rcu_unc_hist_from_p at B = 1000 on the same voxels: THE YARDSTICK of a one-pass kernel (6 bytes read per voxel)
The device path that replaces the CPU oracle is label + compact + table (uploads excluded).  The oracle, scipy.ndimage.label + sum_labels on
one volume of the same mask, is timed on this host when scipy is importable; else the figures measured on the CPU-only development box are
quoted and marked as such.  With --eval-subjects N the per-subject time of the evaluation loop with `--act components` is put next to
`--act ue_curves` on one synthetic run tree of N native-size subjects.
The measurement runs in a child process under a time limit of its own.  Prints one JSON line; ``--out`` also writes it.

    python tools/components_bench.py [--reps 11] [--eval-subjects 4] [--out profiles/components_bench.json]
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
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

VOLUMES, SHAPE = 8, (155, 240, 240)
QUOTED_CPU = {'label_s': 0.12, 'sum_labels_s': 0.25, 'components': 8300, 'note': 'measured on the CPU-only development box, not on this host'}


def blob_mask(torch, dev, seed):
    d, h, w = SHAPE
    g = torch.Generator(device=dev).manual_seed(seed)
    z = torch.arange(d, device=dev).view(d, 1, 1).float()
    y = torch.arange(h, device=dev).view(1, h, 1).float()
    x = torch.arange(w, device=dev).view(1, 1, w).float()
    out = torch.empty((VOLUMES,) + SHAPE, device=dev, dtype=torch.uint8)
    for v in range(VOLUMES):
        blob = ((z - 70 - 3 * v) / 28.0) ** 2 + ((y - 110 + 5 * v) / 40.0) ** 2 + ((x - 128) / (33.0 + v)) ** 2 <= 1.0
        out[v] = (blob | (torch.rand(SHAPE, device=dev, generator=g) < 0.002)).to(torch.uint8)
    return out


def serpentine_mask(torch, dev):
    d, h, w = SHAPE
    m = torch.zeros(SHAPE, device=dev, dtype=torch.uint8)
    m[::2, ::2, :] = 1
    for j, y in enumerate(range(1, h - 1, 2)):
        m[::2, y, (w - 1) if j % 2 == 0 else 0] = 1
    m[1:d - 1:2, 0, 0] = 1
    return m.unsqueeze(0).repeat(VOLUMES, 1, 1, 1).contiguous()


def measure(args):
    import torch
    from rcu_amd import _lib, evaluation as ev
    lib = _lib.load()
    dev = torch.device('cuda:0')
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    v = VOLUMES
    stream = _lib.current_stream()
    rec = {'batch': [v] + list(SHAPE), 'voxels_per_volume': n, 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
           'librcu': lib.rcu_version().decode(), 'masks': {}}

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    g = torch.Generator(device=dev).manual_seed(1)
    p = torch.rand((v, n), device=dev, generator=g)
    target = (torch.rand((v, n), device=dev, generator=g) < 0.3).to(torch.uint8)
    labels = torch.empty((v, n), device=dev, dtype=torch.int32)
    counts = torch.empty(v, device=dev, dtype=torch.int32)
    ws = torch.empty(lib.rcu_cc_workspace_bytes(n, v), device=dev, dtype=torch.uint8)
    hist = torch.empty((v, 4, 1000), device=dev, dtype=torch.int64)
    ws_hist = torch.empty(lib.rcu_unc_hist_workspace_bytes(n, v, 1000), device=dev, dtype=torch.uint8)
    try:
        import scipy
        from scipy import ndimage
    except ImportError:
        scipy = ndimage = None

    for name in ('blob', 'serpentine'):
        mask = (blob_mask(torch, dev, 7) if name == 'blob' else serpentine_mask(torch, dev)).reshape(v, n)

        def label(conn=26):
            _lib.check(lib.rcu_cc_label(_lib.ptr(mask), SHAPE[0], SHAPE[1], SHAPE[2], v, conn, _lib.ptr(labels), stream))

        def compact():
            _lib.check(lib.rcu_cc_compact(_lib.ptr(labels), n, v, _lib.ptr(counts), _lib.ptr(ws), stream))

        first_ms = event_ms(label)                 # (printed at once: the adversarial mask is the one that could be slow)
        print('components_bench: {} first label launch {:.2f} ms'.format(name, first_ms), file=sys.stderr, flush=True)
        compact()
        total = int(counts.cpu().numpy().view('uint32').sum())
        table = torch.empty(max(total, 1) * ev.COMPONENT_DTYPE.itemsize, device=dev, dtype=torch.uint8)

        def fill_table():
            _lib.check(lib.rcu_cc_table(_lib.ptr(labels), _lib.ptr(target), _lib.ptr(p), _lib.RCU_CC_UNC_P, n, v, _lib.ptr(ws), _lib.ptr(table),
                                        total, stream))

        def hist_from_p():
            _lib.check(lib.rcu_unc_hist_from_p(_lib.ptr(p), _lib.ptr(mask), _lib.ptr(target), None, n, v, 1000, _lib.ptr(hist), _lib.ptr(ws_hist), stream))

        paths = {'label': label, 'compact': compact, 'table': fill_table, 'unc_hist_from_p': hist_from_p}
        for fn in paths.values():
            fn()
        torch.cuda.synchronize()
        reps = args.reps if name == 'blob' else max(3, min(args.reps, 5))
        times = {k: [] for k in paths}
        for _ in range(reps):                      # alternated: one launch of each path per round (label first: compact and table need it)
            for k, fn in paths.items():
                times[k].append(event_ms(fn))
        case = {'foreground_share': float(mask.float().mean()), 'components_in_batch': total, 'first_label_launch_ms': round(first_ms, 3),
                'label_6_ms': round(event_ms(lambda: label(6)), 4), 'reps': reps}
        label()
        for k, ts in times.items():
            ms = statistics.median(ts)
            case[k] = {'ms_median': round(ms, 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4), 'ms_per_volume': round(ms / v, 4)}
        device_ms = sum(case[k]['ms_median'] for k in ('label', 'compact', 'table'))
        case['label_compact_table_ms_per_volume'] = round(device_ms / v, 4)
        case['ratio_to_unc_hist_from_p'] = round(device_ms / case['unc_hist_from_p']['ms_median'], 2)
        if ndimage is not None:                    # the oracle on one volume of the same mask, on this host
            host = mask[0].reshape(SHAPE).cpu().numpy() != 0
            unc = ev.normalised_entropy(p[0]).cpu().numpy().reshape(SHAPE)
            t0 = time.perf_counter()
            lab, k = ndimage.label(host, structure=ndimage.generate_binary_structure(3, 3))
            t1 = time.perf_counter()
            ndimage.sum_labels(unc, lab, range(1, k + 1))
            t2 = time.perf_counter()
            case['cpu_oracle'] = {'label_s': round(t1 - t0, 4), 'sum_labels_s': round(t2 - t1, 4), 'components': int(k), 'scipy': scipy.__version__,
                                  'note': 'scipy.ndimage on this host, one volume, one run'}
        else:
            case['cpu_oracle'] = dict(QUOTED_CPU)
        cpu_s = case['cpu_oracle']['label_s'] + case['cpu_oracle']['sum_labels_s']
        case['speedup_over_cpu_oracle'] = round(cpu_s / (device_ms / v * 1e-3), 1)
        case['faster_than_cpu_oracle'] = device_ms / v * 1e-3 < cpu_s
        rec['masks'][name] = case
        del mask, table
        torch.cuda.empty_cache()
    del labels, ws, p, target
    torch.cuda.empty_cache()
    if args.eval_subjects > 0:
        rec['evaluation_loop'] = eval_loop(args.eval_subjects)
    return rec


def eval_loop(subjects):
    """Wall time per subject of evalrun.evaluate_runs (fused loop) for ue_curves alone, components alone and both, on one tree."""
    import numpy as np
    from rcu_amd import evalrun, nifti
    rng = np.random.RandomState(3)
    tmp = tempfile.mkdtemp(prefix='components_bench_')
    try:
        gt_root, run_dir = os.path.join(tmp, 'gt', 'HGG'), os.path.join(tmp, 'pred')
        os.makedirs(run_dir)
        names = ['Brats18_bench_{}_1'.format(i) for i in range(subjects)]
        z, y, x = np.ogrid[:SHAPE[0], :SHAPE[1], :SHAPE[2]]
        for i, sub in enumerate(names):
            os.makedirs(os.path.join(gt_root, sub))
            blob = ((z - 70 - 3 * i) / 28.0) ** 2 + ((y - 110 + 5 * i) / 40.0) ** 2 + ((x - 128) / 33.0) ** 2 <= 1.0
            conf = np.where(blob, 0.7 + 0.3 * rng.rand(*SHAPE), np.where(rng.rand(*SHAPE) < 0.002, 0.6, 0.01 * rng.rand(*SHAPE))).astype(np.float32)
            seg = np.roll(blob, 4, axis=2).astype(np.uint8)
            for mod in ('flair', 't1', 't2', 't1ce'):
                nifti.write(os.path.join(gt_root, sub, '{}_{}.nii.gz'.format(sub, mod)), blob.astype(np.float32))
            nifti.write(os.path.join(gt_root, sub, '{}_seg.nii.gz'.format(sub)), seg)
            nifti.write(os.path.join(run_dir, '{}_probabilities.nii.gz'.format(sub)), conf)
            nifti.write(os.path.join(run_dir, '{}_prediction.nii.gz'.format(sub)), (conf > 0.5).astype(np.uint8))
        entry = evalrun.get_eval_data('baseline', run_dir, evalrun.collect_brats_ground_truth(os.path.join(tmp, 'gt')), expected_subjects=names)
        out = {'subjects': subjects, 'shape': list(SHAPE)}
        for tag, acts in (('warm_up', ['ue_curves', 'components']), ('ue_curves', ['ue_curves']), ('components', ['components']),
                          ('ue_curves_and_components', ['ue_curves', 'components'])):
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
            print('components_bench: the measurement did not finish within {} s'.format(args.timeout), file=sys.stderr)
            return 124
    t0 = time.time()
    rec = measure(args)
    rec['wall_s'] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')
    return 0 if all(c['faster_than_cpu_oracle'] for c in rec['masks'].values()) else 1


if __name__ == '__main__':
    sys.exit(main())
