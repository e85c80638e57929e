#!/usr/bin/env python3
"""Time of the nearest-neighbour feature uncertainty (rcu_knn_distances, rcu_knn_sample_keys; include/rcu_knn.h) on one native BraTS batch,
155 x 240 x 240 voxels of F = 32 features at pitch 32.

kernels   rcu_knn_distances at M = 256 (k = 1 and k = 8) against rcu_density_energy at K = 8 on the same feature tensor -- THE YARDSTICK: it runs
          eight 32-row blocks per voxel group through the same fp32 MFMA, as k-NN at M = 256 does -- in ONE process, alternated launch by launch,
          every path warmed up first, each launch between two events on the launch stream, medians reported.  No target: the ratio is reported.
          At M = 2048: the time at k = 1, 5 and 8 and without normalisation, and the fraction of the fp32 MFMA peak (157.3 TFLOP/s; the product is
          voxels x M x 64 FLOP) -- what the k = 8 run adds over k = 1 is the selection's VALU work, what remains over the MFMA issue time
          (FLOP / peak) is issue gaps, the bank's staging and the selection at k = 1.  The keys of the batch are timed beside them.
step      the eval-mode default step (SegmentationPredictStep(do_probs=True)) on that volume (bench.py's model) against KnnPredictStep at M = 2048,
          k = 5, and against the default step with the feature tap alone (what provide_features pays regardless), alternated.  ``--parent DIR``:
          the default step of another checkout (the parent commit, built) measured by this tool in a child process of its own, before and after
          this checkout's.
Every measurement runs in a child process under a time limit of its own.  Prints one JSON line; ``--out`` also writes it.

    python tools/knn_bench.py [--reps 15] [--parent ../parent] [--out profiles/knn_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from density_bench import H, SLICES, W, alternated, default_step, synthetic_fit, volume_and_model  # noqa: E402

FP32_MFMA_PEAK = 157.3e12


def measure_step_only(args):
    """The eval-mode default step of the checkout this process imports (``--root``)."""
    import torch
    from rcu_amd import _lib, steps
    images, model = volume_and_model(torch)
    ctx = steps.TorchTestContext('cuda:0', model)
    rec = alternated(torch, {'default_step': lambda: default_step(steps, images, ctx)}, args.reps)['default_step']
    return dict(rec, librcu=_lib.load().rcu_version().decode(), root=os.path.basename(args.root.rstrip('/')))


def synthetic_bank(knn, M, F, normalize, seed):
    """A bank of the right shape from post-ReLU-like rows: the kernel's time depends on the values only through the selection's insertions."""
    import numpy as np
    rng = np.random.default_rng(seed)
    rows = np.maximum(rng.normal(0.3, 1.0, (M, F)), 0.0).astype(np.float32)
    return knn.KnnBank(rows, np.zeros(M, np.uint8), np.arange(M, dtype=np.int64), np.zeros(M, np.int64), np.arange(M, dtype=np.int64),
                       normalize=normalize, per_class=(M,), seed=0)


def measure(args):
    import torch
    from rcu_amd import _lib, density, knn, steps
    lib = _lib.load()
    dev = torch.device('cuda:0')
    voxels, F = SLICES * H * W, 32
    rec = {'batch': [SLICES, H, W], 'voxels': voxels, 'F': F, 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
           'librcu': lib.rcu_version().decode(), 'fp32_mfma_peak_flops': FP32_MFMA_PEAK}
    gen = torch.Generator(device=dev).manual_seed(5)
    nhwc = torch.relu(torch.randn(SLICES, H, W, F, device=dev, generator=gen) + 0.3)
    feats = nhwc.permute(0, 3, 1, 2)                       # the view UNet.features hands out: read in place
    fit8 = synthetic_fit(torch, density, F, 8, F)
    small, large, plain = synthetic_bank(knn, 256, F, True, 1), synthetic_bank(knn, 2048, F, True, 2), synthetic_bank(knn, 2048, F, False, 2)
    index = torch.arange(SLICES, device=dev, dtype=torch.int64)
    paths = {'density_energy_K8': lambda: density.energy(fit8, feats),
             'knn_M256_k1': lambda: knn.distances(small, feats, 1), 'knn_M256_k8': lambda: knn.distances(small, feats, 8),
             'knn_M2048_k1': lambda: knn.distances(large, feats, 1), 'knn_M2048_k5': lambda: knn.distances(large, feats, 5),
             'knn_M2048_k8': lambda: knn.distances(large, feats, 8), 'knn_M2048_k5_not_normalized': lambda: knn.distances(plain, feats, 5),
             'knn_M2048_k5_with_neighbours': lambda: knn.distances(large, feats, 5, with_neighbours=True),
             'sample_keys': lambda: knn.sample_keys(SLICES, H * W, index, 0)}
    got = alternated(torch, paths, args.reps)
    yard = got['density_energy_K8']['ms_median']
    for name, entry in got.items():
        entry['ratio_to_yardstick'] = round(entry['ms_median'] / yard, 3)
        if name.startswith('knn_M'):
            m = int(name.split('_')[1][1:])
            flops = voxels * m * 64.0
            entry['flops'] = flops
            entry['mfma_issue_ms'] = round(flops / FP32_MFMA_PEAK * 1e3, 4)
            entry['fraction_of_fp32_mfma_peak'] = round(flops / (entry['ms_median'] * 1e-3) / FP32_MFMA_PEAK, 4)
    rec['kernels'] = got
    del nhwc, feats
    torch.cuda.empty_cache()
    # the step
    images, model = volume_and_model(torch)
    ctx = steps.TorchTestContext('cuda:0', model)
    kstep = steps.KnnPredictStep(large, 5)

    def knn_step():
        bc = steps.BatchContext({'images': images}, 0, sample_offset=0)
        kstep(bc, None, ctx)
        return bc

    def tap_step():
        with density.eval_features(model):
            return default_step(steps, images, ctx)

    step = alternated(torch, {'default_step': lambda: default_step(steps, images, ctx), 'default_step_with_feature_tap': tap_step,
                              'knn_step': knn_step}, args.reps)
    base, tap, full = (step[k]['ms_median'] for k in ('default_step', 'default_step_with_feature_tap', 'knn_step'))
    step.update({'M': 2048, 'k': 5, 'added_ms': round(full - base, 4), 'added_share': round((full - base) / base, 5),
                 'added_ms_feature_tap': round(tap - base, 4), 'added_ms_distance_kernel': round(full - tap, 4)})
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
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: its default step is measured too')
    ap.add_argument('--timeout', type=int, default=420, help='seconds each measuring child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--root', default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--step-only', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, os.path.abspath(args.root))
        print(json.dumps(measure_step_only(args) if args.step_only else measure(args)))
        return 0
    t0 = time.time()
    reps = ['--reps', str(args.reps)]
    try:
        parent = [child(os.path.abspath(args.parent), reps + ['--step-only'], args.timeout)] if args.parent else []
        rec = child(os.path.abspath(args.root), reps, args.timeout)
        if args.parent:
            parent.append(child(os.path.abspath(args.parent), reps + ['--step-only'], args.timeout))
            rec['step']['parent_commit_default_step'] = parent
            rec['step']['this_checkout_default_step_only'] = child(os.path.abspath(args.root), reps + ['--step-only'], args.timeout)
    except subprocess.TimeoutExpired:
        print('knn_bench: a measurement did not finish within {} s'.format(args.timeout), file=sys.stderr)
        return 124
    except subprocess.CalledProcessError as e:
        print('knn_bench: a measuring process failed with status {}'.format(e.returncode), file=sys.stderr)
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
