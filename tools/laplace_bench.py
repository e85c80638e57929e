#!/usr/bin/env python3
"""Time of the last-layer Laplace kernels (rcu_laplace_predict, rcu_laplace_moments; include/rcu.h "Last-layer Laplace") on one native BraTS batch,
155 x 240 x 240 voxels of F = 32 features at pitch 32, C = 2 classes.

kernels   rcu_laplace_predict (probabilities and std: 2 C floats written, C logits read) against rcu_density_energy at K = 2 with d2 -- THE
          YARDSTICK: the same quadratic forms through the same fp32 MFMA on the same feature tensor; target at most 1.5 x.  rcu_laplace_moments
          (P = 3 pairs: three B operands, one pass) against rcu_density_moments at K = 3 (three B operands, one pass): the ratio, no target.  ONE
          process, all four through the C entry points on preallocated outputs, alternated launch by launch, every path warmed up first, each
          launch between two events on the launch stream, medians.
          F = 64, C = 4 on a pitch-64 tensor (against density at K = 4) is reported with its ratios, no target.
step      the eval-mode default step (SegmentationPredictStep(do_probs=True)) on that volume (bench.py's model) against LaplacePredictStep, and
          against the default step with the classifier tap alone (what the unfused head pays), alternated.  ``--parent DIR``: the default step of
          another checkout (the parent commit, built) measured by this tool in a child process of its own, before and after this checkout's.
Every measurement runs in a child process under a time limit of its own.  Prints one JSON line; ``--out`` also writes it.

    python tools/laplace_bench.py [--reps 15] [--parent ../parent] [--out profiles/laplace_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from density_bench import H, SLICES, W, alternated, default_step, volume_and_model      # noqa: E402  (the same volume, model and timing loop)

TARGET_RATIO = 1.5


def measure_step_only(args):
    """The eval-mode default step of the checkout this process imports (``--root``)."""
    import torch
    from rcu_amd import _lib, steps
    images, model = volume_and_model(torch)
    ctx = steps.TorchTestContext('cuda:0', model)
    rec = alternated(torch, {'default_step': lambda: default_step(steps, images, ctx)}, args.reps)['default_step']
    return dict(rec, librcu=_lib.load().rcu_version().decode(), root=os.path.basename(args.root.rstrip('/')))


def synthetic_fits(laplace, density, F, C, K, seed):
    """Well-conditioned fits of the right shapes: the kernels' time does not depend on the parameters' values."""
    import numpy as np
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((1, 4096, F)) @ (rng.standard_normal((F, F)) / F ** 0.5 + np.eye(F)) + rng.standard_normal(F), 0.0)
    y = rng.integers(0, K, (1, 4096))
    n = np.stack([[(y[0] == c).sum() for c in range(K)]])
    S = np.stack([[x[0][y[0] == c].sum(0) for c in range(K)]])
    G = np.stack([[x[0][y[0] == c].T @ x[0][y[0] == c] for c in range(K)]])
    theta = rng.standard_normal((C, F + 1)) / F ** 0.5
    z = x[0] @ theta[:, :F].T + theta[:, F]
    p = np.exp(z - z.max(1, keepdims=True))
    p = (p / p.sum(1, keepdims=True)).astype(np.float32).astype(np.float64)
    pairs = laplace.pairs(C)
    om = np.stack([p[:, a] * (1 - p[:, a]) if a == b else -p[:, a] * p[:, b] for a, b in pairs], 1)
    w, Sl, Gl = om.sum(0)[None], np.einsum('vq,vi->qi', om, x[0])[None], np.einsum('vq,vi,vj->qij', om, x[0], x[0], optimize=True)[None]
    return laplace.fit_from_moments(w, Sl, Gl, theta, 1.0, 1.0), density.fit_from_moments(n, S, G)


def measure(args):
    import torch
    from rcu_amd import _lib, density, laplace, steps
    lib = _lib.load()
    dev = torch.device('cuda:0')
    voxels = SLICES * H * W
    rec = {'batch': [SLICES, H, W], 'voxels': voxels, 'reps': args.reps, 'target_ratio_predict': TARGET_RATIO, 'device': torch.cuda.get_device_name(0),
           'librcu': lib.rcu_version().decode(), 'kernels': {}}
    gen = torch.Generator(device=dev).manual_seed(5)
    for F, C, KD, KM in ((32, 2, 2, 3), (64, 4, 4, 4)):      # KD / KM: the classes of the density yardsticks of predict / moments
        P = C * (C + 1) // 2
        nhwc = torch.randn(SLICES, H, W, F, device=dev, generator=gen).abs_()
        logits = torch.randn(SLICES, C, H, W, device=dev, generator=gen) * 3
        probs = steps.softmax(logits)
        labels = torch.randint(0, KM, (SLICES, H, W), device=dev, generator=gen, dtype=torch.int64).to(torch.uint8)
        lfit, dfit = synthetic_fits(laplace, density, F, C, KD, F)
        out_p, out_s = torch.empty_like(logits), torch.empty_like(logits)
        a, b, kappa = lfit.device_parameters(dev)
        da, db, dk = dfit.device_parameters(dev)
        energy_out = torch.empty((SLICES, 1, H, W), device=dev, dtype=torch.float32)
        d2_out = torch.empty((SLICES, H, W, KD), device=dev, dtype=torch.float32)
        # the kernels through the C entry points on preallocated outputs: allocations and wrapper checks are host time, not the kernels'
        w_out = torch.empty((SLICES, P), device=dev, dtype=torch.float64)
        s_out = torch.empty((SLICES, P, F), device=dev, dtype=torch.float64)
        g_out = torch.empty((SLICES, P, F, F), device=dev, dtype=torch.float64)
        ws = torch.empty(lib.rcu_laplace_moments_workspace_bytes(SLICES, H * W, F, C) // 8, device=dev, dtype=torch.float64)
        counts = torch.empty((SLICES, KM), device=dev, dtype=torch.int64)
        ds_out = torch.empty((SLICES, KM, F), device=dev, dtype=torch.float64)
        dg_out = torch.empty((SLICES, KM, F, F), device=dev, dtype=torch.float64)
        dws = torch.empty(lib.rcu_density_moments_workspace_bytes(SLICES, H * W, F, KM) // 8, device=dev, dtype=torch.float64)

        def predict():
            _lib.check(lib.rcu_laplace_predict(_lib.ptr(nhwc), F, F, _lib.ptr(logits), SLICES, H * W, C, _lib.ptr(a), _lib.ptr(b), _lib.ptr(kappa),
                                               _lib.ptr(out_p), _lib.ptr(out_s), None, None, _lib.current_stream()))

        def density_energy():
            _lib.check(lib.rcu_density_energy(_lib.ptr(nhwc), F, F, SLICES * H * W, KD, _lib.ptr(da), _lib.ptr(db), _lib.ptr(dk), _lib.ptr(energy_out),
                                              _lib.ptr(d2_out), _lib.current_stream()))

        def moments():
            _lib.check(lib.rcu_laplace_moments(_lib.ptr(nhwc), F, F, _lib.ptr(probs), SLICES, H * W, C, _lib.ptr(w_out), _lib.ptr(s_out),
                                               _lib.ptr(g_out), _lib.ptr(ws), _lib.current_stream()))

        def density_moments():
            _lib.check(lib.rcu_density_moments(_lib.ptr(nhwc), F, F, _lib.ptr(labels), SLICES, H * W, KM, _lib.ptr(counts), _lib.ptr(ds_out),
                                               _lib.ptr(dg_out), _lib.ptr(dws), _lib.current_stream()))

        paths = {'density_energy_with_d2': density_energy, 'laplace_predict': predict,
                 'density_moments': density_moments, 'laplace_moments': moments}
        got = alternated(torch, paths, args.reps)
        for k, entry in got.items():
            entry['feature_bytes_per_s'] = voxels * F * 4 / (entry['ms_median'] * 1e-3)
        got['laplace_predict']['ratio_to_yardstick'] = round(got['laplace_predict']['ms_median'] / got['density_energy_with_d2']['ms_median'], 3)
        got['laplace_moments']['ratio_to_yardstick'] = round(got['laplace_moments']['ms_median'] / got['density_moments']['ms_median'], 3)
        if (F, C) == (32, 2):
            got['laplace_predict']['within_target'] = got['laplace_predict']['ratio_to_yardstick'] <= TARGET_RATIO
        got['yardstick_classes'] = {'density_energy_with_d2': KD, 'density_moments': KM}
        got['moments_workspace_bytes'] = ws.numel() * 8
        rec['kernels']['F{}_C{}'.format(F, C)] = got
        del nhwc, logits, probs, labels, out_p, out_s, energy_out, d2_out, w_out, s_out, g_out, ws, counts, ds_out, dg_out, dws
        torch.cuda.empty_cache()
    # the step
    images, model = volume_and_model(torch)
    ctx = steps.TorchTestContext('cuda:0', model)
    fit = synthetic_fits(laplace, density, 32, 2, 2, 1)[0]
    lstep = steps.LaplacePredictStep(fit)

    def laplace_step():
        bc = steps.BatchContext({'images': images}, 0, sample_offset=0)
        lstep(bc, None, ctx)
        return bc

    def tap_step():
        with laplace.eval_head_features(model):
            return default_step(steps, images, ctx)

    step = alternated(torch, {'default_step': lambda: default_step(steps, images, ctx), 'default_step_with_classifier_tap': tap_step,
                              'laplace_step': laplace_step}, args.reps)
    base, tap, full = (step[k]['ms_median'] for k in ('default_step', 'default_step_with_classifier_tap', 'laplace_step'))
    step.update({'added_ms': round(full - base, 4), 'added_share': round((full - base) / base, 5), 'added_ms_classifier_tap': round(tap - base, 4),
                 'added_ms_predict_kernel_minus_softmax': round(full - tap, 4), 'density_step_added_share_for_comparison': 0.061})
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
        print('laplace_bench: a measurement did not finish within {} s'.format(args.timeout), file=sys.stderr)
        return 124
    except subprocess.CalledProcessError as e:
        print('laplace_bench: a measuring process failed with status {}'.format(e.returncode), file=sys.stderr)
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
