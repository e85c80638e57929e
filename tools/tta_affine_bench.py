#!/usr/bin/env python3
"""Time of the affine test-time augmentation (rcu_warp_affine, rcu_mc_accumulate_warped; include/rcu_warp.h) on one native BraTS batch,
155 x 4 x 240 x 240, at 10 degrees / scale 1.1.

warp        rcu_warp_affine with one matrix against rcu_tta_transform(flip_h) on the same tensor -- THE YARDSTICK: both move the same 8 bytes
            per element -- in ONE process, alternated launch by launch, every path warmed up first, each launch between two events on the launch
            stream, medians reported.  No target: the ratio is reported.  The identity matrix is timed beside it (the same kernel, coalesced taps).
accumulate  rcu_mc_accumulate_warped with one group and EXACT|MI against rcu_mc_accumulate on the same logits and the same kind of blob; the
            probability form and four groups in one call beside it.
step        AffineTtaMcPredictStep at V = 4, T = 5 against TtaMcPredictStep with the four flips x 5, both followed by MultiPredictionSummary
            (bench.py's model), alternated.
``--library PATH``: the two kernels once more from another build of the library (csrc/Makefile: BUILD= / OUT= / EXTRA=-DRCU_WARP_BX=64
-DRCU_WARP_BY=4, the row footprint), in a process of its own.  ``--parent DIR``: ``bench.py --gpus 1 --steps 20 --warmup 5`` of this checkout and
of a built checkout of the parent commit, alternated, two runs each.
Every measurement runs in a child process under a time limit of its own.  Prints one JSON line; ``--out`` also writes it.

    python tools/tta_affine_bench.py [--reps 15] [--library ../librcu_hip_rows.so] [--parent ../parent] [--out profiles/tta_affine_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from density_bench import C, H, SLICES, W, alternated, volume_and_model  # noqa: E402

ROTATION, SCALE = 10.0, 1.1
CLASSES = 2


def measure_kernels(torch, reps):
    from rcu_amd import _lib, steps
    lib, dev = _lib.load(), torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(SLICES, C, H, W, device=dev, generator=gen)
    out = torch.empty((1, SLICES, C, H, W), device=dev, dtype=torch.float32)
    forward = steps.affine_matrix(ROTATION, SCALE)
    mats = {name: torch.from_numpy(steps._affine_array(m)).to(dev) for name, m in
            (('warp', forward), ('identity', steps.AFFINE_IDENTITY), ('back', steps.affine_inverse(forward)),
             ('back4', [steps.affine_inverse(forward)] * 4))}
    stream = _lib.current_stream

    def warp(name):
        _lib.check(lib.rcu_warp_affine(_lib.ptr(x), SLICES, C, H, W, _lib.ptr(mats[name]), 1, _lib.ptr(out), stream()))

    def flip():
        _lib.check(lib.rcu_tta_transform(_lib.ptr(x), SLICES, C, H, W, 1, _lib.ptr(out), stream()))

    got = alternated(torch, {'tta_transform_flip_h': flip, 'warp_affine': lambda: warp('warp'), 'warp_affine_identity': lambda: warp('identity')}, reps)
    yard = got['tta_transform_flip_h']['ms_median']
    moved = SLICES * C * H * W * 8.0
    for entry in got.values():
        entry['ratio_to_yardstick'] = round(entry['ms_median'] / yard, 3)
        entry['bytes_per_s'] = moved / (entry['ms_median'] * 1e-3)
    rec = {'warp': got}
    del x, out
    torch.cuda.empty_cache()

    logits = torch.randn(4, SLICES, CLASSES, H, W, device=dev, generator=gen)
    probs = torch.softmax(logits, 2)
    stats = steps.McStatistics(SLICES, CLASSES, H, W, dev, do_mi=True, exact=True)
    flags = stats.flags

    def accumulate():
        _lib.check(lib.rcu_mc_accumulate(_lib.ptr(logits), _lib.ptr(stats.blob), SLICES, H * W, CLASSES, flags, stream()))

    def warped(src, name, groups, more=0):
        _lib.check(lib.rcu_mc_accumulate_warped(_lib.ptr(src), _lib.ptr(stats.blob), SLICES, H, W, CLASSES, flags | more, _lib.ptr(mats[name]), groups,
                                                stream()))

    got = alternated(torch, {'mc_accumulate': accumulate, 'mc_accumulate_warped': lambda: warped(logits, 'back', 1),
                             'mc_accumulate_warped_identity': lambda: warped(logits, 'identity', 1),
                             'mc_accumulate_warped_from_probs': lambda: warped(probs, 'back', 1, _lib.RCU_MC_INPUT_PROBS),
                             'mc_accumulate_warped_4_groups': lambda: warped(logits, 'back4', 4)}, reps)
    yard = got['mc_accumulate']['ms_median']
    for entry in got.values():
        entry['ratio_to_yardstick'] = round(entry['ms_median'] / yard, 3)
    rec['accumulate'] = got
    rec['accumulate']['flags'] = 'EXACT|MI'
    return rec


def measure(args):
    import torch
    from rcu_amd import _lib, steps
    rec = {'batch': [SLICES, C, H, W], 'classes': CLASSES, 'rotation_deg': ROTATION, 'scale': SCALE, 'reps': args.reps,
           'device': torch.cuda.get_device_name(0), 'librcu': _lib.load().rcu_version().decode(), 'library': os.path.basename(_lib.LIB_PATH)}
    if not args.only_step:
        rec.update(measure_kernels(torch, args.reps))
    if args.kernels_only:
        return rec
    torch.cuda.empty_cache()
    images, model = volume_and_model(torch)
    ctx = steps.TorchTestContext('cuda:0', model)
    affine = steps.AffineTtaMcPredictStep(4, mc_steps=5, seed=20, rotation=ROTATION, scale=SCALE - 1.0)
    flips = steps.TtaMcPredictStep(['identity', 'flip_h', 'flip_v', 'rot180'], mc_steps=5, seed=20)
    summary = steps.MultiPredictionSummary()

    def run(step):
        bc = steps.BatchContext({'images': images}, 0, sample_offset=0)
        step(bc, None, ctx)
        summary(bc, None, ctx)
        return bc

    paths = {'tta_d4_step': lambda: run(flips), 'tta_affine_step': lambda: run(affine)}
    if args.only_step:      # one of the two alone, for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/tta_affine_bench.py --child ...
        rec['step'] = alternated(torch, {args.only_step: paths[args.only_step]}, args.reps)
        return rec
    got = alternated(torch, paths, args.reps)
    got['V'], got['T'] = 4, 5
    got['ratio'] = round(got['tta_affine_step']['ms_median'] / got['tta_d4_step']['ms_median'], 4)
    got['pass_group_size'] = steps.pass_group_size(model, SLICES, H, W, affine.group_pixels)
    rec['step'] = got
    return rec


def child(root, extra, timeout, env=None):
    """This tool's measurement from the checkout ``root``, in a process of its own under a time limit -> its JSON record."""
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--root', root] + extra
    done = subprocess.run(cmd, timeout=timeout, stdout=subprocess.PIPE, check=True, cwd=root, env=env)
    return json.loads(done.stdout.decode().strip().splitlines()[-1])


def headline(root, timeout):
    """``bench.py --gpus 1 --steps 20 --warmup 5`` of the checkout ``root`` -> its JSON result line."""
    done = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '20', '--warmup', '5'], timeout=timeout, stdout=subprocess.PIPE,
                          check=True, cwd=root)
    lines = [line for line in done.stdout.decode().splitlines() if line.startswith('{')]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--library', default=None, help='another build of librcu_hip.so: the two kernels are timed from it too')
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: bench.py is run from both, alternated')
    ap.add_argument('--timeout', type=int, default=420, help='seconds each measuring child process may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--root', default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--kernels-only', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--only-step', choices=('tta_d4_step', 'tta_affine_step'), default=None,
                    help='with --child: run this step alone, --reps times after the warm-up (the program of a kernel trace)')
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, os.path.abspath(args.root))
        print(json.dumps(measure(args)))
        return 0
    t0 = time.time()
    reps = ['--reps', str(args.reps)]
    root = os.path.abspath(args.root)
    try:
        rec = child(root, reps, args.timeout)
        if args.library:
            env = dict(os.environ, RCU_HIP_LIBRARY=os.path.abspath(args.library))
            rec['other_build'] = child(root, reps + ['--kernels-only'], args.timeout, env)
        if args.parent:
            parent = os.path.abspath(args.parent)
            runs = [(name, headline(where, args.timeout)) for name, where in (('this', root), ('parent', parent), ('this', root), ('parent', parent))]
            rec['headline'] = [dict(checkout=name, value=r.get('value'), metric=r.get('metric'), unit=r.get('unit')) for name, r in runs]
    except subprocess.TimeoutExpired:
        print('tta_affine_bench: a measurement did not finish within {} s'.format(args.timeout), file=sys.stderr)
        return 124
    except subprocess.CalledProcessError as e:
        print('tta_affine_bench: a measuring process failed with status {}'.format(e.returncode), file=sys.stderr)
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
