"""Test-time augmentation against plain MC dropout at equal sample count, on BraTS-shaped volumes (160 x 4 x 192 x 128):
    TTA-MC    TtaMcPredictStep over the four flips (identity, flip_h, flip_v, rot180) x T = 5 seeded dropout passes
    plain MC  McPredictStep, T = 20
Both give 20 samples per volume (exact float64 statistics, mean + entropy as bench.py's default run; --all-outputs adds MI + variance),
without the weight-scaling pass.  Prints one JSON line with both rates in MC-sample-volumes/s and their ratio; ``--out`` also writes it.

    python tools/tta_bench.py --steps 10 --warmup 3 [--out profiles/tta_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -o tta -- python tools/tta_bench.py --steps 3 --warmup 1
    python tools/tta_bench.py --kernel-stats DIR/.../tta_results.db --traced-volumes 4 --ms-per-volume 109.4   # the TTA kernels' share
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PARAMS = dict(nb_classes=2, in_channels=4, depth=4, start_filters=32, dropout=0.05)   # bench.py's MODEL_PARAMS
FLIPS = ['identity', 'flip_h', 'flip_v', 'rot180']
TTA_KERNELS = ('tta_rows_kernel', 'tta_tile_kernel')


def kernel_times(path):
    """rocprofv3 kernel trace -> list of (kernel name, total ns, calls): the --stats CSV table or the rocpd SQLite database."""
    if path.endswith('.db'):
        import sqlite3
        with sqlite3.connect(path) as db:
            return [(n, float(t), int(c)) for n, t, c in db.execute('select name, sum(duration), count(*) from kernels group by name')]
    with open(path) as f:
        return [(row['Name'], float(row['TotalDurationNs']), int(row['Calls'])) for row in csv.DictReader(f)]


def kernel_share(path, volumes=None, ms_per_volume=None):
    """The TTA kernels' time in a trace of this tool's run (both configurations): per kernel instance, in total, per TTA-MC volume when
    ``volumes`` (TTA-MC volumes traced) is given, and as a share of a TTA-MC volume's wall time when ``ms_per_volume`` is too."""
    rows = kernel_times(path)
    total = sum(t for _, t, _ in rows)
    tta = {n: {'ms': t / 1e6, 'calls': c} for n, t, c in rows if any(k in n for k in TTA_KERNELS)}
    tta_ms = sum(v['ms'] for v in tta.values())
    out = {'trace_kernel_ms': total / 1e6, 'tta_kernels': tta, 'tta_ms': tta_ms, 'tta_share_of_trace_kernel_time': tta_ms / (total / 1e6) if total else 0.0}
    if volumes:
        out['tta_ms_per_volume'] = tta_ms / volumes
        if ms_per_volume:
            out['tta_share_of_tta_mc_volume'] = tta_ms / volumes / ms_per_volume
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--slices', type=int, default=160)
    ap.add_argument('--all-outputs', action='store_true', help='track MI and variance too (S = 5 float64 planes)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-stats', default=None, help='summarise a rocprofv3 trace of this tool (kernel_stats.csv or the rocpd .db) instead of running')
    ap.add_argument('--traced-volumes', type=int, default=None, help='with --kernel-stats: TTA-MC volumes in the trace (warmup + steps)')
    ap.add_argument('--ms-per-volume', type=float, default=None, help='with --kernel-stats: a TTA-MC volume\'s wall time (ms) of an untraced run')
    args = ap.parse_args()
    if args.kernel_stats:
        print(json.dumps(kernel_share(args.kernel_stats, args.traced_volumes, args.ms_per_volume)))
        return

    import torch
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    from rcu_amd.model import UNet

    dev = torch.device('cuda:0')
    model = UNet(**PARAMS)
    model.load_state_dict(uo.synthetic_state(1, **PARAMS))
    model = model.to(dev).eval()
    x = torch.randn(args.slices, 4, 192, 128, generator=torch.Generator().manual_seed(0)).to(dev)
    mi = var = bool(args.all_outputs)
    configs = {
        'tta_mc': lambda: steps.TtaMcPredictStep(FLIPS, mc_steps=5, seed=20, ws_pass=False, do_mi=mi, do_var=var),
        'plain_mc': lambda: steps.McPredictStep(20, seed=20, ws_pass=False, do_mi=mi, do_var=var),
    }
    ctx = steps.TorchTestContext('cuda', model)
    summary = steps.MultiPredictionSummary(do_mi=mi, do_var=var)

    def volume(step, k):
        bc = steps.BatchContext({'images': x}, k, k * args.slices)
        step(bc, None, ctx)
        summary(bc, None, ctx)
        return bc.output['probabilities']

    rates, seconds = {}, {}
    for name, make in configs.items():
        step = make()
        for k in range(args.warmup):
            volume(step, k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(args.steps):
            volume(step, args.warmup + k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        seconds[name] = dt / args.steps
        rates[name] = 20 * args.steps / dt
    record = {'metric': 'MC-sample-volumes/s', 'volume': [args.slices, 4, 192, 128], 'samples_per_volume': 20,
              'statistics': 'exact float64, ' + ('mean + entropy + MI + variance' if mi else 'mean + entropy'),
              'tta_mc': {'transforms': FLIPS, 'mc_steps': 5, 'rate': rates['tta_mc'], 'ms_per_volume': 1e3 * seconds['tta_mc']},
              'plain_mc': {'mc_steps': 20, 'rate': rates['plain_mc'], 'ms_per_volume': 1e3 * seconds['plain_mc']},
              'ratio': rates['tta_mc'] / rates['plain_mc'], 'steps': args.steps, 'warmup': args.warmup,
              'device': torch.cuda.get_device_name(dev)}
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
