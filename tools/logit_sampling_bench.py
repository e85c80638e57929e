"""Cost of test-time logit sampling on one native BraTS volume (155 slices of 240 x 240, bench.py's model with the sigma head):
    step      AleatoricMcPredictStep(T = 20, seeded masks, logit_samples = S) + MultiPredictionSummary, S in {0, 1, 10, 50}: ms per volume
              and the ms each sampled pass adds over S = 0 (T passes + the weight-scaling pass: 21 sampled heads per volume)
    kernel    rcu_logit_sampling alone over the volume's materialised logits (S = 10): the sampling's own rate
Reports the achieved rate of vector lane-operations under the issue's estimate of 80-150 lane-operations per (voxel, sample) at C = 2
(half a Philox call, one Box-Muller pair, one two-class softmax) against the 39 T lane-ops/s the MI355X issues, and the S = 10 cost
against the target of 3 % of a T = 20 volume.  Prints one JSON line; ``--out`` also writes it.

    python tools/logit_sampling_bench.py --steps 3 --warmup 1 [--out profiles/logit_sampling_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PARAMS = dict(nb_classes=2, in_channels=4, depth=4, start_filters=32, dropout=0.05, sigma_out=True)   # bench.py's MODEL_PARAMS + sigma
SLICES, H, W, T = 155, 240, 240, 20
CUS, SIMDS, LANES, CLOCK_GHZ = 256, 4, 64, 2.4     # MI355X_MICROARCH.md constants
LANE_OPS_PEAK = CUS * SIMDS * LANES / 4 * CLOCK_GHZ * 1e9      # one wave-instruction per 4 cycles per SIMD: 39.3 T lane-ops/s
ESTIMATE = (80, 150)                                # lane-operations per (voxel, sample) at C = 2 (the issue's estimate)


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def rates(voxel_samples, ms):
    per_s = voxel_samples / (ms * 1e-3)
    return {'voxel_samples_per_s': per_s,
            'lane_ops_per_s_at_estimate': [per_s * e for e in ESTIMATE],
            'share_of_lane_op_peak_at_estimate': [round(per_s * e / LANE_OPS_PEAK, 4) for e in ESTIMATE]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    from rcu_amd.model import UNet
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(3)
    model = UNet(**PARAMS)
    model.load_state_dict(uo.synthetic_state(20, **PARAMS))
    model = model.to(dev).eval()
    images = torch.randn(SLICES, 4, H, W, device=dev, generator=gen)
    ctx = steps.TorchTestContext('cuda:0', model)
    voxels = SLICES * H * W
    rec = {'volume': [SLICES, H, W], 'classes': 2, 'mc_steps': T, 'steps': args.steps, 'warmup': args.warmup,
           'lane_op_peak_per_s': LANE_OPS_PEAK, 'estimate_lane_ops_per_voxel_sample': list(ESTIMATE), 'step': {}}

    def run(S):
        bc = steps.BatchContext({'images': images}, 0)
        steps.AleatoricMcPredictStep(T, logit_samples=S, seed=20)(bc, None, ctx)
        steps.MultiPredictionSummary()(bc, None, ctx)
        return bc

    base = None
    for S in (0, 1, 10, 50):
        ms = timed(lambda: run(S), args.steps, args.warmup)
        entry = {'ms_per_volume': round(ms, 3)}
        if S == 0:
            base = ms
        else:
            added = ms - base
            entry.update({'added_ms': round(added, 3), 'added_share': round(added / base, 4), 'added_ms_per_pass': round(added / (T + 1), 4)})
            if added > 0:
                entry.update(rates(voxels * S * (T + 1), added))
        rec['step']['S{}'.format(S)] = entry
    # the standalone kernel over materialised logits: the sampling's own rate, without the forward around it
    logits, raw = model(images)
    out = torch.empty_like(logits)
    for S in (1, 10):
        ms = timed(lambda: steps.sample_logits(logits, raw, S, 7, 0, out=out), args.steps * 4, args.warmup)
        rec['kernel_S{}'.format(S)] = dict({'ms': round(ms, 3)}, **rates(voxels * S, ms))
    s10 = rec['step']['S10']
    rec['target'] = {'S10_added_share': s10['added_share'], 'target_share': 0.03, 'review_above_share': 0.05,
                     'within_target': s10['added_share'] <= 0.03}
    rec['wall_s'] = round(time.time() - T0, 1)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')


T0 = time.time()
if __name__ == '__main__':
    main()
