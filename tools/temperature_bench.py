"""Cost of the temperature fit on one native BraTS volume (155 slices of 240 x 240, two classes, the 97 candidates of
rcu_amd.calibration.CANDIDATES):
    sweep     rcu_temperature_nll over synthetic logits, P = 1 and P = 20 passes
    fit step  the P = 20 grouped dropout forwards of the volume (calibration.pass_logits: what fit_temperature runs per batch) + the sweep
Reports the sweep's share of a P = 20 fit step and its rate of transcendental instructions (one exp and one reciprocal per
(voxel, candidate, pass) on binary models) against the issue's cost estimate of 4 per (voxel, candidate, pass) at 8 cycles per
wave-instruction.  Prints one JSON line; ``--out`` also writes it.

    python tools/temperature_bench.py --steps 5 --warmup 2 [--out profiles/temperature_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PARAMS = dict(nb_classes=2, in_channels=4, depth=4, start_filters=32, dropout=0.05)   # bench.py's MODEL_PARAMS
SLICES, H, W = 155, 240, 240
CUS, SIMDS, CLOCK_GHZ = 256, 4, 2.4            # MI355X_MICROARCH.md constants
TRANS_CYCLES = 8                               # cycles per wave-instruction of v_exp_f32 / v_log_f32 / v_rcp_f32 (the issue's bound)


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from oracle import unet_oracle as uo
    from rcu_amd import calibration as cal
    from rcu_amd.model import UNet
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(3)
    voxels = SLICES * H * W
    k = len(cal.CANDIDATES)
    target = (torch.rand(SLICES, H, W, device=dev, generator=gen) < 0.1).to(torch.uint8)
    rec = {'volume': [SLICES, H, W], 'classes': 2, 'candidates': k, 'steps': args.steps, 'warmup': args.warmup, 'sweep': {}}
    for p in (1, 20):
        logits = torch.randn(p * SLICES, 2, H, W, device=dev, generator=gen) * 4
        sweep = cal.NllSweep(dev)
        ms = timed(lambda: sweep.add(logits, target, passes=p), args.steps, args.warmup)
        sweep.sums()
        trans = 2.0 * voxels * k * p
        wave_instr = trans / 64
        bound_ms = 4 * wave_instr * TRANS_CYCLES / (CUS * SIMDS * CLOCK_GHZ * 1e9) * 1e3
        rec['sweep']['P{}'.format(p)] = {'ms': round(ms, 3), 'transcendental_per_s': trans / (ms * 1e-3),
                                         'transcendental_share_of_peak': round(wave_instr * TRANS_CYCLES / (CUS * SIMDS * CLOCK_GHZ * 1e9) / (ms * 1e-3), 4),
                                         'issue_estimate_ms': round(bound_ms, 3)}
        del logits
    torch.cuda.empty_cache()
    model = UNet(**PARAMS)
    model.load_state_dict(uo.synthetic_state(20, **PARAMS))
    model = model.to(dev).eval()
    images = torch.randn(SLICES, 4, H, W, device=dev, generator=gen)
    sweep = cal.NllSweep(dev)

    def forwards():
        return cal.pass_logits(model, images, mc_steps=20, seed=20)

    def step():
        sweep.add(forwards(), target, passes=20)

    fwd_ms = timed(forwards, args.steps, args.warmup)
    step_ms = timed(step, args.steps, args.warmup)
    sweep.sums()
    sweep_ms = rec['sweep']['P20']['ms']
    rec['fit_step'] = {'passes': 20, 'forwards_ms': round(fwd_ms, 3), 'step_ms': round(step_ms, 3), 'sweep_ms': sweep_ms,
                       'sweep_share_of_step': round(sweep_ms / step_ms, 4)}
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
