"""The protocol of tests/stream_order.py one layer up: the Python wrappers under ``torch.cuda.stream(side)``, behind the delay.  Here the wrapper
allocates its outputs, temporaries and host arrays itself; the inputs are device tensors that hold poison until the copy of the real values, queued
on ``side`` behind the delay, has run.  The expected value is the same wrapper on the default stream of a synchronised device, bit for bit."""
import numpy as np
import torch

import stream_order as so
from stream_order import N, VOL, f32, prob, rng, u8

# wrapper -> why it returns with the stream drained (no query() assertion; the bytes are still compared)
_TO_HOST = 'returns host arrays: it waits for its own result (.cpu())'
BLOCKS_THE_HOST = {
    'evaluation.calibration_histogram': _TO_HOST,
    'evaluation.uncertainty_counts': _TO_HOST,
    'evaluation.uncertainty_counts_from_p': _TO_HOST,
    'evaluation.uncertainty_histogram': _TO_HOST,
    'evaluation.calibration_levels': _TO_HOST,
    'evaluation.patch_table': _TO_HOST,
    'evaluation.patch_histogram': _TO_HOST,
    'evaluation.component_pairs': 'reads the largest labels and every table\'s dropped counter on the host: one wait per try of its retry loop',
}

WRAPPERS = {}
_models, _fits = {}, {}


def wrapper(name):
    def register(build):
        WRAPPERS[name] = build
        return build
    return register


def _host_bytes(values):
    out = []
    for v in values:
        if torch.is_tensor(v):
            out.append(so.as_bytes(v).cpu())
        else:
            out.append(torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()))
    return out


def _keep(values):
    return [v.clone() if torch.is_tensor(v) else v for v in values]


def run_plain(row):
    row.reset()
    torch.cuda.synchronize()
    row.fill()
    torch.cuda.synchronize()
    kept = _keep(row.call(None))
    torch.cuda.synchronize()
    return _host_bytes(kept)


def run_behind_delay(row, side, delay):
    row.reset()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        delay.enqueue()
        row.fill()
        values = row.call(None)
        idle = side.query()
        kept = _keep(values)
    side.synchronize()
    torch.cuda.synchronize()
    return _host_bytes(kept), idle


# ---- models: made once, warm by the time the protocol runs (the quiet-stream call comes first)
PARAMS = dict(nb_classes=2, in_channels=4, depth=4, start_filters=32, dropout=0.05)
H, W = 48, 32


def _model(dev, **extra):
    from oracle import unet_oracle as uo
    from rcu_amd.model import UNet
    key = tuple(sorted(extra.items()))
    if key not in _models:
        params = dict(PARAMS, **extra)
        model = UNet(**params)
        model.load_state_dict(uo.sensitive_state(22, **params))
        _models[key] = model.to(dev)
    return _models[key]


def _images(row, tag):
    return row.inp(f32(rng('wrapper', tag), N, 4, H, W))


def _context(dev, model):
    from rcu_amd import steps
    return steps.TorchTestContext(str(dev), model)


def _outputs(bc):
    return [bc.output[k] for k in sorted(bc.output) if torch.is_tensor(bc.output[k])]


@wrapper('UNet.__call__ eval')
def _unet_eval(dev):
    row = so.Row(dev)
    model, x = _model(dev), _images(row, 'eval')
    row.call = lambda s: [model(x)]
    return row


@wrapper('UNet.__call__ masks')
def _unet_masks(dev):
    row = so.Row(dev)
    model, x = _model(dev), _images(row, 'masks')
    r = rng('wrapper', 'mask factors')
    masks = row.inp(np.concatenate([((r.random_sample((N, c)) < 0.7) / 0.7).astype(np.float32).reshape(-1) for _, c in model.dropout_sites()]))
    row.call = lambda s: [model(x, masks)]
    return row


@wrapper('McPredictStep lanes=2 + MultiPredictionSummary')
def _mc_step(dev):
    """Four seeded passes, one per launch, over two stream lanes: StreamLanes has to fork from and join back to the CALLER's stream."""
    from rcu_amd import steps
    row = so.Row(dev)
    model, x = _model(dev), _images(row, 'mc')

    def call(s):
        bc = steps.BatchContext({'images': x}, 0, 40)
        ctx = _context(dev, model)
        steps.McPredictStep(4, do_mi=True, do_var=True, lanes=2, seed=11, group_pixels=N * H * W)(bc, None, ctx)
        steps.MultiPredictionSummary(do_mi=True, do_var=True)(bc, None, ctx)
        return _outputs(bc)
    row.call = call
    return row


@wrapper('McStatistics accumulate + finalize')
def _mc_statistics(dev):
    from rcu_amd import steps
    row = so.Row(dev)
    r = rng('wrapper', 'stats')
    a, b = row.inp(f32(r, N, 3, 25, 40)), row.inp(f32(r, N, 3, 25, 40))

    def call(s):
        stats = steps.McStatistics(N, 3, 25, 40, dev, do_mi=True, do_var=True, exact=True)
        stats.accumulate(a)
        stats.accumulate(b)
        out = stats.finalize(do_mi=True, do_var=True)
        return [stats.blob] + [out[k] for k in sorted(out)]
    row.call = call
    return row


def _maps(row, tag, npv=1001):
    r = rng('wrapper', tag)
    return (row.inp(prob(r, N, npv)), row.inp(u8(r, (N, npv), 0.4)), row.inp(u8(r, (N, npv), 0.4)), row.inp(u8(r, (N, npv), 0.8)))


@wrapper('evaluation.calibration_histogram')
def _calibration_histogram(dev):
    from rcu_amd import evaluation as ev
    row = so.Row(dev)
    p, _, target, mask = _maps(row, 'ece')
    row.call = lambda s: list(ev.calibration_histogram(p, target, 10, mask, n_volumes=N))
    return row


@wrapper('evaluation.uncertainty_counts')
def _uncertainty_counts(dev):
    from rcu_amd import evaluation as ev
    row = so.Row(dev)
    u, pred, target, mask = _maps(row, 'unc')
    row.call = lambda s: [ev.uncertainty_counts(pred, target, u, mask=mask, n_volumes=N)]
    return row


@wrapper('evaluation.uncertainty_counts_from_p')
def _uncertainty_counts_from_p(dev):
    from rcu_amd import evaluation as ev
    row = so.Row(dev)
    p, pred, target, mask = _maps(row, 'uncp')
    row.call = lambda s: [ev.uncertainty_counts_from_p(pred, target, p, mask=mask, n_volumes=N)]
    return row


@wrapper('evaluation.uncertainty_histogram')
def _uncertainty_histogram(dev):
    from rcu_amd import evaluation as ev
    row = so.Row(dev)
    u, pred, target, mask = _maps(row, 'uh')
    row.call = lambda s: [ev.uncertainty_histogram(pred, target, u, mask=mask, n_volumes=N), ev.uncertainty_histogram_from_p(pred, target, u, mask=mask, n_volumes=N)]
    return row


@wrapper('evaluation.calibration_levels')
def _calibration_levels(dev):
    from rcu_amd import evaluation as ev
    row = so.Row(dev)
    p, _, target, mask = _maps(row, 'levels')
    row.call = lambda s: list(ev.calibration_levels(p, target, mask=mask, n_volumes=N))
    return row


@wrapper('evaluation.quantile_rescale')
def _quantile_rescale(dev):
    from rcu_amd import evaluation as ev
    row = so.Row(dev)
    x = f32(rng('wrapper', 'quantile'), N, 1001)
    keys = np.sort(ev.float_key(x.reshape(-1)))
    Q = 16
    ranks = ev.quantile_ranks(x.size, Q)
    table = ev.QuantileTable(Q, x.size, keys[[int(r) - 1 for r in ranks]], ranks, 'all')
    x = row.inp(x)
    row.call = lambda s: list(ev.quantile_rescale(table, x, return_levels=True))
    return row


def _volume_maps(row, tag):
    r = rng('wrapper', tag)
    shape = (N,) + VOL
    return r, row.inp(u8(r, shape, 0.3)), row.inp(u8(r, shape, 0.3)), row.inp(u8(r, shape, 0.8)), row.inp(prob(r, *shape))


@wrapper('evaluation.patch_table')
def _patch_table(dev):
    from rcu_amd import evaluation as ev
    row = so.Row(dev)
    _, pred, target, mask, p = _volume_maps(row, 'patch')
    row.call = lambda s: ev.patch_table(pred, target, foreground_probability=p, patch=(2, 4, 8), mask=mask, n_volumes=N)
    return row


@wrapper('evaluation.patch_histogram')
def _patch_histogram(dev):
    from rcu_amd import evaluation as ev
    row = so.Row(dev)
    _, pred, target, mask, p = _volume_maps(row, 'phist')
    row.call = lambda s: [ev.patch_histogram(pred, target, foreground_probability=p, patch=(2, 4, 8), mask=mask, n_volumes=N, levels=100)]
    return row


@wrapper('evaluation.component_pairs')
def _component_pairs(dev):
    """From 64 slots per volume: the table reports dropped voxels and is made again, several times (the retry loop)."""
    from rcu_amd import evaluation as ev
    row = so.Row(dev)
    r = rng('wrapper', 'pairs')
    a = ev.canonical_labels(u8(r, (N,) + VOL, 0.15), 26, n_volumes=N)
    b = ev.canonical_labels(u8(r, (N,) + VOL, 0.15), 6, n_volumes=N)
    a, b, inside = row.inp(np.asarray(a, dtype=np.int32)), row.inp(np.asarray(b, dtype=np.int32)), row.inp(u8(r, (N,) + VOL, 0.5))
    row.call = lambda s: ev.component_pairs(a, b, inside, n_volumes=N, capacity=64)
    return row


@wrapper('steps.tta_transform + fold_transformed')
def _tta(dev):
    """The images transformed, statistics of the transformed logits, folded back into the canonical statistics."""
    from rcu_amd import steps
    row = so.Row(dev)
    r = rng('wrapper', 'tta')
    x, y = row.inp(f32(r, N, 2, 31, 31)), row.inp(f32(r, N, 2, 31, 31))

    def call(s):
        moved = steps.tta_transform(x, 'rot90')
        dst = steps.McStatistics(N, 2, 31, 31, dev, do_mi=True, exact=True)
        src = steps.McStatistics(N, 2, 31, 31, dev, do_mi=True, exact=True)
        dst.accumulate(y)
        src.accumulate(moved)
        steps.fold_transformed(src, dst, 'rot90')
        return [moved, dst.blob] + [t for _, t in sorted(dst.finalize(do_mi=True).items())]
    row.call = call
    return row


@wrapper('DensityPredictStep')
def _density_step(dev):
    from rcu_amd import density, steps
    row = so.Row(dev)
    model = _model(dev)
    if 'density' not in _fits:
        g = torch.Generator().manual_seed(3)
        images = torch.randn(6, 4, H, W, generator=g).to(dev)
        target = (torch.rand(6, H, W, generator=g) < 0.35).to(torch.uint8).to(dev)
        _fits['density'] = density.fit_density(model, [(images, target)])
        torch.cuda.synchronize()
    fit, x = _fits['density'], _images(row, 'density')

    def call(s):
        bc = steps.BatchContext({'images': x}, 0, 0)
        steps.DensityPredictStep(fit)(bc, None, _context(dev, model))
        return _outputs(bc)
    row.call = call
    return row


@wrapper('LaplacePredictStep')
def _laplace_step(dev):
    from rcu_amd import laplace, steps
    row = so.Row(dev)
    model = _model(dev)
    if 'laplace' not in _fits:
        images = torch.randn(6, 4, H, W, generator=torch.Generator().manual_seed(4)).to(dev)
        _fits['laplace'] = laplace.fit_laplace(model, [(images,)], hessian_scale=0.1, prior_precision='evidence')
        torch.cuda.synchronize()
    fit, x = _fits['laplace'], _images(row, 'laplace')

    def call(s):
        out = []
        for kwargs in (dict(), dict(link='sample', samples=4, seed=5)):
            bc = steps.BatchContext({'images': x}, 0, 0)
            steps.LaplacePredictStep(fit, **kwargs)(bc, None, _context(dev, model))
            out += _outputs(bc)
        return out
    row.call = call
    return row


@wrapper('corruption.corrupt')
def _corrupt(dev):
    from rcu_amd import corruption
    row = so.Row(dev)
    x = _images(row, 'corrupt')
    stages = corruption.parse([dict(kind='gaussian_blur', severity=2), dict(kind='bias_field', severity=3), dict(kind='contrast', severity=3),
                               dict(kind='gaussian_noise', severity=2)])
    row.call = lambda s: [corruption.corrupt(x, stages, 7, 100)]
    return row
