"""EXTENSION -- seeded input corruptions for dataset-shift runs of the test scripts (include/rcu.h, "Input corruptions"; the reference tests on
clean volumes only).  Appearance corruptions only: the labels stay valid, so every writer, Dice count and evaluation action runs unchanged.

    others:
      corruption: [{kind: gaussian_blur, severity: 2}, {kind: gaussian_noise, amount: 0.25}, {kind: channel_drop, channels: [1]}]

``parse`` turns that value into stages, ``corrupt`` runs them on a device batch (one ``rcu_corrupt`` per stage), ``steps.CorruptInputStep`` puts
the result in front of the predict steps.  The corrupted slice is a function of (the slice, the stages, the seed, its global index): a run is
reproducible and does not depend on ``batch_size``, the coalescing or the number of ranks.
"""
import collections
import collections.abc
import ctypes
import functools
import math
import operator

import numpy as np

from . import _lib

KINDS = _lib.CORRUPTION_KINDS          # code -> name
MAX_STAGES = 8

# severity 1..5 -> amount, in input units (BraTS inputs are per-channel z-scores).  Part of the feature's definition (repeated in include/rcu.h).
SEVERITY = {
    'gaussian_noise': (0.1, 0.2, 0.3, 0.5, 0.8),
    'gaussian_blur': (0.5, 1.0, 1.5, 2.0, 3.0),
    'downsample': (2.0, 3.0, 4.0, 6.0, 8.0),
    'contrast': (0.8, 0.6, 0.45, 0.3, 0.2),
    'intensity_shift': (0.1, 0.2, 0.3, 0.5, 0.8),
    'bias_field': (0.1, 0.2, 0.3, 0.45, 0.6),
    'ghosting': (0.05, 0.1, 0.15, 0.25, 0.4),
}

Stage = collections.namedtuple('Stage', 'kind code amount severity channels')


def amount_of(kind, severity):
    """The amount of ``kind`` at severity 1..5 (ValueError for channel_drop, which has none, an unknown kind or another severity)."""
    if kind not in KINDS:
        raise ValueError('corruption: unknown kind {!r} (one of {})'.format(kind, ', '.join(KINDS)))
    if kind not in SEVERITY:
        raise ValueError('corruption: kind {!r} has no severity: name its channels'.format(kind))
    if isinstance(severity, bool) or not isinstance(severity, int) or not 1 <= severity <= 5:
        raise ValueError('corruption: severity of {} must be an integer in 1..5, got {!r}'.format(kind, severity))
    return SEVERITY[kind][severity - 1]


def blur_radius(sigma):
    """scipy.ndimage.gaussian_filter's radius at truncate = 4: int(4 sigma + 0.5)."""
    return int(4.0 * float(sigma) + 0.5)


def _check_amount(kind, amount, where):
    """The limits of include/rcu.h, kind by kind -> float(amount)."""
    if isinstance(amount, bool) or not isinstance(amount, (int, float)) or not math.isfinite(amount):
        raise ValueError('{}: amount of {} must be a finite number, got {!r}'.format(where, kind, amount))
    a = float(amount)
    ok = {
        'gaussian_noise': a >= 0.0,
        'gaussian_blur': 0.0 < a <= 8.0,
        'downsample': 2 <= int(a) <= 16,
        'contrast': 0.0 <= a <= 4.0,
        'intensity_shift': True,
        'bias_field': 0.0 <= a <= 2.0,
        'ghosting': 0.0 <= a <= 1.0,
        'channel_drop': a == int(a) and 1 <= a < 2 ** 30,
    }[kind]
    if not ok:
        limits = {'gaussian_noise': '>= 0', 'gaussian_blur': 'in (0, 8]', 'downsample': 'in 2..16', 'contrast': 'in [0, 4]', 'bias_field': 'in [0, 2]',
                  'ghosting': 'in [0, 1]', 'channel_drop': 'a channel mask (an integer >= 1)'}[kind]
        raise ValueError('{}: amount of {} must be {}, got {!r}'.format(where, kind, limits, amount))
    return a


def _parse_stage(entry, index):
    where = 'corruption stage {}'.format(index)
    if not isinstance(entry, collections.abc.Mapping):
        raise ValueError('{}: expected a mapping with the key kind, got {!r}'.format(where, entry))
    if 'kind' not in entry:
        raise ValueError('{}: the key kind is missing'.format(where))
    kind = entry['kind']
    if kind not in KINDS:
        raise ValueError('{}: unknown kind {!r} (one of {})'.format(where, kind, ', '.join(KINDS)))
    allowed = ('kind', 'amount', 'channels') if kind == 'channel_drop' else ('kind', 'severity', 'amount')
    for key in entry:
        if key not in allowed:
            raise ValueError('{}: unknown key {!r} for {} (it takes {})'.format(where, key, kind, ', '.join(allowed)))
    severity = channels = None
    if kind == 'channel_drop':
        if ('channels' in entry) == ('amount' in entry):
            raise ValueError('{}: channel_drop takes either channels or amount (the channel mask), not both and not neither'.format(where))
        if 'channels' in entry:
            channels = entry['channels']
            channels = [channels] if isinstance(channels, int) and not isinstance(channels, bool) else channels
            if (not isinstance(channels, (list, tuple)) or not channels
                    or any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < 30 for c in channels) or len(set(channels)) != len(channels)):
                raise ValueError('{}: channels must be a non-empty list of distinct channel indices in 0..29, got {!r}'.format(where, entry['channels']))
            channels = tuple(sorted(channels))
            amount = float(sum(1 << c for c in channels))
        else:
            amount = _check_amount(kind, entry['amount'], where)
            channels = tuple(c for c in range(30) if (int(amount) >> c) & 1)
    else:
        if ('severity' in entry) == ('amount' in entry):
            raise ValueError('{}: {} takes either severity or amount, not both and not neither'.format(where, kind))
        if 'severity' in entry:
            severity = entry['severity']
            try:
                amount = amount_of(kind, severity)
            except ValueError as e:
                raise ValueError('{}: {}'.format(where, e)) from None
        else:
            amount = entry['amount']
        amount = _check_amount(kind, amount, where)
    return Stage(kind, KINDS.index(kind), amount, severity, channels)


def parse(spec):
    """``others.corruption`` -> a tuple of Stage(kind, code, amount, severity, channels), applied in order.  ``spec``: one mapping or a list of at
    most 8.  Each names its ``kind`` and either ``severity: 1..5`` or an explicit ``amount:`` (channel_drop: ``channels: [..]``, or the channel
    mask as ``amount``).  ValueError naming the key for an unknown kind or key, ``severity`` together with ``amount``, a value outside the limits."""
    if isinstance(spec, collections.abc.Mapping):
        spec = [spec]
    if not isinstance(spec, (list, tuple)) or not spec:
        raise ValueError('corruption: expected a mapping or a non-empty list of mappings, got {!r}'.format(spec))
    if len(spec) > MAX_STAGES:
        raise ValueError('corruption: at most {} stages, got {}'.format(MAX_STAGES, len(spec)))
    return tuple(_parse_stage(entry, i) for i, entry in enumerate(spec))


def describe(stages, seed):
    """What ``<test_dir>/corruption.json`` records: the parsed stages with their amounts, and the seed."""
    rows = []
    for s in stages:
        row = {'kind': s.kind, 'amount': s.amount}
        if s.severity is not None:
            row['severity'] = s.severity
        if s.channels is not None:
            row['channels'] = list(s.channels)
        rows.append(row)
    return {'stages': rows, 'seed': int(seed)}


def corruption_seed(seed, stage):
    """Key of corruption stage ``stage`` (0..7) of a run seeded with ``seed``: ``pass_seed(seed, 0)`` + (16 + stage) * 2^40.  The mask keys of the
    MC passes are ``pass_seed(seed, 1..2048)``, test-time augmentation adds 0..7 * 2^40 to those (``steps.tta_pass_seed``) and the logit sampling
    uses a pass's mask key: every one of them lies within 2048 + 7 * 2^40 of ``pass_seed(seed, 0)``, the corruption keys start at 16 * 2^40 above it
    and everything is far below the modulus 2^63 - 1 -- no corruption key equals a mask key, a TTA key or a logit-sampling key of the same seed."""
    from . import steps
    stage = operator.index(stage)
    if not 0 <= stage < MAX_STAGES:
        raise ValueError('corruption stage index must be in 0..{}, got {}'.format(MAX_STAGES - 1, stage))
    return (steps.pass_seed(seed, 0) + (16 + stage) * (1 << 40)) % (2 ** 63 - 1)


_M64 = (1 << 64) - 1


def _splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def bias_coefficients(key, channels):
    """float64 ``[channels, 8]``: the coefficients of the bias field's terms (u, v) in {0, 1, 2}^2 without (0, 0), raster order.  Term e of channel c
    is 2 u - 1 with u = (t >> 11) * 2^-53 and t = SplitMix64(key + (8 c + e + 1) * 0x9E3779B97F4A7C15); each channel is divided by its sum of
    absolute values, so that the field stays within [-1, 1]."""
    coef = np.empty((int(channels), 8), dtype=np.float64)
    for c in range(int(channels)):
        for e in range(8):
            t = _splitmix64((int(key) + (8 * c + e + 1) * 0x9E3779B97F4A7C15) & _M64)
            coef[c, e] = 2.0 * ((t >> 11) * 2.0 ** -53) - 1.0
        coef[c] /= np.abs(coef[c]).sum()
    return coef


def bias_tables(height, width):
    """float64 A ``[3, height]``, B ``[3, width]``: A[u][i] = cos(pi u (i + 0.5) / height), B[v][j] likewise."""
    u = np.arange(3, dtype=np.float64)[:, None]
    return (np.cos(np.pi * u * (np.arange(height, dtype=np.float64)[None] + 0.5) / height),
            np.cos(np.pi * u * (np.arange(width, dtype=np.float64)[None] + 0.5) / width))


def blur_taps(sigma):
    """float64 taps w_k = exp(-k^2 / (2 sigma^2)) / sum, k = -r..r, r = int(4 sigma + 0.5): scipy.ndimage's Gaussian kernel at truncate = 4."""
    sigma = float(sigma)
    r = blur_radius(sigma)
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return w / w.sum()


@functools.lru_cache(maxsize=64)
def _aux(kind, amount, key, channels, height, width):
    """The ``aux_host`` of a stage as (ctypes float array or None, count): float64 on the host, rounded to float32."""
    if kind == 'gaussian_blur':
        values = blur_taps(amount)
    elif kind == 'bias_field':
        a, b = bias_tables(height, width)
        values = np.concatenate([bias_coefficients(key, channels).ravel(), a.ravel(), b.ravel()])
    else:
        return None, 0
    values = values.astype(np.float32)
    return (ctypes.c_float * values.size)(*values.tolist()), int(values.size)


def corrupt_stage(images, stage, key, first_sample, out):
    """One ``rcu_corrupt``: ``out`` = stage(``images``), both contiguous float32 ``[N, C, H, W]`` on one device, on the current stream."""
    import torch
    n, c, h, w = images.shape
    lib = _lib.load()
    aux, n_aux = _aux(stage.kind, stage.amount, int(key), c, h, w)
    ws_bytes = lib.rcu_corrupt_workspace_bytes(n, c, h, w, stage.code)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=images.device) if ws_bytes else None
    _lib.check(lib.rcu_corrupt(_lib.ptr(images), n, c, h, w, stage.code, float(stage.amount), int(key), int(first_sample), aux, n_aux, _lib.ptr(out),
                               _lib.ptr(ws), _lib.current_stream()))
    return out


def corrupt(images, stages, seed, first_sample, out=None):
    """``stages`` (``parse``) applied in order to a contiguous float32 CUDA tensor ``[N, C, H, W]`` whose image i is the slice with global index
    ``first_sample + i``; stage s runs under the key ``corruption_seed(seed, s)``.  One ``rcu_corrupt`` per stage, ping-pong between two buffers;
    returns the result (``out`` when given) and never modifies ``images``."""
    import torch
    if not torch.is_tensor(images) or images.dim() != 4 or images.dtype != torch.float32 or not images.is_cuda or not images.is_contiguous():
        raise ValueError('corrupt: images must be a contiguous float32 [N, C, H, W] tensor on the GPU')
    if out is not None and (out.shape != images.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != images.device):
        raise ValueError('corrupt: out must be a contiguous float32 tensor of the shape and device of the images')
    if out is not None and out.data_ptr() == images.data_ptr():
        raise ValueError('corrupt: out must not be the images')
    stages = tuple(stages)
    if not stages or len(stages) > MAX_STAGES or not all(isinstance(s, Stage) for s in stages):
        raise ValueError('corrupt: 1..{} stages as corruption.parse returns them'.format(MAX_STAGES))
    buffers = [torch.empty_like(images) if out is None else out, None]
    source = images
    for s, stage in enumerate(stages):
        slot = (len(stages) - 1 - s) % 2       # the last stage writes buffers[0]
        if buffers[slot] is None:
            buffers[slot] = torch.empty_like(images)
        source = corrupt_stage(source, stage, corruption_seed(seed, s), first_sample, buffers[slot])
    return source
