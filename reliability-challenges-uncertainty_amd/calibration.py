"""EXTENSION: post-hoc temperature scaling (the reference has no calibration fitting).

One scalar T divides every pass's logits before the softmax -- Guo et al. 2017 for one deterministic pass, Laves et al. 2019 for MC dropout
(the NLL of the MC-averaged prediction) -- and T is fitted to minimise that NLL on held-out volumes:

    sweep = NllSweep(device)                      # the NLL of every candidate of CANDIDATES, summed on the device as exact integers
    sweep.add(logits, target, passes=P)           # logits [P * n, C, H, W] pass-major, target [n, H, W]
    fit = refine(sweep.temperatures, sweep.sums())
    model.set_temperature(fit.temperature)        # every forward path honours it (rcu_amd.model.UNet.set_temperature)

``fit_temperature`` runs the passes of a model over batches of validation slices and does the above; ``load_temperature`` reads the value the
test scripts take as ``others.temperature``.
"""
import collections
import ctypes
import json
import logging
import math
import os

import torch

from . import _lib
from . import steps

# T_k = 2^((k - 48) / 16), k = 0..96: 1/8 .. 8, candidate 48 is exactly 1 (the sweep also gives the NLL before scaling)
CANDIDATES = tuple(2.0 ** ((k - 48) / 16.0) for k in range(97))
UNSCALED = 48
SCALE = 1 << 20          # the device sums hold round(l * 2^20) per voxel (include/rcu.h, rcu_temperature_nll)
DRAIN_VOXELS = 1 << 30   # voxels the device buffer takes before it is added to the host's Python ints (a term is at most 2^32 units)

Refined = collections.namedtuple('Refined', 'temperature at_edge index')


def _valid_temperature(value):
    return not isinstance(value, bool) and isinstance(value, (int, float)) and math.isfinite(value) and value > 0


class NllSweep:
    """The NLL of the pass-averaged prediction under every candidate temperature, over all voxels added so far (include/rcu.h,
    rcu_temperature_nll).  The sums are exact integers: they do not depend on how the voxels are split into ``add`` calls."""

    def __init__(self, device, temperatures=CANDIDATES):
        temperatures = tuple(float(t) for t in temperatures)
        if not 1 <= len(temperatures) <= _lib.RCU_TEMPERATURE_MAX_CANDIDATES:
            raise ValueError('1..{} candidate temperatures, got {}'.format(_lib.RCU_TEMPERATURE_MAX_CANDIDATES, len(temperatures)))
        if not all(_valid_temperature(t) for t in temperatures):
            raise ValueError('candidate temperatures must be finite and > 0')
        self.temperatures = temperatures
        self.device = torch.device(device)
        k = len(temperatures)
        self._betas = (ctypes.c_float * k)(*[1.0 / t for t in temperatures])
        self._out = torch.zeros(k + 2, dtype=torch.int64, device=self.device)    # uint64 slots (values stay far below 2^63)
        self._workspace = None
        self._pending = 0                    # voxels added on the device since the last drain
        self._sums = [0] * k
        self._voxels = 0
        self._invalid = 0

    def add(self, logits, target, mask=None, passes=1):
        """``logits``: float32 ``[passes * n, C, H, W]`` (or ``[passes, n, C, H, W]``), sample t * n + i = slice i in pass t; ``target``:
        ``[n, H, W]`` class indices; ``mask``: ``[n, H, W]`` (voxels where it is non-zero) or None (all voxels).  Stream-ordered, no sync."""
        passes = int(passes)
        if logits.dim() == 5:
            logits = logits.reshape(-1, *logits.shape[2:])
        if logits.dim() != 4 or passes < 1 or logits.shape[0] % passes:
            raise ValueError('logits must be [passes * n, C, H, W] with passes = {}, got {}'.format(passes, tuple(logits.shape)))
        n, c = logits.shape[0] // passes, logits.shape[1]
        hw = logits.shape[2] * logits.shape[3]
        logits = logits.to(self.device, torch.float32).contiguous()
        target = self._bytes(target, n * hw, 'target')
        mask = None if mask is None else self._bytes(mask != 0 if torch.is_tensor(mask) else torch.as_tensor(mask) != 0, n * hw, 'mask')
        need = _lib.load().rcu_temperature_nll_workspace_bytes(n * hw, len(self.temperatures))
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        if self._pending + n * hw > DRAIN_VOXELS:
            self._drain()
        _lib.check(_lib.load().rcu_temperature_nll(_lib.ptr(logits), passes, n, hw, c, _lib.ptr(target), _lib.ptr(mask), self._betas,
                                                   len(self.temperatures), _lib.ptr(self._out), _lib.ptr(self._workspace),
                                                   _lib.current_stream()))
        self._pending += n * hw

    def _bytes(self, t, count, name):
        t = torch.as_tensor(t)
        if t.numel() != count:
            raise ValueError('{} has {} elements, expected {}'.format(name, t.numel(), count))
        return t.to(self.device).to(torch.uint8).contiguous()

    def _drain(self):
        host = [int(v) for v in self._out.cpu().tolist()]
        self._out.zero_()
        self._pending = 0
        k = len(self.temperatures)
        self._sums = [a + b for a, b in zip(self._sums, host[:k])]
        self._voxels += host[k]
        self._invalid += host[k + 1]
        if self._invalid:
            raise ValueError('{} voxels inside the mask have a target >= the number of classes'.format(self._invalid))

    def sums(self):
        """Per candidate: the sum over voxels of round(l * 2^20), as exact Python ints."""
        self._drain()
        return list(self._sums)

    @property
    def voxels(self):
        self._drain()
        return self._voxels

    def mean_nll(self):
        """Per candidate: the mean NLL per voxel, float64."""
        sums, voxels = self.sums(), self.voxels
        if not voxels:
            raise ValueError('no voxels were added')
        return [s / SCALE / voxels for s in sums]


def refine(temperatures, sums):
    """The argmin k* of ``sums`` over ``temperatures`` (the smallest k on ties), refined by the vertex of the parabola in log2 T through k* - 1,
    k*, k* + 1, clamped to that bracket.  At either end of the grid: T_k* with ``at_edge`` set (and a warning)."""
    temperatures, sums = list(temperatures), list(sums)
    if len(temperatures) != len(sums) or not temperatures:
        raise ValueError('one sum per candidate temperature')
    k = min(range(len(sums)), key=lambda i: (sums[i], i))
    if k == 0 or k == len(sums) - 1:
        logging.warning('temperature scaling: the NLL is smallest at the %s end of the candidate grid (T = %g); the best T may lie beyond it',
                        'lower' if k == 0 else 'upper', temperatures[k])
        return Refined(float(temperatures[k]), True, k)
    x0, x1, x2 = (math.log2(temperatures[i]) for i in (k - 1, k, k + 1))
    y0, y1, y2 = (float(sums[i]) for i in (k - 1, k, k + 1))
    # vertex of the parabola through (x0, y0), (x1, y1), (x2, y2)
    num = (x1 - x0) ** 2 * (y1 - y2) - (x1 - x2) ** 2 * (y1 - y0)
    den = (x1 - x0) * (y1 - y2) - (x1 - x2) * (y1 - y0)
    x = x1 if den == 0 else x1 - 0.5 * num / den
    x = min(max(x, x0), x2)
    return Refined(2.0 ** x, False, k)


class TemperatureFit:
    """What ``fit_temperature`` found: the refined ``temperature``, whether the minimum sat at an end of the grid (``at_edge``), the mean NLL at
    T = 1 and at the best candidate, the voxels and passes it saw, the mask seed and the whole curve [(T_k, mean NLL)]."""

    def __init__(self, temperature, at_edge, mean_nll_at_1, mean_nll_at_best_candidate, voxels, passes, seed, curve):
        self.temperature, self.at_edge = temperature, at_edge
        self.mean_nll_at_1, self.mean_nll_at_best_candidate = mean_nll_at_1, mean_nll_at_best_candidate
        self.voxels, self.passes, self.seed, self.curve = voxels, passes, seed, curve

    def as_dict(self):
        return {'temperature': self.temperature, 'at_edge': self.at_edge, 'mean_nll_at_1': self.mean_nll_at_1,
                'mean_nll_at_best_candidate': self.mean_nll_at_best_candidate, 'voxels': self.voxels, 'passes': self.passes,
                'seed': self.seed, 'curve': [[t, v] for t, v in self.curve]}


def pass_logits(model, images, mc_steps=0, seed=0, first_sample=0, group_pixels=None):
    """Logits of the passes of one batch, ``[P * n, C, H, W]`` pass-major: P = 1 in eval mode for ``mc_steps`` = 0, else the ``mc_steps``
    dropout passes (no weight-scaling pass) with the masks the MC test step draws for these slices -- key ``steps.pass_seed(seed, j)`` at the
    slices' global index ``first_sample`` -- run as grouped forwards of g * n samples (g from ``steps.pass_group_size``)."""
    steps.set_dropout_mode(model, False)
    if mc_steps <= 0:
        return model(images)
    n, _, h, w = images.shape
    group = steps.pass_group_size(model, n, h, w, steps.McPredictStep.GROUP_PIXELS if group_pixels is None else group_pixels)
    out = []
    for j0 in range(1, mc_steps + 1, group):
        jobs = list(range(j0, min(j0 + group, mc_steps + 1)))
        steps.set_dropout_mode(model, True)          # (sites in eval mode get factors of one)
        try:
            masks = model.seeded_masks(n, images.device, [steps.pass_seed(seed, j) for j in jobs], first_sample)
        finally:
            steps.set_dropout_mode(model, False)
        x = images if len(jobs) == 1 else images.repeat(len(jobs), 1, 1, 1)
        out.append(model(x, masks))
    return out[0] if len(out) == 1 else torch.cat(out)


def fit_temperature(model, batches, mc_steps=0, seed=0, group_pixels=None):
    """Fit T on ``batches``: an iterable of ``(images [n, C_in, H, W], target [n, H, W])`` or ``(images, target, mask)``, in the order of the
    run's stream of slices (the masks of MC pass j of a slice are keyed by its running global index, as in the MC test step).  ``mc_steps``
    = 0: one eval-mode pass; T > 0: the T dropout passes of each slice, averaged inside the log.  -> TemperatureFit."""
    mc_steps = int(mc_steps or 0)
    sweep = None
    first = 0
    for batch in batches:
        images, target = batch[0], batch[1]
        mask = batch[2] if len(batch) > 2 else None
        if sweep is None:
            sweep = NllSweep(images.device)
        logits = pass_logits(model, images, mc_steps, seed, first, group_pixels)
        sweep.add(logits, target, mask, passes=max(mc_steps, 1))
        first += images.shape[0]
    if sweep is None:
        raise ValueError('fit_temperature: no batches')
    sums, means = sweep.sums(), sweep.mean_nll()
    best = refine(sweep.temperatures, sums)
    return TemperatureFit(best.temperature, best.at_edge, means[UNSCALED], means[best.index], sweep.voxels, max(mc_steps, 1), seed,
                          list(zip(sweep.temperatures, means)))


def load_temperature(value):
    """``others.temperature``: a finite positive number, or the path of a JSON file with a ``"temperature"`` key (what the fit scripts write).
    Anything else raises ValueError."""
    if isinstance(value, (str, os.PathLike)):
        path = os.fspath(value)
        try:
            with open(path) as f:
                doc = json.load(f)
        except (OSError, ValueError) as e:
            raise ValueError('temperature file {!r} cannot be read: {}'.format(path, e)) from None
        if not isinstance(doc, dict) or 'temperature' not in doc:
            raise ValueError('temperature file {!r} has no "temperature" key'.format(path))
        value = doc['temperature']
    if not _valid_temperature(value):
        raise ValueError('the temperature must be a finite number > 0, got {!r}'.format(value))
    return float(value)
