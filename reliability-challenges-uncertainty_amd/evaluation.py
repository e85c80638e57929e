"""Metric seam: calibration / uncertainty-error metrics with the reference's protocol, on librcu_hip.

Mirrors
  ece_binary, uncertainty, error_dice/recall/precision, dice, confusion_matrx, accuracy
                                            common/evalutation/numpyfunctions.py:6-151
  EvaluationStrategy family                 common/evalutation/eval.py:9-226
  preparation helpers                       rechun/eval/helper.py:7-47, rechun/eval/analysis.py:147-285
``EvaluationStrategy.__call__(to_evaluate, results)`` takes numpy arrays (or device tensors) in
``to_evaluate`` and writes python / numpy scalars and small arrays into ``results`` under the
reference's keys.  The per-voxel scans run on the GPU: the reliability histogram (bit-exact bin
indices), the 8 confusion x uncertain counts for all thresholds in one pass, the normalised entropy.
What is left on the host is arithmetic on ~30 numbers (ECE from the histogram, Dice from counts).
"""
import abc
import bisect
import ctypes
import math
import warnings

import numpy as np
import torch

from . import _lib

UE_THRESHOLDS = (0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95)  # bin-eval/eval_uncertainty.py:239


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('rcu_amd.evaluation needs a GPU (librcu_hip); there is no CPU fallback')
    return torch.device('cuda')


def _to_dev(a, dtype):
    # (Measured and NOT done: staging through pinned buffers + asynchronous copies.  Next to a test loop that has run ahead -- every CU held by a
    # persistent conv kernel -- a small operation of the metric seam waits tens of milliseconds whichever way its bytes travel, and the pinned
    # form was the slower one on the same box: tools/host_costs_probe.py, 0.175-0.25 against 0.139 s per subject.  The drop-in scripts
    # therefore take their per-subject Dice counts at batch time, on the compute stream: scripts.ConfusionOnDeviceStep.)
    if isinstance(a, torch.Tensor):
        return a.to(device=_device(), dtype=dtype).contiguous()
    a = np.ascontiguousarray(a)
    if dtype == torch.uint8 and a.dtype.kind in 'iub' and a.dtype.itemsize > 1:
        a = a.astype(np.uint8)       # the cast torch would make on the device (wraps alike), made before the copy: an eighth of the bytes for int64 label maps
    return torch.from_numpy(a).to(device=_device(), dtype=dtype)


def _flat(a, dtype, n_volumes, like=None, names=None):
    """An array or tensor (or None) -> device ``[n_volumes, n]`` of ``dtype``; with ``like``, another size than that map's is refused."""
    if a is None:
        return None
    a = _to_dev(a, dtype).reshape(n_volumes, -1)
    if like is not None and a.shape != like.shape:
        raise ValueError('{} differ in size'.format(names))
    return a


def _float_map(uncertainty, n_volumes):
    """-> (device ``[n_volumes, n]`` map, is64): a float64 uncertainty map stays float64, everything else goes up as float32."""
    is64 = uncertainty.dtype == (torch.float64 if isinstance(uncertainty, torch.Tensor) else np.float64)
    return _flat(uncertainty, torch.float64 if is64 else torch.float32, n_volumes), is64


# ------------------------------------------------ the per-voxel scans: device arrays [V, n] in, device result out, nothing waits
def _thresholds_array(thresholds):
    return (ctypes.c_double * len(thresholds))(*[float(t) for t in thresholds])


def _ece_launch(p, target, mask, n_bins):
    v, n = target.shape
    lib = _lib.load()
    raw = torch.empty(v * ctypes.sizeof(_lib.EceResult), device=p.device, dtype=torch.uint8)
    ws = torch.empty(max(lib.rcu_ece_workspace_bytes(n, v), 8), device=p.device, dtype=torch.uint8)
    _lib.check(lib.rcu_ece_hist(_lib.ptr(p), _lib.ptr(target), _lib.ptr(mask), n, v, _lib.ece_thresholds(n_bins), n_bins, _lib.ptr(raw),
                                _lib.ptr(ws), _lib.current_stream()))
    return raw


def _ece_unpack(raw, v, n_bins):
    """``_ece_launch``'s result on the host -> (count int64 [v, n_bins], sum_conf float64, sum_pos int64)."""
    raw = raw.numpy().view(np.uint64).reshape(v, 3, _lib.RCU_MAX_BINS)
    return raw[:, 0, :n_bins].astype(np.int64), raw[:, 1, :n_bins].copy().view(np.float64), raw[:, 2, :n_bins].astype(np.int64)


def _unc_counts_launch(unc, is64, prediction, target, mask, thresholds):
    v, n = target.shape
    lib = _lib.load()
    out = torch.empty((v, len(thresholds), 8), device=unc.device, dtype=torch.int64)
    ws = torch.empty(max(lib.rcu_unc_workspace_bytes(n, v), 8), device=unc.device, dtype=torch.uint8)
    _lib.check(lib.rcu_unc_counts(_lib.ptr(unc), int(is64), _lib.ptr(prediction), _lib.ptr(target), _lib.ptr(mask), n, v, _thresholds_array(thresholds),
                                  len(thresholds), _lib.ptr(out), _lib.ptr(ws), _lib.current_stream()))
    return out


def _unc_counts_from_p_launch(p, prediction, target, mask, thresholds):
    v, n = target.shape
    lib = _lib.load()
    out = torch.empty((v, len(thresholds), 8), device=p.device, dtype=torch.int64)
    ws = torch.empty(lib.rcu_unc_from_p_workspace_bytes(n, v), device=p.device, dtype=torch.uint8)
    _lib.check(lib.rcu_unc_counts_from_p(_lib.ptr(p), _lib.ptr(prediction), _lib.ptr(target), _lib.ptr(mask), n, v, _thresholds_array(thresholds),
                                         len(thresholds), _lib.ptr(out), _lib.ptr(ws), _lib.current_stream()))
    return out


def _unc_hist_launch(source, is64, prediction, target, mask, levels):
    """``source``: an uncertainty map (``is64`` says which), or with ``is64`` None the float32 foreground probability (rcu_unc_hist_from_p).
    -> device int64 [v, 4, levels] holding the uint64 counts."""
    v, n = target.shape
    levels = int(levels)
    lib = _lib.load()
    out = torch.empty((v, 4, max(levels, 1)), device=source.device, dtype=torch.int64)
    ws = torch.empty(max(lib.rcu_unc_hist_workspace_bytes(n, v, levels), 8), device=source.device, dtype=torch.uint8)
    rest = (_lib.ptr(prediction), _lib.ptr(target), _lib.ptr(mask), n, v, levels, _lib.ptr(out), _lib.ptr(ws), _lib.current_stream())
    _lib.check(lib.rcu_unc_hist_from_p(_lib.ptr(source), *rest) if is64 is None else lib.rcu_unc_hist(_lib.ptr(source), int(is64), *rest))
    return out


def _calib_curve_launch(p, target, mask, levels):
    """-> device int64 (levels [v, 3, levels], totals [v, 2, 4]) holding the uint64 integers of rcu_calib_curve."""
    v, n = target.shape
    levels = int(levels)
    lib = _lib.load()
    out = torch.empty((v, 3, max(levels, 1)), device=p.device, dtype=torch.int64)
    totals = torch.empty((v, 2, 4), device=p.device, dtype=torch.int64)
    ws = torch.empty(max(lib.rcu_calib_curve_workspace_bytes(n, v, levels), 8), device=p.device, dtype=torch.uint8)
    _lib.check(lib.rcu_calib_curve(_lib.ptr(p), _lib.ptr(target), _lib.ptr(mask), n, v, levels, _lib.ptr(out), _lib.ptr(totals), _lib.ptr(ws),
                                   _lib.current_stream()))
    return out, totals


# ------------------------------------------------------------------------------------------- ECE
def _foreground(probabilities, target_ndim):
    """numpyfunctions.py:27-33."""
    if probabilities.ndim > target_ndim:
        if probabilities.shape[-1] > 2:
            raise ValueError('can only evaluate the calibration for binary classification')
        if probabilities.shape[-1] == 2:
            return probabilities[..., 1]
        return probabilities.squeeze(-1) if isinstance(probabilities, torch.Tensor) else np.squeeze(probabilities, -1)
    return probabilities


def calibration_histogram(probabilities, target, n_bins=10, mask=None, threshold_range=None, n_volumes=1):
    """Raw reliability histogram(s) on the GPU -> (count int64 [V, n_bins], sum_conf float64, sum_pos int64).
    ``probabilities``: foreground probability (or ``[..., 2]``), float32; ``n_volumes`` > 1 treats the
    leading axis as independent volumes (one launch for a whole test split)."""
    p = _foreground(probabilities, np.ndim(target) if not isinstance(target, torch.Tensor) else target.dim())
    p = _flat(p, torch.float32, n_volumes)
    t = _flat(target, torch.uint8, n_volumes)
    m = _flat(mask, torch.uint8, n_volumes)
    if threshold_range is not None:  # numpyfunctions.py:39-43: open interval on the confidence
        lo, hi = threshold_range
        keep = ((p < hi) & (p > lo)).to(torch.uint8)
        m = keep if m is None else (m != 0).to(torch.uint8) * keep
    return _ece_unpack(_ece_launch(p, t, m, n_bins).cpu(), n_volumes, n_bins)


def bin_ids(p, n_bins=10):
    """Bin index per voxel exactly as ``np.digitize(p, linspace(0, 1+1e-8, n_bins+1)) - 1``."""
    p = _to_dev(p, torch.float32).reshape(-1)
    ids = torch.empty(p.numel(), device=p.device, dtype=torch.uint8)
    _lib.check(_lib.load().rcu_ece_bin_ids(_lib.ptr(p), p.numel(), _lib.ece_thresholds(n_bins), n_bins, _lib.ptr(ids),
                                           _lib.current_stream()))
    return ids.cpu().numpy()


def _bin_proportions(bin_weighting, bin_count, non_zero_bins, n_dim):
    # numpyfunctions.py:72-83
    if bin_weighting == 'proportion':
        return bin_count / bin_count.sum()
    if bin_weighting == 'log_proportion':
        return np.log(bin_count) / np.log(bin_count).sum()
    if bin_weighting == 'power_proportion':
        return bin_count ** (1 / n_dim) / (bin_count ** (1 / n_dim)).sum()
    if bin_weighting == 'mean_proportion':
        return 1 / non_zero_bins.sum()
    raise ValueError('unknown bin weighting "{}"'.format(bin_weighting))


def ece_from_histogram(count, sum_conf, sum_pos, n_dim=3, out_bins=None, bin_weighting='proportion'):
    """numpyfunctions.py:65-69 and 14-22 on one volume's raw histogram."""
    nonzero = count != 0
    bin_count = count[nonzero]
    pos_frac = sum_pos[nonzero] / bin_count
    mean_confidence = sum_conf[nonzero] / bin_count
    if out_bins is not None:
        out_bins['bins_count'] = bin_count
        out_bins['bins_avg_confidence'] = mean_confidence
        out_bins['bins_positive_fraction'] = pos_frac
        out_bins['bins_non_zero'] = nonzero
    return (np.abs(mean_confidence - pos_frac) * _bin_proportions(bin_weighting, bin_count, nonzero, n_dim)).sum()


def ece_binary(probabilities, target, n_bins=10, threshold_range: tuple = None, mask=None, out_bins: dict = None,
               bin_weighting='proportion'):
    n_dim = target.dim() if isinstance(target, torch.Tensor) else np.ndim(target)
    count, sum_conf, sum_pos = calibration_histogram(probabilities, target, n_bins, mask, threshold_range)
    return ece_from_histogram(count[0], sum_conf[0], sum_pos[0], n_dim, out_bins, bin_weighting)


# ------------------------------------------------------ everything the evaluation asks of a probability map, from ONE resident copy
class SubjectBatch:
    """``count`` subjects of ``n`` voxels each, resident on the device as [count, n] arrays: foreground probability (float32), prediction,
    target and (optionally) evaluation mask (uint8).  Filled slot by slot from pinned staging buffers (numpy arrays) or device tensors;
    ``metrics`` runs every per-voxel scan of the evaluation script on it in one launch each."""

    def __init__(self, count, n, device=None, with_mask=False):
        self.count, self.n = int(count), int(n)
        self.device = torch.device(device) if device is not None else _device()
        self.with_mask = bool(with_mask)
        shape = (self.count, self.n)
        self.p = torch.empty(shape, device=self.device, dtype=torch.float32)
        self.prediction = torch.empty(shape, device=self.device, dtype=torch.uint8)
        self.target = torch.empty(shape, device=self.device, dtype=torch.uint8)
        self.mask = torch.empty(shape, device=self.device, dtype=torch.uint8) if with_mask else None
        self._pinned = None
        self._staged = set()        # (entry, slot) pairs filled on the host since the last upload
        self.used = 0
        self.shapes = {}            # slot -> the shape its prediction was put with (what the 'components' scan labels)

    def _staging(self):
        if self._pinned is None:       # one pinned image of the batch: the slots are filled on the host, the batch goes up in four copies
            shape = (self.count, self.n)
            self._pinned = {'p': torch.empty(shape, dtype=torch.float32, pin_memory=True),
                            'prediction': torch.empty(shape, dtype=torch.uint8, pin_memory=True),
                            'target': torch.empty(shape, dtype=torch.uint8, pin_memory=True)}
            if self.with_mask:
                self._pinned['mask'] = torch.empty(shape, dtype=torch.uint8, pin_memory=True)
        return self._pinned

    def put(self, slot, p, prediction, target, mask=None):
        """Subject ``slot`` of the batch: numpy arrays (staged in pinned memory, uploaded by ``upload``) or device tensors (copied in place)."""
        arrays = {'p': p, 'prediction': prediction, 'target': target}
        if self.with_mask:
            if mask is None:
                raise ValueError('this batch was made with a mask')
            arrays['mask'] = mask
        for key, a in arrays.items():
            dst_dev = getattr(self, key)[slot]
            if isinstance(a, torch.Tensor) and a.is_cuda:
                dst_dev.copy_(a.reshape(-1).to(dst_dev.dtype), non_blocking=True)
            else:
                a = np.asarray(a)
                if a.size != self.n:
                    raise ValueError('subject of {} voxels in a batch of {}-voxel slots'.format(a.size, self.n))
                dst = self._staging()[key][slot].numpy()
                np.copyto(dst, a.reshape(-1), casting='unsafe')      # (bool / int64 label maps -> uint8, as torch's cast on the device would)
                self._staged.add((key, slot))
        self.used = max(self.used, slot + 1)
        self.shapes[slot] = tuple(int(v) for v in (prediction.shape if hasattr(prediction, 'shape') else np.shape(prediction)))

    def upload(self):
        """Host-staged entries -> device (entries that were put as device tensors are there already and stay untouched)."""
        for key in ('p', 'prediction', 'target', 'mask'):
            slots = sorted(s_ for k_, s_ in self._staged if k_ == key)
            if not slots:
                continue
            host, dev = self._pinned[key], getattr(self, key)
            if slots == list(range(slots[0], slots[-1] + 1)):       # the usual case: a run of slots, one copy
                dev[slots[0]:slots[-1] + 1].copy_(host[slots[0]:slots[-1] + 1], non_blocking=True)
            else:
                for s_ in slots:
                    dev[s_].copy_(host[s_], non_blocking=True)
        self._staged = set()

    def metrics(self, n_bins=10, thresholds=UE_THRESHOLDS, want=('minmax', 'ece', 'ue'), levels=1000, connectivity=26, bands=10, merge_radius=0,
                patch=(1, 4, 4), accuracy_per_mille=500):
        """-> dict of host arrays over the ``used`` subjects: ``min`` / ``max`` (float32), ``hist`` = (count, sum_conf, sum_pos) of the
        reliability histogram inside the mask, ``counts`` [used, len(thresholds), 8] of the uncertainty-error action on the WHOLE volume
        (bin-eval/eval_uncertainty.py:176-202 uses no mask; tp, tn, fp, fn of it are the confusion matrix of ece_dice) and, with
        ``'ue_hist'`` in ``want``, ``ue_hist`` uint64 [used, 4, levels]: the level histogram of ``uncertainty_histogram_from_p``, on the whole
        volume like the counts.  One launch per scan for all subjects, one synchronisation for all results.  With ``'components'`` in
        ``want``, ``components`` = per subject the pair (table of the prediction's components with the target as the other map and the
        entropy of p as the uncertainty, table of the target's components with the prediction as the other map) of ``component_table``,
        labelled under ``connectivity`` in the shapes the subjects were put with -- from the resident maps, all subjects in one call.  With
        ``'boundary'`` in ``want``, ``boundary`` = per subject the triple (``boundary_table`` of ``bands`` bands with the entropy of p as the
        uncertainty, ``surface_distance_histograms``, the level histogram ``ue_hist_off_border`` [4, levels] of the voxels outside the
        target's border shell ``boarder_mask(target, 1, 1)``), all subjects of one shape in one call per kernel.  With ``'calib_levels'`` in
        ``want``, ``calib_levels`` uint64 [used, 3, levels] and ``calib_totals`` uint64 [used, 2, 4]: the calibration level histogram of
        ``calibration_levels`` inside the mask, exactly as ``hist`` uses it, in one launch.  With ``'lesions'`` in ``want``, ``lesions`` = per
        subject the triple of ``lesion_tables`` (entropy of p as the uncertainty, ``connectivity``, ``merge_radius``), all subjects of one shape
        through each kernel in one call; with ``'components'`` as well the prediction is labelled once for both.  With ``'patches'`` in
        ``want``, ``patch_hist`` uint64 [used, 3, levels]: ``patch_histogram`` of the grid of ``patch`` windows at the accuracy cut
        ``accuracy_per_mille``, with the entropy of p as the uncertainty, on the whole volume like ``ue_hist``; all subjects of one shape in one
        call per kernel, the patch tables never leave the device."""
        v = self.used
        out, keep = {}, []
        p, prediction, target = self.p[:v], self.prediction[:v], self.target[:v]
        if 'minmax' in want:
            lo, hi = torch.aminmax(p, dim=1)
            keep.append(('minmax', torch.stack([lo, hi])))
        if 'ece' in want:
            keep.append(('ece', _ece_launch(p, target, None if self.mask is None else self.mask[:v], n_bins)))
        if 'ue' in want:
            keep.append(('ue', _unc_counts_from_p_launch(p, prediction, target, None, thresholds)))
        if 'ue_hist' in want:
            keep.append(('ue_hist', _unc_hist_launch(p, None, prediction, target, None, levels)))
        if 'calib_levels' in want:
            calib = _calib_curve_launch(p, target, None if self.mask is None else self.mask[:v], levels)
            keep.extend([('calib_levels', calib[0]), ('calib_totals', calib[1])])
        if 'patches' in want:
            keep.append(('patch_hist', self._patches(v, _check_patch(patch), _check_levels(levels), _check_per_mille(accuracy_per_mille))))
        if 'components' in want or 'lesions' in want:
            regions = self._regions(v, connectivity, 'components' in want, _check_merge_radius(merge_radius) if 'lesions' in want else None)
            out.update({key: value for key, value in zip(('components', 'lesions'), regions) if value is not None})
        if 'boundary' in want:
            out['boundary'] = self._boundary(v, _check_bands(bands), levels)
        host = {k: t.cpu() for k, t in keep}          # (the first .cpu() waits for the stream: the others are ready by then)
        if 'minmax' in host:
            mm = host['minmax'].numpy()
            out['min'], out['max'] = mm[0].copy(), mm[1].copy()
        if 'ece' in host:
            out['hist'] = _ece_unpack(host['ece'], v, n_bins)
        if 'ue' in host:
            out['counts'] = host['ue'].numpy()
        if 'ue_hist' in host:
            out['ue_hist'] = host['ue_hist'].numpy().view(np.uint64)
        for key in ('calib_levels', 'calib_totals', 'patch_hist'):
            if key in host:
                out[key] = host[key].numpy().view(np.uint64)
        return out

    def _by_shape(self, v):
        """(slots, dims, p, prediction, target) per distinct shape of the first ``v`` subjects: subjects of one size are of one shape but for
        transposed images, so the scans that need the shape take one call per shape (the whole arrays, or a gathered copy)."""
        shapes = [self.shapes[slot] for slot in range(v)]
        for shape in sorted(set(shapes)):
            slots = [slot for slot in range(v) if shapes[slot] == shape]
            index = slice(v) if len(slots) == v else torch.as_tensor(slots, device=self.device)
            yield slots, _volume_dims(shape), self.p[index], self.prediction[index], self.target[index]

    def _regions(self, v, connectivity, want_components, merge_radius):
        """-> (the 'components' pairs or None, the 'lesions' triples or None; ``merge_radius`` None: no lesions).  The prediction's labelling
        and its table serve both."""
        pairs, triples = ([None] * v if want_components else None), ([None] * v if merge_radius is not None else None)
        for slots, dims, p, pr, tg in self._by_shape(v):
            labelling = _labelling_on_device(pr, dims, connectivity)
            of_prediction = _tables_of_labels(*labelling, tg, _lib.RCU_CC_UNC_P, p)
            if want_components:
                of_target = _component_tables_on_device(tg, dims, pr, _lib.RCU_CC_UNC_NONE, None, connectivity)
                for k, slot in enumerate(slots):
                    pairs[slot] = (of_prediction[k], of_target[k])
            if merge_radius is not None:
                found = _lesion_tables_on_device(pr, tg, dims, _lib.RCU_CC_UNC_P, p, connectivity, merge_radius, labelling, of_prediction)
                for k, slot in enumerate(slots):
                    triples[slot] = found[k]
        return pairs, triples

    def _patches(self, v, patch, levels, accuracy_per_mille):
        """-> device int64 [v, 3, levels]: the patch histograms of the first ``v`` subjects, one table and one histogram launch per shape."""
        out = None
        for slots, dims, p, pr, tg in self._by_shape(v):
            hist = _patch_hist_on_device(_patch_table_on_device(pr, tg, None, _lib.RCU_CC_UNC_P, p, dims, patch), levels, accuracy_per_mille)
            if len(slots) == v:
                return hist
            if out is None:
                out = torch.empty((v, 3, levels), device=self.device, dtype=torch.int64)
            out[torch.as_tensor(slots, device=self.device)] = hist
        return out

    def _boundary(self, v, bands, levels):
        triples = [None] * v
        for slots, dims, p, pr, tg in self._by_shape(v):
            for k, triple in enumerate(_boundary_on_device(p, pr, tg, dims, bands, levels)):
                triples[slots[k]] = triple
        return triples


# ---------------------------------------------------------------------- uncertainty-error counts
def _uncertainty_counts_device(prediction, target, uncertainty, thresholds, mask, n_volumes):
    """-> device int64 ``[n_volumes, len(thresholds), 8]`` (see ``uncertainty_counts``); asynchronous on the current stream."""
    u, is64 = _float_map(uncertainty, n_volumes)
    return _unc_counts_launch(u, is64, _flat(prediction, torch.uint8, n_volumes), _flat(target, torch.uint8, n_volumes),
                              _flat(mask, torch.uint8, n_volumes), thresholds)


def uncertainty_counts(prediction, target, uncertainty, thresholds=UE_THRESHOLDS, mask=None, n_volumes=1):
    """int64 ``[n_volumes, len(thresholds), 8]`` = tp, tn, fp, fn, tpu, tnu, fpu, fnu with
    uncertain := uncertainty > threshold (numpyfunctions.py:86-107), all thresholds in one GPU pass."""
    return _uncertainty_counts_device(prediction, target, uncertainty, thresholds, mask, n_volumes).cpu().numpy()


def from_p_supported(thresholds):
    """True when the library's table of the reference's uncertain-voxel sets covers these thresholds (strictly ascending, each one of
    bin-eval/eval_uncertainty.py:239's eleven): ``uncertainty_counts_from_p`` then reproduces the reference's counts integer for integer."""
    thresholds = [float(t) for t in thresholds]
    if not 1 <= len(thresholds) <= _lib.RCU_MAX_THRESHOLDS:
        return False
    return bool(_lib.load().rcu_unc_from_p_supported(_thresholds_array(thresholds), len(thresholds)))


def uncertainty_counts_from_p(prediction, target, foreground_probability, thresholds=UE_THRESHOLDS, mask=None, n_volumes=1):
    """``uncertainty_counts`` for uncertainty = ToEntropy([1 - p, p]) (the 'probabilities' confidence entry, analysis.py:249-252) computed
    from the float32 probability map itself: "uncertain" is looked up in the table of the reference's own float32 sets (include/rcu.h,
    rcu_unc_counts_from_p; fixture g20), so neither an entropy map nor a device log enters -- the counts are the reference's."""
    return _unc_counts_from_p_launch(_flat(foreground_probability, torch.float32, n_volumes), _flat(prediction, torch.uint8, n_volumes),
                                     _flat(target, torch.uint8, n_volumes), _flat(mask, torch.uint8, n_volumes), thresholds).cpu().numpy()


class EntropyOfProbability:
    """What ``ToEntropy`` leaves under ``uncertainty``: the normalised entropy of ``[1 - p, p]`` as a function of the float32 foreground
    map it holds.  The uncertainty-error strategies hand the MAP to ``uncertainty_counts_from_p`` (exact counts, no entropy volume);
    anything that wants the array (``np.asarray``, arithmetic, indexing) gets the device-computed float64 map, made once."""

    def __init__(self, foreground_probability):
        self.foreground_probability = foreground_probability
        self._array = None

    def materialise(self):
        if self._array is None:
            self._array = normalised_entropy(self.foreground_probability).cpu().numpy()
        return self._array

    def __array__(self, dtype=None, copy=None):
        a = self.materialise()
        return a if dtype is None else a.astype(dtype)

    shape = property(lambda self: tuple(self.foreground_probability.shape))
    dtype = np.dtype(np.float64)

    def __getitem__(self, item):
        return self.materialise()[item]

    def __gt__(self, other):
        return self.materialise() > other

    def min(self):
        return self.materialise().min()

    def max(self):
        return self.materialise().max()


# ------------------------------------------------ quantile rescale of unbounded uncertainty maps (EXTENSION; include/rcu.h "Quantile rescale")
QUANTILES = 1000                     # default number of boundaries Q (= the default number of levels of the level histograms)
QUANTILE_PLAN = (16, 16)             # digit widths of the radix passes, from the top of the key: the run is read twice
QUANTILE_PLAN_NARROW = (16, 8, 8)    # ... where the second pass's table of the default plan would not fit QUANTILE_TABLE_BYTES
QUANTILE_TABLE_BYTES = 1 << 30
QUANTILE_POPULATIONS = ('all', 'mask')


def float_key(values):
    """The order-preserving uint32 of float32 values (include/rcu.h: -0.0 as +0.0; ``~b`` below zero, ``b | 0x80000000`` else).  NaN has no key."""
    b = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)
    b = np.where(b == np.uint32(0x80000000), np.uint32(0), b)
    return np.where(b >> np.uint32(31) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_float(keys):
    """The float32 value of a key (the inverse of ``float_key`` up to the sign of zero)."""
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    return np.where(k >> np.uint32(31) != 0, k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def quantile_ranks(n, quantiles):
    """r_k = ceil(k n / Q) for k = 1 .. Q-1, in Python integers."""
    n, q = int(n), int(quantiles)
    return [(k * n + q - 1) // q for k in range(1, q)]


def _check_quantiles(quantiles):
    if not 2 <= int(quantiles) <= _lib.RCU_UNC_HIST_MAX_LEVELS:
        raise ValueError('quantiles must be in 2..{}, got {}'.format(_lib.RCU_UNC_HIST_MAX_LEVELS, quantiles))
    return int(quantiles)


def _check_plan(plan):
    plan = tuple(int(b) for b in plan)
    if not plan or sum(plan) != 32 or any(not 1 <= b <= 16 for b in plan):
        raise ValueError('the digit widths of a quantile plan must lie in 1..16 and add up to 32, got {}'.format(plan))
    return plan


class QuantileTable:
    """Q, the population size N, the Q-1 boundary keys (uint32) and their ranks r_k (int64, 1-based), and which population they are of."""

    def __init__(self, quantiles, n, keys, ranks, population='all'):
        self.Q, self.N = int(quantiles), int(n)
        self.keys = np.ascontiguousarray(keys, dtype=np.uint32)
        self.ranks = np.ascontiguousarray(ranks, dtype=np.int64)
        self.population = population
        if self.keys.shape != (self.Q - 1,) or self.ranks.shape != (self.Q - 1,):
            raise ValueError('a quantile table of Q = {} has {} boundaries'.format(self.Q, self.Q - 1))

    values = property(lambda self: key_float(self.keys))

    def __eq__(self, other):
        return (isinstance(other, QuantileTable) and (self.Q, self.N, self.population) == (other.Q, other.N, other.population)
                and np.array_equal(self.keys, other.keys) and np.array_equal(self.ranks, other.ranks))


def quantile_refine(hist, ranks, slots=None, prefixes=None):
    """One step of the selection, on the host in integers: ``hist`` is the pass's ``[slots, 2^bits]`` table, ``ranks[k]`` boundary k's residual
    rank (1-based) inside row ``slots[k]`` (default: row 0), ``prefixes[s]`` the key prefix row s stands for (default: the one empty prefix 0).
    -> (digits, ranks inside those digits, the distinct prefixes ``prefix << bits | digit`` of the next pass in increasing order, each boundary's
    row among them).  No device."""
    hist = np.asarray(hist)
    if hist.ndim != 2 or hist.shape[1] < 2 or hist.shape[1] & (hist.shape[1] - 1):
        raise ValueError('hist must be [slots, 2^bits], got {}'.format(hist.shape))
    bits = hist.shape[1].bit_length() - 1
    ranks = [int(r) for r in ranks]
    slots = [0] * len(ranks) if slots is None else [int(s) for s in slots]
    prefixes = [0] * hist.shape[0] if prefixes is None else [int(p) for p in prefixes]
    if len(prefixes) != hist.shape[0] or len(slots) != len(ranks):
        raise ValueError('one prefix per row of hist and one slot per rank')
    digits, inside, grown = [], [], []
    cumulative = {}
    for rank, slot in zip(ranks, slots):
        if slot not in cumulative:
            cumulative[slot] = np.cumsum(hist[slot].astype(np.int64))        # (a run has fewer than 2^63 voxels)
        c = cumulative[slot]
        if not 1 <= rank <= int(c[-1]):
            raise ValueError('rank {} outside row {} of {} voxels'.format(rank, slot, int(c[-1])))
        d = int(np.searchsorted(c, rank, side='left'))                       # the first digit whose cumulative count reaches the rank
        digits.append(d)
        inside.append(rank - (int(c[d - 1]) if d else 0))
        grown.append((prefixes[slot] << bits) | d)
    next_prefixes = sorted(set(grown))
    index = {p: i for i, p in enumerate(next_prefixes)}
    return digits, inside, next_prefixes, [index[p] for p in grown]


def _key_hist_launch(maps, mask, prefixes, shift, bits, hist, counts):
    """rcu_key_hist over device ``[v, n]`` float32 maps (and uint8 mask or None): adds to the device int64 ``hist`` and ``counts`` [2]."""
    v, n = maps.shape
    lib = _lib.load()
    table = (ctypes.c_uint32 * max(len(prefixes), 1))(*prefixes)
    ws = torch.empty(max(lib.rcu_key_hist_workspace_bytes(len(prefixes)), 8), device=maps.device, dtype=torch.uint8)
    _lib.check(lib.rcu_key_hist(_lib.ptr(maps), _lib.ptr(mask), n, v, table, len(prefixes), int(shift), int(bits), _lib.ptr(hist), _lib.ptr(counts),
                                _lib.ptr(ws), _lib.current_stream()))


def key_histogram(maps, mask=None, prefixes=(), shift=16, bits=16, n_volumes=1, out=None):
    """One radix pass (include/rcu.h, rcu_key_hist) over ``n_volumes`` float32 volumes -> (int64 ``[max(len(prefixes), 1), 2^bits]`` counts,
    NaNs among the population voxels, population voxels).  ``out``: a device (hist, counts) pair of an earlier call that is added to and
    returned as it is (nothing waits)."""
    maps = _flat(maps, torch.float32, n_volumes)
    mask = _flat(mask, torch.uint8, n_volumes, maps, 'map and mask')
    prefixes = [int(p) for p in prefixes]
    if out is None:
        hist = torch.zeros((max(len(prefixes), 1), 1 << int(bits) if 1 <= int(bits) <= 16 else 1), device=maps.device, dtype=torch.int64)
        counts = torch.zeros(2, device=maps.device, dtype=torch.int64)
    else:
        hist, counts = out
    _key_hist_launch(maps, mask, prefixes, shift, bits, hist, counts)
    if out is not None:
        return out
    counts = counts.cpu().numpy()
    return hist.cpu().numpy(), int(counts[0]), int(counts[1])


def _volumes(volumes_iter):
    """``volumes_iter``: a callable that returns a fresh iterator, or something that can be iterated again -> (subject, map, mask or None)."""
    for item in (volumes_iter() if callable(volumes_iter) else volumes_iter):
        subject, map_, mask = item if len(item) == 3 else (item[0], item[1], None)
        yield subject, map_, mask


def quantile_table(volumes_iter, quantiles=QUANTILES, plan=None, population=None):
    """The exact quantile table of a run (include/rcu.h, "Quantile rescale"): ``volumes_iter`` yields ``(subject, map, mask or None)`` per
    subject and is walked once per radix pass -- the default plan ``(16, 16)`` reads the run twice; where the D prefixes that survive the
    first pass would need more than 1 GiB for its second table (D * 2^16 * 8 bytes) the plan is ``(16, 8, 8)``.  ``plan``: forced digit
    widths (they add up to 32).  One resident int64 table per pass collects the whole run; the host refines it in integers
    (``quantile_refine``).  A NaN inside the population is refused with a ValueError that names the subject.  -> QuantileTable."""
    q = _check_quantiles(quantiles)
    forced = plan is not None
    plan = _check_plan(plan if forced else QUANTILE_PLAN)
    dev = _device()
    ranks = slots = None
    prefixes, n_total, shift, done = [], None, 32, 0
    masked = False
    while done < len(plan):
        bits = plan[done]
        shift -= bits
        hist = torch.zeros((max(len(prefixes), 1), 1 << bits), device=dev, dtype=torch.int64)
        per_subject = []
        for subject, map_, mask in _volumes(volumes_iter):
            counts = torch.zeros(2, device=dev, dtype=torch.int64)
            maps = _flat(map_, torch.float32, 1)
            _key_hist_launch(maps, _flat(mask, torch.uint8, 1, maps, 'map and mask of subject {}'.format(subject)), prefixes, shift, bits, hist, counts)
            per_subject.append((subject, counts))
            masked = masked or mask is not None
        if not per_subject:
            raise ValueError('quantile_table: no volumes')
        totals = torch.stack([c for _, c in per_subject]).cpu().numpy()
        for (subject, _), (nans, _) in zip(per_subject, totals):
            if nans:
                raise ValueError('quantile_table: subject {} holds {} NaN value(s) inside the population; a NaN has no rank'.format(subject, int(nans)))
        n_pass = int(totals[:, 1].sum())
        if n_total is None:
            n_total = n_pass
            if n_total == 0:
                raise ValueError('quantile_table: the population is empty')
            ranks, slots = quantile_ranks(n_total, q), [0] * (q - 1)
        elif n_pass != n_total:
            raise ValueError('quantile_table: the run changed between two passes ({} population voxels, then {})'.format(n_total, n_pass))
        _, ranks, prefixes, slots = quantile_refine(hist.cpu().numpy(), ranks, slots, prefixes or None)
        done += 1
        if done == 1 and not forced and len(prefixes) * (1 << plan[1]) * 8 > QUANTILE_TABLE_BYTES:
            plan = QUANTILE_PLAN_NARROW
    keys = np.array([prefixes[s] for s in slots], dtype=np.uint32)
    return QuantileTable(q, n_total, keys, quantile_ranks(n_total, q), population or ('mask' if masked else 'all'))


QUANTILE_COLUMNS = ('k', 'rank', 'key', 'value')


def save_quantiles(table, path):
    """``k, rank, key, value`` per boundary; ``key`` (the uint32 in decimal) is authoritative, ``value`` the float32's shortest round-trip text.
    The first data row is ``0, N, Q, population kind``."""
    import csv
    with open(path, 'w', newline='') as f:
        writer = csv.writer(f)
        writer.writerow(QUANTILE_COLUMNS)
        writer.writerow([0, table.N, table.Q, table.population])
        for k, (rank, key, value) in enumerate(zip(table.ranks, table.keys, table.values), start=1):
            writer.writerow([k, int(rank), int(key), str(value)])


def load_quantiles(path):
    import csv
    with open(path, newline='') as f:
        rows = list(csv.reader(f))
    if len(rows) < 2 or tuple(rows[0]) != QUANTILE_COLUMNS or rows[1][0] != '0' or rows[1][3] not in QUANTILE_POPULATIONS:
        raise ValueError('{} is not a quantile table'.format(path))
    n, q = int(rows[1][1]), int(rows[1][2])
    body = rows[2:]
    if len(body) != q - 1 or [int(r[0]) for r in body] != list(range(1, q)):
        raise ValueError('{}: {} boundaries for Q = {}'.format(path, len(body), q))
    return QuantileTable(q, n, [int(r[2]) for r in body], [int(r[1]) for r in body], rows[1][3])


def quantile_rescale(table, map_, return_levels=False):
    """The rank transform of a map under a QuantileTable (include/rcu.h, rcu_quantile_apply): a device float32 tensor of ``(l + 0.5) / Q`` in the
    map's shape, l = #{k : key(u) > b_k}; with ``return_levels`` also the levels themselves (an int16 tensor: Q <= 4096)."""
    shape = tuple(map_.shape)
    src = _to_dev(map_, torch.float32).reshape(-1)
    lib = _lib.load()
    out = torch.empty_like(src)
    levels = torch.empty(src.shape, device=src.device, dtype=torch.int16) if return_levels else None
    bounds = (ctypes.c_uint32 * (table.Q - 1))(*[int(k) for k in table.keys])
    ws = torch.empty(max(lib.rcu_quantile_apply_workspace_bytes(table.Q), 8), device=src.device, dtype=torch.uint8)
    _lib.check(lib.rcu_quantile_apply(_lib.ptr(src), src.numel(), bounds, table.Q, _lib.ptr(out), _lib.ptr(levels), _lib.ptr(ws), _lib.current_stream()))
    out = out.reshape(shape)
    return (out, levels.reshape(shape)) if return_levels else out


# ------------------------------------------------ threshold-free uncertainty-error metrics from a level histogram (EXTENSION)
UE_LEVELS = 1000       # default number of levels: every threshold of UE_THRESHOLDS is then a level boundary k / 1000
UE_CURVE_KEYS = ('n', 'n_errors', 'auroc', 'auprc', 'aurc', 'eaurc', 'ue_dice_max', 'ue_dice_max_threshold')


def _histogram(source, is64, prediction, target, levels, mask, n_volumes):
    return _unc_hist_launch(source, is64, _flat(prediction, torch.uint8, n_volumes), _flat(target, torch.uint8, n_volumes),
                            _flat(mask, torch.uint8, n_volumes), levels).cpu().numpy().view(np.uint64)


def uncertainty_histogram(prediction, target, uncertainty, levels=UE_LEVELS, mask=None, n_volumes=1):
    """uint64 ``[n_volumes, 4, levels]``: per volume the joint histogram of (confusion cell tp, tn, fp, fn; uncertainty level), with
    level(u) = #{k in 1..levels-1 : u > k / levels} compared in float64 (include/rcu.h, rcu_unc_hist), in one GPU pass.  For every k the
    sums over the levels >= k are the "uncertain" counts ``uncertainty_counts`` returns for the threshold k / levels, the sums over all
    levels its base counts.  Accepts what ``uncertainty_counts`` accepts; an ``EntropyOfProbability`` goes through
    ``uncertainty_histogram_from_p`` (no entropy volume)."""
    if isinstance(uncertainty, EntropyOfProbability):
        return uncertainty_histogram_from_p(prediction, target, uncertainty.foreground_probability, levels, mask, n_volumes)
    return _histogram(*_float_map(uncertainty, n_volumes), prediction, target, levels, mask, n_volumes)


def uncertainty_histogram_from_p(prediction, target, foreground_probability, levels=UE_LEVELS, mask=None, n_volumes=1):
    """``uncertainty_histogram`` for uncertainty = ToEntropy([1 - p, p]), from the float32 foreground-probability map itself: the entropy
    is computed in registers with ``normalised_entropy``'s arithmetic, so the result equals
    ``uncertainty_histogram(..., normalised_entropy(p))`` integer for integer and the float64 map is never made."""
    return _histogram(_flat(foreground_probability, torch.float32, n_volumes), None, prediction, target, levels, mask, n_volumes)


def _rank_metrics(groups):
    """(auroc, auprc) of ranking positives above negatives by a score, ties counted half, from the ascending sequence of (positives,
    negatives) per distinct score.  Python integers, every ratio rounded once:
      auroc   sum_g pos_g (neg_{<g} + neg_g / 2) / (P N): twice the numerator is an integer, one division
      auprc   sum_{g: pos_g > 0} (pos_g / P) (pos_{>=g} / n_{>=g}): scores descending, math.fsum of the terms
    NaN where undefined (P = 0 or N = 0 for auroc, P = 0 for auprc)."""
    groups = list(groups)
    n_pos, n_neg = sum(pos for pos, _ in groups), sum(neg for _, neg in groups)
    below, twice = 0, 0
    for pos, neg in groups:
        twice += pos * (2 * below + neg)
        below += neg
    terms, pos_ge, n_ge = [], 0, 0
    for pos, neg in reversed(groups):
        pos_ge += pos
        n_ge += pos + neg
        if pos:
            terms.append((pos * pos_ge) / (n_pos * n_ge))
    nan = float('nan')
    return twice / (2 * n_pos * n_neg) if n_pos and n_neg else nan, math.fsum(terms) if n_pos else nan


def ue_curve_metrics(hist):
    """Threshold-free uncertainty-error metrics of ONE level histogram ``[4, B]`` (cells tp, tn, fp, fn; a subject's, or the sum of
    several subjects': histograms add) -> dict with the keys ``UE_CURVE_KEYS``.  Host arithmetic on Python integers, every ratio rounded once.
    With e_l = fp_l + fn_l (errors of level l), c_l = tp_l + tn_l, n_l = e_l + c_l and totals E, C, N:
      auroc   sum_l e_l (C_{<l} + c_l / 2) / (E C): the probability that an erroneous voxel is ranked more uncertain than a correct one,
              ties counted half (sklearn.metrics.roc_auc_score(error, level))
      auprc   sum_{l: e_l > 0} (e_l / E) (E_{>=l} / N_{>=l}): average precision of detecting errors, levels descending
              (sklearn.metrics.average_precision_score(error, level))
      aurc    sum_{l: n_l > 0} (n_l / N) (E_{<=l} / N_{<=l}): mean selective risk, voxels accepted from the most certain level upwards, a
              whole level at a time;  eaurc = aurc minus the same sum for the ideal ranking of the same E and N at the same coverages
      ue_dice_max, ue_dice_max_threshold   the maximum over k = 1..B-1 of ``error_dice`` on the counts at the threshold k / B, and the
              smallest such threshold that attains it
    Undefined cases (E = 0 or C = 0 for auroc, E = 0 for auprc, N = 0 for all four) are ``float('nan')``."""
    h = np.asarray(hist)
    if h.ndim != 2 or h.shape[0] != 4 or h.shape[1] < 2:
        raise ValueError('expected one level histogram of shape [4, levels >= 2], got {}'.format(h.shape))
    tp, tn, fp, fn = ([int(v) for v in row] for row in h)
    levels = len(tp)
    e = [fp[l] + fn[l] for l in range(levels)]
    c = [tp[l] + tn[l] for l in range(levels)]
    n_errors, n_correct = sum(e), sum(c)
    n = n_errors + n_correct
    nan = float('nan')
    out = {'n': n, 'n_errors': n_errors}
    out['auroc'], out['auprc'] = _rank_metrics(zip(e, c))
    # aurc / eaurc: levels ascending
    risk, ideal, e_le, n_le = [], [], 0, 0
    for l in range(levels):
        n_l = e[l] + c[l]
        e_le += e[l]
        n_le += n_l
        if n_l:
            risk.append((n_l * e_le) / (n * n_le))
            ideal.append((n_l * max(0, n_le - n_correct)) / (n * n_le))
    out['aurc'] = math.fsum(risk) if n else nan
    out['eaurc'] = out['aurc'] - math.fsum(ideal) if n else nan
    # uncertainty-error Dice at its best threshold: suffix sums from the top
    fp_all, fn_all = sum(fp), sum(fn)
    dice_at, tpu, tnu, fpu, fnu = [None] * levels, 0, 0, 0, 0
    for k in range(levels - 1, 0, -1):
        tpu, tnu, fpu, fnu = tpu + tp[k], tnu + tn[k], fpu + fp[k], fnu + fn[k]
        dice_at[k] = error_dice(fp_all, fn_all, tpu, tnu, fpu, fnu)
    best = max(range(1, levels), key=lambda k: (dice_at[k], -k))
    out['ue_dice_max'] = dice_at[best]
    out['ue_dice_max_threshold'] = best / levels
    return out


# ------------------------------------------------ calibration metrics from a level histogram (EXTENSION)
CALIB_CURVE_KEYS = ('n', 'n_pos', 'brier', 'nll', 'bias', 'ece', 'mce', 'ace', 'ks', 'brier_reliability', 'brier_resolution', 'brier_uncertainty')
CALIB_RECAL_KEYS = ('brier_recal', 'nll_recal', 'ece_recal')
_Q_ONE = 1 << 32          # the integer of a confidence of 1: Q(p) = rint(clamp(p, 0, 1) * 2^32)
_NLL_ONE = 1 << 20        # the integer of an NLL term of 1: N = rint(l * 2^20)
_P_FLOOR = 2.0 ** -23     # the probability floor of the NLL (include/rcu.h, rcu_calib_curve; rcu_temperature_nll's convention)


def calibration_thresholds(levels=UE_LEVELS):
    """float32 [levels - 1]: the thresholds t_k of the calibration level histogram, ``rcu_ece_thresholds``' for any number of levels (host only)."""
    return np.array(_lib.calib_curve_thresholds(levels)[:int(levels) - 1], dtype=np.float32)


def calibration_levels(probabilities, target, levels=UE_LEVELS, mask=None, n_volumes=1):
    """The calibration level histogram in one GPU pass (include/rcu.h, rcu_calib_curve) -> (``levels`` uint64 [n_volumes, 3, B], ``totals``
    uint64 [n_volumes, 2, 4]).  level(p) = #{k : p >= t_k} on the thresholds of ``calibration_histogram`` extended to B levels (merging B / n
    consecutive levels gives its n-bin histogram for every n that divides B); planes: voxels with target == 0, with target != 0, sum of
    Q(p) = rint(p * 2^32); totals per target class: n, sum Q(p), sum rint(p^2 * 2^32), sum rint(l * 2^20) of the NLL terms.  Takes the
    foreground map the way ``calibration_histogram`` does.  Integers: the results of disjoint voxel sets (subjects of a run) add."""
    p = _foreground(probabilities, np.ndim(target) if not isinstance(target, torch.Tensor) else target.dim())
    out, totals = _calib_curve_launch(_flat(p, torch.float32, n_volumes), _flat(target, torch.uint8, n_volumes), _flat(mask, torch.uint8, n_volumes),
                                      levels)
    return out.cpu().numpy().view(np.uint64), totals.cpu().numpy().view(np.uint64)


def _level_rows(levels):
    h = np.asarray(levels)
    if h.ndim != 2 or h.shape[0] != 3 or h.shape[1] < 2:
        raise ValueError('expected one calibration level histogram of shape [3, levels >= 2], got {}'.format(h.shape))
    return ([int(v) for v in row] for row in h)


def _pava(blocks):
    """Pool adjacent violators on [positives, count] blocks in ascending order (exact: fractions compared by cross-multiplication)."""
    out = []
    for pos, cnt in blocks:
        out.append([pos, cnt, 1])
        while len(out) > 1 and out[-2][0] * out[-1][1] > out[-1][0] * out[-2][1]:
            pos_, cnt_, k_ = out.pop()
            out[-1][0] += pos_
            out[-1][1] += cnt_
            out[-1][2] += k_
    return out


def isotonic_levels(levels):
    """float64 [B]: the isotonic (monotone non-decreasing) recalibration map of one level histogram ``[3, B]`` -- pool-adjacent-violators over
    the non-empty levels with weight = voxels of the level and value = its positive fraction, what
    ``sklearn.isotonic.IsotonicRegression(y_min=0, y_max=1)`` fits on (level, target) per voxel.  An empty level takes the value of the
    nearest non-empty level below it, leading empty levels the first value (NaN everywhere for an empty histogram)."""
    n0, n1, _ = _level_rows(levels)
    filled = [l for l in range(len(n0)) if n0[l] + n1[l]]
    out = np.full(len(n0), np.nan)
    if not filled:
        return out
    values = []
    for pos, cnt, k in _pava([n1[l], n0[l] + n1[l]] for l in filled):
        values.extend([pos / cnt] * k)
    cursor, current = 0, values[0]
    for l in range(len(n0)):
        if cursor < len(filled) and filled[cursor] == l:
            current = values[cursor]
            cursor += 1
        out[l] = current
    return out


def calibration_curve_metrics(levels, totals, bins=10, mass_bins=10, recalibration=None):
    """Calibration metrics of ONE level histogram ``levels`` [3, B] with its class totals ``totals`` [2, 4] (a subject's, or the sum of several
    subjects': the integers add) -> dict with the keys ``CALIB_CURVE_KEYS``.  Host arithmetic on Python integers and float64.  With n0_l, n1_l
    the voxels of level l per class, n_l their sum, S_l the level's sum of Q, and n_y, S1_y, S2_y, N_y the totals of class y:
      brier    (S2_0 + n_1 2^32 - 2 S1_1 + S2_1) / (n 2^32): mean of (p - y)^2;   nll  (N_0 + N_1) / (n 2^20);   bias  S1 / (n 2^32) - n_1 / n
      ece      the equal-width ECE of ``ece_from_histogram`` on the levels merged into ``bins`` bins (``bins`` must divide B);  mce  the largest
               |mean confidence - positive fraction| of a non-empty merged bin
      ace      equal-mass ECE at level resolution: level l goes to mass bin min(M - 1, floor(M C_l / n)), M = ``mass_bins``, C_l the voxels of the
               lower levels;  sum_b |S_b - n1_b 2^32| / (n 2^32)
      ks       max_l |sum_{l' <= l} (S_l' - n1_l' 2^32)| / (n 2^32): the Kolmogorov-Smirnov calibration error, evaluated at the level boundaries
      brier_reliability, brier_resolution, brier_uncertainty   Murphy's decomposition over the levels with forecast f_l = S_l / (n_l 2^32) and
               o_l = n1_l / n_l: sum n_l (f_l - o_l)^2 / n, sum n_l (o_l - o)^2 / n, o (1 - o);  reliability - resolution + uncertainty is the
               Brier score of the level-mean forecast
    An empty selection (n = 0) gives NaN for everything but the counts.  ``recalibration``: a map g [B] (``isotonic_levels`` of ANOTHER run's
    pooled histogram, typically the validation run's) adds ``CALIB_RECAL_KEYS``, computed from the counts alone with every voxel of level l at
    g_l: brier_recal; nll_recal with g clipped to [2^-23, 1 - 2^-23]; ece_recal over the distinct values of g."""
    n0, n1, sq = _level_rows(levels)
    t = np.asarray(totals)
    if t.shape != (2, 4):
        raise ValueError('expected class totals of shape [2, 4], got {}'.format(t.shape))
    t = [[int(v) for v in row] for row in t]
    B = len(n0)
    bins, mass_bins = int(bins), int(mass_bins)
    if bins < 1 or B % bins:
        raise ValueError('bins = {} does not divide the {} levels'.format(bins, B))
    if mass_bins < 1:
        raise ValueError('mass_bins must be >= 1, got {}'.format(mass_bins))
    g = None
    if recalibration is not None:
        g = np.asarray(recalibration, dtype=np.float64).reshape(-1)
        if g.size != B:
            raise ValueError('the recalibration map has {} levels, the histogram {}'.format(g.size, B))
    n, n_pos = t[0][0] + t[1][0], t[1][0]
    if n != sum(n0) + sum(n1) or n_pos != sum(n1):
        raise ValueError('the class totals and the level histogram count different voxels')
    nan = float('nan')
    out = {'n': n, 'n_pos': n_pos}
    if n == 0:
        out.update({k: nan for k in CALIB_CURVE_KEYS[2:]})
        if g is not None:
            out.update({k: nan for k in CALIB_RECAL_KEYS})
        return out
    one = n * _Q_ONE
    out['brier'] = (t[0][2] + n_pos * _Q_ONE - 2 * t[1][1] + t[1][2]) / one
    out['nll'] = (t[0][3] + t[1][3]) / (n * _NLL_ONE)
    out['bias'] = (t[0][1] + t[1][1] - n_pos * _Q_ONE) / one
    # equal width: the reference's histogram of `bins` bins
    width = B // bins
    merged = [(sum(n0[b:b + width]) + sum(n1[b:b + width]), sum(sq[b:b + width]), sum(n1[b:b + width])) for b in range(0, B, width)]
    count = np.array([m[0] for m in merged], dtype=np.int64)
    out['ece'] = float(ece_from_histogram(count, np.array([m[1] / _Q_ONE for m in merged]), np.array([m[2] for m in merged], dtype=np.int64)))
    out['mce'] = max(abs(s_ - pos * _Q_ONE) / (cnt * _Q_ONE) for cnt, s_, pos in merged if cnt)
    # equal mass and Kolmogorov-Smirnov: levels ascending
    gap = [0] * mass_bins
    below, running, ks = 0, 0, 0
    for l in range(B):
        d = sq[l] - n1[l] * _Q_ONE
        gap[min(mass_bins - 1, (mass_bins * below) // n)] += d
        below += n0[l] + n1[l]
        running += d
        ks = max(ks, abs(running))
    out['ace'] = sum(abs(d) for d in gap) / one
    out['ks'] = ks / one
    # Murphy's decomposition over the non-empty levels
    base = n_pos / n
    rel, res = [], []
    for l in range(B):
        n_l = n0[l] + n1[l]
        if n_l:
            f_l, o_l = sq[l] / (n_l * _Q_ONE), n1[l] / n_l
            rel.append(n_l * (f_l - o_l) ** 2)
            res.append(n_l * (o_l - base) ** 2)
    out['brier_reliability'] = math.fsum(rel) / n
    out['brier_resolution'] = math.fsum(res) / n
    out['brier_uncertainty'] = base * (1.0 - base)
    if g is not None:
        used = [l for l in range(B) if n0[l] + n1[l]]
        if any(not 0.0 <= g[l] <= 1.0 for l in used):       # (NaN fails both compares)
            raise ValueError('the recalibration map leaves [0, 1] (or is NaN) at a level that holds voxels')
        gc = np.clip(g, _P_FLOOR, 1.0 - _P_FLOOR)
        out['brier_recal'] = math.fsum(n0[l] * g[l] ** 2 + n1[l] * (1.0 - g[l]) ** 2 for l in used) / n
        out['nll_recal'] = -math.fsum(n1[l] * math.log(gc[l]) + n0[l] * math.log1p(-gc[l]) for l in used) / n
        groups = {}
        for l in used:
            cnt, pos = groups.get(g[l], (0, 0))
            groups[g[l]] = (cnt + n0[l] + n1[l], pos + n1[l])
        out['ece_recal'] = math.fsum(abs(cnt * value - pos) for value, (cnt, pos) in sorted(groups.items())) / n
    return out


# ------------------------------------------------ component-level metrics from connected components on the GPU (EXTENSION)
# one row per component (include/rcu.h, rcu_cc_entry: unc_max sits in front of unc_sum in memory)
COMPONENT_DTYPE = np.dtype({'names': ['root', 'voxels', 'other_voxels', 'unc_sum', 'unc_max'], 'formats': ['<i4', '<u4', '<u4', '<u8', '<u4'],
                            'offsets': [0, 4, 8, 16, 12], 'itemsize': 24})
COMPONENT_UNC_ONE = 1 << 24       # the integer of an uncertainty of 1: q(u) = rint(clamp(u, 0, 1) * 2^24)
COMPONENT_METRIC_KEYS = ('n_components', 'n_fp_components', 'fp_voxels', 'n_target_components', 'n_missed_target_components', 'auroc_fp',
                         'auprc_fp', 'dice', 'dice_filtered_max', 'dice_filtered_max_threshold')


def _volume_dims(shape):
    """(depth, height, width) of a volume of this shape: up to three axes, the missing leading ones of extent 1 (2-D images: depth 1)."""
    shape = tuple(int(v) for v in shape)
    if not 1 <= len(shape) <= 3:
        raise ValueError('a volume has one to three axes, got shape {}'.format(shape))
    return (1,) * (3 - len(shape)) + shape


def _split_volumes(shape, n_volumes):
    """The shape of ONE volume: the whole array for n_volumes = 1, else the axes behind a leading axis of n_volumes."""
    shape = tuple(int(v) for v in shape)
    if n_volumes == 1:
        return shape
    if not shape or shape[0] != n_volumes:
        raise ValueError('n_volumes = {} needs a leading axis of that extent, got shape {}'.format(n_volumes, shape))
    return shape[1:]


def _labels_on_device(mask, dims, connectivity):
    """mask: device uint8 [V, n] -> device int32 [V, n] canonical labels (0 background, else 1 + the component's smallest linear index)."""
    v, n = mask.shape
    labels = torch.empty((v, n), device=mask.device, dtype=torch.int32)
    _lib.check(_lib.load().rcu_cc_label(_lib.ptr(mask), dims[0], dims[1], dims[2], v, int(connectivity), _lib.ptr(labels), _lib.current_stream()))
    return labels


def _compact_on_device(labels):
    """-> (components per volume as a host int64 array, the workspace that holds the roots' ranks).  Waits for the stream."""
    v, n = labels.shape
    lib = _lib.load()
    ws = torch.empty(max(lib.rcu_cc_workspace_bytes(n, v), 8), device=labels.device, dtype=torch.uint8)
    counts = torch.empty(v, device=labels.device, dtype=torch.int32)
    _lib.check(lib.rcu_cc_compact(_lib.ptr(labels), n, v, _lib.ptr(counts), _lib.ptr(ws), _lib.current_stream()))
    return counts.cpu().numpy().view(np.uint32).astype(np.int64), ws


def _tables_of_labels(labels, counts, ws, other, unc_kind, unc):
    """Canonical labels [V, n] with their compaction (``_compact_on_device``) -> list of V host tables of COMPONENT_DTYPE."""
    v, n = labels.shape
    total = int(counts.sum())
    table = torch.empty(max(total, 1) * COMPONENT_DTYPE.itemsize, device=labels.device, dtype=torch.uint8)
    _lib.check(_lib.load().rcu_cc_table(_lib.ptr(labels), _lib.ptr(other), _lib.ptr(unc), int(unc_kind), n, v, _lib.ptr(ws), _lib.ptr(table), total,
                                        _lib.current_stream()))
    rows = table.cpu().numpy()[:total * COMPONENT_DTYPE.itemsize].view(COMPONENT_DTYPE)
    ends = np.cumsum(counts)
    return [rows[int(e - c):int(e)].copy() for c, e in zip(counts, ends)]


def _component_tables_on_device(mask, dims, other, unc_kind, unc, connectivity, labelling=None):
    """Device arrays [V, n] (mask, other: uint8 or None; unc as ``unc_kind`` says) -> list of V host tables of COMPONENT_DTYPE.
    ``labelling``: the mask's (labels, counts, workspace) where somebody made them already."""
    if labelling is None:
        labels = _labels_on_device(mask, dims, connectivity)
        labelling = (labels,) + _compact_on_device(labels)
    return _tables_of_labels(*labelling, other, unc_kind, unc)


def connected_components(mask, connectivity=26, n_volumes=1):
    """Connected components of a binary mask (foreground: not 0) on the GPU -> ``(labels, counts)``: ``labels`` int32 of the mask's shape, 0
    for background and 1..K per volume in raster order of the components' first voxels (scipy.ndimage.label's numbering), ``counts``
    int64 ``[n_volumes]`` = K per volume.  The mask's own shape gives depth / height / width (2-D arrays: depth 1, where connectivity 6 / 26
    are the 4- / 8-neighbourhoods); ``n_volumes`` > 1 treats the leading axis as independent volumes.  A device tensor gets a device tensor."""
    dims = _volume_dims(_split_volumes(mask.shape, n_volumes))
    m = _flat(mask, torch.uint8, n_volumes)
    labels = _labels_on_device(m, dims, connectivity)
    counts, ws = _compact_on_device(labels)
    dense = torch.empty_like(labels)
    _lib.check(_lib.load().rcu_cc_relabel(_lib.ptr(labels), m.shape[1], n_volumes, _lib.ptr(ws), _lib.ptr(dense), _lib.current_stream()))
    dense = dense.reshape(tuple(mask.shape))
    return (dense if isinstance(mask, torch.Tensor) and mask.is_cuda else dense.cpu().numpy()), counts


def canonical_labels(mask, connectivity=26, n_volumes=1):
    """The labelling before it is made dense (include/rcu.h, rcu_cc_label): int32 of the mask's shape, 0 for background, else 1 + the
    smallest linear index (C order within the volume) of the voxel's component.  Host array."""
    dims = _volume_dims(_split_volumes(mask.shape, n_volumes))
    return _labels_on_device(_flat(mask, torch.uint8, n_volumes), dims, connectivity).cpu().numpy().reshape(tuple(mask.shape))


def component_table(mask, other=None, uncertainty=None, connectivity=26, n_volumes=1):
    """One structured array (COMPONENT_DTYPE) per volume -> list of ``n_volumes`` tables, the components of ``mask`` in the order of
    ``connected_components``' labels with the fields
      root           linear index of the component's first voxel          voxels         its size
      other_voxels   its voxels where ``other`` is not 0 (0 without it)
      unc_sum        sum of q(u) over its voxels, q(u) = rint(clamp(u, 0, 1) * 2^24) in float64 (NaN -> 0);     unc_max   max of q(u)
    Integer sums: the same bits whatever the launch geometry or batching.  ``uncertainty``: a float64 or float32 map, or an
    ``EntropyOfProbability`` whose entropy is computed in registers (the table of its materialised map, integer for integer); numpy
    arrays or device tensors."""
    dims = _volume_dims(_split_volumes(mask.shape, n_volumes))
    m = _flat(mask, torch.uint8, n_volumes)
    o = _flat(other, torch.uint8, n_volumes, m, 'mask and other')
    kind, u = _uncertainty_source(uncertainty, None, n_volumes, m, 'mask and uncertainty')
    return _component_tables_on_device(m, dims, o, kind, u, connectivity)


def component_metrics(pred_table, target_table, levels=UE_LEVELS):
    """Component-level metrics of the prediction's table (other map: the target) and the target's table (other map: the prediction) --
    one subject's, or several subjects' tables concatenated: tables add by concatenation, and nothing here depends on the order of the
    rows -> dict with the keys ``COMPONENT_METRIC_KEYS``.  Host arithmetic on Python integers, every ratio rounded once.
      m_k = unc_sum_k / (voxels_k * 2^24), one float64 division: the mean uncertainty of predicted component k
      a predicted component is a false positive iff its other_voxels == 0; a target component is missed iff its other_voxels == 0
      auroc_fp, auprc_fp   detection of the false-positive components by m_k, ties counted half: the formulas of ``ue_curve_metrics`` with
                           components in place of voxels and the distinct values of m_k in place of the levels (NaN where undefined)
      dice                 2 TP / (P + T): P, TP = the sums of the prediction table's voxels, other_voxels, T = the target table's voxels
      dice_filtered_max, dice_filtered_max_threshold   over the thresholds k / levels, k = 0..levels, the predicted components with
                           m_k > k / levels (float64) removed: 2 (TP - removed other_voxels) / (P - removed voxels + T); the maximum and the
                           smallest threshold that attains it"""
    levels = int(levels)
    if levels < 1:
        raise ValueError('levels must be >= 1, got {}'.format(levels))
    voxels = [int(x) for x in pred_table['voxels']]
    overlap = [int(x) for x in pred_table['other_voxels']]
    mean = [int(s_) / (v_ * COMPONENT_UNC_ONE) for s_, v_ in zip(pred_table['unc_sum'], voxels)]
    is_fp = [o == 0 for o in overlap]
    p_all, tp, t_all = sum(voxels), sum(overlap), sum(int(x) for x in target_table['voxels'])
    out = {'n_components': len(voxels), 'n_fp_components': sum(is_fp), 'fp_voxels': sum(v_ for v_, f in zip(voxels, is_fp) if f),
           'n_target_components': len(target_table), 'n_missed_target_components': int(sum(1 for x in target_table['other_voxels'] if int(x) == 0))}
    # the distinct scores ascending, with their false-positive and true-positive component counts
    groups = {}
    for m_, f in zip(mean, is_fp):
        g = groups.setdefault(m_, [0, 0])
        g[0 if f else 1] += 1
    out['auroc_fp'], out['auprc_fp'] = _rank_metrics(groups[score] for score in sorted(groups))
    out['dice'] = _dice(tp, p_all - tp, t_all - tp)
    # component k is removed at the thresholds below m_k: at k' / levels for k' < c_k = #{k' : k' / levels < m_k}
    grid = [k / levels for k in range(levels + 1)]
    gone_voxels, gone_overlap = [0] * (levels + 2), [0] * (levels + 2)
    for m_, v_, o in zip(mean, voxels, overlap):
        c = bisect.bisect_left(grid, m_)
        gone_voxels[c] += v_
        gone_overlap[c] += o
    removed_v, removed_o = sum(gone_voxels), sum(gone_overlap)
    best, best_k = None, None
    for k in range(levels + 1):
        removed_v -= gone_voxels[k]          # now the sums over c > k
        removed_o -= gone_overlap[k]
        d = _dice(tp - removed_o, (p_all - removed_v) - (tp - removed_o), t_all - (tp - removed_o))
        if best is None or d > best:
            best, best_k = d, k
    out['dice_filtered_max'] = best
    out['dice_filtered_max_threshold'] = best_k / levels
    return out


# ------------------------------------------------ boundary-aware metrics from an exact distance transform on the GPU (EXTENSION)
# one cell per (side of the target's boundary, distance band) (include/rcu.h, rcu_boundary_cell)
BOUNDARY_DTYPE = np.dtype([('voxels', '<u8'), ('errors', '<u8'), ('unc_sum', '<u8'), ('unc_err_sum', '<u8')])
BOUNDARY_BAND_KEYS = ('error_rate', 'mean_uncertainty', 'mean_uncertainty_of_errors', 'mean_uncertainty_of_correct')
BOUNDARY_TABLE_KEYS = ('n', 'n_border', 'errors', 'errors_border_share', 'uncertainty_border_share')
SURFACE_DISTANCE_KEYS = ('hd', 'hd95', 'assd', 'n_surface_prediction', 'n_surface_target')
EDT_NONE = _lib.RCU_EDT_NONE       # the squared distance where the volume has no feature voxel


def _edt_on_device(mask, dims, zero_is_feature):
    """mask: device uint8 [V, n] -> device int32 [V, n] holding the uint32 squared distances (torch has no arithmetic on uint32: the bits)."""
    v, n = mask.shape
    out = torch.empty((v, n), device=mask.device, dtype=torch.int32)
    _lib.check(_lib.load().rcu_edt_sq(_lib.ptr(mask), dims[0], dims[1], dims[2], v, int(zero_is_feature), _lib.ptr(out), _lib.current_stream()))
    return out


def distance_transform_sq(mask, n_volumes=1, invert=False):
    """Exact squared Euclidean distance transform on the GPU -> uint32 array of the mask's shape: per voxel the squared distance (unit
    spacing) to the nearest voxel of the same volume where ``mask`` is 0 -- ``scipy.ndimage.distance_transform_edt(mask) ** 2``, as an exact
    integer -- or, with ``invert``, to the nearest voxel where it is not 0 (the transform of ``~mask``).  A volume without such a voxel is
    ``EDT_NONE`` everywhere (scipy's values there are an artefact and are not copied).  The mask's own shape gives depth / height / width
    (2-D arrays: the 2-D transform); ``n_volumes`` > 1 treats the leading axis as independent volumes.  A device tensor gets a device
    tensor (int32 holding the uint32 bits where torch lacks uint32)."""
    dims = _volume_dims(_split_volumes(mask.shape, n_volumes))
    out = _edt_on_device(_flat(mask, torch.uint8, n_volumes), dims, 0 if invert else 1).reshape(tuple(mask.shape))
    if isinstance(mask, torch.Tensor) and mask.is_cuda:
        return out.view(torch.uint32) if hasattr(torch, 'uint32') else out
    return out.cpu().numpy().view(np.uint32)


def _border_on_device(d_in, d_out, distance_in, distance_out, want_distance):
    """Device squared distances [V, n] -> (device float64 distance or None, device uint8 border mask)."""
    mask = torch.empty(d_in.shape, device=d_in.device, dtype=torch.uint8)
    distance = torch.empty(d_in.shape, device=d_in.device, dtype=torch.float64) if want_distance else None
    _lib.check(_lib.load().rcu_border_mask(_lib.ptr(d_in), _lib.ptr(d_out), d_in.numel(), int(distance_in), int(distance_out), _lib.ptr(mask),
                                           _lib.ptr(distance), _lib.current_stream()))
    return distance, mask


def boarder_mask(binary_label_map, distance_in, distance_out):
    """common/utils/labelhelper.py:12-20 on the GPU -> ``(distance float64, mask bool)``: the distance to the label map's boundary (inside: to
    the nearest background voxel, outside: to the nearest foreground voxel) and the shell of the voxels at most ``distance_in`` inside and
    ``distance_out`` outside of it.  From two exact squared transforms: the mask is compared in integers, the distance is the correctly
    rounded float64 square root -- the reference's arrays bit for bit wherever the map holds both classes.  Where it holds one class only
    the reference's values are scipy's artefact; here the distance is ``inf`` and the mask empty."""
    dims = _volume_dims(binary_label_map.shape)
    m = _flat(binary_label_map, torch.uint8, 1)
    distance, mask = _border_on_device(_edt_on_device(m, dims, 1), _edt_on_device(m, dims, 0), distance_in, distance_out, True)
    distance, mask = distance.reshape(tuple(binary_label_map.shape)), mask.reshape(tuple(binary_label_map.shape)).to(torch.bool)
    if isinstance(binary_label_map, torch.Tensor) and binary_label_map.is_cuda:
        return distance, mask
    return distance.cpu().numpy(), mask.cpu().numpy()


def _check_bands(bands):
    bands = int(bands)
    if not 1 <= bands <= _lib.RCU_BOUNDARY_MAX_BANDS:
        raise ValueError('bands must be in 1..{}, got {}'.format(_lib.RCU_BOUNDARY_MAX_BANDS, bands))
    return bands


def _uncertainty_source(uncertainty, foreground_probability, n_volumes, like, names):
    """-> (RCU_CC_UNC_* kind, device map [V, n] or None) of an uncertainty given as a float map, an ``EntropyOfProbability`` or a probability
    map; a map of another size than ``like`` is refused (``names`` differ in size)."""
    if foreground_probability is not None and uncertainty is not None:
        raise ValueError('give uncertainty or foreground_probability, not both')
    if isinstance(uncertainty, EntropyOfProbability):
        foreground_probability = uncertainty.foreground_probability
    if foreground_probability is not None:
        return _lib.RCU_CC_UNC_P, _flat(foreground_probability, torch.float32, n_volumes, like, names)
    if uncertainty is None:
        return _lib.RCU_CC_UNC_NONE, None
    u, is64 = _float_map(uncertainty, n_volumes)
    if u.shape != like.shape:
        raise ValueError('{} differ in size'.format(names))
    return (_lib.RCU_CC_UNC_F64 if is64 else _lib.RCU_CC_UNC_F32), u


def _boundary_table_on_device(prediction, target, d_in, d_out, unc_kind, unc, bands):
    """Device arrays [V, n] -> device uint8 buffer of V x 2 x (bands + 1) cells; asynchronous on the current stream."""
    v, n = target.shape
    table = torch.empty(v * 2 * (bands + 1) * BOUNDARY_DTYPE.itemsize, device=target.device, dtype=torch.uint8)
    _lib.check(_lib.load().rcu_boundary_table(_lib.ptr(prediction), _lib.ptr(target), _lib.ptr(d_in), _lib.ptr(d_out), _lib.ptr(unc), int(unc_kind),
                                              n, v, bands, _lib.ptr(table), _lib.current_stream()))
    return table


def boundary_table(prediction, target, uncertainty=None, foreground_probability=None, bands=10, n_volumes=1):
    """Structured array (BOUNDARY_DTYPE) ``[n_volumes, 2, bands + 1]``: the voxels of every volume by side of the TARGET's boundary (0:
    background, 1: foreground) and distance band -- with d the squared distance to the nearest voxel of the other class, band k < ``bands``
    holds k^2 < d <= (k + 1)^2 and the last band d > bands^2 (and every voxel of a target with one class only).  Band 0 of both sides
    together is ``boarder_mask(target, 1, 1)``'s shell.  Per cell ``voxels``, ``errors`` (prediction and target disagree), ``unc_sum`` = the
    sum of q(u) over its voxels and ``unc_err_sum`` over its error voxels, q(u) = rint(clamp(u, 0, 1) * 2^24) as in ``component_table``.
    Integer sums: the same bits whatever the batching.  The uncertainty is a float64 / float32 map or an ``EntropyOfProbability``
    (``uncertainty``), or a float32 foreground-probability map whose entropy is computed in registers (``foreground_probability``)."""
    bands = _check_bands(bands)
    dims = _volume_dims(_split_volumes(target.shape, n_volumes))
    tg = _flat(target, torch.uint8, n_volumes)
    pr = _flat(prediction, torch.uint8, n_volumes, tg, 'prediction and target')
    kind, u = _uncertainty_source(uncertainty, foreground_probability, n_volumes, tg, 'target and uncertainty')
    table = _boundary_table_on_device(pr, tg, _edt_on_device(tg, dims, 1), _edt_on_device(tg, dims, 0), kind, u, bands)
    return table.cpu().numpy().view(BOUNDARY_DTYPE).reshape(n_volumes, 2, bands + 1).copy()


def _surface_histograms_on_device(prediction, target, dims):
    """Device uint8 [V, n] label maps -> (device (volume, bin) index pairs of the occupied bins [K, 2], their two counts [K, 2], bins);
    asynchronous but for the size of the compaction."""
    v, n = prediction.shape
    lib = _lib.load()
    bins = int(lib.rcu_surface_distance_bins(dims[0], dims[1], dims[2]))
    hist = torch.empty((v, 2, bins), device=prediction.device, dtype=torch.int32)
    ws = torch.empty(max(lib.rcu_surface_distance_workspace_bytes(n, v), 8), device=prediction.device, dtype=torch.uint8)
    _lib.check(lib.rcu_surface_distance_hist(_lib.ptr(prediction), _lib.ptr(target), dims[0], dims[1], dims[2], v, _lib.ptr(hist), _lib.ptr(ws),
                                             _lib.current_stream()))
    where = ((hist[:, 0] != 0) | (hist[:, 1] != 0)).nonzero()       # [K, 2]: volume, bin -- in ascending order of both
    return where, hist[where[:, 0], :, where[:, 1]], bins


def _surface_histograms_to_host(where, counts, bins, n_volumes):
    where, counts = where.cpu().numpy(), counts.cpu().numpy().view(np.uint32).astype(np.int64)
    out = []
    for v in range(n_volumes):
        rows = where[:, 0] == v
        sq = where[rows, 1].astype(np.int64)
        sq[sq == bins - 1] = EDT_NONE       # the last bin: the other surface is empty
        out.append((sq, counts[rows, 0].copy(), counts[rows, 1].copy()))
    return out


def surface_distance_histograms(prediction, target, n_volumes=1):
    """The directed surface distances of two label maps -> per volume ``(sq_values, count_p_to_t, count_t_to_p)``: the distinct squared
    distances (int64, ascending) with the number of surface voxels of the prediction at that squared distance from the target's surface
    and of the target's surface voxels from the prediction's.  The surface of a map A is the voxels of A that are face-adjacent to a voxel
    outside A inside the volume (``A & ~scipy.ndimage.binary_erosion(A, border_value=1)``; medpy's ``border_value=0`` differs only where A
    touches the volume face).  Where the other surface is empty the squared distance is ``EDT_NONE``, as ``distance_transform_sq``'s."""
    dims = _volume_dims(_split_volumes(target.shape, n_volumes))
    tg = _flat(target, torch.uint8, n_volumes)
    pr = _flat(prediction, torch.uint8, n_volumes, tg, 'prediction and target')
    return _surface_histograms_to_host(*_surface_histograms_on_device(pr, tg, dims), n_volumes)


def surface_distance_metrics(hist):
    """Hausdorff distance, its 95th percentile and the average symmetric surface distance from ONE volume's ``surface_distance_histograms``
    -> dict with the keys ``SURFACE_DISTANCE_KEYS``.  Host float64 arithmetic on the integers:
      hd     the square root of the largest squared distance of either direction
      hd95   ``numpy.percentile(.., 95)`` (linear interpolation) of both directions' distances together, from the counts
      assd   the sum of sqrt(d^2) * count over both directions, added in ascending d^2, over the number of surface voxels of both
    All three are NaN if either surface is empty."""
    sq, c_pt, c_tp = hist
    sq = [int(s_) for s_ in sq]
    count = [int(a) + int(b) for a, b in zip(c_pt, c_tp)]
    n_p, n_t = sum(int(a) for a in c_pt), sum(int(b) for b in c_tp)
    out = {'n_surface_prediction': n_p, 'n_surface_target': n_t}
    if n_p == 0 or n_t == 0 or any(s_ == EDT_NONE and c for s_, c in zip(sq, count)):
        out.update(hd=float('nan'), hd95=float('nan'), assd=float('nan'))
        return out
    present = [(math.sqrt(s_), c) for s_, c in zip(sq, count) if c]
    n = n_p + n_t
    total = 0.0
    for d, c in present:
        total += d * c
    out['hd'] = present[-1][0]
    out['assd'] = total / n
    # numpy.percentile's default method: the virtual index (n - 1) * 0.95 between the two order statistics around it, numpy's _lerp
    virtual = (n - 1) * (95 / 100)
    lo = int(math.floor(virtual))
    t = virtual - lo
    hi = min(lo + 1, n - 1)

    def order_statistic(k):
        seen = 0
        for d, c in present:
            seen += c
            if k < seen:
                return d
        return present[-1][0]
    a, b = order_statistic(lo), order_statistic(hi)
    out['hd95'] = b - (b - a) * (1 - t) if t >= 0.5 else a + (b - a) * t
    return out


def boundary_metrics(table):
    """Host arithmetic on ONE boundary table ``[2, bands + 1]`` (a subject's, or the sum of several subjects': tables add) -> dict with
      per side and band, float64 ``[2, bands + 1]`` (NaN for an empty denominator): ``error_rate`` = errors / voxels, ``mean_uncertainty`` =
          unc_sum / (voxels * 2^24), ``mean_uncertainty_of_errors`` = unc_err_sum / (errors * 2^24), ``mean_uncertainty_of_correct`` =
          (unc_sum - unc_err_sum) / ((voxels - errors) * 2^24)
      per table: ``n``, ``n_border`` (band 0 of both sides: the border shell), ``errors``, ``errors_border_share`` = the share of the errors
          that lie in the shell, ``uncertainty_border_share`` = the share of the summed uncertainty that lies there (NaN for 0 / 0)
    Python integers, every ratio rounded once."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[0] != 2 or t.shape[1] < 2:
        raise ValueError('expected one boundary table of shape [2, bands + 1], got {}'.format(t.shape))
    nan = float('nan')

    def ratio(num, den):
        return num / den if den else nan
    out = {k: np.full(t.shape, nan, dtype=np.float64) for k in BOUNDARY_BAND_KEYS}
    n = n_border = errors = errors_border = unc = unc_border = 0
    for s_ in range(2):
        for b in range(t.shape[1]):
            vox, err, us, ues = (int(t[s_, b][k]) for k in ('voxels', 'errors', 'unc_sum', 'unc_err_sum'))
            out['error_rate'][s_, b] = ratio(err, vox)
            out['mean_uncertainty'][s_, b] = ratio(us, vox * COMPONENT_UNC_ONE)
            out['mean_uncertainty_of_errors'][s_, b] = ratio(ues, err * COMPONENT_UNC_ONE)
            out['mean_uncertainty_of_correct'][s_, b] = ratio(us - ues, (vox - err) * COMPONENT_UNC_ONE)
            n, errors, unc = n + vox, errors + err, unc + us
            if b == 0:
                n_border, errors_border, unc_border = n_border + vox, errors_border + err, unc_border + us
    out.update(n=n, n_border=n_border, errors=errors, errors_border_share=ratio(errors_border, errors),
               uncertainty_border_share=ratio(unc_border, unc))
    return out


def add_boundary_tables(tables):
    """The sum of boundary tables of one shape (integers: whatever the order)."""
    total = np.zeros(np.shape(tables[0]), dtype=BOUNDARY_DTYPE)
    for t in tables:
        for k in BOUNDARY_DTYPE.names:
            total[k] += t[k]
    return total


def _boundary_on_device(p, prediction, target, dims, bands, levels):
    """Everything the 'boundary' action needs of a batch of resident subjects of one shape (device arrays [V, n]; p: the float32 foreground
    probability) -> per volume (boundary table, surface histograms, level histogram off the target's border shell)."""
    v = target.shape[0]
    d_in, d_out = _edt_on_device(target, dims, 1), _edt_on_device(target, dims, 0)
    table = _boundary_table_on_device(prediction, target, d_in, d_out, _lib.RCU_CC_UNC_P, p, bands)
    _, shell = _border_on_device(d_in, d_out, 1, 1, False)
    off_border = (shell == 0).to(torch.uint8)
    ue_hist = _unc_hist_launch(p, None, prediction, target, off_border, levels)
    surfaces = _surface_histograms_to_host(*_surface_histograms_on_device(prediction, target, dims), v)
    tables = table.cpu().numpy().view(BOUNDARY_DTYPE).reshape(v, 2, bands + 1)
    hists = ue_hist.cpu().numpy().view(np.uint64)
    return [(tables[k].copy(), surfaces[k], hists[k].copy()) for k in range(v)]


# ------------------------------------------------ patch accuracy vs. patch uncertainty from a patch table on the GPU (EXTENSION)
# one row per patch of the grid (include/rcu.h, rcu_patch_table)
PATCH_DTYPE = np.dtype([('n', '<u8'), ('errors', '<u8'), ('foreground', '<u8'), ('sum_q', '<u8')])
PATCH_DEFAULT = (1, 4, 4)
_PAVPU_BASE_KEYS = ('n_patches', 'n_inaccurate', 'pavpu_max', 'pavpu_max_threshold', 'p_ac_at_max', 'p_ui_at_max', 'pavpu_mean', 'auroc', 'auprc')
PAVPU_KEYS = _PAVPU_BASE_KEYS + tuple(k + '_fg' for k in _PAVPU_BASE_KEYS)


def _check_patch(patch):
    patch = tuple(int(v) for v in patch)
    if len(patch) != 3 or not all(1 <= v <= _lib.RCU_PATCH_MAX_EXTENT for v in patch):
        raise ValueError('patch must be three extents (depth, height, width) in 1..{}, got {}'.format(_lib.RCU_PATCH_MAX_EXTENT, patch))
    return patch


def _check_per_mille(accuracy_per_mille):
    if not 0 <= int(accuracy_per_mille) <= 999:
        raise ValueError('accuracy_per_mille must be in 0..999, got {}'.format(accuracy_per_mille))
    return int(accuracy_per_mille)


def _check_levels(levels):
    if not 2 <= int(levels) <= _lib.RCU_UNC_HIST_MAX_LEVELS:
        raise ValueError('levels must be in 2..{}, got {}'.format(_lib.RCU_UNC_HIST_MAX_LEVELS, levels))
    return int(levels)


def _patch_table_on_device(prediction, target, mask, unc_kind, unc, dims, patch):
    """Device arrays [V, n] -> device int64 [V, patches, 4] holding the uint64 rows; asynchronous on the current stream."""
    v = target.shape[0]
    lib = _lib.load()
    patches = lib.rcu_patch_count(*dims, *patch)
    table = torch.empty((v, patches, 4), device=target.device, dtype=torch.int64)
    _lib.check(lib.rcu_patch_table(_lib.ptr(prediction), _lib.ptr(target), _lib.ptr(mask), _lib.ptr(unc), int(unc_kind), *dims, v, *patch,
                                   _lib.ptr(table), _lib.current_stream()))
    return table


def _patch_hist_on_device(table, levels, accuracy_per_mille):
    """Device int64 [V, patches, 4] -> device int64 [V, 3, levels] holding the uint64 counts; asynchronous on the current stream."""
    v, patches = table.shape[0], table.shape[1]
    hist = torch.empty((v, 3, levels), device=table.device, dtype=torch.int64)
    _lib.check(_lib.load().rcu_patch_hist(_lib.ptr(table), patches, v, levels, accuracy_per_mille, _lib.ptr(hist), _lib.current_stream()))
    return hist


def _patch_table_of(prediction, target, uncertainty, foreground_probability, patch, mask, n_volumes):
    dims = _volume_dims(_split_volumes(target.shape, n_volumes))
    tg = _flat(target, torch.uint8, n_volumes)
    pr = _flat(prediction, torch.uint8, n_volumes, tg, 'prediction and target')
    mk = _flat(mask, torch.uint8, n_volumes, tg, 'mask and target')
    kind, u = _uncertainty_source(uncertainty, foreground_probability, n_volumes, tg, 'target and uncertainty')
    return _patch_table_on_device(pr, tg, mk, kind, u, dims, patch)


def patch_table(prediction, target, uncertainty=None, foreground_probability=None, patch=PATCH_DEFAULT, mask=None, n_volumes=1):
    """List of ``n_volumes`` structured arrays (PATCH_DTYPE), one row per patch of the volume's grid of non-overlapping windows of ``patch`` =
    (depth, height, width) voxels, each extent in 1..16, anchored at the origin and numbered in raster order; the windows at the far edges are
    partial, a 2-D image is a volume of depth 1.  Per patch, over its voxels inside ``mask`` (all of them without one): ``n``, ``errors``
    (prediction and target disagree), ``foreground`` (prediction or target set) and ``sum_q`` = the sum of q(u) = rint(clamp(u, 0, 1) * 2^24)
    as in ``component_table`` -- the patch's mean uncertainty is sum_q / (n * 2^24).  Integer sums, one GPU lane per patch: the same rows
    whatever the batching.  The uncertainty is given as for ``boundary_table``."""
    table = _patch_table_of(prediction, target, uncertainty, foreground_probability, _check_patch(patch), mask, n_volumes)
    host = table.cpu().numpy().view(np.uint64)
    return [host[k].copy().view(PATCH_DTYPE).reshape(-1) for k in range(n_volumes)]


def patch_histogram(prediction, target, uncertainty=None, foreground_probability=None, patch=PATCH_DEFAULT, mask=None, n_volumes=1,
                    levels=UE_LEVELS, accuracy_per_mille=500):
    """uint64 ``[n_volumes, 3, levels]``: the patches of ``patch_table`` that hold a voxel, counted by cell -- 0: accurate patch that holds
    foreground, 1: inaccurate patch, 2: accurate patch of pure background; accurate := 1000 (n - errors) > accuracy_per_mille n -- and by the
    level of their mean uncertainty, level(u) = #{k in 1..levels-1 : u > k / levels} taken in integers on sum_q and n (include/rcu.h,
    rcu_patch_hist).  Table and histogram are made on the GPU; the table never leaves it."""
    levels, accuracy_per_mille = _check_levels(levels), _check_per_mille(accuracy_per_mille)
    table = _patch_table_of(prediction, target, uncertainty, foreground_probability, _check_patch(patch), mask, n_volumes)
    return _patch_hist_on_device(table, levels, accuracy_per_mille).cpu().numpy().view(np.uint64)


def patch_histogram_of_table(table, levels=UE_LEVELS, accuracy_per_mille=500):
    """``patch_histogram`` from tables that ``patch_table`` returned, in host integer arithmetic: another ``levels`` or accuracy cut needs no
    second GPU pass.  One structured array -> uint64 ``[3, levels]``; a list of them -> ``[len, 3, levels]``."""
    levels, accuracy_per_mille = _check_levels(levels), _check_per_mille(accuracy_per_mille)
    if not isinstance(table, np.ndarray):
        return np.stack([patch_histogram_of_table(t, levels, accuracy_per_mille) for t in table]) if len(table) else np.zeros((0, 3, levels), np.uint64)
    u64 = np.uint64
    n, errors, foreground, sum_q = (np.ascontiguousarray(table[k]).reshape(-1).astype(u64) for k in PATCH_DTYPE.names)
    used = n != 0
    n, errors, foreground, sum_q = n[used], errors[used], foreground[used], sum_q[used]
    accurate = u64(1000) * (n - errors) > u64(accuracy_per_mille) * n
    cell = np.where(accurate, np.where(foreground != 0, 0, 2), 1)
    # level = #{k in 1..B-1 : sum_q B > k n 2^24}: the products stay below 2^49
    level = np.where(sum_q != 0, np.minimum(u64(levels - 1), (np.maximum(sum_q, u64(1)) * u64(levels) - u64(1)) // (n << u64(24))), u64(0))
    return np.bincount(cell * levels + level.astype(np.int64), minlength=3 * levels).astype(np.uint64).reshape(3, levels)


def _pavpu_curve(accurate, inaccurate):
    """Per level k of the accurate and the inaccurate patches per level (Python integers): (pavpu, p_ac, p_ui) at the threshold k / B, where a
    patch is uncertain iff its level is >= k -- suffix sums from the top; entry 0 (no threshold) is None."""
    levels, n_acc, n_inacc = len(accurate), sum(accurate), sum(inaccurate)
    n, nan = n_acc + n_inacc, float('nan')
    curve, n_au, n_iu = [None] * levels, 0, 0
    for k in range(levels - 1, 0, -1):
        n_au, n_iu = n_au + accurate[k], n_iu + inaccurate[k]
        n_ac, n_ic = n_acc - n_au, n_inacc - n_iu
        curve[k] = ((n_ac + n_iu) / n if n else nan, n_ac / (n_ac + n_ic) if n_ac + n_ic else nan, n_iu / n_inacc if n_inacc else nan)
    return curve


def _pavpu_of(accurate, inaccurate):
    """The keys ``_PAVPU_BASE_KEYS`` from the accurate and the inaccurate patches per level (Python integers)."""
    levels = len(accurate)
    out = {'n_patches': sum(accurate) + sum(inaccurate), 'n_inaccurate': sum(inaccurate)}
    if out['n_patches'] == 0:
        out.update({k: float('nan') for k in _PAVPU_BASE_KEYS[2:]})
        return out
    curve = _pavpu_curve(accurate, inaccurate)
    best = max(range(1, levels), key=lambda k: (curve[k][0], -k))
    out['pavpu_max'], out['p_ac_at_max'], out['p_ui_at_max'] = curve[best]
    out['pavpu_max_threshold'] = best / levels
    out['pavpu_mean'] = math.fsum(c[0] for c in curve[1:]) / (levels - 1)
    out['auroc'], out['auprc'] = _rank_metrics(zip(inaccurate, accurate))
    return {k: out[k] for k in _PAVPU_BASE_KEYS}


def pavpu_curve(hist):
    """ONE patch histogram ``[3, B]`` -> the list of (pavpu, p_ac, p_ui) over all patches per level k = 0..B-1 at the threshold k / B (see
    ``pavpu_metrics``); entry 0, where there is no threshold, is None."""
    h = _one_patch_histogram(hist)
    return _pavpu_curve([a + b for a, b in zip(h[0], h[2])], h[1])


def _one_patch_histogram(hist):
    h = np.asarray(hist)
    if h.ndim != 2 or h.shape[0] != 3 or h.shape[1] < 2:
        raise ValueError('expected one patch histogram of shape [3, levels >= 2], got {}'.format(h.shape))
    return [[int(v) for v in row] for row in h]


def pavpu_metrics(hist):
    """Patch accuracy vs. patch uncertainty (Mukhoti & Gal, 2018) of ONE patch histogram ``[3, B]`` (cells accurate with foreground, inaccurate,
    accurate pure background; a subject's, or the sum of several subjects': histograms add) -> dict with the keys ``PAVPU_KEYS``.  Host
    arithmetic on Python integers, every ratio rounded once.  A patch is uncertain at the threshold k / B (k = 1..B-1) iff its level is >= k;
    with n_ac, n_au, n_ic, n_iu the accurate / inaccurate patches that are certain / uncertain there and N their sum:
      p_ac = n_ac / (n_ac + n_ic)   p(accurate | certain)        p_ui = n_iu / (n_ic + n_iu)   p(uncertain | inaccurate)
      pavpu = (n_ac + n_iu) / N
      pavpu_max, pavpu_max_threshold   the maximum of pavpu over the thresholds and the smallest threshold that attains it; p_ac_at_max,
                                       p_ui_at_max there;  pavpu_mean: the mean over the B - 1 thresholds (math.fsum)
      auroc, auprc                     of detecting the inaccurate patches by their level (``_rank_metrics``: ties counted half)
    and every key again with the suffix ``_fg`` over the patches that hold foreground only (cells 0 and 1): a volume that is mostly
    background is mostly patches that are trivially accurate and certain.  Undefined values are ``float('nan')``."""
    h = _one_patch_histogram(hist)
    out = _pavpu_of([a + b for a, b in zip(h[0], h[2])], h[1])
    out.update({k + '_fg': v for k, v in _pavpu_of(h[0], h[1]).items()})
    return out


# ------------------------------------------------ lesion-wise matching from the joint table of two labellings on the GPU (EXTENSION)
# one row per pair of labels that share a voxel (include/rcu.h, rcu_cc_pair)
PAIR_DTYPE = np.dtype([('a', '<u4'), ('b', '<u4'), ('voxels', '<u4'), ('inside_voxels', '<u4')])
PAIR_MIN_CAPACITY, PAIR_MAX_CAPACITY = 64, 1 << 26
LESION_COUNT_KEYS = ('n_lesions', 'n_predicted', 'n_matched', 'n_fp_components', 'n_missed_lesions')
LESION_METRIC_KEYS = LESION_COUNT_KEYS + ('lesion_dice', 'lesion_recall', 'lesion_precision', 'lesion_f1', 'sq', 'pq', 'auroc_unmatched',
                                          'auprc_unmatched', 'lesion_dice_filtered_max', 'lesion_dice_filtered_max_threshold',
                                          'lesion_f1_filtered_max', 'lesion_f1_filtered_max_threshold')
LESION_CURVE_KEYS = ('n_predicted', 'n_matched', 'lesion_recall', 'fdr', 'lesion_dice')
LESION_LIST_KEYS = ('lesion', 'root_index', 'voxels', 'dilated_voxels', 'n_touching', 'touching_voxels', 'overlap', 'dice', 'matched_component', 'iou')
MERGE_RADIUS_MAX = 46340        # its square stays below 2^31: the squared distances are compared as int32 bit patterns


def _next_power_of_two(x):
    return 1 << max(0, int(x) - 1).bit_length()


def pair_capacity(n_a, n_b):
    """The default slots per volume for labellings with ids up to ``n_a`` and ``n_b``: the next power of two >= 4 (n_a + n_b + 2), at least 1024."""
    return max(1024, _next_power_of_two(4 * (int(n_a) + int(n_b) + 2)))


def _pairs_launch(a, b, inside, capacity):
    """Device label maps [V, n] -> the device buffer of rcu_cc_pairs (slots, then counters); asynchronous on the current stream."""
    v, n = a.shape
    lib = _lib.load()
    nbytes = lib.rcu_cc_pairs_bytes(int(capacity), v)
    table = torch.empty(max(nbytes, 8), device=a.device, dtype=torch.uint8)
    _lib.check(lib.rcu_cc_pairs(_lib.ptr(a), _lib.ptr(b), _lib.ptr(inside), n, v, int(capacity), _lib.ptr(table), _lib.current_stream()))
    return table


def _pairs_unpack(table, capacity, v):
    """-> (counters uint32 [V, 2] = used, dropped; list of V host tables of PAIR_DTYPE sorted by (a, b)).  Only the claimed slots travel."""
    slot_bytes = (v * capacity * PAIR_DTYPE.itemsize + 255) & ~255
    counters = table[slot_bytes:slot_bytes + 8 * v].cpu().numpy().view(np.uint32).reshape(v, 2).copy()
    slots = table[:v * capacity * PAIR_DTYPE.itemsize].view(torch.int32).reshape(v, capacity, 4)
    where = (slots[:, :, 0] != 0).nonzero()        # (a claimed slot holds a > 0)
    volume = where[:, 0].cpu().numpy()
    rows = slots[where[:, 0], where[:, 1]].cpu().numpy().reshape(-1, 4)
    out = []
    for k in range(v):
        mine = np.ascontiguousarray(rows[volume == k]).view(PAIR_DTYPE).reshape(-1)
        out.append(mine[np.lexsort((mine['b'], mine['a']))].copy())
    return counters, out


def _pairs_on_device(a, b, inside, capacity):
    """``component_pairs`` for device arrays [V, n]: a table that reports dropped voxels is made again with twice the slots -- a reaction to
    a full table, at most log2 steps: the next power of two >= 2 n holds any volume's pairs."""
    v, n = a.shape
    enough = min(PAIR_MAX_CAPACITY, max(PAIR_MIN_CAPACITY, _next_power_of_two(2 * n)))
    while True:
        counters, tables = _pairs_unpack(_pairs_launch(a, b, inside, capacity), capacity, v)
        if not counters[:, 1].any():
            return tables
        if capacity >= enough:
            raise RuntimeError('rcu_cc_pairs dropped voxels at capacity {}: more pairs than the largest table holds'.format(capacity))
        capacity = min(enough, 2 * capacity)


def component_pairs(a_labels, b_labels, inside=None, n_volumes=1, capacity=None):
    """The sparse joint table of two labellings on the GPU -> one structured array (PAIR_DTYPE) per volume, sorted by (a, b): for every pair of
    a positive label a of ``a_labels`` and a positive label b of ``b_labels`` that share a voxel, ``voxels`` = how many and ``inside_voxels`` =
    how many of those where ``inside`` is not 0 (0 without it) -- ``np.unique`` over the stacked label pairs, in one pass over resident maps.
    int32 label maps (0 and negative values: background; dense labels or canonical ones), numpy arrays or device tensors.  ``capacity``:
    hash slots per volume, a power of two in 64..2^26; by default ``pair_capacity`` of the largest labels, and whenever the table reports
    dropped voxels it is made again with twice the slots, up to the next power of two >= 2 n, which always suffices.  Integer adds: the
    same table whatever the launch geometry, the batching or the capacity."""
    a = _flat(a_labels, torch.int32, n_volumes)
    b = _flat(b_labels, torch.int32, n_volumes, a, 'a_labels and b_labels')
    i = _flat(inside, torch.uint8, n_volumes, a, 'a_labels and inside')
    if capacity is None:
        n = a.shape[1]
        capacity = min(pair_capacity(min(max(int(a.max()), 0), n), min(max(int(b.max()), 0), n)),
                       max(PAIR_MIN_CAPACITY, _next_power_of_two(2 * n)), PAIR_MAX_CAPACITY)
    capacity = int(capacity)
    if not PAIR_MIN_CAPACITY <= capacity <= PAIR_MAX_CAPACITY or capacity & (capacity - 1):
        raise ValueError('capacity must be a power of two in 64..2^26, got {}'.format(capacity))
    return _pairs_on_device(a, b, i, capacity)


def _check_merge_radius(merge_radius):
    if int(merge_radius) != merge_radius or not 0 <= int(merge_radius) <= MERGE_RADIUS_MAX:
        raise ValueError('merge_radius must be an integer in 0..{}, got {}'.format(MERGE_RADIUS_MAX, merge_radius))
    return int(merge_radius)


def _labelling_on_device(mask, dims, connectivity):
    """-> (canonical labels, components per volume, the workspace with the roots' ranks) of device masks [V, n]."""
    labels = _labels_on_device(mask, dims, connectivity)
    return (labels,) + _compact_on_device(labels)


def _dense_of_labelling(labels, ws):
    dense = torch.empty_like(labels)
    _lib.check(_lib.load().rcu_cc_relabel(_lib.ptr(labels), labels.shape[1], labels.shape[0], _lib.ptr(ws), _lib.ptr(dense), _lib.current_stream()))
    return dense


def _lesion_tables_on_device(prediction, target, dims, unc_kind, unc, connectivity, merge_radius, labelling=None, pred_tables=None):
    """``lesion_tables`` for device arrays [V, n]; ``labelling`` / ``pred_tables``: the prediction's, where somebody made them already."""
    v, n = prediction.shape
    if labelling is None:
        labelling = _labelling_on_device(prediction, dims, connectivity)
    if pred_tables is None:
        pred_tables = _tables_of_labels(*labelling, target, unc_kind, unc)
    if merge_radius == 0:
        dilated = target
    else:       # the Euclidean ball: squared distance to the nearest target voxel <= r^2, compared as unsigned (EDT_NONE's int32 view is -1)
        sq = _edt_on_device(target, dims, 0)
        dilated = ((sq >= 0) & (sq <= merge_radius * merge_radius)).to(torch.uint8)
    lesions = _labelling_on_device(dilated, dims, connectivity)
    lesion_tables = _tables_of_labels(*lesions, target, _lib.RCU_CC_UNC_NONE, None)
    capacity = min(pair_capacity(labelling[1].max() if v else 0, lesions[1].max() if v else 0), PAIR_MAX_CAPACITY)
    pairs = _pairs_on_device(_dense_of_labelling(labelling[0], labelling[2]), _dense_of_labelling(lesions[0], lesions[2]), target, capacity)
    return [(pred_tables[k], lesion_tables[k], pairs[k]) for k in range(v)]


def lesion_tables(prediction, target, uncertainty=None, connectivity=26, merge_radius=0, n_volumes=1):
    """Everything the lesion-wise metrics need of a prediction and a target, on the GPU, all volumes through each kernel once -> per volume the
    triple
      components   ``component_table(prediction, target, uncertainty, connectivity)``: the predicted components
      lesions      the table (COMPONENT_DTYPE) of the target's LESIONS: with ``merge_radius`` r = 0 the target's components; with r > 0 the
                   components of the Euclidean dilation {squared distance to the nearest target voxel <= r^2} (``distance_transform_sq``), each
                   owning the target voxels inside it -- lesions closer than the dilation are one lesion (BraTS 2023, with a Euclidean ball
                   where BraTS iterates a 3 x 3 x 3 box).  ``voxels`` = the dilated size, ``other_voxels`` = the lesion's true size; a volume
                   without target voxels has no lesions
      pairs        ``component_pairs(predicted labels, lesion labels, inside=target)``, both labellings dense (1..K in table order): ``voxels`` =
                   the overlap of component a with the dilation of lesion b, ``inside_voxels`` = its overlap with the lesion itself
    Accepts what ``component_table`` accepts."""
    merge_radius = _check_merge_radius(merge_radius)
    dims = _volume_dims(_split_volumes(prediction.shape, n_volumes))
    pr = _flat(prediction, torch.uint8, n_volumes)
    tg = _flat(target, torch.uint8, n_volumes, pr, 'prediction and target')
    kind, u = _uncertainty_source(uncertainty, None, n_volumes, pr, 'prediction and uncertainty')
    return _lesion_tables_on_device(pr, tg, dims, kind, u, connectivity, merge_radius)


class _ExactSum:
    """A running sum of float64 terms that can take a term back: Shewchuk's non-overlapping partials (what ``math.fsum`` keeps) hold the
    exact sum, ``value`` rounds it once -- whatever the order of the additions and removals."""

    def __init__(self):
        self.partials = []

    def add(self, x):
        i = 0
        for y in self.partials:
            if abs(x) < abs(y):
                x, y = y, x
            hi = x + y
            lo = y - (hi - x)
            if lo:
                self.partials[i] = lo
                i += 1
            x = hi
        self.partials[i:] = [x]

    def value(self):
        return math.fsum(self.partials)


def _is_one_subject(tables):
    return len(tables) == 3 and all(isinstance(t, np.ndarray) and t.dtype.names is not None for t in tables)


def _ratio(num, den):
    return num / den if den else float('nan')


def lesion_analysis(tables, levels=UE_LEVELS, match_iou=0.5, min_lesion_voxels=0):
    """-> (metrics: dict with the keys ``LESION_METRIC_KEYS``, curve: one dict with the keys ``LESION_CURVE_KEYS`` per threshold k / levels,
    k = 0..levels, lesions: per subject one dict with the keys ``LESION_LIST_KEYS`` per kept lesion).  ``lesion_metrics`` says what they are."""
    levels, min_lesion_voxels, match_iou = int(levels), int(min_lesion_voxels), float(match_iou)
    if levels < 1:
        raise ValueError('levels must be >= 1, got {}'.format(levels))
    if not 0.5 <= match_iou < 1.0:
        raise ValueError('match_iou must be in [0.5, 1): only above an IoU of 0.5 is the matching one-to-one; got {}'.format(match_iou))
    if min_lesion_voxels < 0:
        raise ValueError('min_lesion_voxels must be >= 0, got {}'.format(min_lesion_voxels))
    subjects = [tables] if _is_one_subject(tables) else list(tables)
    grid = [k / levels for k in range(levels + 1)]
    size, mean, cut, touched_by, matched_iou = {}, {}, {}, {}, {}       # per predicted component (subject, a)
    true_size, touching = {}, {}                               # per kept lesion (subject, g): t_g, [(component id, i(a, g))]
    listed = []
    for s_, (components, lesions, pairs) in enumerate(subjects):
        for k, row in enumerate(components):
            voxels = int(row['voxels'])
            a = (s_, k + 1)
            size[a], mean[a], touched_by[a] = voxels, int(row['unc_sum']) / (voxels * COMPONENT_UNC_ONE), 0
            cut[a] = bisect.bisect_left(grid, mean[a])
        kept = {}
        for k, row in enumerate(lesions):
            if int(row['other_voxels']) >= max(min_lesion_voxels, 1):
                kept[k + 1] = row
                true_size[(s_, k + 1)] = int(row['other_voxels'])
                touching[(s_, k + 1)] = []
        for row in pairs:
            a, g = (s_, int(row['a'])), (s_, int(row['b']))
            if g in touching and int(row['voxels']) > 0:
                touching[g].append((a, int(row['inside_voxels'])))
                touched_by[a] += 1
        rows = []
        for k, row in kept.items():
            g = (s_, k)
            t_g, mine = true_size[g], sorted(touching[g])
            overlap, union = sum(i for _, i in mine), sum(size[a] for a, _ in mine)
            best, best_a = 0.0, 0
            for a, i in mine:
                iou = i / (size[a] + t_g - i)
                if iou > best:
                    best, best_a = iou, a[1]
                if iou > match_iou:
                    matched_iou[a] = iou
            rows.append({'lesion': k, 'root_index': int(row['root']), 'voxels': t_g, 'dilated_voxels': int(row['voxels']), 'n_touching': len(mine),
                         'touching_voxels': union, 'overlap': overlap, 'dice': 2 * overlap / (t_g + union),
                         'matched_component': best_a if best > match_iou else 0, 'iou': best})
        listed.append(rows)
    n_lesions, n_predicted, n_matched = len(true_size), len(size), len(matched_iou)
    total_iou = math.fsum(matched_iou.values())
    out = {'n_lesions': n_lesions, 'n_predicted': n_predicted, 'n_matched': n_matched,
           'n_fp_components': sum(1 for t in touched_by.values() if t == 0), 'n_missed_lesions': sum(1 for t in touching.values() if not t)}
    # detection of the unmatched components by their mean uncertainty: the distinct scores ascending, (unmatched, matched) counts
    groups = {}
    for a, m_ in mean.items():
        groups.setdefault(m_, [0, 0])[1 if a in matched_iou else 0] += 1
    # the filtering curve: component a is there from threshold cut_a / levels on; per-lesion sums and the exact sum of the lesions' Dice follow
    arriving = {}
    for a, c in cut.items():
        arriving.setdefault(c, []).append(a)
    of_component = {}
    for g, mine in touching.items():
        for a, i in mine:
            of_component.setdefault(a, []).append((g, i))
    overlap, union, dice = dict.fromkeys(touching, 0), dict.fromkeys(touching, 0), dict.fromkeys(touching, 0.0)
    dice_sum = _ExactSum()
    present = present_matched = present_fp = 0
    curve, best_dice, best_f1 = [], None, None
    for k in range(levels + 1):
        for a in arriving.get(k, ()):
            present += 1
            present_matched += a in matched_iou
            present_fp += touched_by[a] == 0
            for g, i in of_component.get(a, ()):
                overlap[g] += i
                union[g] += size[a]
                d = 2 * overlap[g] / (true_size[g] + union[g])
                dice_sum.add(-dice[g])
                dice_sum.add(d)
                dice[g] = d
        row = {'n_predicted': present, 'n_matched': present_matched, 'lesion_recall': _ratio(present_matched, n_lesions),
               'fdr': _ratio(present - present_matched, present), 'lesion_dice': _ratio(dice_sum.value(), n_lesions + present_fp)}
        curve.append(row)
        f1 = _ratio(2 * present_matched, n_lesions + present)
        if best_dice is None or row['lesion_dice'] > best_dice[0] or (best_dice[0] != best_dice[0] and row['lesion_dice'] == row['lesion_dice']):
            best_dice = (row['lesion_dice'], k)       # (a NaN -- nothing to judge at that threshold -- loses to any number)
        if best_f1 is None or f1 > best_f1[0] or (best_f1[0] != best_f1[0] and f1 == f1):
            best_f1 = (f1, k)
    last = curve[-1]       # m_a <= 1: the last threshold removes nothing
    out.update(lesion_dice=last['lesion_dice'], lesion_recall=_ratio(n_matched, n_lesions), lesion_precision=_ratio(n_matched, n_predicted),
               lesion_f1=_ratio(2 * n_matched, n_lesions + n_predicted), sq=_ratio(total_iou, n_matched), pq=_ratio(2 * total_iou, n_lesions + n_predicted))
    out['auroc_unmatched'], out['auprc_unmatched'] = _rank_metrics(groups[score] for score in sorted(groups))
    out.update(lesion_dice_filtered_max=best_dice[0], lesion_dice_filtered_max_threshold=best_dice[1] / levels,
               lesion_f1_filtered_max=best_f1[0], lesion_f1_filtered_max_threshold=best_f1[1] / levels)
    return out, curve, listed


def lesion_metrics(tables, levels=UE_LEVELS, match_iou=0.5, min_lesion_voxels=0):
    """Lesion-wise metrics of one subject's ``lesion_tables`` triple, or of a list of subjects' triples -- the subject is then part of every
    id, and nothing depends on the order of the subjects or of the rows -> dict with the keys ``LESION_METRIC_KEYS``.  Host arithmetic on
    Python integers, every ratio rounded once, sums of ratios exactly rounded (``math.fsum``).  With s_a and m_a = unc_sum_a / (s_a 2^24) the
    size and mean uncertainty of predicted component a, t_g the true size of lesion g (``other_voxels`` of its row), v(a, g) and i(a, g) the
    pair's ``voxels`` and ``inside_voxels``:
      lesions with t_g < ``min_lesion_voxels`` are dropped as if they were background, their pairs with them
      touch(g) = {a : v(a, g) > 0};   d_g = 2 sum_{a in touch(g)} i(a, g) / (t_g + sum_{a in touch(g)} s_a): the Dice of lesion g against the
                 union of the predicted components that touch its dilation;   a component that touches no kept lesion is a false positive
      lesion_dice   sum_g d_g / (n_lesions + n_fp_components) (BraTS 2023's lesion-wise Dice);   n_missed_lesions: touch(g) empty
      IoU(a, g) = i(a, g) / (s_a + t_g - i(a, g));   a and g MATCH iff IoU > ``match_iou``, in [0.5, 1): one-to-one, because the regions of
                 either side are disjoint;   n_matched = TP
      lesion_recall TP / n_lesions, lesion_precision TP / n_predicted, lesion_f1 2 TP / (n_lesions + n_predicted), sq = the mean IoU of the
                 matches, pq = sum IoU / (TP + (n_predicted - TP) / 2 + (n_lesions - TP) / 2) (panoptic quality, Kirillov et al. 2019)
      auroc_unmatched, auprc_unmatched   detection of the unmatched predicted components by m_a (``component_metrics``' auroc_fp formulas)
      lesion_dice_filtered_max, lesion_f1_filtered_max, each with _threshold   over the thresholds k / levels, k = 0..levels, the components
                 with m_a > k / levels (float64) removed: the maximum and the smallest threshold that attains it (Nair et al. 2020's
                 filtering of lesions by their uncertainty)
    Every ratio with a zero denominator is NaN."""
    return lesion_analysis(tables, levels, match_iou, min_lesion_voxels)[0]


def _counts(prediction, target, uncertainty, thresholds, mask=None):
    """The 8 x len(thresholds) counts of one volume: through the probability table when the uncertainty is ToEntropy's and the
    thresholds are the table's, else by comparing the uncertainty map."""
    if isinstance(uncertainty, EntropyOfProbability):
        if from_p_supported(thresholds):
            return uncertainty_counts_from_p(prediction, target, uncertainty.foreground_probability, thresholds, mask)[0]
        uncertainty = uncertainty.materialise()
    return uncertainty_counts(prediction, target, uncertainty, thresholds, mask)[0]


def uncertainty(prediction, target, thresholded_uncertainty, mask=None):
    """numpyfunctions.py:86-107 for an already thresholded (boolean) map."""
    u = _to_dev(thresholded_uncertainty, torch.uint8).to(torch.float32)
    c = uncertainty_counts(prediction, target, u, thresholds=(0.5,), mask=mask)[0, 0]
    return tuple(int(v) for v in c)


def error_dice(fp, fn, tpu, tnu, fpu, fnu):
    if ((fnu + fpu) == 0) and ((fn + fp + fnu + fpu + tnu + tpu) == 0):
        return 1.
    return (2 * (fnu + fpu)) / (fn + fp + fnu + fpu + tnu + tpu)


def error_recall(fp, fn, fpu, fnu):
    if ((fnu + fpu) == 0) and ((fn + fp) == 0):
        return 1.
    return (fnu + fpu) / (fn + fp)


def error_precision(tpu, tnu, fpu, fnu):
    if ((fnu + fpu) == 0) and ((fnu + fpu + tpu + tnu) == 0):
        return 1.
    return (fnu + fpu) / (fnu + fpu + tpu + tnu)


# ------------------------------------------------ sample agreement (EXTENSION; include/rcu.h "Sample agreement")
AGREEMENT_KEYS = ('passes', 'mean_pairwise_dice', 'min_pairwise_dice', 'pooled_pairwise_dice', 'iou_all', 'volume_mean', 'volume_cv', 'union',
                  'intersection')


def agreement_row_length(passes):
    """Entries of one ``hist`` + ``pairs`` row for T passes: (T + 1) + T (T + 1) / 2."""
    return (passes + 1) + passes * (passes + 1) // 2


def agreement_tables_on_device(plane, passes, n_volumes=1):
    """A device int32 vote plane ``[n_words, ...]`` of ``n_volumes`` equal volumes -> device int64 (hist ``[n_volumes, T + 1]``, pairs
    ``[n_volumes, T (T + 1) / 2]``, the packed upper triangle), asynchronous on the current stream (rcu_agreement_tables)."""
    passes, n_volumes = int(passes), int(n_volumes)
    if not 1 <= passes <= _lib.RCU_VOTES_MAX_PASSES:
        raise ValueError('passes must be in 1..{}, got {}'.format(_lib.RCU_VOTES_MAX_PASSES, passes))
    if plane.dtype != torch.int32 or not plane.is_contiguous() or plane.dim() < 2:
        raise ValueError('a vote plane is a contiguous int32 tensor [n_words, ...]')
    n_words, total = plane.shape[0], plane[0].numel()
    if n_words != (passes + 31) // 32:
        raise ValueError('{} passes need a plane of {} words, got {}'.format(passes, (passes + 31) // 32, n_words))
    if n_volumes < 1 or total % n_volumes:
        raise ValueError('the plane does not split into {} equal volumes'.format(n_volumes))
    hist = torch.empty((n_volumes, passes + 1), device=plane.device, dtype=torch.int64)
    pairs = torch.empty((n_volumes, passes * (passes + 1) // 2), device=plane.device, dtype=torch.int64)
    _lib.check(_lib.load().rcu_agreement_tables(_lib.ptr(plane), n_words, total // n_volumes, n_volumes, passes, _lib.ptr(hist), _lib.ptr(pairs),
                                                _lib.current_stream()))
    return hist, pairs


def unpack_pairs(packed, passes):
    """The packed upper triangle(s) ``[..., T (T + 1) / 2]`` -> symmetric ``[..., T, T]`` int64."""
    packed = np.asarray(packed, dtype=np.int64)
    iu = np.triu_indices(passes)
    full = np.zeros(packed.shape[:-1] + (passes, passes), dtype=np.int64)
    full[..., iu[0], iu[1]] = packed
    full[..., iu[1], iu[0]] = packed
    return full


def agreement_tables(votes, passes, n_volumes=1):
    """The agreement tables of a vote plane (a ``steps.SampleVotes``, or an int32 / uint32 array or tensor ``[n_words, ...]``) split into
    ``n_volumes`` equal volumes -> numpy int64 (hist ``[n_volumes, T + 1]``, pairs ``[n_volumes, T, T]`` symmetric with the sample volumes on
    the diagonal)."""
    plane = getattr(votes, 'plane', votes)
    if not isinstance(plane, torch.Tensor):
        plane = np.ascontiguousarray(plane)
        if plane.dtype == np.uint32:
            plane = plane.view(np.int32)
        plane = torch.from_numpy(plane)
    plane = plane.to(device=_device(), dtype=torch.int32).contiguous()
    hist, pairs = agreement_tables_on_device(plane, passes, n_volumes)
    return hist.cpu().numpy(), unpack_pairs(pairs.cpu().numpy(), int(passes))


def agreement_metrics(hist, pairs):
    """The structure-wise uncertainties (Roy et al., Bayesian QuickNAT, 2019) of ONE table -- a subject's, or the sum of its slices': ``hist``
    ``[T + 1]`` and ``pairs`` ``[T, T]`` symmetric (or the packed upper triangle) -> dict with ``AGREEMENT_KEYS``.  Host float64 arithmetic;
    n_i = pairs[i][i] the sample volumes, I_ij = pairs[i][j]."""
    hist = np.asarray(hist, dtype=np.int64).reshape(-1)
    t = hist.size - 1
    pairs = np.asarray(pairs, dtype=np.int64)
    if pairs.ndim == 1:
        pairs = unpack_pairs(pairs, t)
    if t < 1 or pairs.shape != (t, t):
        raise ValueError('agreement_metrics takes hist [T + 1] and pairs [T, T] of one table')
    n = np.diag(pairs).astype(np.float64)
    dices = []
    for i in range(t):
        for j in range(i + 1, t):
            den = n[i] + n[j]
            dices.append(2.0 * float(pairs[i, j]) / den if den > 0 else 1.0)
    inter_sum = float(sum(int(pairs[i, j]) for i in range(t) for j in range(i + 1, t)))
    total = float(n.sum())
    union = int(hist[1:].sum())
    mean = total / t
    return {
        'passes': t,
        'mean_pairwise_dice': float(np.mean(dices)) if dices else 1.0,
        'min_pairwise_dice': float(np.min(dices)) if dices else 1.0,
        'pooled_pairwise_dice': 2.0 * inter_sum / ((t - 1) * total) if (t > 1 and total > 0) else 1.0,
        'iou_all': float(hist[t]) / union if union > 0 else 1.0,
        'volume_mean': mean,
        'volume_cv': float(np.std(n)) / mean if mean > 0 else 0.0,
        'union': union,
        'intersection': int(hist[t]),
    }


def spearman(a, b):
    """Spearman's rank correlation of two equally long sequences: Pearson's r of the average ranks (ties share the mean of their ranks);
    NaN for fewer than two points or a constant sequence."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return pearson(average_ranks(a), average_ranks(b))


def average_ranks(x):
    x = np.asarray(x, dtype=np.float64)
    order = np.argsort(x, kind='mergesort')
    ranks = np.empty(x.size, dtype=np.float64)
    i = 0
    while i < x.size:
        j = i
        while j + 1 < x.size and x[order[j + 1]] == x[order[i]]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    return ranks


def pearson(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size != b.size:
        raise ValueError('sequences differ in length')
    if a.size < 2:
        return float('nan')
    da, db = a - a.mean(), b - b.mean()
    den = math.sqrt(float(da @ da) * float(db @ db))
    return float(da @ db) / den if den > 0 else float('nan')


def failure_auroc(score, failed, higher_is_worse):
    """AUROC of detecting the subjects with ``failed`` true by ranking them on ``score`` (through ``_rank_metrics``: ties count half);
    ``higher_is_worse`` false ranks by -score (an agreement score is LOW where the segmentation fails).  NaN without both classes."""
    score = np.asarray(score, dtype=np.float64) * (1.0 if higher_is_worse else -1.0)
    failed = np.asarray(failed, dtype=bool)
    groups = []
    for value in np.unique(score):
        here = score == value
        groups.append((int((here & failed).sum()), int((here & ~failed).sum())))
    return _rank_metrics(groups)[0]


# pymia 0.2.1 ConfusionMatrix / DiceCoefficient / Accuracy are absent from the reference tree: restated from the call sites
# (numpyfunctions.py:128-151) and pinned against scikit-learn's confusion_matrix / f1_score / accuracy_score (fixture g19); the 0 / 0
# Dice (no foreground in prediction and target) is 1, pymia's convention.
def confusion_matrx(prediction, target):
    c = uncertainty_counts(prediction, target, _zeros_like_map(prediction), thresholds=(0.5,))[0, 0]
    tp, tn, fp, fn = (int(v) for v in c[:4])
    return tp, tn, fp, fn, tp + tn + fp + fn


_zero_maps = {}
_ZERO_MAP_CACHED_ELEMENTS = 1 << 24      # maps up to 64 MB are kept (a BraTS subject: 15.7 MB; a loader batch of 32 slices: 3.1 MB)


def _zeros_like_map(a):
    """An all-zero uncertainty map of a's size (nothing is "uncertain": the first four of the eight counts are the confusion matrix).  Kept
    per size -- read-only to every kernel -- so that a subject's Dice does not start with an allocation and a memset kernel."""
    n = a.numel() if isinstance(a, torch.Tensor) else int(np.prod(np.shape(a)))
    if n > _ZERO_MAP_CACHED_ELEMENTS:
        return torch.zeros(n, device=_device(), dtype=torch.float32)
    z = _zero_maps.get(n)
    if z is None:
        if len(_zero_maps) >= 4:
            _zero_maps.clear()
        z = _zero_maps[n] = torch.zeros(n, device=_device(), dtype=torch.float32)
    return z


def confusion_counts_on_device(prediction, target):
    """Device tensors ``[N, ...]`` uint8 (N slices / images) -> device int64 ``[N, 4]`` = tp, tn, fp, fn per slice, asynchronous on the current
    stream: ``confusion_matrx``'s counts taken where the prediction is made (scripts.ConfusionOnDeviceStep).  Counts are integers: the
    rows of a subject's slices add up to the counts of the assembled subject."""
    n = prediction.shape[0]
    counts = _uncertainty_counts_device(prediction, target, _zeros_like_map(prediction), (0.5,), None, n)
    return counts[:, 0, :4].contiguous()


def dice_from_counts(tp, fp, fn):
    """Dice from ``confusion_matrx``'s integers (0 / 0 = 1: pymia's convention, see above)."""
    return _dice(int(tp), int(fp), int(fn))


def _dice(tp, fp, fn):
    den = 2 * tp + fp + fn
    return 2 * tp / den if den else 1.0


def dice(prediction, target):
    tp, tn, fp, fn, n = confusion_matrx(prediction, target)
    return _dice(tp, fp, fn)


def accuracy(prediction, target):
    tp, tn, fp, fn, n = confusion_matrx(prediction, target)
    return (tp + tn) / n if n else 0.0


def correction_results(counts):
    """All entries UncertaintyAndCorrectionEvalNumpy writes (eval.py:182-226), from the eight counts."""
    tp, tn, fp, fn, tpu, tnu, fpu, fnu = (int(c) for c in counts)
    n = tp + tn + fp + fn
    r = {'tpu': tpu, 'tnu': tnu, 'fpu': fpu, 'fnu': fnu, 'tp': tp, 'tn': tn, 'fp': fp, 'fn': fn}
    with np.errstate(divide='ignore', invalid='ignore'):
        tpu_fpu_ratio = np.float64(tpu) / np.float64(fpu)
        jaccard_index = np.float64(tp) / np.float64(tp + fp + fn)
    r['dice_benefit'] = tpu_fpu_ratio < jaccard_index
    r['accuracy_benefit'] = tpu_fpu_ratio < 1
    r['dice'] = _dice(tp, fp, fn)
    r['accuracy'] = (tp + tn) / n if n else 0.0
    # uncertain voxels set to background: tpu leave tp (become fn), fpu leave fp (become tn)
    r['corrected_dice'] = _dice(tp - tpu, fp - fpu, fn + tpu)
    r['corrected_accuracy'] = (tp - tpu + tn + fpu) / n if n else 0.0
    r['dice_benefit_correct'] = (r['corrected_dice'] > r['dice']) == r['dice_benefit']
    r['accuracy_benefit_correct'] = (r['corrected_accuracy'] > r['accuracy']) == r['accuracy_benefit']
    # uncertain voxels set to foreground: fnu become tp, tnu become fp
    r['corrected_add_dice'] = _dice(tp + fnu, fp + tnu, fn - fnu)
    r['corrected_add_accuracy'] = (tp + fnu + tn - tnu) / n if n else 0.0
    return r


# -------------------------------------------------------------------------------- preparation
def check_min_max(arr, min_=0, max_=1, only_warn=False):
    # rechun/eval/helper.py:31-47
    for bad, txt, val in ((arr.max() > max_, 'larger than {}'.format(max_), arr.max()),
                          (arr.min() < min_, 'smaller than {}'.format(min_), arr.min())):
        if bad:
            message = 'Found value {}: "{}"'.format(txt, val)
            if not only_warn:
                raise ValueError(message)
            warnings.warn(message)


def add_background_probability(probability_np):
    check_min_max(probability_np)
    return np.stack([1 - probability_np, probability_np], axis=-1)


def rescale_uncertainties(uncertainty_np, min_, max_, epsilon=1e-5):
    return (uncertainty_np - min_) / (max_ - min_) * (1 - 2 * epsilon) + epsilon


def uncertainty_to_foreground_probabilities(uncertainty_np, prediction_np):
    if prediction_np.shape != uncertainty_np.shape:
        raise ValueError('shapes must agree. Found {} and {}'.format(uncertainty_np.shape, prediction_np.shape))
    check_min_max(uncertainty_np)
    if prediction_np.max() > 1:
        raise ValueError('Found class larger than 1. Only works for binary problems')
    foreground = uncertainty_np * 0.5
    sel = prediction_np == 1
    foreground[sel] = 1 - foreground[sel]
    return foreground


def normalised_entropy(foreground_probability, as_float64=True):
    """ToEntropy (analysis.py:196-203) of ``[1-p, p]`` on the GPU, from the foreground map alone."""
    p = _to_dev(foreground_probability, torch.float32)
    out = torch.empty(p.shape, device=p.device, dtype=torch.float64 if as_float64 else torch.float32)
    _lib.check(_lib.load().rcu_normalised_entropy(_lib.ptr(p), p.numel(), _lib.ptr(out) if as_float64 else None,
                                                  None if as_float64 else _lib.ptr(out), _lib.current_stream()))
    return out


class PrepareData(abc.ABC):
    @abc.abstractmethod
    def __call__(self, to_eval: dict) -> dict:
        pass


class ComposePreparation(PrepareData):
    def __init__(self, prepare_data_list: list) -> None:
        self.prepare_data_list = prepare_data_list

    def __call__(self, to_eval: dict) -> dict:
        for prepare_data in self.prepare_data_list:
            to_eval = prepare_data(to_eval)
        return to_eval


class AddBackgroundProbabilities(PrepareData):
    def __call__(self, to_eval: dict) -> dict:
        to_eval['probabilities'] = add_background_probability(to_eval['probabilities'])
        return to_eval


class RescaleLinear(PrepareData):
    def __init__(self, entry: str, min_: float, max_: float, epsilon=1e-5) -> None:
        self.entry, self.min, self.max, self.epsilon = entry, min_, max_, epsilon

    def __call__(self, to_eval: dict) -> dict:
        to_eval[self.entry] = rescale_uncertainties(to_eval[self.entry], self.min, self.max, self.epsilon)
        return to_eval


class RescaleSubjectMinMax(PrepareData):
    def __init__(self, entry: str, epsilon=1e-5) -> None:
        self.entry, self.epsilon = entry, epsilon

    def __call__(self, to_eval: dict) -> dict:
        a = to_eval[self.entry]
        to_eval[self.entry] = rescale_uncertainties(a, a.min(), a.max(), self.epsilon)
        return to_eval


class ToForegroundProbabilities(PrepareData):
    def __call__(self, to_eval: dict) -> dict:
        to_eval['probabilities'] = uncertainty_to_foreground_probabilities(to_eval['probabilities'],
                                                                           to_eval['prediction'])
        return to_eval


class ToEntropy(PrepareData):
    def __init__(self, entropy_entry='uncertainty') -> None:
        self.nb_classes = 2
        self.entropy_entry = entropy_entry

    def __call__(self, to_eval: dict) -> dict:
        prob = to_eval['probabilities']
        if prob.shape[-1] != self.nb_classes:
            raise ValueError('last dimension of probability array ({}) must be equal to nb_classes ({})'
                             .format(prob.shape, self.nb_classes))
        # (the reference's check_min_max(..., only_warn=True) can only ever warn here: the entropy of a probability pair lies in
        # [0, 1 + 2e-7]; the map itself is made when somebody asks for it)
        to_eval[self.entropy_entry] = EntropyOfProbability(np.ascontiguousarray(prob[..., 1]))
        return to_eval


class MoveEntry(PrepareData):
    def __init__(self, from_entry: str, to_entry: str) -> None:
        self.from_entry, self.to_entry = from_entry, to_entry

    def __call__(self, to_eval: dict) -> dict:
        to_eval[self.to_entry] = to_eval[self.from_entry]
        return to_eval


class RescaleQuantile(PrepareData):
    """EXTENSION: the entry's rank transform under the run's QuantileTable (``quantile_rescale``), handed on as ``RescaleLinear`` hands its map
    on -- a host array, float32 here.  (The consumers take device tensors as well, but the preparations behind this one -- ``MoveEntry``, and the
    range check of ``check_min_max`` -- and the loaders' caches are written for host arrays: the map comes back once, 4 bytes per voxel.)"""

    def __init__(self, entry: str, table) -> None:
        self.entry, self.table = entry, table

    def __call__(self, to_eval: dict) -> dict:
        to_eval[self.entry] = quantile_rescale(self.table, to_eval[self.entry]).cpu().numpy()
        return to_eval


def _rescale_prep_and_idstr(confidence_entry, rescale_type, min_max=None):
    # analysis.py:277-285 ('global' reads the min/max CSV; here the pair is passed in)
    if rescale_type == 'quantile':       # rcu_amd extension: ``min_max`` is the run's QuantileTable; its files never collide with the _globalrescale ones
        return RescaleQuantile(confidence_entry, min_max), '_quantilerescale'
    if rescale_type == 'global':
        return RescaleLinear(confidence_entry, min_max[0], min_max[1]), '_globalrescale'
    if rescale_type == 'subject':
        return RescaleSubjectMinMax(confidence_entry), '_rescale'
    return None, ''


def get_probability_preparation(confidence_entry, id_, rescale_confidence='subject', rescale_sigma='subject',
                                min_max=None):
    """analysis.py:218-246 -> (preparation, run id with rescale suffix)."""
    if confidence_entry == 'probabilities':
        return ComposePreparation([AddBackgroundProbabilities()]), id_
    rescale = rescale_confidence if confidence_entry == 'confidence' else rescale_sigma
    prepare = []
    prep, suffix = _rescale_prep_and_idstr(confidence_entry, rescale, min_max)
    if prep is not None:
        prepare.append(prep)
    prepare.extend([MoveEntry(confidence_entry, 'probabilities'), ToForegroundProbabilities(),
                    AddBackgroundProbabilities()])
    return ComposePreparation(prepare), id_ + suffix


def get_uncertainty_preparation(confidence_entry, id_, rescale_confidence='', rescale_sigma='global', min_max=None):
    """analysis.py:249-274."""
    if confidence_entry == 'probabilities':
        return ComposePreparation([AddBackgroundProbabilities(), ToEntropy()]), id_
    rescale = rescale_confidence if confidence_entry == 'confidence' else rescale_sigma
    prepare = []
    prep, suffix = _rescale_prep_and_idstr(confidence_entry, rescale, min_max)
    if prep is not None:
        prepare.append(prep)
    prepare.append(MoveEntry(confidence_entry, 'uncertainty'))
    return ComposePreparation(prepare), id_ + suffix


# ----------------------------------------------------------------------- evaluation strategies
class EvaluationStrategy(metaclass=abc.ABCMeta):
    def __init__(self, result_entry=None) -> None:
        self.result_entry = result_entry

    @abc.abstractmethod
    def __call__(self, to_evaluate: dict, results: dict) -> None:
        pass


class ComposeEvaluation(EvaluationStrategy):
    def __init__(self, eval_strategies) -> None:
        super().__init__()
        self.eval_strategies = eval_strategies

    def __call__(self, to_evaluate: dict, results: dict) -> None:
        for eval_ in self.eval_strategies:
            eval_(to_evaluate, results)


class LambdaEvaluation(EvaluationStrategy):
    def __init__(self, lambda_fn, entry_keys: tuple, result_entry) -> None:
        super().__init__(result_entry)
        self.lamda_fn = lambda_fn
        self.entry_keys = entry_keys

    def __call__(self, to_evaluate: dict, results: dict) -> None:
        results[self.result_entry] = self.lamda_fn(*[to_evaluate[k] for k in self.entry_keys])


class DiceNumpy(EvaluationStrategy):
    def __init__(self, result_entry='dice') -> None:
        super().__init__(result_entry)

    def __call__(self, to_evaluate: dict, results: dict) -> None:
        results[self.result_entry] = dice(to_evaluate['prediction'], to_evaluate['target'])


class ConfusionMatrix(EvaluationStrategy):
    def __init__(self, result_entries=('tp', 'tn', 'fp', 'fn', 'n')) -> None:
        super().__init__(result_entries)

    def __call__(self, to_evaluate: dict, results: dict) -> None:
        for key, val in zip(self.result_entry, confusion_matrx(to_evaluate['prediction'], to_evaluate['target'])):
            results[key] = val


class EceBinaryNumpy(EvaluationStrategy):
    def __init__(self, n_bins=10, result_entry='ece', threshold_range: tuple = None, with_mask=False,
                 return_bins=False, bin_weighting='proportion') -> None:
        super().__init__(result_entry)
        self.n_bins = n_bins
        self.threshold_range = threshold_range
        self.with_mask = with_mask
        self.return_bins = return_bins
        self.bin_weighting = bin_weighting

    def __call__(self, to_evaluate: dict, results: dict) -> None:
        mask = to_evaluate['mask'] if self.with_mask else None
        out_bins = results if self.return_bins else None
        results[self.result_entry] = ece_binary(to_evaluate['probabilities'], to_evaluate['target'], self.n_bins,
                                                self.threshold_range, mask, out_bins, self.bin_weighting)


class UncertaintyErrorDiceNumpy(EvaluationStrategy):
    def __init__(self, uncertainty_threshold, result_prefix: str = None, with_mask=False) -> None:
        super().__init__()
        self.uncertainty_threshold = uncertainty_threshold
        self.prefix = '' if result_prefix is None else result_prefix + '_'
        self.with_mask = with_mask

    def __call__(self, to_evaluate: dict, results: dict):
        mask = ~to_evaluate['target_boarder'] if self.with_mask else None
        c = _counts(to_evaluate['prediction'], to_evaluate['target'], to_evaluate['uncertainty'], (self.uncertainty_threshold,), mask)[0]
        tp, tn, fp, fn, tpu, tnu, fpu, fnu = (int(v) for v in c)
        results['{}precision'.format(self.prefix)] = error_precision(tpu, tnu, fpu, fnu)
        results['{}recall'.format(self.prefix)] = error_recall(fp, fn, fpu, fnu)
        results['{}dice'.format(self.prefix)] = error_dice(fp, fn, tpu, tnu, fpu, fnu)


class UncertaintyAndCorrectionEvalNumpy(EvaluationStrategy):
    def __init__(self, uncertainty_threshold) -> None:
        super().__init__()
        self.uncertainty_threshold = uncertainty_threshold

    def __call__(self, to_evaluate: dict, results: dict) -> None:
        c = _counts(to_evaluate['prediction'], to_evaluate['target'], to_evaluate['uncertainty'], (self.uncertainty_threshold,))[0]
        results.update(correction_results(c))


class UncertaintyAndCorrectionSweep(EvaluationStrategy):
    """All thresholds of the 'bnf_ue' action (eval_uncertainty.py:176-202, 239) in ONE pass over the
    volume; ``results[threshold]`` holds what UncertaintyAndCorrectionEvalNumpy would write for it."""

    def __init__(self, thresholds=UE_THRESHOLDS) -> None:
        super().__init__()
        self.thresholds = tuple(thresholds)

    def __call__(self, to_evaluate: dict, results: dict) -> None:
        c = _counts(to_evaluate['prediction'], to_evaluate['target'], to_evaluate['uncertainty'], self.thresholds)
        for i, thr in enumerate(self.thresholds):
            results[thr] = correction_results(c[i])
