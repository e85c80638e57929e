"""Step seam: batch steps with the reference's call protocol, computing on librcu_hip.

Mirrors (names, arguments, output keys, error behaviour):
  BatchStep                     common/trainloop/steps.py:14-17
  SegmentationPredictStep       common/trainloop/steps.py:69-89
  McPredictStep                 rechun/dl/customsteps.py:10-39
  MultiPredictionSummary        rechun/dl/customsteps.py:42-71
  EnsemblePredictionStep        bin-dl/brats_test_ensemble.py:72-94
  AleatoricPredictStep          bin-dl/brats_test_aleatoric.py:51-73
  AleatoricMcPredictStep        extension (BASELINE config 'aleatoric + MC'): composition of the two above
  (both with logit_samples = S)  extension: test-time logit sampling, the predictive E_eps[softmax(mu + sigma eps)] (include/rcu.h)
  TtaMcPredictStep              extension: test-time augmentation (D4 transforms), alone or composed with MC dropout
  AffineTtaMcPredictStep        extension: test-time augmentation with bilinear affine warps (include/rcu_warp.h), alone or with MC dropout
  BatchContext / TaskContext    common/trainloop/context.py:334-355
A step is called as ``step(batch_context, task_context, context)``, reads
``batch_context.input['images']`` and writes torch tensors with the channel dim at 1 into
``batch_context.output``.

MI355X-first difference: by default the T (or K) probability volumes are never stacked in HBM.
``McPredictStep`` / ``EnsemblePredictionStep`` put a ``McStatistics`` object (per-voxel running
sums, updated by the fused forward+softmax+accumulate kernel) under ``multi_probabilities`` and
``MultiPredictionSummary`` finalises it.  ``materialize=True`` restores the reference behaviour
(a real ``[T, N, C, H, W]`` tensor), and the summary accepts either form.
"""
import abc
import fractions
import logging
import operator

import torch

from . import _lib
from . import model as model_mod


class BatchContext:
    def __init__(self, batch: dict, batch_index: int, sample_offset: int = None) -> None:
        self.input = batch
        self.batch_index = batch_index
        # global index of the batch's first sample in the run's stream of slices / images (the test loop counts them; None: batch_index x the
        # batch's size): what the seeded Dropout2d masks of a stochastic step are keyed by -- a slice's MC sample must not depend on batch_size
        self.sample_offset = sample_offset
        self.output = {}
        self.metrics = {}
        self.score = None
        self.more = {}


class TaskContext:
    def __init__(self, epoch: int = 0, task_data=None, task_data_config=None) -> None:
        self.epoch = epoch
        self.data = task_data
        self.data_config = task_data_config
        self.scores = []
        self.more = {}


class Context:
    """Base of the contexts a step accepts (reference: ctx.TorchTrainContext / ctx.TorchTestContext)."""


class TorchTestContext(Context):
    """The two attributes a step touches: ``model`` and ``device`` (common/trainloop/context.py:256-322).
    The reference hard-codes 'cuda' in its scripts (bin-dl/brats_test_default.py:39)."""

    def __init__(self, device_str: str = 'cuda', model=None) -> None:
        self.device = torch.device(device_str)
        self.model = model
        self.more = {}


def _type_error_msg(obj, *expected):
    names = ','.join(e.__name__ for e in expected)
    return 'expected type is "({})" but object is of type "{}"'.format(names, obj.__class__.__name__)


def _check_context(context):
    # The reference means to raise ValueError here (customsteps.py:17-18); its message helper trips over the
    # tuple argument first (common/utils/messages.py:5) -- the intended ValueError is what we raise.
    if not isinstance(context, Context):
        raise ValueError(_type_error_msg(context, TorchTestContext))


def set_dropout_mode(model, is_train=True):
    """common/utils/torchhelper.py:44-50: toggles only the Dropout modules; BatchNorm stays in eval."""
    # (model.UNet keeps the list of its Dropout2d modules -- its module tree is fixed after construction: no walk over 150 modules four
    # times per batch)
    sites = getattr(model, '_site_modules', None) if isinstance(model, model_mod.UNet) else None
    for m in (model.modules() if sites is None else sites):
        if isinstance(m, (torch.nn.Dropout, torch.nn.Dropout2d, torch.nn.Dropout3d)):
            if is_train:
                m.train()
            else:
                m.eval()


def job_seed(seed, step_index, job):
    """Seed of the dropout masks of MC pass ``job`` (1..T) of batch / volume ``step_index``: a function of (seed, batch, pass) only -- not
    of the pass groups, the stream lanes, the rank that runs the pass or the number of ranks."""
    return (int(seed) * 1000003 + int(step_index) * 10007 + int(job)) % (2 ** 63 - 1)


def pass_seed(seed, job):
    """Key of the library's counter-based mask draw (include/rcu.h, rcu_dropout_masks) for MC pass ``job`` (1..T): a function of (seed, pass) --
    the draw's counter carries the sample's GLOBAL index, so a slice's masks do not depend on the batch it is loaded in either."""
    return job_seed(seed, 0, job)


def first_sample_of(batch_context, n):
    """Global index of a batch's first sample: what the test loop counted (``BatchContext.sample_offset``), else batch_index x n."""
    offset = getattr(batch_context, 'sample_offset', None)
    return int(batch_context.batch_index) * int(n) if offset is None else int(offset)


class McStatistics:
    """Per-voxel sufficient statistics of the passes seen so far (the ``stats`` blob of include/rcu.h).
    Plain additive: blobs of disjoint pass subsets merge by ``+`` (one RCCL sum-reduce, see
    rcu_amd.distributed).  ``exact`` (RCU_MC_EXACT; what the predict steps use): float64 planes whose addends are rounded to multiples
    of 2^-40 first -- every addition is then exact, so the sums (and everything finalised from them) carry the same bits whatever the order of
    the passes, the pass groups, the stream lanes, the ranks and the collective's reduction tree."""

    def __init__(self, n, nb_classes, height, width, device, do_mi=False, do_var=False, blob=None, exact=False):
        self.n, self.nb_classes, self.height, self.width = n, nb_classes, height, width
        self.hw = height * width
        self.flags = self.flags_of(do_mi, do_var, exact)
        elems = self.blob_elements(n, nb_classes, self.hw, do_mi, do_var, exact)
        dtype = self.dtype_of(do_var, exact)
        if blob is None:
            blob = torch.empty(elems, device=device, dtype=dtype)
        elif blob.numel() != elems or blob.dtype != dtype or not blob.is_contiguous():
            raise ValueError('statistics blob must be a contiguous {} tensor of {} elements'.format(dtype, elems))
        self.blob = blob
        self.count = 0
        # set by the predict steps: recipe(do_mi, do_var, materialize=False) runs the SAME passes again (same inputs, same dropout
        # masks) into fresh statistics with other flags, or into a real [T, N, C, H, W] tensor
        self.recipe = None
        _lib.check(_lib.load().rcu_mc_begin(_lib.ptr(self.blob), n, self.hw, nb_classes, self.flags,
                                            _lib.current_stream()))

    @staticmethod
    def flags_of(do_mi=False, do_var=False, exact=False):
        return (_lib.RCU_MC_MI if do_mi else 0) | (_lib.RCU_MC_VAR if do_var else 0) | (_lib.RCU_MC_EXACT if exact else 0)

    @staticmethod
    def dtype_of(do_var=False, exact=False):
        return torch.float64 if (do_var or exact) else torch.float32

    @staticmethod
    def blob_elements(n, nb_classes, hw, do_mi=False, do_var=False, exact=False):
        flags = McStatistics.flags_of(do_mi, do_var, exact)
        return _lib.load().rcu_mc_stats_bytes(n, hw, nb_classes, flags) // (8 if (do_var or exact) else 4)

    @property
    def exact(self):
        return bool(self.flags & _lib.RCU_MC_EXACT)

    @property
    def do_mi(self):
        return bool(self.flags & _lib.RCU_MC_MI)

    @property
    def do_var(self):
        return bool(self.flags & _lib.RCU_MC_VAR)

    def accumulate(self, tensor, is_probabilities=False):
        """Add one ``[N, C, H, W]`` logits (softmax applied on the fly) or probability volume."""
        t = tensor.to(torch.float32).contiguous()
        if tuple(t.shape) != (self.n, self.nb_classes, self.height, self.width):
            raise ValueError('expected shape {}'.format((self.n, self.nb_classes, self.height, self.width)))
        flags = self.flags | (_lib.RCU_MC_INPUT_PROBS if is_probabilities else 0)
        _lib.check(_lib.load().rcu_mc_accumulate(_lib.ptr(t), _lib.ptr(self.blob), self.n, self.hw, self.nb_classes,
                                                 flags, _lib.current_stream()))
        self.count += 1

    def as_tensor(self):
        """The stacked ``[T, N, C, H, W]`` probabilities the reference keeps under ``multi_probabilities`` (customsteps.py:36): the
        statistics do not hold them, so the passes run again, materialised, under the same masks.  For foreign steps that read
        the key between the predict step and the summary; costs T forward passes and T volumes of HBM."""
        if self.recipe is None:
            raise ValueError('these statistics were not produced by a predict step: the passes cannot be replayed')
        return self.recipe(self.do_mi, self.do_var, materialize=True)

    def finalize(self, do_mi=False, do_var=False, count=None):
        """-> dict with the reference's keys: probabilities, entropy[, mutual_info][, variance]."""
        if do_mi and not self.do_mi:
            raise ValueError('mutual information was not tracked (construct the predict step with do_mi=True)')
        if do_var and not self.do_var:
            raise ValueError('variance was not tracked (construct the predict step with do_var=True)')
        t = self.count if count is None else count
        dev = self.blob.device
        shape1 = (self.n, 1, self.height, self.width)
        mean = torch.empty((self.n, self.nb_classes, self.height, self.width), device=dev, dtype=torch.float32)
        entropy = torch.empty(shape1, device=dev, dtype=torch.float32)
        mi = torch.empty(shape1, device=dev, dtype=torch.float32) if do_mi else None
        var = torch.empty(shape1, device=dev, dtype=torch.float32) if do_var else None
        self._finalize_into(t, mean, entropy, mi, var)
        out = {'probabilities': mean, 'entropy': entropy}
        if do_mi:
            out['mutual_info'] = mi
        if do_var:
            out['variance'] = var
        return out

    def _finalize_into(self, t, mean, entropy, mi, var):
        _lib.check(_lib.load().rcu_mc_finalize(_lib.ptr(self.blob), self.n, self.hw, self.nb_classes, int(t), self.flags,
                                               _lib.ptr(mean), _lib.ptr(entropy), _lib.ptr(mi), _lib.ptr(var),
                                               _lib.current_stream()))


# ------------------------------------------------------------------------------------------------------------------------------
# EXTENSION adaptive MC (include/rcu.h "Adaptive MC"): slices settled at a pass checkpoint are retired and finalised from fewer passes
# ------------------------------------------------------------------------------------------------------------------------------
def adaptive_threshold(tolerance, t):
    """``thr_q`` of checkpoint t: ceil((1.0 - tolerance) * t * 2^40) in exact rational arithmetic on the float64 value of ``1.0 - tolerance``
    -- the integer the leading class sum of a voxel (times 2^40) has to reach for the voxel to be settled.  Nothing rounds."""
    x = fractions.Fraction(1.0 - float(tolerance)) * int(t) * (1 << 40)
    return -((-x.numerator) // x.denominator)


def check_adaptive(adaptive, mc_steps):
    """The schedule ``dict(check_at=[t1 < t2 < ...], tolerance=eps, max_unsettled=0)`` of ``McPredictStep(adaptive=...)`` -> the same with plain
    values, or a ValueError that names the limit: 2 <= t1, the last checkpoint < T, at most 4 checkpoints, 0 <= eps < 1, max_unsettled >= 0."""
    if not isinstance(adaptive, dict):
        raise ValueError('adaptive must be a dict with the keys check_at, tolerance[, max_unsettled], got {!r}'.format(adaptive))
    unknown = set(adaptive) - {'check_at', 'tolerance', 'max_unsettled'}
    if unknown:
        raise ValueError('adaptive: unknown keys {} (check_at, tolerance, max_unsettled)'.format(sorted(unknown)))
    for key in ('check_at', 'tolerance'):
        if key not in adaptive:
            raise ValueError('adaptive: {} is missing'.format(key))
    try:
        check_at = [operator.index(t) for t in adaptive['check_at']]
    except TypeError:
        raise ValueError('adaptive: check_at must be a list of integer pass counts, got {!r}'.format(adaptive['check_at'])) from None
    if not 1 <= len(check_at) <= _lib.RCU_ADAPTIVE_MAX_CHECKPOINTS:
        raise ValueError('adaptive: check_at needs 1..{} checkpoints, got {}'.format(_lib.RCU_ADAPTIVE_MAX_CHECKPOINTS, len(check_at)))
    if any(b <= a for a, b in zip(check_at, check_at[1:])):
        raise ValueError('adaptive: check_at must be strictly increasing, got {}'.format(check_at))
    if check_at[0] < 2:
        raise ValueError('adaptive: the first checkpoint must be at least 2 passes, got {}'.format(check_at[0]))
    if check_at[-1] >= int(mc_steps):
        raise ValueError('adaptive: the last checkpoint ({}) must be below mc_steps ({})'.format(check_at[-1], mc_steps))
    tolerance = float(adaptive['tolerance'])
    if not 0.0 <= tolerance < 1.0:
        raise ValueError('adaptive: tolerance must be in [0, 1), got {}'.format(adaptive['tolerance']))
    max_unsettled = operator.index(adaptive.get('max_unsettled', 0))
    if max_unsettled < 0:
        raise ValueError('adaptive: max_unsettled must be >= 0, got {}'.format(max_unsettled))
    return dict(check_at=check_at, tolerance=tolerance, max_unsettled=max_unsettled)


def adaptive_counts(n, check_at, mc_steps, spans):
    """Pass count per slice from the index lists ``spans`` of a step over n slices: spans[0] = all slices (passes 1..t_1), spans[k] = the slices
    still active after checkpoint k (passes t_k + 1 .. t_{k+1}, the last span to T).  A slice that is in spans[k - 1] and not in spans[k] was
    retired at t_k.  -> list of n ints."""
    ends = list(check_at) + [int(mc_steps)]
    counts = [0] * n
    for k, span in enumerate(spans):
        for i in span:
            counts[i] = ends[k]
    return counts


def compact_group_size(model, m, h, w, group_pixels, plan_samples):
    """MC passes per launch of a compact batch of m slices: ``pass_group_size`` for m, capped so that no launch exceeds the ``plan_samples``
    samples of the plan the full batch reserved (``reserve_canonical_plans``): a compact span never re-plans."""
    return max(1, min(pass_group_size(model, m, h, w, group_pixels), int(plan_samples) // int(m)))


def slice_scores(stats, thr_q, out=None):
    """rcu_mc_slice_scores of exact statistics -> one int64 device tensor ``[2 n]`` (``out``): margin_q in [:n], the unsettled counts as the
    int32 view of [n:] -- one buffer, so one device-to-host copy brings both (``split_scores``)."""
    if not stats.exact:
        raise ValueError('slice scores need exact statistics (exact=True): the decision is made on exact integer sums')
    n = stats.n
    buf = torch.empty(2 * n, device=stats.blob.device, dtype=torch.int64) if out is None else out
    _lib.check(_lib.load().rcu_mc_slice_scores(_lib.ptr(stats.blob), n, stats.hw, stats.nb_classes, stats.flags, int(thr_q),
                                               _lib.ptr(buf[n:]), _lib.ptr(buf[:n]), _lib.current_stream()))
    return buf


def split_scores(buf):
    """The host copy of a ``slice_scores`` buffer -> (unsettled, margin_q), two lists of n ints."""
    host = buf.cpu()
    n = host.numel() // 2
    return host[n:].view(torch.int32)[:n].tolist(), host[:n].tolist()


def merge_slices(src, dst, index):
    """rcu_mc_merge_slices: the statistics of the m slices of ``src`` added into the slices ``index`` (int32 device tensor ``[m]``, distinct
    entries; negative ones are skipped) of ``dst``."""
    if (src.hw, src.nb_classes, src.flags) != (dst.hw, dst.nb_classes, dst.flags):
        raise ValueError('merge_slices: the two statistics differ in shape, classes or flags')
    if index.dtype != torch.int32 or index.numel() != src.n or not index.is_contiguous() or index.device != dst.blob.device:
        raise ValueError('merge_slices: index must be a contiguous int32 tensor of {} entries on the statistics device'.format(src.n))
    _lib.check(_lib.load().rcu_mc_merge_slices(_lib.ptr(src.blob), src.n, _lib.ptr(dst.blob), dst.n, dst.hw, dst.nb_classes, dst.flags,
                                               _lib.ptr(index), _lib.current_stream()))


class AdaptiveMcStatistics(McStatistics):
    """The statistics of an adaptive step: exact sums in which slice i holds the passes 1..counts[i].  ``counts``: int32 ``[n]`` on the device;
    ``checkpoints``: one record per checkpoint reached, ``dict(t=, thr_q=, active=[slice indices scored], unsettled=[...], margin_q=[...],
    retired=[slice indices retired])``; ``spans``: the index lists the pass spans ran on (``adaptive_counts``).  ``finalize`` divides every
    slice by its own count (rcu_mc_finalize_counts); the stacked tensor does not exist (slices have different pass counts): ``as_tensor``
    raises.  The ``recipe`` replays the recorded index lists -- it does not decide again."""

    def __init__(self, n, nb_classes, height, width, device, do_mi=False, do_var=False, blob=None):
        super().__init__(n, nb_classes, height, width, device, do_mi, do_var, blob=blob, exact=True)
        self.counts = None
        self.checkpoints = []
        self.spans = []
        self.passes_run = 0       # slice passes of the stochastic spans (a plain step runs n * T)

    def as_tensor(self):
        raise ValueError('adaptive MC statistics have no [T, N, C, H, W] stack: the slices have seen different numbers of passes')

    def _finalize_into(self, t, mean, entropy, mi, var):
        """Every slice by its own count (``t``, the largest of them, is not used)."""
        if self.counts is None:
            raise ValueError('adaptive MC statistics without pass counts: they are set by the predict step')
        _lib.check(_lib.load().rcu_mc_finalize_counts(_lib.ptr(self.blob), self.n, self.hw, self.nb_classes, _lib.ptr(self.counts), self.flags,
                                                      _lib.ptr(mean), _lib.ptr(entropy), _lib.ptr(mi), _lib.ptr(var), _lib.current_stream()))


class StreamLanes:
    """The launches of one batch spread over ``count`` HIP streams in turn (lane 0 = the caller's stream).  Consecutive layers of a
    forward pass depend on each other, so a stream idles while a layer's last workgroups finish and the next layer's first ones
    start; MC passes / ensemble members are independent, and a second lane fills those gaps (tools/stream_overlap_probe.py: 6.63 ->
    6.27 ms per pass on the 160-slice volume).  Every lane needs an activation workspace (``lane=`` of UNet.forward_accumulate) and a
    statistics blob of its own; blobs are plain sums, so the side lanes' are added into lane 0's at the end.  The assignment launch ->
    lane is fixed (round robin), so the result does not depend on timing.

        lanes = StreamLanes(device, 2)
        lane_stats = lanes.begin(stats, make_side_stats, inputs=(images,))
        for each launch: lanes.run(lambda st, lane: model.forward_accumulate(images, st, masks, lane=lane))
        lanes.end(merge)            # merge(stats, side_stats) on the caller's stream
    """

    _side = {}       # (device index, lane) -> stream: side streams are shared by all steps of the process

    def __init__(self, device, count):
        device = torch.device(device)
        self.count = max(1, int(count)) if device.type == 'cuda' else 1
        self.device = device
        self.streams = []
        for lane in range(1, self.count):
            key = (device.index if device.index is not None else torch.cuda.current_device(), lane)
            if key not in StreamLanes._side:
                StreamLanes._side[key] = torch.cuda.Stream(device=device)
            self.streams.append(StreamLanes._side[key])
        self._stats, self._launch, self._current = [], 0, None

    def begin(self, stats, make_side_stats, inputs=(), first=0):
        """``first``: lane of the first launch (a runner that gives a rank only two or three launches per volume rotates it from
        volume to volume, so that the lanes carry the same load over a stream of volumes)."""
        self._stats, self._launch = [stats], int(first) % self.count
        if self.count > 1:
            self._current = torch.cuda.current_stream(self.device)
            for side in self.streams:
                side.wait_stream(self._current)          # the inputs (and whatever else the caller prepared) are ready
                for t in inputs:
                    t.record_stream(side)
                with torch.cuda.stream(side):
                    self._stats.append(make_side_stats())     # zeroed on its own stream
        return self._stats

    def run(self, launch, lane=None):
        """launch(statistics of the lane, lane index) on the next lane (or on ``lane``)."""
        if lane is None:
            lane = self._launch % self.count
            self._launch += 1
        if lane == 0:
            launch(self._stats[0], 0)
        else:
            with torch.cuda.stream(self.streams[lane - 1]):
                launch(self._stats[lane], lane)

    def end(self, merge):
        for side, st in zip(self.streams, self._stats[1:]):
            self._current.wait_stream(side)
            merge(self._stats[0], st)                    # on the caller's stream, behind the lane's last launch
            for t in vars(st).values():
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(self._current)
        self._stats = self._stats[:1]


def balanced_groups(count, group, lanes):
    """Sizes of the pass groups ``count`` MC passes run in, at most ``group`` passes each, for launches that take ``lanes`` stream lanes in
    turn: rounds of one group per lane, every group of a round the same size, the last rounds smaller instead of a full group for one
    lane and nothing for the other -- T = 20 in groups of 4 on two lanes is 4 4 | 4 4 | 2 2 (10 passes per lane), not 4 4 | 4 4 | 4
    (12 against 8: the lanes fill each other's gaps only while both have work).  One lane, or a group size that divides count / lanes:
    plain groups of ``group``."""
    group, lanes, left, sizes = max(1, int(group)), max(1, int(lanes)), int(count), []
    while left > 0:
        for k in range(lanes):         # one round: lane k takes its share of what the lanes from k on still have to run
            if left <= 0:
                break
            sizes.append(min(group, -(-left // (lanes - k))))
            left -= sizes[-1]
    return sizes


def pass_group_size(model, n, h, w, group_pixels):
    """MC passes per launch for batches of n images of h x w: ``group_pixels`` worth of pixels, and no tensor of the plan beyond the 2 GB
    the Winograd kernels address (model.UNet.max_group_samples)."""
    g = max(1, int(group_pixels) // (n * h * w))
    cap = getattr(model, 'max_group_samples', None)
    return g if cap is None else max(1, min(g, cap(h, w) // n))


def reserve_canonical_plans(model, n, h, w, mc_steps, group, lanes):
    """Plans (and workspaces) of ``model`` for batches of n images of h x w whose T = ``mc_steps`` passes run up to ``group`` per launch, on
    ``lanes`` stream lanes: all sized for n * min(group, T) samples, whatever launches this process will really make."""
    plan = n * max(1, min(int(group), max(int(mc_steps), 1)))
    for lane in range(max(1, int(lanes))):
        model.reserve(h, w, plan, lane)
    return plan


def merge_statistics(stats, side):
    """Add the statistics of a side lane into ``stats`` (plain sums, include/rcu.h rcu_mc_*)."""
    stats.blob.add_(side.blob)
    stats.count += side.count
    if getattr(side, 'sigma_sum', None) is not None:
        stats.sigma_sum.add_(side.sigma_sum)


# ------------------------------------------------------------------------------------------------------------------------------
# the scheduler of the fused paths: the one-process predict steps and the sharded runners (rcu_amd.distributed) run their passes
# through ``launch_plan`` + ``run_plan`` on an engine
# ------------------------------------------------------------------------------------------------------------------------------
def launch_plan(jobs, elements=(0,), per_element=1, group=1, lanes=1, first=0, members=False):
    """The launches of one batch -> ``[(kind, lane, element, jobs)]``, in launch order; plain values in, plain values out.
    ``jobs``: the job ids this process runs -- 0 the weight-scaling pass, j >= 1 pass (j - 1) % per_element + 1 of the images transformed by
    ``elements[(j - 1) // per_element]`` (plain MC: ``elements=(0,)``), or with ``members`` ensemble member j - 1.  Kinds:
      'ws'      the weight-scaling pass: lane 0, first, outside the rotation;
      'passes'  a pass group of one element; the groups of element v are ``balanced_groups`` of its jobs, launch q on lane
                (first + v + q) % lanes (``first``: a rank of a multi-rank run rotates it with the volume);
      'fold'    after the last group of an element other than the identity: on every lane that element used, in lane order, fold the
                lane's scratch statistics into the lane's statistics (rcu_mc_fold_transformed) and restart them;
      'member'  one ensemble member, always on lane (j - 1) % lanes (the members of a lane share its workspace from batch to batch)."""
    lanes = max(1, int(lanes))
    plan = [('ws', 0, 0, (0,))] if 0 in jobs else []
    if members:
        return plan + [('member', (j - 1) % lanes, 0, (j,)) for j in jobs if j != 0]
    runs = {}
    for j in jobs:
        if j != 0:
            runs.setdefault((j - 1) // per_element, []).append(j)
    for v, run in runs.items():
        e, used, b = elements[v], set(), 0
        for q, size in enumerate(balanced_groups(len(run), group, lanes)):
            lane = (first + v + q) % lanes
            plan.append(('passes', lane, e, tuple(run[b:b + size])))
            used.add(lane)
            b += size
        if e != 0:
            plan += [('fold', lane, e, ()) for lane in sorted(used)]
    return plan


def launch_masks(engine, x, element, jobs, per_element, seed=None, first_sample=0, mask_sets=None):
    """``masks`` argument of the launch of ``jobs`` (see ``launch_plan``): injected sets (indexed by pass), the library's seeded draw under
    ``tta_pass_seed(seed, element, pass)`` (the identity's key is ``pass_seed``) at the samples' global indices, or None -- drawn inside the
    launch from the device's default generator."""
    passes = [(j - 1) % per_element + 1 for j in jobs]
    if mask_sets is not None:
        return mask_sets[passes[0] - 1] if len(passes) == 1 else [mask_sets[t - 1] for t in passes]
    if seed is None:
        return None
    return engine.seeded_masks(x, [tta_pass_seed(seed, element, t) for t in passes], first_sample)


def run_plan(plan, engine, x, stats, ws=None, lanes=1, draw=None, reserve=None, members=()):
    """Run ``plan`` (``launch_plan``) on ``engine`` over the images x into ``stats`` (the weight-scaling pass into ``ws``) on ``lanes``
    StreamLanes.  ``reserve = (passes per element, group)``: the canonical plans of the batch, on every lane, before the first forward
    (``reserve_canonical_plans``).  ``draw(element, jobs)``: the masks of a pass group, called INSIDE the launch -- on the stream of the lane
    that reads them; None: eval-mode passes (TTA alone).  ``lanes`` is the count the plan was made for (1 for engines without
    ``side_statistics``)."""
    lanes = StreamLanes(x.device, lanes)
    if reserve is not None and hasattr(engine, 'reserve'):
        engine.reserve(x, reserve[0], reserve[1], lanes.count)
    xs = {}
    for kind, _, e, _ in plan:
        if kind == 'passes' and e not in xs:
            xs[e] = x if e == 0 else tta_transform(x, e)
    lanes.begin(stats, lambda: engine.side_statistics(x), inputs=(x,) + tuple(v for e, v in xs.items() if e != 0))
    scratch = [None] * lanes.count       # per lane: the statistics of the current element's passes (elements other than the identity)

    def launch(st, lane, kind, e, jobs):
        # keywords at their defaults are left out: engines that only ever run one lane (one pass per launch) need not take them
        kw = {'lane': lane} if lane else {}
        if kind == 'member':
            engine.member_pass(members[jobs[0] - 1], x, st, **kw)
        elif kind == 'fold':
            fold_transformed(scratch[lane], st, e)
            restart_statistics(scratch[lane])
        else:
            if e != 0:
                if scratch[lane] is None:
                    scratch[lane] = engine.side_statistics(x)          # (zeroed on the lane's stream)
                st = scratch[lane]
            if draw is None:
                engine.member_pass(engine.model, xs[e], st, **kw)
                return
            if getattr(engine, 'takes_jobs', False):      # an engine that keys its passes by the pass number (AleatoricHipEngine sampling)
                kw['jobs'] = jobs
            if len(jobs) == 1:
                engine.mc_pass(xs[e], st, draw(e, jobs), **kw)
            else:
                engine.mc_pass(xs[e], st, draw(e, jobs), passes=len(jobs), **kw)

    for kind, lane, e, jobs in plan:
        if kind == 'ws':
            engine.ws_pass(x, ws)          # on the caller's stream, beside the side lanes' first launches
        else:
            lanes.run(lambda st, lane, kind=kind, e=e, jobs=jobs: launch(st, lane, kind, e, jobs), lane=lane)
    if lanes.count > 1:
        lanes.end(engine.merge)
    return stats


class HipEngine:
    """The product engine of the fused paths: forward + softmax + accumulate on librcu_hip.  The one-process steps and the sharded runners
    touch the model through its ``ws_pass``, ``mc_pass``, ``member_pass``, ``side_statistics`` and ``merge`` only."""

    def __init__(self, model, do_mi=False, do_var=False, exact=True):
        self.model = model
        self.do_mi, self.do_var = do_mi, do_var
        # exact sums (McStatistics, include/rcu.h RCU_MC_EXACT): float64 planes whose additions are all exact -- the merged statistics carry
        # the same bits for every world size, job rotation, lane count and reduction tree of the collective
        self.exact = bool(exact)

    def _statistics(self, x, blob=None):
        n, _, h, w = x.shape
        return McStatistics(n, self.model.nb_classes, h, w, x.device, self.do_mi, self.do_var, blob=blob, exact=self.exact)

    def buffers(self, x, with_ws):
        """-> (flat reduce buffer, statistics object living in its head, ws tensor or None): the weight-scaling
        probabilities live in the tail of the ONE flat buffer (as float64 when the statistics are float64 -- a float32
        value is exact in float64, and a sum with the other ranks' zeros is too), so a volume is always one collective."""
        n, _, h, w = x.shape
        c = self.model.nb_classes
        n_stats = McStatistics.blob_elements(n, c, h * w, self.do_mi, self.do_var, self.exact)
        flat = torch.empty(n_stats + (n * c * h * w if with_ws else 0), device=x.device, dtype=McStatistics.dtype_of(self.do_var, self.exact))
        stats = self._statistics(x, flat[:n_stats])
        ws = None
        if with_ws:
            ws = flat[n_stats:].view(n, c, h, w)
            ws.zero_()
        return flat, stats, ws

    def reserve(self, x, mc_steps, group, lanes):
        """The canonical plans of the batch (reserve_canonical_plans): the bits of a pass must not depend on which launches THIS process
        happens to make."""
        n, _, h, w = x.shape
        reserve_canonical_plans(self.model, n, h, w, mc_steps, group, lanes)

    def ws_pass(self, x, ws_out):
        set_dropout_mode(self.model, False)
        if ws_out.dtype == torch.float32 and ws_out.is_contiguous():
            softmax(self.model(x), out=ws_out)
        else:                                                     # float64 statistics: the reduce buffer's tail is float64 too
            ws_out.copy_(softmax(self.model(x)))

    def seeded_masks(self, x, seeds, first_sample=0, sample_index=None):
        """The masks of the passes seeded with ``seeds`` over x, in the layout of their group launch (UNet.seeded_masks: one kernel, the factors
        of sample i in pass t a function of seeds[t] and the sample's global index ``first_sample + i`` -- or ``sample_index[i]``, an int64
        device tensor -- alone)."""
        set_dropout_mode(self.model, True)
        try:
            if sample_index is not None:
                return self.model.seeded_masks(x.shape[0], x.device, seeds, sample_index=sample_index)
            return self.model.seeded_masks(x.shape[0], x.device, seeds, first_sample)
        finally:
            set_dropout_mode(self.model, False)

    def sample_masks(self, x, generator, passes=1):
        """Dropout factors of ``passes`` stochastic passes over x (rows [site][passes * N][C_site]) from ``generator``."""
        set_dropout_mode(self.model, True)
        try:
            return self.model.sample_masks(x.shape[0] * passes, x.device, generator=generator)
        finally:
            set_dropout_mode(self.model, False)

    def mc_pass(self, x, stats, masks=None, passes=1, lane=0):
        set_dropout_mode(self.model, True)
        try:
            self.model.forward_accumulate(x, stats, masks, passes=passes, lane=lane)
        finally:
            set_dropout_mode(self.model, False)

    def member_pass(self, member, x, stats, lane=0):
        set_dropout_mode(member, False)
        member.forward_accumulate(x, stats, lane=lane)

    def side_statistics(self, x):
        """Fresh (zeroed) statistics: a stream lane's own, or a one-process step's."""
        return self._statistics(x)

    def merge(self, stats, side):
        merge_statistics(stats, side)

    def finalize(self, stats, count):
        return stats.finalize(self.do_mi, self.do_var, count=count)

    def ws_outputs(self, ws):
        return {'ws_probabilities': ws if ws.dtype == torch.float32 else ws.float()}


class AleatoricHipEngine(HipEngine):
    """EXTENSION (BASELINE config "aleatoric + MC", see AleatoricMcPredictStep): passes of a sigma-head U-Net; statistics carry a float32
    ``sigma_sum`` [n, C, H, W] next to the blob.  ``exact`` applies to the probability statistics only (the sigmas are unbounded addends:
    no exact form).  The sharded runner's reduce buffer is float32 throughout, one dtype per collective:
    flat = [statistics | sigma sum | ws probabilities | ws sigma].
    ``logit_samples`` = S > 0 (test-time logit sampling): every pass adds the sampled predictive of its (mu, sigma) in place of softmax(mu),
    pass j under the key ``pass_seed(seed, j)`` (the weight-scaling pass: j = 0), image i of the batch being slice ``first_sample + i``; the
    engine then ``takes_jobs``: run_plan tells ``mc_pass`` the pass numbers of each launch."""

    def __init__(self, model, is_log_sigma=False, do_mi=False, do_var=False, exact=False, logit_samples=0, seed=0, first_sample=0):
        super().__init__(model, do_mi, do_var, exact)
        if not getattr(model, 'sigma_out', False):
            raise ValueError('AleatoricHipEngine needs a model built with sigma_out=True')
        self.is_log_sigma = is_log_sigma
        self.logit_samples = check_logit_samples(logit_samples)
        self.seed = 0 if seed is None else int(seed)
        self.first_sample = int(first_sample)

    @property
    def takes_jobs(self):
        return self.logit_samples > 0

    def buffers(self, x, with_ws):
        if self.exact or self.do_var:
            raise ValueError('the reduce buffer of the sigma-head engine is float32: no exact or do_var statistics')
        n, _, h, w = x.shape
        c = self.model.nb_classes
        n_stats = McStatistics.blob_elements(n, c, h * w, self.do_mi, False)
        n_vol = n * c * h * w
        flat = torch.empty(n_stats + n_vol * (3 if with_ws else 1), device=x.device, dtype=torch.float32)
        stats = McStatistics(n, c, h, w, x.device, self.do_mi, False, blob=flat[:n_stats])
        flat[n_stats:].zero_()
        stats.sigma_sum = flat[n_stats:n_stats + n_vol].view(n, c, h, w)
        ws = flat[n_stats + n_vol:].view(2, n, c, h, w) if with_ws else None
        return flat, stats, ws

    def ws_pass(self, x, ws_out):
        """-> ws_out[0] = the probabilities, ws_out[1] = sigma of the deterministic pass."""
        set_dropout_mode(self.model, False)
        logits, raw = self.model(x)
        n, c, h, w = logits.shape
        sampled = self.logit_samples > 0
        _lib.check(_lib.load().rcu_aleatoric(_lib.ptr(logits), _lib.ptr(raw.contiguous()), n, h * w, c, int(self.is_log_sigma),
                                             None if sampled else _lib.ptr(ws_out[0]), _lib.ptr(ws_out[1]), None, None, _lib.current_stream()))
        if sampled:
            sample_logits(logits, raw, self.logit_samples, pass_seed(self.seed, 0), self.first_sample, self.is_log_sigma, out=ws_out[0])

    def mc_pass(self, x, stats, masks=None, passes=1, lane=0, jobs=None):
        set_dropout_mode(self.model, True)
        try:
            if self.logit_samples > 0:
                if jobs is None or len(jobs) != passes:
                    raise ValueError('a sampling pass needs the pass numbers of its launch (jobs)')
                self.model.forward_sample_sigma(x, stats, stats.sigma_sum, [pass_seed(self.seed, j) for j in jobs], self.first_sample,
                                                self.logit_samples, masks, self.is_log_sigma, lane=lane)
            else:
                self.model.forward_accumulate_sigma(x, stats, stats.sigma_sum, masks, self.is_log_sigma, lane=lane, passes=passes)
        finally:
            set_dropout_mode(self.model, False)

    def side_statistics(self, x):
        stats = super().side_statistics(x)
        stats.sigma_sum = torch.zeros((x.shape[0], self.model.nb_classes) + tuple(x.shape[2:]), device=x.device)
        return stats

    def finalize(self, stats, count):
        out = stats.finalize(self.do_mi, self.do_var, count=count)
        out['sigma'] = stats.sigma_sum / float(max(count, 1))
        return out

    def ws_outputs(self, ws):
        return {'ws_probabilities': ws[0], 'ws_sigma': ws[1]}


# ------------------------------------------------------------------------------------------------------------------------------
# sample agreement (EXTENSION; include/rcu.h "Sample agreement"): the T samples as whole segmentations
# ------------------------------------------------------------------------------------------------------------------------------
def check_agreement_passes(passes):
    """T of a vote plane: an int in 2..RCU_VOTES_MAX_PASSES (agreement is between samples); ValueError otherwise."""
    try:
        value = None if isinstance(passes, bool) else operator.index(passes)
    except TypeError:
        value = None
    if value is None or not 2 <= value <= _lib.RCU_VOTES_MAX_PASSES:
        raise ValueError('agreement needs mc_steps in 2..{} (one vote bit per pass), got {!r}'.format(_lib.RCU_VOTES_MAX_PASSES, passes))
    return value


def vote_bit(job):
    """Bit of MC pass ``job`` (1..T, the job numbers of ``launch_plan``) in a vote plane: bit (job - 1) % 32 of word (job - 1) // 32.  The
    weight-scaling pass (job 0) casts no vote."""
    if not 1 <= int(job) <= _lib.RCU_VOTES_MAX_PASSES:
        raise ValueError('only passes 1..{} vote, got job {}'.format(_lib.RCU_VOTES_MAX_PASSES, job))
    return int(job) - 1


class SampleVotes:
    """The vote plane of a batch (include/rcu.h): int32 ``[n_words, N, H, W]``, bit (j - 1) % 32 of word (j - 1) // 32 set where pass j's
    arg-max is not background.  4 bytes per voxel for T <= 32 passes; zeroed on the stream it is created on."""

    def __init__(self, n, height, width, passes, device):
        self.passes = int(passes)
        if not 1 <= self.passes <= _lib.RCU_VOTES_MAX_PASSES:
            raise ValueError('a vote plane holds 1..{} passes, got {}'.format(_lib.RCU_VOTES_MAX_PASSES, passes))
        self.n, self.height, self.width = int(n), int(height), int(width)
        self.plane = torch.zeros(((self.passes + 31) // 32, self.n, self.height, self.width), device=device, dtype=torch.int32)

    @property
    def n_words(self):
        return self.plane.shape[0]

    def cast(self, volume, job, is_probabilities=True):
        """Pass ``job``'s vote over one ``[N, C, H, W]`` probability (or logits) volume (rcu_mc_votes)."""
        t = volume.to(torch.float32).contiguous()
        if t.dim() != 4 or (t.shape[0], t.shape[2], t.shape[3]) != (self.n, self.height, self.width) or t.device != self.plane.device:
            raise ValueError('expected a [{}, C, {}, {}] volume on the plane\'s device'.format(self.n, self.height, self.width))
        bit = vote_bit(job)
        if bit >= 32 * self.n_words:
            raise ValueError('pass {} does not fit a plane of {} passes'.format(job, self.passes))
        _lib.check(_lib.load().rcu_mc_votes(_lib.ptr(t), self.n, self.height * self.width, t.shape[1],
                                            _lib.RCU_MC_INPUT_PROBS if is_probabilities else 0, _lib.ptr(self.plane), self.n_words, bit,
                                            _lib.current_stream()))

    def merge(self, side):
        """OR another plane of the same batch in (a side lane's: its passes own other bits)."""
        self.plane.bitwise_or_(side.plane)


def sample_votes(multi_probabilities):
    """A stacked ``[T, N, C, H, W]`` probability tensor (what ``materialize=True`` / ``McStatistics.as_tensor()`` give) -> its ``SampleVotes``:
    volume t votes as pass t + 1."""
    if not torch.is_tensor(multi_probabilities) or multi_probabilities.dim() != 5:
        raise ValueError('sample_votes takes a [T, N, C, H, W] tensor of probabilities')
    t, n, _, h, w = multi_probabilities.shape
    votes = SampleVotes(n, h, w, t, multi_probabilities.device)
    for i in range(t):
        votes.cast(multi_probabilities[i], i + 1)
    return votes


class VotingHipEngine(HipEngine):
    """HipEngine whose statistics each carry a vote plane of their own (``stats.votes``): a lane's launches are stream-ordered, so the head
    kernel reads and writes the voxel's word without atomics; ``merge`` ORs the side lanes' planes into lane 0's.  The engine ``takes_jobs``:
    pass j of a launch votes bit ``vote_bit(j)``."""

    takes_jobs = True

    def __init__(self, model, passes, do_mi=False, do_var=False, exact=True):
        super().__init__(model, do_mi, do_var, exact)
        self.passes = check_agreement_passes(passes)

    def side_statistics(self, x):
        stats = super().side_statistics(x)
        stats.votes = SampleVotes(x.shape[0], x.shape[2], x.shape[3], self.passes, x.device)
        return stats

    def mc_pass(self, x, stats, masks=None, passes=1, lane=0, jobs=None):
        if jobs is None or len(jobs) != passes:
            raise ValueError('a voting pass needs the pass numbers of its launch (jobs)')
        set_dropout_mode(self.model, True)
        try:
            self.model.forward_accumulate(x, stats, masks, passes=passes, lane=lane, votes=stats.votes, bits=[vote_bit(j) for j in jobs])
        finally:
            set_dropout_mode(self.model, False)

    def merge(self, stats, side):
        merge_statistics(stats, side)
        stats.votes.merge(side.votes)
        side.votes.plane.record_stream(torch.cuda.current_stream(side.votes.plane.device))


def check_logit_samples(samples):
    """``logit_samples`` of the aleatoric steps: an int in 0..RCU_LOGIT_MAX_SAMPLES (0: softmax(mu), no sampling); ValueError otherwise."""
    try:
        value = None if isinstance(samples, bool) else operator.index(samples)
    except TypeError:
        value = None
    if value is None or not 0 <= value <= _lib.RCU_LOGIT_MAX_SAMPLES:
        raise ValueError('logit_samples must be an integer in 0..{} (0: no sampling), got {!r}'.format(_lib.RCU_LOGIT_MAX_SAMPLES, samples))
    return value


def sample_logits(logits, sigma_raw, samples, key, first_sample, is_log_sigma=False, out=None):
    """Test-time logit sampling on the HIP path (include/rcu.h rcu_logit_sampling): p_bar = (1/S) sum_s softmax(mu + sigma * z_s) of the
    ``[N, C, H, W]`` logits and raw sigma of a sigma head (sigma = |raw|, or exp(raw) with ``is_log_sigma``), the noise of image i keyed by
    ``key`` and the slice index ``first_sample + i``.  ``out``: a contiguous float32 tensor of the logits' shape to write into."""
    logits = logits.to(torch.float32).contiguous()
    sigma_raw = sigma_raw.to(torch.float32).contiguous()
    if logits.dim() != 4 or sigma_raw.shape != logits.shape or sigma_raw.device != logits.device:
        raise ValueError('logits and sigma_raw must be [N, C, H, W] tensors of one shape on one device')
    n, c, h, w = logits.shape
    if out is None:
        out = torch.empty_like(logits)
    elif out.shape != logits.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != logits.device:
        raise ValueError('out must be a contiguous float32 tensor of the shape and device of the logits')
    _lib.check(_lib.load().rcu_logit_sampling(_lib.ptr(logits), _lib.ptr(sigma_raw), n, h * w, c, int(bool(is_log_sigma)), int(samples), int(key),
                                              int(first_sample), _lib.ptr(out), None, 0, _lib.current_stream()))
    return out


def softmax(logits, out=None):
    """F.softmax(logits, 1) on the HIP path (``out``: a contiguous float32 tensor of the same shape to write into)."""
    logits = logits.to(torch.float32).contiguous()
    n, c, h, w = logits.shape
    if out is None:
        out = torch.empty_like(logits)
    elif out.shape != logits.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != logits.device:
        raise ValueError('out must be a contiguous float32 tensor of the shape and device of the logits')
    _lib.check(_lib.load().rcu_softmax(_lib.ptr(logits), _lib.ptr(out), n, h * w, c, _lib.current_stream()))
    return out


class BatchStep(abc.ABC):
    @abc.abstractmethod
    def __call__(self, batch_context: BatchContext, task_context: TaskContext, context: Context) -> None:
        pass


def _images_to_device(batch_context, context):
    # non_blocking: a no-op for pageable host memory, asynchronous when the loader pinned the batch (rcu_amd.loops.prefetch)
    images = batch_context.input['images'].float().to(context.device, non_blocking=True)
    if not images.is_contiguous():
        # the volume loader hands the file's channel-last order over (data.VolumeDataset.__getitems__; the copy keeps the strides): the
        # re-ordering to [N, C, H, W] is a kernel behind the upload, not a strided copy on the loader thread
        images = images.contiguous()
    batch_context.input['images'] = images
    return images


class CorruptInputStep(BatchStep):
    """EXTENSION -- seeded input corruption for dataset-shift runs (rcu_amd.corruption, include/rcu.h "Input corruptions").  Put in front of the
    predict steps: uploads the batch's images as they do and replaces ``batch_context.input['images']`` with the corrupted device tensor, image i
    being the slice with global index ``first_sample_of(batch_context, n) + i``.  Every predict step that follows picks it up --
    ``.float().to(device)`` on that tensor is a no-op -- and none of them needs to know.  ``stages``: ``corruption.parse``'s result (or what it
    takes); ``seed``: the run's seed, stage s runs under ``corruption.corruption_seed(seed, s)``."""

    def __init__(self, stages, seed) -> None:
        super().__init__()
        from . import corruption
        if isinstance(stages, (list, tuple)) and stages and all(isinstance(s, corruption.Stage) for s in stages):
            self.stages = tuple(stages)
        else:
            self.stages = corruption.parse(stages)
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError('CorruptInputStep needs an integer seed, got {!r}'.format(seed))
        self.seed = seed
        corruption.corruption_seed(seed, len(self.stages) - 1)

    def __call__(self, batch_context, task_context, context) -> None:
        from . import corruption
        _check_context(context)
        images = _images_to_device(batch_context, context)
        batch_context.input['images'] = corruption.corrupt(images, self.stages, self.seed, first_sample_of(batch_context, images.shape[0]))


class SegmentationPredictStep(BatchStep):

    def __init__(self, has_labels=False, do_probs=False) -> None:
        super().__init__()
        self.has_labels = has_labels
        self.do_probs = do_probs

    def __call__(self, batch_context, task_context, context) -> None:
        _check_context(context)
        images = _images_to_device(batch_context, context)
        if self.has_labels:
            batch_context.input['labels'] = batch_context.input['labels'].long().to(context.device)
        logits = context.model(images)
        batch_context.output['logits'] = logits
        if self.do_probs:
            batch_context.output['probabilities'] = softmax(logits)


class DensityPredictStep(BatchStep):
    """EXTENSION -- feature-space density uncertainty (rcu_amd.density, include/rcu.h "Feature-space density") in place of the default predict step:
    one eval-mode forward with the feature tap, ``output['logits']`` and ``output['probabilities']`` as SegmentationPredictStep(do_probs=True) gives
    them, and ``output['density']``, the float32 energy ``[N, 1, H, W]`` of ``fit`` (a density.DensityFit), computed from the feature view while
    it is valid -- before any other forward on that plan."""

    def __init__(self, fit) -> None:
        super().__init__()
        from . import density
        if not isinstance(fit, density.DensityFit):
            raise ValueError('DensityPredictStep needs a density.DensityFit, got {}'.format(type(fit).__name__))
        self.fit = fit

    def __call__(self, batch_context, task_context, context) -> None:
        from . import density
        _check_context(context)
        model = context.model
        channels = density._feature_channels(model)
        if channels != self.fit.F:
            raise ValueError('the density fit has F = {} feature channels, the model has {}'.format(self.fit.F, channels))
        images = _images_to_device(batch_context, context)
        with density.eval_features(model):
            logits = model(images)
            batch_context.output['density'] = density.energy(self.fit, model.features)
        batch_context.output['logits'] = logits
        batch_context.output['probabilities'] = softmax(logits)


class KnnPredictStep(BatchStep):
    """EXTENSION -- nearest-neighbour feature uncertainty (rcu_amd.knn, include/rcu_knn.h) in place of the default predict step: one eval-mode
    forward with the feature tap, ``output['logits']`` and ``output['probabilities']`` as SegmentationPredictStep(do_probs=True) gives them, and
    ``output['knn']``, the float32 distance ``[N, 1, H, W]`` of every voxel's feature vector to its ``k``-th nearest row of ``bank`` (a
    knn.KnnBank), computed from the feature view while it is valid -- before any other forward on that plan."""

    def __init__(self, bank, k=5) -> None:
        super().__init__()
        from . import knn
        if not isinstance(bank, knn.KnnBank):
            raise ValueError('KnnPredictStep needs a knn.KnnBank, got {}'.format(type(bank).__name__))
        self.bank = bank
        self.k = knn.check_k(bank, k)

    def __call__(self, batch_context, task_context, context) -> None:
        from . import knn
        _check_context(context)
        model = context.model
        channels = knn.check_model(model)
        if channels != self.bank.F:
            raise ValueError('the k-NN bank has F = {} feature channels, the model has {}'.format(self.bank.F, channels))
        images = _images_to_device(batch_context, context)
        with knn.eval_features(model):
            logits = model(images)
            batch_context.output['knn'] = knn.distances(self.bank, model.features, self.k)
        batch_context.output['logits'] = logits
        batch_context.output['probabilities'] = softmax(logits)


class LaplacePredictStep(BatchStep):
    """EXTENSION -- last-layer Laplace uncertainty (rcu_amd.laplace, include/rcu.h "Last-layer Laplace") in place of the default predict step: one
    eval-mode forward with the classifier tap; ``output['logits']`` keeps the bits of SegmentationPredictStep, ``output['probabilities']`` is the
    predictive of ``fit`` (a laplace.LaplaceFit) and ``output['laplace_std']``, float32 ``[N, 1, H, W]``, the standard deviation of the predicted
    class's logit -- computed from the tap's view while it is valid, before any other forward on that plan.
    ``link='probit'``: the mean-field probit softmax(z / sqrt(1 + pi/8 s2)), one kernel.  ``link='sample'``: (1/S) sum_s softmax(z + std * eps_s)
    with ``samples`` = S draws of diagonal noise by ``sample_logits`` (rcu_logit_sampling), the noise of slice g keyed by ``pass_seed(seed, 0)``
    and g as AleatoricPredictStep keys it -- the same bits for any batching."""

    LINKS = ('probit', 'sample')

    def __init__(self, fit, link='probit', samples=0, seed=0) -> None:
        super().__init__()
        from . import laplace
        if not isinstance(fit, laplace.LaplaceFit):
            raise ValueError('LaplacePredictStep needs a laplace.LaplaceFit, got {}'.format(type(fit).__name__))
        if link not in self.LINKS:
            raise ValueError('link must be one of {}, got {!r}'.format(', '.join(self.LINKS), link))
        self.fit, self.link = fit, link
        self.samples = check_logit_samples(samples) if link == 'sample' else 0
        if link == 'sample' and self.samples < 1:
            raise ValueError("link='sample' needs samples >= 1, got {!r}".format(samples))
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError('LaplacePredictStep needs an integer seed, got {!r}'.format(seed))
        self.seed = seed

    def __call__(self, batch_context, task_context, context) -> None:
        from . import laplace
        _check_context(context)
        model = context.model
        laplace.check_model(model, self.fit)
        images = _images_to_device(batch_context, context)
        sampled = self.link == 'sample'
        with laplace.eval_head_features(model):
            logits = model(images)
            out = laplace.predict(self.fit, model.head_features, logits, std=sampled, std_pred=not sampled, prediction=False)
        batch_context.output['logits'] = logits
        if sampled:
            probs = sample_logits(logits, out['std'], self.samples, pass_seed(self.seed, 0), first_sample_of(batch_context, logits.shape[0]))
            # the std of the class the sampled predictive chooses: its first maximum, as the writers take it
            chosen = prediction_and_foreground(probs)[0].long().unsqueeze(1)
            batch_context.output['probabilities'] = probs
            batch_context.output['laplace_std'] = torch.gather(out['std'], 1, chosen)
        else:
            batch_context.output['probabilities'] = out['probabilities']
            batch_context.output['laplace_std'] = out['std_pred']


class SampleAgreementStep(BatchStep):
    """Behind the summary: pops ``sample_votes`` (McPredictStep with ``agreement=True``) and writes ``output['agreement']``, one int64 row
    ``[(T + 1) + T (T + 1) / 2]`` per slice -- ``hist`` then the upper triangle ``pairs`` of include/rcu.h's rcu_agreement_tables, one image per
    volume.  Integers: the rows of a subject's slices add up to the subject's table (``evaluation.agreement_metrics`` on the sum)."""

    def __call__(self, batch_context, task_context, context) -> None:
        from . import evaluation
        votes = batch_context.output.pop('sample_votes', None)
        if votes is None:
            return
        hist, pairs = evaluation.agreement_tables_on_device(votes.plane, votes.passes, votes.n)
        batch_context.output['agreement'] = torch.cat([hist, pairs], dim=1)


class McPredictStep(BatchStep):
    """T stochastic passes (plus the deterministic 'weight scaling' pass the reference always runs
    first, customsteps.py:22-25).
    ``seed``: the Dropout2d factors of pass j for the slice with global index g (``batch_context.sample_offset`` + its position in the batch: the
    test loop counts the slices it has handed out) are drawn under the key ``pass_seed(seed, j)`` at the counter of (g, site, channel)
    (UNet.seeded_masks: one kernel per launch, include/rcu.h rcu_dropout_masks) instead of from the device's default generator: the T samples of a
    SLICE are then a function of (seed, slice, pass) alone -- the same whatever ``batch_size`` the YAML file sets and however the loop coalesces
    batches (round 6; rounds 1-5 keyed the draw by the batch), whatever the pass groups and stream lanes, and the same when the passes are
    sharded over several GPUs (rcu_amd.distributed.ShardedMcPredictStep).  The drop-in scripts pass the YAML file's ``seed``.
    ``exact`` (default): the statistics are exact sums (McStatistics), so that ``MultiPredictionSummary``'s outputs do not depend on
    how the passes were grouped, laned or sharded either; ``exact=False`` keeps float32 sums (float64 with ``do_var``)."""

    # A forward pass fills the GPU from about 160 BraTS slices (3.9 M pixels) on, and the deep levels of the U-Net -- few, long
    # work items per launch -- only from two to four times that (their last round of workgroups is 75-88 % full at 160 slices, 94 % at
    # 320, full at 640); the shipped configs use batch_size 32.  The T passes of a batch are independent, so the fused path runs them in
    # groups of g = GROUP_PIXELS // (N*H*W) as one batch of N * g samples (include/rcu.h: rcu_unet_forward_accumulate_passes) -- same
    # statistics bit for bit; the workspace grows to that of a 640-slice batch (12 GB per lane of the 288), not beyond, and
    # pass_group_size keeps every tensor below the 2 GB the kernels' 32-bit buffer offsets reach (640 BraTS slices x 32 channels: 2.01e9 bytes).
    GROUP_PIXELS = 4 * 160 * 192 * 128
    LANES = 2      # HIP streams the pass groups of a batch alternate over (StreamLanes); the ``lanes`` argument overrides it

    def __init__(self, mc_steps, do_mi=False, do_var=False, materialize=False, masks=None, ws_pass=True,
                 group_pixels=None, lanes=None, seed=None, exact=True, agreement=False, adaptive=None) -> None:
        super().__init__()
        # EXTENSION ``adaptive`` (include/rcu.h "Adaptive MC"): ``dict(check_at=[t1 < t2 < ...], tolerance=eps, max_unsettled=0)``.  At checkpoint
        # t a slice whose voxels all (but max_unsettled) have a leading class of mean probability >= 1 - eps over its t passes is retired: it
        # keeps those t passes and is finalised from them, the other slices run on as a smaller batch.  ``multi_probabilities`` is then an
        # AdaptiveMcStatistics and ``output['mc_passes']`` the int32 pass count per slice.  Approximate by design, opt-in.
        self.adaptive = None
        if adaptive is not None:
            self.adaptive = check_adaptive(adaptive, mc_steps)
            if not exact or mc_steps > _lib.RCU_MC_EXACT_MAX_PASSES:
                raise ValueError('adaptive MC needs exact statistics (exact=True, mc_steps <= {}): the decision is made on exact integer '
                                 'sums'.format(_lib.RCU_MC_EXACT_MAX_PASSES))
            if seed is None and masks is None:
                raise ValueError('adaptive MC needs a seed (or injected masks): a slice moved into a smaller batch must keep its samples')
            if materialize:
                raise ValueError('adaptive MC needs the fused path (materialize=False): there is no [T, N, C, H, W] stack of slices with '
                                 'different pass counts')
            if agreement:
                raise ValueError('adaptive MC needs agreement=False: the vote planes assume every slice sees every pass')
        # EXTENSION ``agreement`` (include/rcu.h "Sample agreement"): ``output['sample_votes']`` (SampleVotes) -- one bit per (voxel, pass), set
        # where the pass's arg-max is not background; written by the head kernel of the fused path (every lane votes into a plane of its own,
        # OR-merged at the end), by ``sample_votes`` on the materialised one.  The weight-scaling pass casts no vote.
        self.agreement = bool(agreement)
        if self.agreement:
            check_agreement_passes(mc_steps)
        self.mc_steps = mc_steps
        self.do_mi, self.do_var = do_mi, do_var
        self.materialize = materialize
        self.masks = masks          # optional: list (one per pass) of mask sets to inject instead of sampling
        self.ws_pass = ws_pass
        self.group_pixels = self.GROUP_PIXELS if group_pixels is None else group_pixels
        self.lanes = self.LANES if lanes is None else max(1, int(lanes))
        self.seed = seed
        self.exact = bool(exact) and mc_steps <= _lib.RCU_MC_EXACT_MAX_PASSES      # (beyond the exact form's 2,048 passes: plain float sums)

    def _seeded_masks(self, model, images, first_sample, job):
        """The mask tensor of MC pass ``job`` (1..T) of the batch whose first sample has global index ``first_sample`` under ``self.seed``
        (dropout mode is on)."""
        return model.seeded_masks(images.shape[0], images.device, [pass_seed(self.seed, job)], first_sample)

    def _pass_masks(self, model, images, first_sample, job):
        """Masks of the single pass ``job`` (1..T) of the materialised paths: injected, seeded, or None = drawn by the forward from the
        device's default generator (dropout mode is on)."""
        if self.masks is not None:
            return self.masks[job - 1]
        return None if self.seed is None else self._seeded_masks(model, images, first_sample, job)

    def __call__(self, batch_context, task_context, context) -> None:
        _check_context(context)
        images = _images_to_device(batch_context, context)
        model = context.model
        k = first_sample_of(batch_context, images.shape[0])      # global index of the batch's first sample: what the seeded masks are keyed by
        if self.adaptive is not None:
            if not isinstance(model, model_mod.UNet):
                raise ValueError('adaptive MC needs the fused path: the model must be a rcu_amd.model.UNet, got {}'.format(type(model).__name__))
            if model.nb_classes < 2:
                raise ValueError('adaptive MC needs nb_classes >= 2: the criterion is the mean probability of the leading class')
        if not self.materialize and isinstance(model, model_mod.UNet):
            n, _, h, w = images.shape
            ws = torch.empty((n, model.nb_classes, h, w), device=images.device, dtype=torch.float32) if self.ws_pass else None
            if ws is not None:
                batch_context.output['ws_probabilities'] = ws
            if self.adaptive is not None:
                stats = self._fused_adaptive(model, images, self.do_mi, self.do_var, k, ws)
                batch_context.output['mc_passes'] = stats.counts.view(n, 1)      # (a column: slice rows travel like 'confusion' rows, channel last)
                batch_context.more['adaptive_checkpoints'] = stats.checkpoints
            else:
                stats = self._fused(model, images, self.do_mi, self.do_var, k, ws, votes=self.agreement)
            batch_context.output['multi_probabilities'] = stats
            if self.agreement:
                batch_context.output['sample_votes'] = stats.votes
            return
        unet = isinstance(model, model_mod.UNet)
        if unet:      # the canonical plan of the fused path (reserve_canonical_plans): a pass's bits are a property of the plan
            n, _, h, w = images.shape
            reserve_canonical_plans(model, n, h, w, self.mc_steps, pass_group_size(model, n, h, w, self.group_pixels), 1)
        if self.ws_pass:
            batch_context.output['ws_probabilities'] = softmax(model(images))
        set_dropout_mode(model, is_train=True)
        try:
            probs = []
            for j in range(1, self.mc_steps + 1):
                masks = self._pass_masks(model, images, k, j) if unet else None
                probs.append(softmax(model(images) if masks is None else model(images, masks)))
            batch_context.output['multi_probabilities'] = torch.stack(probs)
            if self.agreement:
                batch_context.output['sample_votes'] = sample_votes(batch_context.output['multi_probabilities'])
        finally:
            set_dropout_mode(model, is_train=False)   # reset to eval for the next batch (customsteps.py:39)

    def _fused(self, model, images, do_mi, do_var, first_sample=0, ws=None, votes=False):
        """The T passes (and, into ``ws``, the weight-scaling pass) into per-voxel statistics, on ``run_plan``.  The statistics carry a recipe
        that replays the passes -- same images, same masks (seeded: the same draws again; unseeded: the device generator is put back to where
        the sampling started) -- so that ``MultiPredictionSummary(do_mi / do_var)`` decides alone which outputs exist, as in the reference
        (customsteps.py:44-48)."""
        n, _, h, w = images.shape
        dev = images.device
        unseeded = self.masks is None and self.seed is None
        rng_state = torch.cuda.get_rng_state(dev) if (unseeded and dev.type == 'cuda') else None
        # (``votes``: the statistics carry the vote plane of the passes, ``stats.votes``; a replay through the recipe does not vote again)
        engine = VotingHipEngine(model, self.mc_steps, do_mi, do_var, self.exact) if votes else HipEngine(model, do_mi, do_var, self.exact)
        stats = engine.side_statistics(images)
        group = pass_group_size(model, n, h, w, self.group_pixels)
        # (every lane gets work whenever there are two passes: T = 20 on batches of 32 slices is 10 | 10 on two lanes, not one launch of 20 on one)
        lanes = min(self.lanes, max(self.mc_steps, 1))
        plan = launch_plan(([0] if ws is not None else []) + list(range(1, self.mc_steps + 1)), (0,), max(self.mc_steps, 1), group, lanes)
        try:
            run_plan(plan, engine, images, stats, ws, lanes, reserve=(self.mc_steps, group),
                     draw=lambda e, jobs: launch_masks(engine, images, e, jobs, max(self.mc_steps, 1), self.seed, first_sample, self.masks))
        finally:
            set_dropout_mode(model, is_train=False)

        def recipe(mi, var, materialize=False):
            now = torch.cuda.get_rng_state(dev) if rng_state is not None else None
            if rng_state is not None:
                torch.cuda.set_rng_state(rng_state, dev)
            set_dropout_mode(model, is_train=True)
            try:
                if not materialize:
                    return self._fused(model, images, mi, var, first_sample)
                probs = []
                for _, _, _, jobs in (launch for launch in plan if launch[0] == 'passes'):      # the draws the fused path makes: one per group
                    g = len(jobs)
                    if not unseeded:
                        sets = [self._pass_masks(model, images, first_sample, j) for j in jobs]
                    elif g == 1:
                        sets = [None]
                    else:                            # rows [site][pass * n + i]: split the group's draw into its passes
                        flat = model.sample_masks(n * g, dev)
                        per_site = torch.split(flat, [n * g * c for _, c in model.dropout_sites()])
                        sets = [[ps.view(g, n, -1)[i] for ps in per_site] for i in range(g)]
                    for ms in sets:
                        probs.append(softmax(model(images) if ms is None else model(images, ms)))
                return torch.stack(probs)
            finally:
                set_dropout_mode(model, is_train=False)
                if now is not None:
                    torch.cuda.set_rng_state(now, dev)

        stats.recipe = recipe
        return stats

    def _gathered_mask_set(self, model, mask_set, n, index):
        """The rows ``index`` (device int64 tensor) of one injected mask set over n images -> a list of per-site ``[m, C_site]`` device tensors."""
        sites = model.dropout_sites()
        if isinstance(mask_set, (list, tuple)):
            rows = [torch.as_tensor(a, dtype=torch.float32).to(index.device) for a in mask_set]
        else:
            rows = [r.view(n, c) for r, (_, c) in zip(torch.split(mask_set.to(index.device), [n * c for _, c in sites]), sites)]
        return [r.index_select(0, index) for r in rows]

    def _fused_adaptive(self, model, images, do_mi, do_var, first_sample=0, ws=None, replay=None):
        """The adaptive form of ``_fused`` (include/rcu.h "Adaptive MC").  Passes 1..t_1 run on all slices through ``launch_plan`` / ``run_plan``
        as ``McPredictStep(mc_steps=t_1)`` runs them; at every checkpoint the lanes are joined, the slices are scored on the device
        (rcu_mc_slice_scores: one small copy to the host) and the still-active ones are gathered into a compact batch whose next span of passes
        runs -- under the same keys: pass j is drawn under ``pass_seed(seed, j)`` at the slices' GLOBAL indices -- into compact statistics that
        rcu_mc_merge_slices adds into the rows of the full ones.  Everything runs on the plans the plain step reserves for (n, T): a compact
        launch never holds more samples than they do.  ``replay``: the ``spans`` of an earlier run -- they are used as recorded and nothing is
        scored (the statistics' recipe)."""
        n, _, h, w = images.shape
        dev = images.device
        cfg, total = self.adaptive, self.mc_steps
        engine = HipEngine(model, do_mi, do_var, True)
        stats = AdaptiveMcStatistics(n, model.nb_classes, h, w, dev, do_mi, do_var)
        group = pass_group_size(model, n, h, w, self.group_pixels)
        lanes = min(self.lanes, total)
        plan_samples = reserve_canonical_plans(model, n, h, w, total, group, lanes)
        ends = cfg['check_at'] + [total]
        active = list(range(n))
        scores = torch.empty(2 * n, device=dev, dtype=torch.int64) if replay is None else None
        try:
            for k, end in enumerate(ends):
                begin = ends[k - 1] if k else 0
                jobs = list(range(begin + 1, end + 1))
                stats.spans.append(list(active))
                stats.passes_run += len(active) * len(jobs)
                if k == 0:
                    span_lanes = min(lanes, len(jobs))
                    plan = launch_plan(([0] if ws is not None else []) + jobs, (0,), total, group, span_lanes)
                    run_plan(plan, engine, images, stats, ws, span_lanes,
                             draw=lambda e, js: launch_masks(engine, images, e, js, total, self.seed, first_sample, self.masks))
                else:
                    m = len(active)
                    index = torch.tensor(active, device=dev, dtype=torch.int64)
                    x = images.index_select(0, index)
                    sample_index = index + int(first_sample)
                    if self.masks is not None:
                        sets = {j: self._gathered_mask_set(model, self.masks[j - 1], n, index) for j in jobs}

                        def draw(e, js, sets=sets):
                            return sets[js[0]] if len(js) == 1 else [sets[j] for j in js]
                    else:
                        def draw(e, js, x=x, sample_index=sample_index):
                            return engine.seeded_masks(x, [pass_seed(self.seed, j) for j in js], sample_index=sample_index)
                    compact = engine.side_statistics(x)
                    span_lanes = min(lanes, len(jobs))
                    plan = launch_plan(jobs, (0,), total, compact_group_size(model, m, h, w, self.group_pixels, plan_samples), span_lanes)
                    run_plan(plan, engine, x, compact, None, span_lanes, draw=draw)
                    merge_slices(compact, stats, index.to(torch.int32))
                if k == len(ends) - 1:
                    break
                # the checkpoint: behind run_plan the lanes are joined on the caller's stream
                if replay is not None:
                    active = list(replay[k + 1]) if k + 1 < len(replay) else []
                else:
                    thr = adaptive_threshold(cfg['tolerance'], end)
                    unsettled, margin_q = split_scores(slice_scores(stats, thr, out=scores))
                    gone = [i for i in active if unsettled[i] <= cfg['max_unsettled']]
                    stats.checkpoints.append(dict(t=end, thr_q=thr, active=list(active), unsettled=[unsettled[i] for i in active],
                                                  margin_q=[margin_q[i] for i in active], retired=gone))
                    active = [i for i in active if unsettled[i] > cfg['max_unsettled']]
                if not active:
                    break
        finally:
            set_dropout_mode(model, is_train=False)
        counts = adaptive_counts(n, cfg['check_at'], total, stats.spans)
        stats.counts = torch.tensor(counts, device=dev, dtype=torch.int32)
        stats.count = max(counts)
        spans = [list(s) for s in stats.spans]

        def recipe(mi, var, materialize=False):
            if materialize:
                raise ValueError('adaptive MC statistics have no [T, N, C, H, W] stack: the slices have seen different numbers of passes')
            again = self._fused_adaptive(model, images, mi, var, first_sample, replay=spans)
            again.checkpoints = stats.checkpoints
            return again

        stats.recipe = recipe
        return stats


def share_member_workspaces(members):
    """Members 2..K of an ensemble borrow the activation workspaces of the first (model.UNet.share_workspace): the K models the
    reference keeps resident (bin-dl/brats_test_ensemble.py:44-57) differ in their weights only.  Members of another architecture,
    foreign modules and members that already borrow are left alone."""
    donor = members[0] if members and isinstance(members[0], model_mod.UNet) else None
    if donor is None:
        return
    if donor._donor is not None:
        donor = donor._donor         # the first member borrows already (the same models in another order): its owner lends to the rest
    for m in members[1:]:
        if isinstance(m, model_mod.UNet) and m is not donor and m._donor is None:
            try:
                m.share_workspace(donor)
            except ValueError:
                pass        # a different architecture keeps its own workspace


class EnsemblePredictionStep(BatchStep):
    """context.model plus ``additional_models``, all in eval mode (brats_test_ensemble.py:78-94)."""

    def __init__(self, additional_models, do_mi=False, do_var=False, materialize=False, share_workspace=True, lanes=None,
                 exact=True) -> None:
        super().__init__()
        self.additional_models = additional_models
        self.do_mi, self.do_var = do_mi, do_var
        self.materialize = materialize
        self.share_workspace = share_workspace
        self.lanes = McPredictStep.LANES if lanes is None else max(1, int(lanes))
        self.exact = bool(exact)       # exact sums (McStatistics): the member order / lanes / ranks do not change the bits

    def __call__(self, batch_context, task_context, context) -> None:
        _check_context(context)
        images = _images_to_device(batch_context, context)
        members = [context.model] + list(self.additional_models)
        fused = not self.materialize and all(isinstance(m, model_mod.UNet) for m in members)
        if self.share_workspace:
            share_member_workspaces(members)
        if fused:
            def run(mi, var, materialize=False):
                if materialize:
                    return torch.stack([softmax(m(images)) for m in members])
                engine = HipEngine(members[0], mi, var, self.exact and len(members) <= _lib.RCU_MC_EXACT_MAX_PASSES)
                stats = engine.side_statistics(images)
                lanes = min(self.lanes, len(members))
                run_plan(launch_plan(range(1, len(members) + 1), lanes=lanes, members=True), engine, images, stats, lanes=lanes, members=members)
                stats.recipe = run
                return stats
            batch_context.output['multi_probabilities'] = run(self.do_mi, self.do_var)
        else:
            batch_context.output['multi_probabilities'] = torch.stack([softmax(m(images)) for m in members])


class MultiPredictionSummary(BatchStep):
    _replay_warned = False

    def __init__(self, do_mi=False, do_var=False, remove_multi_probs=True) -> None:
        super().__init__()
        self.do_mi = do_mi
        self.do_var = do_var
        self.remove_multi_probs = remove_multi_probs

    def __call__(self, batch_context, task_context, context) -> None:
        if self.remove_multi_probs:
            multi = batch_context.output.pop('multi_probabilities')
        else:
            multi = batch_context.output['multi_probabilities']
        if multi is None:      # a rank other than the root of a sharded predict step (rcu_amd.distributed): the root alone has the merged statistics
            return
        if hasattr(multi, 'finalize_when_merged'):
            # the root of a sharded predict step: the statistics are merged by a collective that is still in flight.  The finalize runs on a
            # side stream behind it; the outputs carry an event (wait_for_outputs) instead of holding the compute stream up
            out, event = multi.finalize_when_merged(self.do_mi, self.do_var)
            batch_context.output.update(out)
            if event is not None:
                batch_context.more['outputs_ready'] = event
            return
        if isinstance(multi, McStatistics):
            stats = multi
            if (self.do_mi and not stats.do_mi) or (self.do_var and not stats.do_var):
                # the predict step did not track what this summary asks for (the reference's summary alone decides,
                # customsteps.py:44-48): replay the passes with the flags of both
                if stats.recipe is None:
                    raise ValueError('the statistics lack {} and cannot be replayed'.format(
                        'the entropy sum (do_mi)' if self.do_mi and not stats.do_mi else 'the squared sums (do_var)'))
                if not MultiPredictionSummary._replay_warned:
                    MultiPredictionSummary._replay_warned = True
                    logging.getLogger(__name__).warning(
                        'MultiPredictionSummary(do_mi=%s, do_var=%s) asks for more than the predict step tracked: the passes run a '
                        'second time under the same masks (construct the predict step with the same flags to avoid it)',
                        self.do_mi, self.do_var)
                stats = stats.recipe(self.do_mi or stats.do_mi, self.do_var or stats.do_var)
        else:
            t, n, c, h, w = multi.shape
            # (exact sums: a materialised stack gives the bits the fused statistics of the same passes give)
            stats = McStatistics(n, c, h, w, multi.device, self.do_mi, self.do_var, exact=t <= _lib.RCU_MC_EXACT_MAX_PASSES)
            for i in range(t):
                stats.accumulate(multi[i], is_probabilities=True)
        out = stats.finalize(self.do_mi, self.do_var)
        batch_context.output['probabilities'] = out['probabilities']
        batch_context.output['entropy'] = out['entropy']
        if self.do_mi:
            batch_context.output['mutual_info'] = out['mutual_info']
        if self.do_var:
            batch_context.output['variance'] = out['variance']


class AleatoricPredictStep(BatchStep):
    """bin-dl/brats_test_aleatoric.py:51-73: ``logits``, ``sigma`` (|raw| or exp(raw)) and ``probabilities`` = softmax(logits) of one
    eval-mode pass of a sigma-head model.  EXTENSION ``logit_samples`` = S > 0 (test-time logit sampling, include/rcu.h): ``probabilities`` is the
    predictive the model was trained for (AleatoricLoss, Kendall & Gal 2017), p_bar = (1/S) sum_s softmax(mu + sigma * z_s), the noise of slice g
    keyed by ``pass_seed(seed, 0)`` and g (the batch's ``first_sample_of`` + position) -- the same bits for any batching.  ``logits`` and
    ``sigma`` do not change."""

    def __init__(self, is_log_sigma=False, logit_samples=0, seed=0) -> None:
        super().__init__()
        self.is_log_sigma = is_log_sigma
        self.logit_samples = check_logit_samples(logit_samples)
        self.seed = 0 if seed is None else int(seed)

    def __call__(self, batch_context, task_context, context) -> None:
        _check_context(context)
        images = _images_to_device(batch_context, context)
        mean_logits, sigma_raw = context.model(images)
        batch_context.output['logits'] = mean_logits
        n, c, h, w = mean_logits.shape
        probs = torch.empty_like(mean_logits)
        sigma = torch.empty_like(mean_logits)
        sampled = self.logit_samples > 0
        _lib.check(_lib.load().rcu_aleatoric(_lib.ptr(mean_logits), _lib.ptr(sigma_raw.contiguous()), n, h * w, c,
                                             int(self.is_log_sigma), None if sampled else _lib.ptr(probs), _lib.ptr(sigma), None, None,
                                             _lib.current_stream()))
        if sampled:
            sample_logits(mean_logits, sigma_raw, self.logit_samples, pass_seed(self.seed, 0), first_sample_of(batch_context, n),
                          self.is_log_sigma, out=probs)
        batch_context.output['sigma'] = sigma
        batch_context.output['probabilities'] = probs


class AleatoricMcPredictStep(BatchStep):
    """EXTENSION -- BASELINE config "aleatoric + MC" (sigma-head U-Net, T stochastic passes); the reference has no such step
    (McPredictStep cannot take the (logits, sigma) tuple, customsteps.py:32-33).  It is the composition of the reference's
    pieces: per pass t, with dropout on, ``logits_t, raw_t = model(x)``; ``p_t = softmax(logits_t)`` goes into the MC statistics
    (-> ``multi_probabilities`` for MultiPredictionSummary, as McPredictStep); ``sigma_t = |raw_t|`` or ``exp(raw_t)``
    (AleatoricPredictStep, brats_test_aleatoric.py:66-69) is averaged over the passes -> ``sigma`` [N, C, H, W].  The
    deterministic pass that McPredictStep runs first gives ``ws_probabilities`` and ``ws_sigma``.
    ``seed``: the Dropout2d masks are drawn as McPredictStep draws them under its ``seed`` (pass j: ``pass_seed(seed, j)`` at the slices' global
    indices); None: from the device generator (or ``masks``, injected).
    EXTENSION ``logit_samples`` = S > 0 (test-time logit sampling, include/rcu.h): pass j adds its sampled predictive
    p_bar_j = (1/S) sum_s softmax(mu_j + sigma_j * z_s) where it would add softmax(mu_j), the noise keyed by ``pass_seed(seed or 0, j)`` and the
    slice (the weight-scaling pass: j = 0, as AleatoricPredictStep) -- in the head kernel of the fused forward, mu and sigma never reach HBM.
    MultiPredictionSummary then splits the total uncertainty: ``probabilities`` = mean_j p_bar_j, ``entropy`` = H(mean) the total,
    ``mutual_info`` the epistemic part (the dropout's), ``entropy - mutual_info`` = mean_j H(p_bar_j) the aleatoric part."""

    def __init__(self, mc_steps, is_log_sigma=False, do_mi=False, do_var=False, masks=None, ws_pass=True, lanes=None, exact=True,
                 logit_samples=0, seed=None) -> None:
        super().__init__()
        self.mc_steps = mc_steps
        self.logit_samples = check_logit_samples(logit_samples)
        self.seed = seed
        self.is_log_sigma = is_log_sigma
        self.do_mi, self.do_var = do_mi, do_var
        self.masks = masks
        self.ws_pass = ws_pass
        self.lanes = McPredictStep.LANES if lanes is None else max(1, int(lanes))
        self.exact = bool(exact) and mc_steps <= _lib.RCU_MC_EXACT_MAX_PASSES       # the probability statistics; the sigma sums stay float32 (unbounded addends)

    def __call__(self, batch_context, task_context, context) -> None:
        _check_context(context)
        images = _images_to_device(batch_context, context)
        model = context.model
        if not isinstance(model, model_mod.UNet) or not model.sigma_out:
            raise ValueError('AleatoricMcPredictStep needs a rcu_amd.model.UNet built with sigma_out=True')
        n, _, h, w = images.shape
        first_sample = first_sample_of(batch_context, n)
        engine = AleatoricHipEngine(model, self.is_log_sigma, self.do_mi, self.do_var, self.exact, self.logit_samples, self.seed, first_sample)
        ws = torch.empty((2, n, model.nb_classes, h, w), device=images.device, dtype=torch.float32) if self.ws_pass else None
        stats = engine.side_statistics(images)
        # pass groups and stream lanes as in McPredictStep: g passes per launch, launches alternating over two HIP streams
        group = pass_group_size(model, n, h, w, McPredictStep.GROUP_PIXELS)
        lanes = max(1, min(self.lanes, self.mc_steps))
        plan = launch_plan(([0] if ws is not None else []) + list(range(1, self.mc_steps + 1)), (0,), max(self.mc_steps, 1), group, lanes)
        try:
            run_plan(plan, engine, images, stats, ws, lanes, reserve=(self.mc_steps, group),
                     draw=lambda e, jobs: launch_masks(engine, images, e, jobs, max(self.mc_steps, 1), self.seed, first_sample, self.masks))
        finally:
            set_dropout_mode(model, is_train=False)
        if ws is not None:
            batch_context.output['ws_probabilities'], batch_context.output['ws_sigma'] = ws[0], ws[1]
        batch_context.output['multi_probabilities'] = stats
        batch_context.output['sigma'] = stats.sigma_sum.div_(float(max(self.mc_steps, 1)))


# ------------------------------------------------------------------------------------------------------------------------------
# test-time augmentation (EXTENSION; include/rcu.h "Test-time augmentation")
# ------------------------------------------------------------------------------------------------------------------------------
TTA_ELEMENTS = _lib.TTA_ELEMENTS                 # code -> name: the eight elements of D4 on (H, W)
TTA_INVERSE = (0, 1, 2, 3, 4, 6, 5, 7)           # code -> code of the inverse element


def tta_element(transform):
    """Name or code of a D4 element -> its code (include/rcu.h RCU_TTA_*); ValueError for anything else."""
    if isinstance(transform, str):
        if transform not in TTA_ELEMENTS:
            raise ValueError('unknown TTA transform "{}" (one of {})'.format(transform, ', '.join(TTA_ELEMENTS)))
        return TTA_ELEMENTS.index(transform)
    if isinstance(transform, bool) or not isinstance(transform, int) or not 0 <= transform < len(TTA_ELEMENTS):
        raise ValueError('unknown TTA transform {!r} (a name or a code 0..7)'.format(transform))
    return int(transform)


def tta_elements(transforms):
    """List of names / codes -> tuple of codes, in the given order; empty lists, unknown names and duplicates raise ValueError."""
    if isinstance(transforms, (str, int)):
        transforms = [transforms]
    codes = tuple(tta_element(t) for t in transforms)
    if not codes:
        raise ValueError('TTA needs at least one transform')
    if len(set(codes)) != len(codes):
        raise ValueError('duplicate TTA transforms in {}'.format(list(transforms)))
    return codes


def tta_swaps_axes(element):
    """Codes 4-7 (transpose, rot90, rot270, anti_transpose) swap H and W: square planes only."""
    return tta_element(element) >= 4


def tta_torch(x, element):
    """The torch definition of element ``element`` on the last two axes (the contract the kernels are tested against)."""
    e = tta_element(element)
    if e == 0:
        return x
    if e == 1:
        return x.flip(-1)
    if e == 2:
        return x.flip(-2)
    if e == 3:
        return x.flip(-2, -1)
    if e == 4:
        return x.transpose(-2, -1)
    if e == 5:
        return torch.rot90(x, 1, (-2, -1))
    if e == 6:
        return torch.rot90(x, 3, (-2, -1))
    return torch.rot90(x, 2, (-2, -1)).transpose(-2, -1)


def tta_pass_seed(seed, element, job):
    """Key of the library's mask draw (rcu_dropout_masks) for MC pass ``job`` (1..T) of the images transformed by ``element``: a function of
    (seed, element, pass) alone.  The identity's key IS ``pass_seed(seed, job)`` (TTA over [identity] is McPredictStep bit for bit); element e
    adds e * 2^40, so for passes 1..2048 no key of one element equals a key of another (the differences e * 2^40 + (t - t') are non-zero and
    far below the modulus 2^63 - 1)."""
    return (pass_seed(seed, job) + tta_element(element) * (1 << 40)) % (2 ** 63 - 1)


def tta_transform(x, element, out=None):
    """``[N, C, H, W]`` float32 -> g(x) on the device (include/rcu.h rcu_tta_transform), into a new tensor or ``out``."""
    e = tta_element(element)
    x = x.to(torch.float32).contiguous()
    n, c, h, w = x.shape
    if e >= 4 and h != w:
        raise ValueError('TTA transform "{}" swaps H and W and needs square slices, got {} x {}'.format(TTA_ELEMENTS[e], h, w))
    if out is None:
        out = torch.empty_like(x)
    _lib.check(_lib.load().rcu_tta_transform(_lib.ptr(x), n, c, h, w, e, _lib.ptr(out), _lib.current_stream()))
    return out


def fold_transformed(src, dst, element):
    """``dst += g^-1(src)`` for two McStatistics of the same shape and flags (include/rcu.h rcu_mc_fold_transformed): ``src`` holds the passes
    over images transformed by ``element``; the pass count moves along."""
    if (src.n, src.nb_classes, src.height, src.width, src.flags) != (dst.n, dst.nb_classes, dst.height, dst.width, dst.flags):
        raise ValueError('statistics of different shapes or flags cannot be folded')
    _lib.check(_lib.load().rcu_mc_fold_transformed(_lib.ptr(src.blob), _lib.ptr(dst.blob), dst.n, dst.height, dst.width, dst.nb_classes, dst.flags,
                                                   tta_element(element), _lib.current_stream()))
    dst.count += src.count


def restart_statistics(stats):
    """Zero a statistics blob for reuse (rcu_mc_begin on the current stream)."""
    _lib.check(_lib.load().rcu_mc_begin(_lib.ptr(stats.blob), stats.n, stats.hw, stats.nb_classes, stats.flags, _lib.current_stream()))
    stats.count = 0


def check_tta_shape(elements, h, w):
    for e in elements:
        if e >= 4 and h != w:
            raise ValueError('TTA transform "{}" swaps H and W and needs square slices; the batch is {} x {}'.format(TTA_ELEMENTS[e], h, w))


class TtaMcPredictStep(BatchStep):
    """EXTENSION -- test-time augmentation, alone or composed with MC dropout (the reference has no TTA).  Every batch runs on its images
    transformed by each element g of ``transforms`` (names or codes of include/rcu.h's D4 table, in the order given); the statistics of a
    transform's passes are mapped back with g^-1 and added to the canonical statistics, so ``MultiPredictionSummary`` finalises V x T samples
    (V transforms, T = ``mc_steps`` passes each) exactly as it finalises McPredictStep's T.
      ``mc_steps = 0``: TTA alone, eval mode, one pass per transform (V samples) -- works with any checkpoint, MC config or not.
      ``mc_steps = T``: T seeded dropout passes per transform.  The factors of (transform g, pass t) for the slice with global index s are
      drawn at first_sample = s under ``tta_pass_seed(seed, g, t)`` -- for the identity the key of McPredictStep's pass t, so
      ``transforms=['identity']`` gives McPredictStep's outputs bit for bit.  ``seed=None``: a seed drawn from torch's generator per batch.
    A launch is one transform of the n images with a pass group of passes (the fused forward + softmax + statistics path, on the canonical plan
    of McPredictStep); a transform's launches alternate over the stream lanes (the first lane rotating with the transform), each lane adds them
    into a statistics blob of its own and folds that into the lane's canonical statistics (rcu_mc_fold_transformed) when the transform is done;
    the identity's passes go into the canonical statistics directly.  The side lanes' statistics are added into lane 0's at the end.
    ``exact`` (default; while V x T <= 2048): exact sums, the outputs do not depend on the transform order, the lanes, the pass groups or the
    ranks; otherwise the result is that of the fold order above.  The weight-scaling pass (``ws_probabilities``) is the plain identity pass in
    eval mode.  Transforms 4-7 swap H and W and are refused (ValueError) on batches that are not square."""

    def __init__(self, transforms, mc_steps=0, seed=None, lanes=None, group_pixels=None, exact=True, do_mi=False, do_var=False, ws_pass=True,
                 materialize=False) -> None:
        super().__init__()
        self.elements = tta_elements(transforms)
        if int(mc_steps) < 0:
            raise ValueError('mc_steps must be >= 0')
        self.mc_steps = int(mc_steps)
        self.seed = seed
        self.lanes = McPredictStep.LANES if lanes is None else max(1, int(lanes))
        self.group_pixels = McPredictStep.GROUP_PIXELS if group_pixels is None else group_pixels
        self.samples = len(self.elements) * max(self.mc_steps, 1)
        self.exact = bool(exact) and self.samples <= _lib.RCU_MC_EXACT_MAX_PASSES
        self.do_mi, self.do_var = do_mi, do_var
        self.ws_pass = ws_pass
        self.materialize = materialize

    @property
    def passes_per_transform(self):
        return max(self.mc_steps, 1)

    def __call__(self, batch_context, task_context, context) -> None:
        _check_context(context)
        images = _images_to_device(batch_context, context)
        model = context.model
        if not isinstance(model, model_mod.UNet):
            raise ValueError('TtaMcPredictStep needs a rcu_amd.model.UNet (the transforms and the fold run on librcu_hip)')
        n, _, h, w = images.shape
        check_tta_shape(self.elements, h, w)
        k = first_sample_of(batch_context, n)
        seed = self.seed
        if seed is None and self.mc_steps > 0:
            seed = int(torch.randint(2 ** 31 - 1, (1,)).item())
        if self.materialize:
            reserve_canonical_plans(model, n, h, w, self.mc_steps, pass_group_size(model, n, h, w, self.group_pixels), 1)
            if self.ws_pass:
                set_dropout_mode(model, is_train=False)
                batch_context.output['ws_probabilities'] = softmax(model(images))
            batch_context.output['multi_probabilities'] = self._materialized(model, images, k, seed)
        else:
            ws = torch.empty((n, model.nb_classes, h, w), device=images.device, dtype=torch.float32) if self.ws_pass else None
            if ws is not None:
                batch_context.output['ws_probabilities'] = ws
            batch_context.output['multi_probabilities'] = self._fused(model, images, self.do_mi, self.do_var, k, seed, ws)

    def _fused(self, model, images, do_mi, do_var, first_sample, seed, ws=None):
        n, _, h, w = images.shape
        engine = HipEngine(model, do_mi, do_var, self.exact)
        stats = engine.side_statistics(images)
        group = pass_group_size(model, n, h, w, self.group_pixels)
        lanes = min(self.lanes, self.samples)
        per = self.passes_per_transform
        plan = launch_plan(([0] if ws is not None else []) + list(range(1, self.samples + 1)), self.elements, per, group, lanes)
        draw = None if self.mc_steps == 0 else (lambda e, jobs: launch_masks(engine, images, e, jobs, per, seed, first_sample))
        try:
            run_plan(plan, engine, images, stats, ws, lanes, draw=draw, reserve=(self.mc_steps, group))
        finally:
            set_dropout_mode(model, is_train=False)

        def recipe(mi, var, materialize=False):
            if materialize:
                return self._materialized(model, images, first_sample, seed)
            return self._fused(model, images, mi, var, first_sample, seed)

        stats.recipe = recipe
        return stats

    def _materialized(self, model, images, first_sample, seed):
        """The V x T probability volumes ``[V*T, N, C, H, W]`` in canonical orientation, transform-major in the given order."""
        xs = {e: (images if e == 0 else tta_transform(images, e)) for e in self.elements}
        probs = []
        set_dropout_mode(model, is_train=self.mc_steps > 0)
        try:
            for e in self.elements:
                for j in range(1, self.passes_per_transform + 1):
                    masks = None if self.mc_steps == 0 else model.seeded_masks(images.shape[0], images.device, [tta_pass_seed(seed, e, j)], first_sample)
                    p = softmax(model(xs[e]) if masks is None else model(xs[e], masks))
                    probs.append(p if e == 0 else tta_transform(p, TTA_INVERSE[e]))
        finally:
            set_dropout_mode(model, is_train=False)
        return torch.stack(probs)


# ------------------------------------------------------------------------------------------------------------------------------
# affine test-time augmentation (EXTENSION; include/rcu_warp.h "Affine test-time augmentation")
# ------------------------------------------------------------------------------------------------------------------------------
AFFINE_MAX_TRANSFORMS = _lib.RCU_WARP_MAX_MATRICES
AFFINE_IDENTITY = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
# D4 element code -> the integer-tap matrix whose warp is rcu_tta_transform's gather (codes 4-7 on square planes)
TTA_AFFINE = (((1, 0, 0), (0, 1, 0)), ((1, 0, 0), (0, -1, 0)), ((-1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, -1, 0)),
              ((0, 1, 0), (1, 0, 0)), ((0, 1, 0), (-1, 0, 0)), ((0, -1, 0), (1, 0, 0)), ((0, -1, 0), (-1, 0, 0)))


def _affine_array(mats, name='matrices'):
    """Anything shaped ``[V, 2, 3]`` (or one ``[2, 3]``) -> float64 numpy ``[V, 2, 3]``; ValueError for other shapes, non-finite entries or
    counts outside 1..64."""
    import numpy as np
    a = np.array(mats.detach().cpu().numpy() if torch.is_tensor(mats) else mats, dtype=np.float64)
    if a.shape == (2, 3):
        a = a[None]
    if a.ndim != 3 or a.shape[1:] != (2, 3) or not 1 <= a.shape[0] <= AFFINE_MAX_TRANSFORMS:
        raise ValueError('{} must be 1..{} matrices of 2 x 3 numbers, got shape {}'.format(name, AFFINE_MAX_TRANSFORMS, a.shape))
    if not np.isfinite(a).all():
        raise ValueError('{} must be finite, got {}'.format(name, a.tolist()))
    return np.ascontiguousarray(a)


def affine_matrix(rotation_deg=0.0, scale=1.0, shift_y=0.0, shift_x=0.0, flip=False):
    """The output-to-source matrix (include/rcu_warp.h: float64 ``[2, 3]``, pixel units about the plane centre, rows (y, x)) of the input warp
    "rotate by ``rotation_deg``, magnify by ``scale``, mirror the columns if ``flip``, shift": R(rotation) / scale, its second column negated for
    ``flip``, the shifts in the last column."""
    import numpy as np
    scale = float(scale)
    if not scale > 0.0 or not np.isfinite(scale):
        raise ValueError('scale must be a positive finite number, got {!r}'.format(scale))
    a = np.deg2rad(float(rotation_deg))
    c, s = np.cos(a) / scale, np.sin(a) / scale
    sign = -1.0 if flip else 1.0
    m = np.array([[c, -s * sign, float(shift_y)], [s, c * sign, float(shift_x)]], dtype=np.float64)
    return _affine_array(m, 'the matrix')[0]


def affine_inverse(M):
    """The matrix of the inverse map of ``M`` (float64 on the host): what ``accumulate_warped`` needs for samples whose inputs were warped with
    ``M``.  ValueError for a singular matrix."""
    import numpy as np
    m = _affine_array(M, 'M')[0]
    a, b, c, d = m[0, 0], m[0, 1], m[1, 0], m[1, 1]
    det = a * d - b * c
    if not np.isfinite(det) or abs(det) <= 1e-12 * max(abs(a), abs(b), abs(c), abs(d), 1e-300) ** 2:
        raise ValueError('the matrix {} is singular'.format(m.tolist()))
    lin = np.array([[d, -b], [-c, a]], dtype=np.float64) / det
    out = np.empty((2, 3), dtype=np.float64)
    out[:, :2] = lin
    out[:, 2] = -(lin @ m[:, 2]) + 0.0      # (+ 0.0: no negative zero in the shifts)
    return _affine_array(out, 'the inverse')[0]


def _affine_uniform(seed, v, e):
    """Uniform e (0..4) of transform v under ``seed``: ((x >> 11) + 0.5) * 2^-53 of x = SplitMix64(key + (8 v + e + 1) * 0x9E3779B97F4A7C15), the
    key ``pass_seed(seed, 0)`` + 64 * 2^40 (the step below the mask keys of ``affine_pass_seed``; no other draw uses it)."""
    from .corruption import _M64, _splitmix64
    key = (pass_seed(seed, 0) + 64 * (1 << 40)) % (2 ** 63 - 1)
    x = _splitmix64((key + (8 * int(v) + e + 1) * 0x9E3779B97F4A7C15) & _M64)
    return ((x >> 11) + 0.5) * 2.0 ** -53


def affine_tta_draw(seed, count, rotation=0.0, scale=0.0, shift=0.0, flip=False):
    """The ``count`` (<= 64) forward matrices of a run seeded with ``seed`` -> float64 ``[count, 2, 3]``.  Transform 0 is the identity; transform
    v >= 1 is a function of (seed, v) alone: the rotation uniform in +-``rotation`` degrees, log2 of the magnification uniform in
    +-log2(1 + ``scale``), the two shifts uniform in +-``shift`` pixels, the mirror a fair coin when ``flip`` -- five uniforms from SplitMix64 of
    the key, as ``corruption.bias_coefficients`` draws its coefficients."""
    import math

    import numpy as np
    count = operator.index(count)
    if not 1 <= count <= AFFINE_MAX_TRANSFORMS:
        raise ValueError('samples must be in 1..{}, got {}'.format(AFFINE_MAX_TRANSFORMS, count))
    rotation, scale, shift = float(rotation), float(scale), float(shift)
    for name, value in (('rotation', rotation), ('scale', scale), ('shift', shift)):
        if not (math.isfinite(value) and value >= 0.0):
            raise ValueError('{} must be a finite number >= 0, got {!r}'.format(name, value))
    out = np.empty((count, 2, 3), dtype=np.float64)
    out[0] = AFFINE_IDENTITY
    for v in range(1, count):
        u = [2.0 * _affine_uniform(seed, v, e) - 1.0 for e in range(5)]
        out[v] = affine_matrix(u[0] * rotation, 2.0 ** (u[1] * math.log2(1.0 + scale)), u[2] * shift, u[3] * shift, bool(flip) and u[4] < 0.0)
    return out


def affine_pass_seed(seed, v, job):
    """Key of the library's mask draw for MC pass ``job`` (1..T) of the images warped with transform ``v`` (0..63): a function of (seed, v, pass)
    alone.  Transform 0, the identity, has the key ``pass_seed(seed, job)`` of McPredictStep; transform v >= 1 adds (64 + v) * 2^40, i.e.
    65 .. 127 steps of 2^40.  The D4 elements use steps 0..7 (``tta_pass_seed``), the corruption stages 16..23 (``corruption.corruption_seed``),
    the k-NN bank draw step 32 (``knn.knn_seed``), and the Laplace and logit sampling a pass's own key (step 0): with passes within 1..2048 of
    ``pass_seed(seed, 0)`` no key of one family equals a key of another, and everything is far below the modulus 2^63 - 1."""
    v = operator.index(v)
    if not 0 <= v < AFFINE_MAX_TRANSFORMS:
        raise ValueError('transform index must be in 0..{}, got {}'.format(AFFINE_MAX_TRANSFORMS - 1, v))
    return (pass_seed(seed, job) + ((64 + v) * (1 << 40) if v else 0)) % (2 ** 63 - 1)


def _affine_device(mats, device):
    return torch.from_numpy(_affine_array(mats)).to(device)


def _warp_affine_device(x, m, out=None):
    """``warp_affine`` with the matrices already on the device (float64 ``[V, 2, 3]``, checked when they were uploaded)."""
    x = x.to(torch.float32).contiguous()
    n, c, h, w = x.shape
    if out is None:
        out = torch.empty((m.shape[0], n, c, h, w), device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (m.shape[0], n, c, h, w) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError('out must be a contiguous float32 tensor of shape {}'.format((m.shape[0], n, c, h, w)))
    _lib.check(_lib.load().rcu_warp_affine(_lib.ptr(x), n, c, h, w, _lib.ptr(m), m.shape[0], _lib.ptr(out), _lib.current_stream()))
    return out


def warp_affine(x, mats, out=None):
    """``[N, C, H, W]`` float32 -> ``[V, N, C, H, W]``: x warped with each of the V matrices ``mats`` (include/rcu_warp.h rcu_warp_affine; host
    numbers ``[V, 2, 3]`` or one ``[2, 3]``, refused unless finite), into a new tensor or ``out``."""
    return _warp_affine_device(x, _affine_device(mats, x.device), out)


def _accumulate_warped_device(inp, stats, m, from_probs=False):
    """``accumulate_warped`` with the matrices already on the device (float64 ``[G, 2, 3]``, checked when they were uploaded)."""
    inp = inp.to(torch.float32).contiguous()
    if inp.dim() != 5 or tuple(inp.shape) != (m.shape[0], stats.n, stats.nb_classes, stats.height, stats.width):
        raise ValueError('expected samples of shape {}, got {}'.format((m.shape[0], stats.n, stats.nb_classes, stats.height, stats.width),
                                                                       tuple(inp.shape)))
    flags = stats.flags | (_lib.RCU_MC_INPUT_PROBS if from_probs else 0)
    _lib.check(_lib.load().rcu_mc_accumulate_warped(_lib.ptr(inp), _lib.ptr(stats.blob), stats.n, stats.height, stats.width, stats.nb_classes,
                                                    flags, _lib.ptr(m), m.shape[0], _lib.current_stream()))
    stats.count += m.shape[0]


def accumulate_warped(inp, stats, mats, from_probs=False):
    """Add the G samples ``inp`` ``[G, N, C, H, W]`` (logits, or probabilities with ``from_probs``) to the McStatistics ``stats`` of the N
    canonical slices, each read through the warp with its matrix of ``mats`` (include/rcu_warp.h rcu_mc_accumulate_warped; pass the INVERSE of
    the matrices the inputs were warped with; host numbers, refused unless finite).  ``stats.count`` grows by G."""
    _accumulate_warped_device(inp, stats, _affine_device(mats, inp.device), from_probs)


class AffineTtaMcPredictStep(BatchStep):
    """EXTENSION -- test-time augmentation with small rotations, scalings, shifts and mirrors (Wang et al. 2019), alone or composed with MC
    dropout.  The V = ``samples`` transforms are ``affine_tta_draw(seed, V, rotation, scale, shift, flip)`` -- transform 0 is the identity -- or the
    explicit forward matrices ``matrices``.  Every batch runs on its images warped with each transform (bilinear, border mode: edge values are
    replicated); each sample's softmax is read back through the inverse warp as it enters the canonical statistics (a resampled entropy is not the
    entropy of the resampled probabilities, so nothing is folded afterwards), and ``MultiPredictionSummary`` finalises V x max(T, 1) samples.
      ``mc_steps = 0``: eval mode, one pass per transform.  ``mc_steps = T``: T seeded dropout passes per transform, the factors of (transform v,
      pass t) for the slice with global index s drawn at s under ``affine_pass_seed(seed, v, t)`` -- the identity's key is McPredictStep's.
    A launch stacks G (transform, pass) pairs of the n images into one batch of G * n warped samples (rcu_warp_affine writes that layout), runs
    ``model.forward`` on it and hands the logits to ``accumulate_warped``; G is ``pass_group_size``, and the plan is reserved for n * min(G, V x T)
    samples before the first forward, so a sample's logits do not depend on the launches.  The launches alternate over ``lanes`` stream lanes
    (default McPredictStep.LANES; ``UNet.forward(..., lane=)``), each lane adding into statistics of its own that are added into lane 0's at the
    end.  ``exact`` (default; while V x T <= 2048): exact sums -- the outputs do not depend on the grouping or the lanes; otherwise the result is
    that of the launch and lane order above.  ``ws_probabilities`` is the plain identity pass in eval mode."""

    def __init__(self, samples=None, mc_steps=0, seed=None, rotation=0., scale=0., shift=0., flip=False, matrices=None, group_pixels=None,
                 exact=True, do_mi=False, do_var=False, ws_pass=True, lanes=None) -> None:
        super().__init__()
        if int(mc_steps) < 0:
            raise ValueError('mc_steps must be >= 0')
        self.mc_steps = int(mc_steps)
        self.seed = seed
        self.lanes = McPredictStep.LANES if lanes is None else max(1, int(lanes))
        if matrices is not None:
            self.matrices = _affine_array(matrices, 'matrices')
            if samples is not None and operator.index(samples) != len(self.matrices):
                raise ValueError('samples is {} but {} matrices were given'.format(samples, len(self.matrices)))
        else:
            if samples is None or isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples <= AFFINE_MAX_TRANSFORMS:
                raise ValueError('samples must be an integer in 1..{}, got {!r}'.format(AFFINE_MAX_TRANSFORMS, samples))
            if seed is None and samples > 1:
                raise ValueError('seed is needed to draw the transforms (or pass matrices)')
            self.matrices = affine_tta_draw(0 if seed is None else seed, samples, rotation, scale, shift, flip)
        try:
            self.inverses = _affine_array([affine_inverse(m) for m in self.matrices], 'matrices')
        except ValueError as e:
            raise ValueError('matrices: {}'.format(e)) from None
        self.options = dict(rotation=float(rotation), scale=float(scale), shift=float(shift), flip=bool(flip))
        self.transforms = len(self.matrices)
        self.samples = self.transforms * max(self.mc_steps, 1)
        self.group_pixels = McPredictStep.GROUP_PIXELS if group_pixels is None else group_pixels
        self.exact = bool(exact) and self.samples <= _lib.RCU_MC_EXACT_MAX_PASSES
        self.do_mi, self.do_var = do_mi, do_var
        self.ws_pass = ws_pass

    def __call__(self, batch_context, task_context, context) -> None:
        _check_context(context)
        model = context.model
        if not isinstance(model, model_mod.UNet):
            raise ValueError('model: AffineTtaMcPredictStep needs a rcu_amd.model.UNet (the warps run on librcu_hip), got {}'.format(
                type(model).__name__))
        if model.sigma_out:
            raise ValueError('model: AffineTtaMcPredictStep does not take a sigma-head model (sigma_out)')
        images = _images_to_device(batch_context, context)
        n, _, h, w = images.shape
        k = first_sample_of(batch_context, n)
        seed = self.seed
        if seed is None and self.mc_steps > 0:
            seed = int(torch.randint(2 ** 31 - 1, (1,)).item())
        ws = torch.empty((n, model.nb_classes, h, w), device=images.device, dtype=torch.float32) if self.ws_pass else None
        if ws is not None:
            batch_context.output['ws_probabilities'] = ws
        batch_context.output['multi_probabilities'] = self._fused(model, images, self.do_mi, self.do_var, k, seed, ws)

    def _chunks(self, model, images, lanes=1):
        """The launches of a batch: (first pair, pairs) of at most G (transform, pass) pairs, in pair order; reserves the canonical plan --
        n * min(G, V x T) samples, not a function of the launches made -- on every lane."""
        n, _, h, w = images.shape
        pairs = self._pairs()
        group = pass_group_size(model, n, h, w, self.group_pixels)
        for lane in range(lanes):
            model.reserve(h, w, n * min(group, len(pairs)), lane)
        return [(b, pairs[b:b + group]) for b in range(0, len(pairs), group)]

    def _pairs(self):
        return [(v, t) for v in range(self.transforms) for t in range(1, max(self.mc_steps, 1) + 1)]

    def _pair_matrices(self, device):
        """The forward and the inverse matrix of every pair on the device, ``[2, V x T, 2, 3]``: one upload per batch on the caller's stream (a
        pageable upload inside a launch would make the host wait for that lane's queue), and a launch's matrices are a slice of it."""
        index = [v for v, _ in self._pairs()]
        return _affine_device(self.matrices[index], device), _affine_device(self.inverses[index], device)

    def _logits(self, model, images, forward, first, chunk, first_sample, seed, lane=0):
        """The logits ``[G, n, C, H, W]`` of one launch: the n images warped with the transforms of the G pairs of ``chunk``, one forward."""
        n, _, h, w = images.shape
        x = _warp_affine_device(images, forward[first:first + len(chunk)]).view(len(chunk) * n, images.shape[1], h, w)
        masks = None
        if self.mc_steps > 0:
            masks = HipEngine(model).seeded_masks(images, [affine_pass_seed(seed, v, t) for v, t in chunk], first_sample)
        return model(x, masks, lane=lane).view(len(chunk), n, model.nb_classes, h, w)

    def _fused(self, model, images, do_mi, do_var, first_sample, seed, ws=None):
        engine = HipEngine(model, do_mi, do_var, self.exact)
        set_dropout_mode(model, is_train=False)
        stats = engine.side_statistics(images)
        lanes = StreamLanes(images.device, min(self.lanes, self.samples))
        chunks = self._chunks(model, images, lanes.count)
        forward, back = self._pair_matrices(images.device)
        lanes.begin(stats, lambda: engine.side_statistics(images), inputs=(images, forward, back))
        if ws is not None:
            engine.ws_pass(images, ws)          # on the caller's stream, beside the side lanes' first launches

        def launch(st, lane, first, chunk):
            logits = self._logits(model, images, forward, first, chunk, first_sample, seed, lane)
            _accumulate_warped_device(logits, st, back[first:first + len(chunk)])

        for first, chunk in chunks:
            lanes.run(lambda st, lane, first=first, chunk=chunk: launch(st, lane, first, chunk))
        if lanes.count > 1:
            lanes.end(engine.merge)

        def recipe(mi, var, materialize=False):
            if materialize:
                return self._materialized(model, images, first_sample, seed)
            return self._fused(model, images, mi, var, first_sample, seed)

        stats.recipe = recipe
        return stats

    def _materialized(self, model, images, first_sample, seed):
        """The V x T probability volumes ``[V*T, N, C, H, W]`` warped back to the canonical grid, transform-major."""
        set_dropout_mode(model, is_train=False)
        forward, back = self._pair_matrices(images.device)
        probs = []
        for first, chunk in self._chunks(model, images):
            logits = self._logits(model, images, forward, first, chunk, first_sample, seed)
            for g in range(len(chunk)):
                probs.append(_warp_affine_device(softmax(logits[g]), back[first + g:first + g + 1])[0])
        return torch.stack(probs)


def wait_for_outputs(batch_context):
    """Order the current stream behind outputs a step produced on a stream of its own (``batch_context.more['outputs_ready']``, set by
    MultiPredictionSummary for the root of a sharded predict step).  Steps and hooks that read ``batch_context.output`` tensors on the
    compute stream call this first; the test loop's download waits for the same event on its own stream."""
    event = batch_context.more.get('outputs_ready')
    if event is not None:
        torch.cuda.current_stream().wait_event(event)
        for value in batch_context.output.values():
            if torch.is_tensor(value) and value.is_cuda:
                value.record_stream(torch.cuda.current_stream())


def prediction_and_foreground(probabilities):
    """``[N, C, H, W]`` probabilities -> (uint8 argmax ``[N, H, W]``, float32 foreground probability
    ``[N, H, W]``): what the reference's writers derive with numpy before saving
    ``*_prediction`` / ``*_probabilities`` (bin-dl/brats_test_default.py:96-99)."""
    p = probabilities.to(torch.float32).contiguous()
    n, c, h, w = p.shape
    pred = torch.empty((n, h, w), device=p.device, dtype=torch.uint8)
    fg = torch.empty((n, h, w), device=p.device, dtype=torch.float32)
    _lib.check(_lib.load().rcu_prediction_and_foreground(_lib.ptr(p), n, h * w, c, _lib.ptr(pred), _lib.ptr(fg),
                                                         _lib.current_stream()))
    return pred, fg


def sigma_of_prediction(logits, sigma_raw, is_log_sigma=False):
    """sigma of the predicted class per voxel (bin-dl/brats_test_aleatoric.py:95-97) -> (prediction u8, sigma f32)."""
    logits = logits.to(torch.float32).contiguous()
    sigma_raw = sigma_raw.to(torch.float32).contiguous()
    n, c, h, w = logits.shape
    pred = torch.empty((n, h, w), device=logits.device, dtype=torch.uint8)
    sp = torch.empty((n, h, w), device=logits.device, dtype=torch.float32)
    _lib.check(_lib.load().rcu_aleatoric(_lib.ptr(logits), _lib.ptr(sigma_raw), n, h * w, c, int(is_log_sigma), None,
                                         None, _lib.ptr(pred), _lib.ptr(sp), _lib.current_stream()))
    return pred, sp


def channel_to_end(tensor):
    """NCHW -> NHWC view, as the test loop applies before ``.cpu().numpy()`` (torchhelper.py:10-23; loops.py:214-220)."""
    dims = tensor.dim()
    return tensor.permute(0, *range(2, dims), 1)
