"""The reference's test / evaluation command lines, running on librcu_hip.

Each function is the ``main`` of the same-named reference script (flags unchanged):
    bin-dl/brats_test_default.py   -config_file / -config_id      (bin-dl/brats_test_default.py:22-61, 113-117)
    bin-dl/brats_test_ensemble.py  -config_file                   (bin-dl/brats_test_ensemble.py:25-69)
    bin-dl/brats_test_aleatoric.py -config_file                   (bin-dl/brats_test_aleatoric.py:24-48)
    bin-dl/isic_test_default.py / isic_test_ensemble.py / isic_test_aleatoric.py
    bin-dl/{brats,isic}_test_auxiliary_feat.py -config_file       (bin-dl/brats_test_auxiliary_feat.py:23-61)
    bin-dl/{brats,isic}_test_auxiliary_segm.py -config_file       (bin-dl/brats_test_auxiliary_segm.py:23-47)
    bin-eval/eval_uncertainty.py   --ds --ids --act               (bin-eval/eval_uncertainty.py:13-50, 248-288)
    bin-dl/{brats,isic}_fit_temperature.py -config_file           (EXTENSION: temperature scaling, fit_temperature)
    bin-dl/{brats,isic}_fit_density.py -config_file               (EXTENSION: feature-space density, fit_density)
    bin-dl/{brats,isic}_fit_knn.py -config_file                   (EXTENSION: nearest-neighbour feature uncertainty, fit_knn)
    bin-dl/{brats,isic}_fit_laplace.py -config_file               (EXTENSION: last-layer Laplace, fit_laplace)
Config ids map to the same YAML names under ``<project>/config``; paths inside the YAML stay relative to the
working directory, as in the reference.  Datasets: see rcu_amd.data (volume directories instead of pymia HDF5).
"""
import collections
import csv
import json
import logging
import os

import numpy as np
import torch

from . import _lib
from . import auxiliary as auxiliary_mod
from . import calibration
from . import corruption as corruption_mod
from . import data as data_mod
from . import density as density_mod
from . import distributed as rdist
from . import evalrun
from . import evaluation as ev
from . import knn as knn_mod
from . import laplace as laplace_mod
from . import loops
from . import management as mgt
from . import model as model_mod
from . import nifti
from . import steps

PROJECT_DIR = os.environ.get('RCU_PROJECT_DIR', os.getcwd())
CONFIG_DIR = os.path.join(PROJECT_DIR, 'config')


def _config_path(dataset, config_id, default='baseline'):
    if config_id in ('baseline', 'baseline_mc', 'center', 'center_mc'):
        return os.path.join(CONFIG_DIR, 'test_{}_{}.yaml'.format(dataset, config_id))
    if config_id in ('cv0', 'cv1', 'cv2', 'cv3', 'cv4'):
        return os.path.join(CONFIG_DIR, 'baseline_cv', 'test_{}_baseline_cv{}.yaml'.format(dataset, config_id[-1]))
    return os.path.join(CONFIG_DIR, 'test_{}_{}.yaml'.format(dataset, default))


class EvalSubjectStep(loops.SubjectStep):
    """Dice of the arg-max prediction (brats_test_default.py:63-77; isic_test_default.py:70-86)."""

    def __init__(self, squeeze_labels=False, keep_prediction=False):
        self.evaluate = ev.ComposeEvaluation([ev.DiceNumpy()])
        self.squeeze_labels, self.keep_prediction = squeeze_labels, keep_prediction

    def __call__(self, subject_context, task_context, context) -> None:
        probabilities = subject_context.subject_data['probabilities']
        per_slice = subject_context.subject_data.pop('confusion', None)
        if per_slice is not None:
            # the counts were taken slice by slice on the GPU, behind the predict step (ConfusionOnDeviceStep), and came to the host with the
            # batches: integers, so their sum IS the confusion matrix of the assembled subject.  Nothing here touches the GPU -- and a
            # volume's arg-max for the *_prediction file stays with the writer thread
            tp, _, fp, fn = (int(v) for v in np.asarray(per_slice).reshape(-1, 4).sum(axis=0))
            subject_context.metrics.update({'dice': ev.dice_from_counts(tp, fp, fn)})
            made = subject_context.subject_data.get('prediction')       # 2-D subjects: the arg-max map came with the batch too
            if made is not None:
                made = np.asarray(made, dtype=np.uint8)
                made = made[..., 0] if (made.ndim == np.ndim(probabilities) and made.shape[-1] == 1) else made
                subject_context.more['prediction'] = (made, probabilities)
            if self.keep_prediction:
                if made is None:
                    made = nifti.argmax_last(probabilities, np.uint8)
                    subject_context.more['prediction'] = (made, probabilities)
                subject_context.subject_data['prediction'] = made.astype(np.int64)
            elif made is not None:
                del subject_context.subject_data['prediction']
            return
        prediction = nifti.argmax_last(probabilities, np.uint8)      # (class indices: uint8 holds them; np.argmax's int64 where it is kept)
        if self.keep_prediction:
            subject_context.subject_data['prediction'] = prediction.astype(np.int64)
        # the writer hook takes it from here instead of a second arg-max -- as long as ``probabilities`` still is the array it was taken from
        # (a later subject step may replace it: the reference's writer arg-maxes at write time, brats_test_default.py:96-99)
        subject_context.more['prediction'] = (prediction, probabilities)
        target = subject_context.subject_data['labels']
        if self.squeeze_labels:
            target = target.squeeze(-1)
        results = {}
        self.evaluate({'prediction': prediction, 'probabilities': probabilities, 'target': target}, results)
        subject_context.metrics.update(results)


class WriteHook(loops.TestLoopHook):
    """``{subject}_probabilities|_prediction[|_sigma].nii.gz`` from a background thread
    (brats_test_default.py:80-108; brats_test_aleatoric.py:76-110; isic_test_default.py:89-124)."""

    def __init__(self, with_sigma=False, link_inputs=False, in_background=True):
        self.with_sigma, self.link_inputs, self.in_background = with_sigma, link_inputs, in_background

    def on_test_subject_end(self, subject_context, task_context, context):
        if not isinstance(context, loops.TorchTestContext):
            raise ValueError('expected type is "TorchTestContext" but object is of type "{}"'.format(type(context).__name__))
        data = subject_context.subject_data
        subject = data.get('subject', subject_context.subject_index)
        cached = subject_context.more.get('prediction')
        prediction = cached[0] if (isinstance(cached, tuple) and cached[1] is data['probabilities']) else None
        nifti.write_subject(context.test_dir, subject, data['probabilities'], data.get('properties'),
                            data['sigma'] if self.with_sigma else None, in_background=self.in_background,
                            prediction=prediction)
        if self.link_inputs:   # ISIC: symlink image and label next to the outputs
            files = context.test_data.dataset.get_files_by_id(subject_context.subject_index)
            for key in ('label_paths', 'image_paths'):
                src = os.path.abspath(files[key])
                dst = os.path.join(context.test_dir, os.path.basename(src))
                if not os.path.lexists(dst):
                    os.symlink(src, dst)

    def on_termination(self, context):
        nifti.join_all()


class ConfusionOnDeviceStep(steps.BatchStep):
    """The Dice counts of the subjects' evaluation (EvalSubjectStep: brats_test_default.py:63-77, isic_test_default.py:70-86) taken at BATCH
    time, on the compute stream, right behind the predict steps: tp / tn / fp / fn of every slice (image) of the batch against its labels ->
    ``output['confusion']`` ``[N, 4]`` int64, which travels to the host with the batch's other kept entries and is assembled like them
    (``[D, 4]`` per volume, ``[4]`` per 2-D subject).  2-D subjects also get ``output['prediction']`` -- the arg-max map (uint8) their
    evaluation and their writer want.
    Why: at subject level the same counts cost the test loop's MAIN thread three small synchronous GPU operations, and next to a loop that
    has run ahead -- every CU held by a persistent conv kernel -- each of them waits its turn: 72-94 ms per BraTS subject, 6.8 ms per ISIC
    image (218 ms per batch of 32, whose GPU work takes 61: tools/host_costs_probe.py, tools/isic_script_throughput.py).  Here they are
    stream-ordered work like any kernel of the batch and nobody waits for them.
    Labels reach the device through a ring of pinned buffers (a copy may still be queued behind the batches the loop has run ahead with):
    a volume's labels once per subject -- from the dataset, sliced on the device --, a 2-D batch's own ``labels`` entry once per batch."""

    RING = 16          # > loops.Test.MAX_INFLIGHT: the copy that used a buffer last has long run when its turn comes again

    def __init__(self):
        self._pinned = [None] * self.RING      # (pinned uint8 tensor, event of the copy that read it last)
        self._next = 0
        self._volumes = {}         # subject index -> device uint8 [D, H, W]
        self._side = None          # the root of a sharded run: the stream the counts are taken on (behind the batch's collective)

    def _upload(self, labels, device):
        """host uint8 array -> device tensor of its shape, asynchronously on the current stream."""
        slot = self._next % self.RING
        self._next += 1
        entry = self._pinned[slot]
        if entry is None or entry[0].numel() < labels.size:
            entry = (torch.empty(labels.size, dtype=torch.uint8, pin_memory=True), torch.cuda.Event())
        else:
            entry[1].synchronize()       # the copy that used this buffer RING uploads ago has run
        self._pinned[slot] = entry
        host = entry[0][:labels.size]
        # (numpy's copy, not torch's: a torch CPU copy of this size starts an OpenMP team on the calling thread -- beside the loader thread's
        # own team the 4 MB took 35 ms, tools/host_costs_probe.py)
        np.copyto(host.numpy(), labels.reshape(-1))
        dev = torch.empty(labels.size, dtype=torch.uint8, device=device)
        dev.copy_(host, non_blocking=True)
        entry[1].record()
        return dev.view(labels.shape)

    def _labels_of(self, subject, dataset, device):
        vol = self._volumes.get(subject)
        if vol is None:
            labels = dataset.direct_extract(subject, ('labels',)).get('labels')
            if labels is None:           # a dataset without labels: nothing to count (EvalSubjectStep will say so, as in the reference)
                return None
            labels = np.ascontiguousarray(labels, dtype=np.uint8)
            if labels.ndim == 4 and labels.shape[-1] == 1:
                labels = labels[..., 0]
            vol = self._volumes[subject] = self._upload(labels, device)
            for other in [k for k in self._volumes if k != subject][:-1]:      # this subject and the one before it (a batch may span two)
                del self._volumes[other]
        return vol

    def __call__(self, batch_context, task_context, context) -> None:
        probabilities = batch_context.output.get('probabilities')
        if probabilities is None or not probabilities.is_cuda:
            return            # (a rank other than the root of a sharded run has nothing to evaluate)
        batch = batch_context.input
        dataset = getattr(getattr(task_context, 'data', None), 'dataset', None)
        volumes = 'slice_index' in batch and hasattr(dataset, 'direct_extract')
        labels = None if volumes else batch.get('labels')
        if not volumes and not (torch.is_tensor(labels) and labels.numel() == probabilities.shape[0] * probabilities.shape[2] * probabilities.shape[3]):
            return            # (no labels of the batch's shape at hand: EvalSubjectStep evaluates the assembled subject itself)
        # The root of a sharded run: the summary's outputs come from a side stream BEHIND the batch's collective.  Counting on the compute stream
        # would put that stream -- and with it the next batch's passes -- behind every batch's reduce and finalize, on the one rank every reduce
        # lands on; the counts are taken on a stream of their own that waits for the outputs, and the download waits for the counts instead.
        ready = batch_context.more.get('outputs_ready')
        if ready is None:
            self._count(batch_context, task_context, probabilities, batch, dataset, volumes, labels)
            return
        if self._side is None or self._side.device != probabilities.device:
            self._side = torch.cuda.Stream(device=probabilities.device)
        self._side.wait_event(ready)
        with torch.cuda.stream(self._side):
            if self._count(batch_context, task_context, probabilities, batch, dataset, volumes, labels):
                probabilities.record_stream(self._side)
                done = torch.cuda.Event()
                done.record(self._side)
                batch_context.more['outputs_ready'] = done      # (behind the old event by construction)

    def _count(self, batch_context, task_context, probabilities, batch, dataset, volumes, labels):
        """The arg-max map and the slice-wise confusion counts on the CURRENT stream -> whether they were taken."""
        prediction, _ = steps.prediction_and_foreground(probabilities)
        if volumes:
            subjects = [int(v) for v in batch['subject_index']]
            slices = [int(v) for v in batch['slice_index']]
            pieces, b, n = [], 0, len(subjects)
            while b < n:                                                        # runs of consecutive slices of one subject
                e = b + 1
                while e < n and subjects[e] == subjects[b] and slices[e] == slices[e - 1] + 1:
                    e += 1
                volume = self._labels_of(subjects[b], dataset, prediction.device)
                if volume is None:
                    return False
                pieces.append(volume[slices[b]:slices[b] + (e - b)])
                b = e
            target = pieces[0] if len(pieces) == 1 else torch.cat(pieces)
        else:
            # the cast evaluation._to_dev makes of the assembled subject's labels (the shipped ISIC configs rescale them to float 0 / 1)
            host = labels.detach().cpu().numpy()
            host = host if host.dtype == np.uint8 else host.astype(np.uint8)
            target = self._upload(np.ascontiguousarray(host).reshape(prediction.shape), prediction.device)
            batch_context.output['prediction'] = prediction.unsqueeze(1)      # (outputs carry the channel dim at 1: the loop moves it to the end)
        batch_context.output['confusion'] = ev.confusion_counts_on_device(prediction, target)
        return True


class CollectOnDeviceStep(steps.BatchStep):
    """Part of ``others.device_metrics`` (DeviceMetricsHook): right behind the predict steps, the batch's foreground probability and
    arg-max prediction are copied -- device to device, on the compute stream -- into per-subject volumes that stay in HBM until the subject
    has been evaluated there."""

    def __init__(self, store):
        self.store = store          # subject key -> {'p': [D, H, W] float32, 'prediction': [D, H, W] uint8} (2D subjects: [H, W])

    def __call__(self, batch_context, task_context, context) -> None:
        probabilities = batch_context.output.get('probabilities')
        if probabilities is None or not probabilities.is_cuda:
            return            # (a rank other than the root of a sharded run has nothing to evaluate)
        steps.wait_for_outputs(batch_context)      # (the root of a sharded run: the summary's outputs come from a side stream)
        pred, fg = steps.prediction_and_foreground(probabilities)            # what the writer derives on the host (brats_test_default.py:96-99)
        batch = batch_context.input
        if 'slice_index' in batch:                                          # slices of volumes
            subjects = [int(v) for v in batch['subject_index']]
            slices = [int(v) for v in batch['slice_index']]
            b, n = 0, len(subjects)
            while b < n:                                                    # runs of consecutive slices of one subject: one copy each
                e = b + 1
                while e < n and subjects[e] == subjects[b] and slices[e] == slices[e - 1] + 1:
                    e += 1
                vol = self.store.get(subjects[b])
                if vol is None:
                    depth = int(batch['shape'][b][0])
                    vol = self.store[subjects[b]] = {'p': fg.new_empty((depth,) + tuple(fg.shape[1:])),
                                                     'prediction': pred.new_empty((depth,) + tuple(pred.shape[1:]))}
                vol['p'][slices[b]:slices[b] + (e - b)] = fg[b:e]
                vol['prediction'][slices[b]:slices[b] + (e - b)] = pred[b:e]
                b = e
        else:                                                               # every sample is a subject (ISIC)
            for b, id_ in enumerate(batch['ids']):
                self.store[id_] = {'p': fg[b].clone(), 'prediction': pred[b].clone()}


class DeviceMetricsHook(loops.TestLoopHook):
    """OPT-IN (YAML ``others.device_metrics``, an rcu_amd extension): the calibration / uncertainty-error metrics of
    bin-eval/eval_uncertainty.py computed on every subject while its maps are still in HBM -- no .nii.gz round trip
    (bin-dl/brats_test_default.py:96-108 -> rechun/eval/analysis.py:75-107) -- and written as the CSV files the evaluation script would
    write from the files of this run (same names, columns, rows: the float32 round trip through NIfTI is lossless).

        others:
          device_metrics:
            actions: [minmax, ece_dice, calib, bnf_ue]     # default: all four
            run_id: baseline_mc                            # the test_id column and the file names (default: the config's test_name)
            gt_dir: /data/Brats18/Training                 # ground-truth tree (ISIC: the dataset prefix) the evaluation reads target and T2
                                                           # mask from; without it: the dataset's labels, no mask
            out_dir: null                                  # default: <test_dir>/eval

    The reference's contract stays the file round trip; this hook is the fused path SURVEY.md 8(f)1 leaves optional."""

    def __init__(self, dataset, spec, store):
        spec = dict(spec or {}) if not isinstance(spec, (list, tuple)) else {'actions': list(spec)}
        self.dataset = dataset
        self.action_names = list(spec.get('actions') or ['minmax', 'ece_dice', 'calib', 'bnf_ue'])
        if 'quantiles' in self.action_names:       # (the hook sees probability maps only: there is nothing to rescale, and the action reads a run twice)
            raise ValueError('others.device_metrics: the action "quantiles" works on the files of a sigma / density run (bin-eval/eval_uncertainty.py '
                             '--act quantiles); the hook sees probability maps only')
        self.run_id,self.gt_dir, self.out_dir = spec.get('run_id'), spec.get('gt_dir'), spec.get('out_dir')
        self.store = store
        self.actions, self.rows, self.gts = [], {}, None
        self.batch = None

    def on_test_start(self, task_context, context):
        base = self.out_dir or os.path.join(context.test_dir, 'eval')
        details = 'foreground' if (self.dataset == 'brats' and self.gt_dir) else ''      # eval_uncertainty.py:19-26
        self.actions = evalrun.get_actions(self.action_names, os.path.join(base, evalrun.MINMAX_NAME), base, details)
        entry = evalrun.EvalData(self.run_id or context.config.test_name, context.test_dir, 'probabilities')
        for action in self.actions:
            action.setup_eval(entry)
        if not evalrun._fusable(entry, self.actions):
            raise ValueError('others.device_metrics: unsupported actions {}'.format(self.action_names))
        for action in self.actions:
            action.start_eval()
        self.call, self.want_mask, _ = evalrun.metrics_call(self.actions)
        if self.gt_dir:
            gts = (evalrun.collect_brats_ground_truth if self.dataset == 'brats' else evalrun.collect_isic_ground_truth)(self.gt_dir)
            self.gts = {sf.subject: sf for sf in gts}

    def on_test_subject_end(self, subject_context, task_context, context):
        vol = self.store.pop(subject_context.subject_index, None)
        if vol is None:
            raise ValueError('others.device_metrics: subject {} was not collected on the device'.format(subject_context.subject_index))
        name = str(loops._subject_name(subject_context))
        mask = None
        if self.gts is not None:             # the evaluation's own inputs (analysis.py:88-89, 118-125)
            sf = self.gts[name]
            target = (evalrun.read_label_image(sf.categories['labels']['gt']) > 0).astype(np.uint8)
            if self.want_mask:
                mask = nifti.read(sf.categories['images']['t2'])[0] > 0
        else:
            target = (np.asarray(subject_context.subject_data['labels']) > 0).astype(np.uint8)
        n = vol['p'].numel()
        target = np.squeeze(target) if target.size == n and target.shape != tuple(vol['p'].shape) else target
        if self.batch is None or self.batch.n != n:
            self.batch = ev.SubjectBatch(1, n, device=vol['p'].device, with_mask=self.want_mask)
        self.batch.used = 0
        self.batch.put(0, vol['p'], vol['prediction'], target, mask)
        self.batch.upload()
        self.rows[name] = (self.batch.metrics(**self.call), target.ndim)

    def on_test_end(self, task_context, context):
        for name in sorted(self.rows):       # the evaluation script's subject order (rechun/eval/evaldata.py: sorted by subject)
            res, n_dim = self.rows[name]
            evalrun.record_subject(self.actions, name, res, 0, n_dim)
        for action in self.actions:
            action.finish_eval()
        self.rows = {}


class PrepareSubjectStep(steps.BatchStep):
    def __call__(self, batch_context, task_context, context) -> None:
        batch_context.output['labels'] = batch_context.input['labels'].unsqueeze(1)   # isic_test_default.py:62-66


def _other(context, key, default=None):
    """A key of the YAML file's free-form ``others`` (rcu_amd extensions, absent from the reference's configs): the options coalesce_pixels,
    pipelined, max_inflight, loader_timing, stream_lanes, group_pixels, exact, device_metrics, device_confusion, and the keys of ``_OTHERS``,
    which only some scripts take."""
    return getattr(context.config.others, key, default)


_TEST_SCRIPTS = frozenset(('default', 'ensemble', 'aleatoric', 'auxiliary_feat', 'auxiliary_segm'))
_DEFAULT = frozenset(('default',))
_ONE_PASS_FIT = 'others.{}: the density fit is one eval-mode pass per batch and does not take it'
_ONE_PASS_LAPLACE = 'others.{}: the Laplace fit is one eval-mode pass per batch and does not take it'
_ONE_PASS_AUXILIARY = 'others.{}: the auxiliary fit is one eval-mode pass of the frozen U-Net per batch and does not take it'
_OtherKey = collections.namedtuple('_OtherKey', 'name description home scripts tail overrides', defaults=('', {}))
# The extension keys of ``others`` that not every script takes, in the order they are checked: name, the description and the home its refusal
# names, the scripts that take it, a tail to the refusal, the scripts that refuse it in words of their own.  A new key is a row here and its builder.
_OTHERS = (
    _OtherKey('tta', 'test-time augmentation', 'the default test scripts only', _DEFAULT,
              overrides={'fit_temperature': 'others.tta: the temperature fit does not run under test-time augmentation',
                         'fit_density': _ONE_PASS_FIT.format('tta'), 'fit_laplace': _ONE_PASS_LAPLACE.format('tta'),
                         'fit_auxiliary_feat': _ONE_PASS_AUXILIARY.format('tta')}),
    _OtherKey('mc', None, None, _TEST_SCRIPTS | {'fit_temperature'},
              overrides={'fit_density': _ONE_PASS_FIT.format('mc'), 'fit_laplace': _ONE_PASS_LAPLACE.format('mc'),
                         'fit_auxiliary_feat': _ONE_PASS_AUXILIARY.format('mc')}),
    _OtherKey('temperature', 'temperature scaling', 'the default test scripts only', _DEFAULT | {'fit_laplace'}),
    _OtherKey('agreement', 'MC sample agreement', 'the default test scripts with others.mc only', _DEFAULT),
    _OtherKey('mc_adaptive', 'adaptive MC dropout', 'the default test scripts with others.mc only', _DEFAULT),
    _OtherKey('logit_samples', 'test-time logit sampling', 'the aleatoric test scripts only', frozenset(('aleatoric',))),
    _OtherKey('corruption', 'input corruptions', 'the test scripts only', _TEST_SCRIPTS, tail=': calibration is fitted on clean validation data'),
    _OtherKey('density', 'feature-space density uncertainty', 'the default test scripts only', _DEFAULT),
    _OtherKey('auxiliary_fit', 'the options of the auxiliary fit', 'the auxiliary fit scripts only', frozenset(('fit_auxiliary_feat',))),
    _OtherKey('knn', 'nearest-neighbour feature uncertainty', 'the default test scripts only', _DEFAULT),
    _OtherKey('knn_bank', 'the options of the k-NN bank', 'the k-NN fit scripts only', frozenset(('fit_knn',))),
    _OtherKey('tta_affine', 'affine test-time augmentation', 'the default test scripts only', _DEFAULT,
              overrides={'fit_temperature': 'others.tta_affine: the temperature fit does not run under test-time augmentation',
                         'fit_density': _ONE_PASS_FIT.format('tta_affine'), 'fit_laplace': _ONE_PASS_LAPLACE.format('tta_affine'),
                         'fit_auxiliary_feat': _ONE_PASS_AUXILIARY.format('tta_affine')}),
    _OtherKey('laplace', 'last-layer Laplace uncertainty', 'the default test scripts only', _DEFAULT),
)


def _lacks_mc(others, world):
    return not hasattr(others, 'mc')


def _sharded(others, world):
    return world.world > 1


# What a key of the default script does not compose with: (key, the other key -- set in the YAML file -- or a condition (others, world), message),
# in the order the rules of a key are checked.  ``agreement: false`` is the key switched off.
_RULES = tuple(('density', key, 'others.density does not compose with others.{}: the density map belongs to the one deterministic pass'.format(key))
               for key in ('mc', 'tta', 'agreement', 'mc_adaptive', 'logit_samples')) + (
    ('mc_adaptive', 'tta', 'others.mc_adaptive does not compose with others.tta (test-time augmentation): the transforms of a slice share its statistics'),
    ('mc_adaptive', _lacks_mc, 'others.mc_adaptive needs others.mc: there are no passes to save without MC dropout'),
    ('mc_adaptive', lambda others, world: getattr(others, 'agreement', False),
     'others.mc_adaptive does not compose with others.agreement: the vote planes assume every slice sees every pass'),
    ('mc_adaptive', lambda others, world: not bool(getattr(others, 'exact', True)),
     'others.mc_adaptive needs exact statistics (others.exact: false is refused): the decision is made on exact integer sums'),
    ('mc_adaptive', _sharded, 'others.mc_adaptive is not sharded: run the script in one process'),
    ('agreement', 'tta', 'others.agreement does not compose with others.tta (test-time augmentation): the vote plane holds the passes of MC dropout alone'),
    ('agreement', _lacks_mc, 'others.agreement needs others.mc: there are no samples to compare without MC dropout passes'),
    ('agreement', _sharded, 'others.agreement is not sharded: run the script in one process (a vote plane lives where all passes of a batch run)'),
) + (
    ('tta_affine', 'tta', 'others.tta_affine does not compose with others.tta: a run takes its transforms from one of the two keys'),
    ('tta_affine', 'agreement', 'others.tta_affine does not compose with others.agreement: the vote plane holds the passes of MC dropout alone'),
    ('tta_affine', 'mc_adaptive', 'others.tta_affine does not compose with others.mc_adaptive: the transforms of a slice share its statistics'),
) + tuple(('tta_affine', key, 'others.tta_affine does not compose with others.{}: that map belongs to the one deterministic pass'.format(key))
          for key in ('density', 'laplace', 'knn')) + (
    ('tta_affine', _sharded, 'others.tta_affine is not sharded: run the script in one process'),
) + tuple(('laplace', key, 'others.laplace does not compose with others.{}: the Laplace predictive belongs to the one deterministic pass'.format(key))
          for key in ('mc', 'tta', 'agreement', 'mc_adaptive', 'logit_samples')) + (
    ('laplace', 'density', 'others.laplace does not compose with others.density: each replaces the default predict step with its own'),
) + tuple(('knn', key, 'others.knn does not compose with others.{}: the k-NN map belongs to the one deterministic pass'.format(key))
          for key in ('mc', 'tta', 'agreement', 'mc_adaptive', 'logit_samples')) + tuple(
    ('knn', key, 'others.knn does not compose with others.{}: each replaces the default predict step with its own'.format(key))
    for key in ('density', 'laplace'))


_TAKEN_BY = {row.name: row.scripts for row in _OTHERS}


def _is_set(others, key):
    return hasattr(others, key) and not (key == 'agreement' and others.agreement is False)


def _check_rules(others, world, key):
    """Raises the first rule of ``_RULES`` that the YAML file's ``key`` breaks."""
    for owner, other, message in _RULES:
        if owner == key and (other(others, world) if callable(other) else _is_set(others, other)):
            raise ValueError(message)


def _check_others(context, script, world):
    """Every script's first look at ``others``: the first key of ``_OTHERS`` that ``script`` does not take is refused by name.  (A key the script
    takes that names the refused one in ``_RULES`` speaks first: it says what the two have to do with each other.)"""
    others = context.config.others
    for row in _OTHERS:
        if not hasattr(others, row.name) or script in row.scripts:
            continue
        if script in row.overrides:
            raise ValueError(row.overrides[script])
        for owner, other, _ in _RULES:
            if other == row.name and hasattr(others, owner) and script in _TAKEN_BY[owner]:
                _check_rules(others, world, owner)
        raise ValueError('others.{} ({}) applies to {}; the {} script does not take it{}'.format(row.name, row.description, row.home, script, row.tail))


def _mask_seed(context, world):
    """Seed of the per-(pass, slice) Dropout2d masks: the YAML file's ``seed`` (the reference seeds torch with it,
    common/trainloop/loops.py:183-185).  Without one a one-process run draws from the device generator; a sharded run agrees on a
    random seed (the masks of a pass must not depend on the rank that runs it)."""
    seed = context.config.seed
    if seed is None and world.world > 1:
        import torch
        import torch.distributed as dist
        t = torch.randint(2 ** 31 - 1, (1,), dtype=torch.int64)
        if world.backend == 'nccl':
            t = t.to(world.device)
        dist.broadcast(t, src=0)
        seed = int(t.item())
    return seed


def _tta_steps(context, world):
    """``others.tta`` (an rcu_amd extension): test-time augmentation over the listed D4 transforms (include/rcu.h), composed with ``others.mc``
    when that is set (V transforms x T passes, with the weight-scaling pass as the MC step runs it), else alone in eval mode (V passes, no
    weight-scaling pass) -- in place of the predict step, followed by MultiPredictionSummary, whose ``probabilities`` the writer saves."""
    others = context.config.others
    transforms = others.tta
    if isinstance(transforms, str):
        transforms = [transforms]
    mc = int(getattr(others, 'mc', 0) or 0)
    lanes, group_pixels, exact = _other(context, 'stream_lanes'), _other(context, 'group_pixels'), bool(_other(context, 'exact', True))
    seed = _mask_seed(context, world) if mc > 0 else None
    if world.world > 1:
        step = rdist.ShardedTtaMcPredictStep(transforms, world, mc_steps=mc, seed=0 if seed is None else seed, lanes=lanes,
                                             group_pixels=group_pixels, exact=exact, ws_pass=mc > 0)
    else:
        step = steps.TtaMcPredictStep(transforms, mc_steps=mc, seed=seed, lanes=lanes, group_pixels=group_pixels, exact=exact, ws_pass=mc > 0)
    return [step, steps.MultiPredictionSummary()]


def _agreement(context, world):
    """``others.agreement: true`` (an rcu_amd extension, include/rcu.h "Sample agreement"): the T = ``others.mc`` samples of a subject compared as
    whole segmentations -> ``<test_dir>/agreement.csv``.  One process, MC dropout alone (``_RULES``): a ValueError that names the key otherwise."""
    value = _other(context, 'agreement', False)
    if not isinstance(value, bool):
        raise ValueError('others.agreement must be true or false, got {!r}'.format(value))
    if value:
        _check_rules(context.config.others, world, 'agreement')
        steps.check_agreement_passes(context.config.others.mc)
    return value


class AgreementCsvHook(loops.TestLoopHook):
    """``others.agreement``: ``<test_dir>/agreement.csv``, one row per subject -- subject, the metrics of ``evaluation.agreement_metrics`` on the sum
    of the subject's slice rows (``output['agreement']``, assembled like ``'confusion'``), then the sample volumes volume_1..volume_T."""

    def __init__(self, passes, file_name='agreement.csv'):
        self.passes, self.file_name = int(passes), file_name
        self.rows = []

    def on_test_start(self, task_context, context):
        self.rows.clear()

    def on_test_subject_end(self, subject_context, task_context, context):
        data = subject_context.subject_data
        rows = data.get('agreement')
        if rows is None:
            raise ValueError('others.agreement: subject {} came without its agreement rows'.format(subject_context.subject_index))
        t = self.passes
        total = np.asarray(rows, dtype=np.int64).reshape(-1, ev.agreement_row_length(t)).sum(axis=0)
        hist, pairs = total[:t + 1], ev.unpack_pairs(total[t + 1:], t)
        metrics = ev.agreement_metrics(hist, pairs)
        subject = data.get('subject', subject_context.subject_index)
        self.rows.append([subject] + [metrics[k] for k in ev.AGREEMENT_KEYS] + [int(pairs[i, i]) for i in range(t)])

    def on_test_end(self, task_context, context):
        with open(os.path.join(context.test_dir, self.file_name), 'w', newline='') as f:
            writer = csv.writer(f)
            writer.writerow(['subject'] + list(ev.AGREEMENT_KEYS) + ['volume_{}'.format(i + 1) for i in range(self.passes)])
            writer.writerows(self.rows)


def _adaptive(context, world):
    """``others.mc_adaptive: {check_at: [5, 10], tolerance: 0.01, max_unsettled: 0}`` (an rcu_amd extension, include/rcu.h "Adaptive MC") next to
    ``others.mc``: slices settled at a pass checkpoint are retired and finalised from the passes they have seen -> the checked schedule, or None
    without the key.  One process, MC dropout alone, exact statistics (``_RULES``): a ValueError that names the key otherwise."""
    if not hasattr(context.config.others, 'mc_adaptive'):
        return None
    others = context.config.others
    _check_rules(others, world, 'mc_adaptive')
    value = others.mc_adaptive
    if not isinstance(value, dict):
        value = dict(vars(value)) if hasattr(value, '__dict__') else value
    try:
        return steps.check_adaptive(value, others.mc)
    except ValueError as e:
        raise ValueError('others.mc_adaptive: {}'.format(e)) from None


def _adaptive_seed(context):
    if context.config.seed is None:
        raise ValueError('others.mc_adaptive needs the YAML file\'s seed: a slice moved into a smaller batch keeps its samples through its mask keys')
    return context.config.seed


class AdaptiveRowsStep(steps.BatchStep):
    """Behind the adaptive predict step: ``output['adaptive']``, one int64 row per slice (on the host) -- the slice's pass count, then for every
    checkpoint of the schedule its ``margin_q`` there, or -1 where the slice was no longer active.  Assembled like ``'confusion'`` rows."""

    def __init__(self, check_at):
        self.check_at = [int(t) for t in check_at]

    def __call__(self, batch_context, task_context, context) -> None:
        import torch
        passes = batch_context.output['mc_passes']
        rows = torch.full((passes.shape[0], 1 + len(self.check_at)), -1, dtype=torch.int64)
        rows[:, 0] = passes.view(-1).cpu()
        for record in batch_context.more.get('adaptive_checkpoints', ()):
            k = self.check_at.index(record['t'])
            for i, q in zip(record['active'], record['margin_q']):
                rows[i, 1 + k] = q
        batch_context.output['adaptive'] = rows


def adaptive_csv_row(rows, check_at, mc_steps):
    """The ``adaptive.csv`` columns of one subject from its slice rows (``AdaptiveRowsStep``) -> list: slices, slices retired at each checkpoint,
    passes run, passes a plain run would make, the smallest margin of a retired slice and of a slice that stayed active (each
    ``margin_q / (t * 2^40)`` at the checkpoint of the decision; empty without such a slice)."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 1 + len(check_at))
    passes = rows[:, 0]
    retired_margin, active_margin = [], []
    for k, t in enumerate(check_at):
        scale = float(t) * float(1 << 40)
        retired_margin += [q / scale for q in rows[passes == t, 1 + k]]
        active_margin += [q / scale for q in rows[(passes > t) & (rows[:, 1 + k] >= 0), 1 + k]]
    return ([int(rows.shape[0])] + [int((passes == t).sum()) for t in check_at] + [int(passes.sum()), int(rows.shape[0]) * int(mc_steps)] +
            [min(retired_margin) if retired_margin else '', min(active_margin) if active_margin else ''])


class AdaptiveCsvHook(loops.TestLoopHook):
    """``others.mc_adaptive``: ``<test_dir>/adaptive.csv``, one row per subject (``adaptive_csv_row``)."""

    def __init__(self, check_at, mc_steps, file_name='adaptive.csv'):
        self.check_at, self.mc_steps, self.file_name = [int(t) for t in check_at], int(mc_steps), file_name
        self.rows = []

    def on_test_start(self, task_context, context):
        self.rows.clear()

    def on_test_subject_end(self, subject_context, task_context, context):
        data = subject_context.subject_data
        rows = data.get('adaptive')
        if rows is None:
            raise ValueError('others.mc_adaptive: subject {} came without its adaptive rows'.format(subject_context.subject_index))
        self.rows.append([data.get('subject', subject_context.subject_index)] + adaptive_csv_row(rows, self.check_at, self.mc_steps))

    def on_test_end(self, task_context, context):
        with open(os.path.join(context.test_dir, self.file_name), 'w', newline='') as f:
            writer = csv.writer(f)
            writer.writerow(['subject', 'slices'] + ['retired_at_{}'.format(t) for t in self.check_at] +
                            ['passes_run', 'passes_plain', 'min_margin_retired', 'min_margin_active'])
            writer.writerows(self.rows)


def _logit_samples(context):
    """``others.logit_samples`` (an rcu_amd extension): S in 1..RCU_LOGIT_MAX_SAMPLES, or None when the key is absent."""
    if not hasattr(context.config.others, 'logit_samples'):
        return None
    value = context.config.others.logit_samples
    if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= _lib.RCU_LOGIT_MAX_SAMPLES:
        raise ValueError('others.logit_samples must be an integer in 1..{}, got {!r}'.format(_lib.RCU_LOGIT_MAX_SAMPLES, value))
    return value


def _aleatoric_steps(context, world):
    """The batch steps of the aleatoric script.  ``others.is_log_sigma`` (default false, as the shipped configs: sigma = |raw|; true: exp(raw),
    bin-dl/brats_test_aleatoric.py:34-37).  ``others.logit_samples: S`` (an rcu_amd extension, include/rcu.h "Test-time logit sampling"): the
    written probabilities are the sampled predictive (1/S) sum_s softmax(mu + sigma * z_s) of one eval-mode pass (AleatoricPredictStep) or,
    with ``others.mc: T``, of each of T seeded MC-dropout passes, averaged (AleatoricMcPredictStep + MultiPredictionSummary); the noise and the
    masks are keyed by the YAML file's ``seed``.  Without ``logit_samples`` ``others.mc`` is not read here, as before.  A multi-rank run is rank
    0's alone (one process runs the whole batch: nothing is sharded)."""
    others = context.config.others
    is_log_sigma = bool(getattr(others, 'is_log_sigma', False))
    samples = _logit_samples(context)
    if samples is None:
        return [steps.AleatoricPredictStep(is_log_sigma)]
    seed = context.config.seed
    mc = int(getattr(others, 'mc', 0) or 0)
    if mc > 0:
        return [steps.AleatoricMcPredictStep(mc, is_log_sigma, logit_samples=samples, seed=seed), steps.MultiPredictionSummary()]
    return [steps.AleatoricPredictStep(is_log_sigma, samples, seed)]


class ApplyTemperatureHook(loops.TestLoopHook):
    """``others.temperature`` (an rcu_amd extension): the model loaded by the test loop is scaled by T (UNet.set_temperature) before the first
    batch -- on every rank of a sharded run."""

    def __init__(self, temperature):
        self.temperature = temperature

    def end_startup(self, context):
        set_temperature = getattr(context.model, 'set_temperature', None)
        if set_temperature is None:
            raise ValueError('others.temperature: the model has no temperature scaling')
        set_temperature(self.temperature)


def _temperature_hooks(context):
    """``others.temperature``: a positive float or the path of a temperature.json (calibration.load_temperature), read before the run starts."""
    if not hasattr(context.config.others, 'temperature'):
        return []
    return [ApplyTemperatureHook(calibration.load_temperature(context.config.others.temperature))]


class CorruptionRecordHook(loops.TestLoopHook):
    """``others.corruption``: ``<test_dir>/corruption.json`` -- the parsed stages with their amounts, and the seed -- so that runs can be told
    apart at evaluation time (the written files keep their names).  Written by the rank that writes the run's output."""

    def __init__(self, record, file_name='corruption.json'):
        self.record, self.file_name = record, file_name

    def end_startup(self, context):
        if not getattr(context, 'writes_output', True):
            return
        with open(os.path.join(context.test_dir, self.file_name), 'w') as f:
            json.dump(self.record, f, indent=1, sort_keys=True)
            f.write('\n')


def _corruption(context):
    """``others.corruption`` (an rcu_amd extension, include/rcu.h "Input corruptions"; rcu_amd.corruption.parse): one stage or a list of at most
    8, applied in order to every batch in front of the script's predict steps -- on every rank: the corrupted slice is a function of the slice,
    the stages, the YAML file's ``seed`` (0 without one) and the slice's global index.  -> (steps, startup hooks), both empty without the key."""
    if not hasattr(context.config.others, 'corruption'):
        return [], []
    try:
        stages = corruption_mod.parse(context.config.others.corruption)
    except ValueError as e:
        raise ValueError('others.corruption: {}'.format(e)) from None
    seed = 0 if context.config.seed is None else int(context.config.seed)
    return [steps.CorruptInputStep(stages, seed)], [CorruptionRecordHook(corruption_mod.describe(stages, seed))]


def _density(context):
    """``others.density: <path to density.npz>`` (an rcu_amd extension, include/rcu.h "Feature-space density"; the fit_density scripts write the
    file): the deterministic default run with the energy of the fitted class Gaussians as one more map per subject -> the DensityFit, or None
    without the key.  One eval-mode pass per batch: a ValueError that names both keys beside the keys that sample (mc, tta, agreement, mc_adaptive,
    logit_samples: ``_RULES``).  Composes with others.corruption and others.temperature (which rescales conv_cls.1 alone: the features do not move)."""
    if not hasattr(context.config.others, 'density'):
        return None
    _check_rules(context.config.others, None, 'density')      # (its rules name keys alone: no world to ask)
    value = context.config.others.density
    if not isinstance(value, (str, os.PathLike)):
        raise ValueError('others.density must be the path of a density.npz (bin-dl/*_fit_density.py), got {!r}'.format(value))
    try:
        return density_mod.load_density(value)
    except ValueError as e:
        raise ValueError('others.density: {}'.format(e)) from None


class DensityWriteHook(loops.TestLoopHook):
    """``others.density``: ``{subject}_density.nii.gz``, the float32 energy of the subject's voxels (``output['density']``, assembled like the
    probabilities), written beside the files of the run -- whose names and bytes it leaves alone."""
    KEY = 'density'        # the others.* key that asked for the map
    ENTRY = 'density'      # the assembled entry and the file's suffix

    def __init__(self, in_background=True):
        self.in_background = in_background

    def on_test_subject_end(self, subject_context, task_context, context):
        data = subject_context.subject_data
        energy = data.get(self.ENTRY)
        if energy is None:
            raise ValueError('others.{}: subject {} came without its {} map'.format(self.KEY, subject_context.subject_index, self.ENTRY))
        subject = data.get('subject', subject_context.subject_index)
        energy = np.asarray(energy)
        energy = np.ascontiguousarray(energy[..., 0] if energy.shape[-1] == 1 else energy, dtype=np.float32)
        properties, path = data.get('properties'), os.path.join(context.test_dir, '{}_{}.nii.gz'.format(subject, self.ENTRY))
        nifti.do_work(lambda: nifti.write(path, energy, properties), in_background=self.in_background)

    def on_termination(self, context):
        nifti.join_all()


class LaplaceStdWriteHook(DensityWriteHook):
    """``others.laplace``: ``{subject}_laplace_std.nii.gz``, the float32 std of the predicted class's logit (``output['laplace_std']``), written
    beside the files of the run; the probabilities and prediction files hold the Laplace predictive."""
    KEY = 'laplace'
    ENTRY = 'laplace_std'


class LaplaceRecordHook(CorruptionRecordHook):
    """``others.laplace``: ``<test_dir>/laplace.json`` -- the fit's scalars, its file, the link, the samples and the seed -- written by the rank
    that writes the run's output, as the corruption record is."""

    def __init__(self, record):
        super().__init__(record, 'laplace.json')


def _laplace(context):
    """``others.laplace: <path to laplace.npz>`` (an rcu_amd extension, include/rcu.h "Last-layer Laplace"; the fit_laplace scripts write the
    file) with ``others.laplace_link`` (probit, the default, or sample) and ``others.laplace_samples`` (the draws of the sample link): the
    deterministic default run with the Laplace predictive as its probabilities -> (the predict step, the record of ``laplace.json``), or None
    without the key.  One eval-mode pass per batch: a ValueError that names both keys beside the keys that sample and beside others.density
    (``_RULES``).  Composes with others.corruption, others.device_metrics and others.temperature -- the fit must have been made at that
    temperature, which the step checks against the model."""
    others = context.config.others
    if not hasattr(others, 'laplace'):
        return None
    _check_rules(others, None, 'laplace')      # (its rules name keys alone: no world to ask)
    value = others.laplace
    if not isinstance(value, (str, os.PathLike)):
        raise ValueError('others.laplace must be the path of a laplace.npz (bin-dl/*_fit_laplace.py), got {!r}'.format(value))
    try:
        fit = laplace_mod.load_laplace(value)
        link = _other(context, 'laplace_link', 'probit')
        seed = 0 if context.config.seed is None else int(context.config.seed)
        step = steps.LaplacePredictStep(fit, link=link, samples=_other(context, 'laplace_samples', 0), seed=seed)
    except ValueError as e:
        raise ValueError('others.laplace: {}'.format(e)) from None
    return step, dict(fit.as_dict(), file=os.fspath(value), link=link, samples=step.samples, seed=seed)


class KnnWriteHook(DensityWriteHook):
    """``others.knn``: ``{subject}_knn.nii.gz``, the float32 distance of the subject's voxels to their k-th nearest bank row (``output['knn']``),
    written beside the files of the run -- whose names and bytes it leaves alone."""
    KEY = 'knn'
    ENTRY = 'knn'


class KnnRecordHook(CorruptionRecordHook):
    """``others.knn``: ``<test_dir>/knn.json`` -- the bank's scalars, its file and k -- written by the rank that writes the run's output, as the
    corruption record is."""

    def __init__(self, record):
        super().__init__(record, 'knn.json')


def _knn(context):
    """``others.knn: <path to knn.npz>`` (an rcu_amd extension, include/rcu_knn.h; the fit_knn scripts write the file) with ``others.knn_k``
    (1..8, 5 by default): the deterministic default run with the distance to the k-th nearest bank row as one more map per subject -> (the
    predict step, the record of ``knn.json``), or None without the key.  One eval-mode pass per batch: a ValueError that names both keys beside
    the keys that sample and beside others.density and others.laplace (``_RULES``).  Composes with others.corruption, others.device_metrics and
    others.temperature (which rescales conv_cls.1 alone: the features do not move)."""
    others = context.config.others
    if not hasattr(others, 'knn'):
        return None
    _check_rules(others, None, 'knn')      # (its rules name keys alone: no world to ask)
    value = others.knn
    if not isinstance(value, (str, os.PathLike)):
        raise ValueError('others.knn must be the path of a knn.npz (bin-dl/*_fit_knn.py), got {!r}'.format(value))
    try:
        bank = knn_mod.load_knn(value)
    except ValueError as e:
        raise ValueError('others.knn: {}'.format(e)) from None
    try:
        step = steps.KnnPredictStep(bank, _other(context, 'knn_k', 5))
    except ValueError as e:
        raise ValueError('others.knn_k: {}'.format(e)) from None
    return step, dict(bank.as_dict(), file=os.fspath(value), k=step.k)


TTA_AFFINE_OPTIONS = ('samples', 'rotation', 'scale', 'shift', 'flip')


class TtaAffineRecordHook(CorruptionRecordHook):
    """``others.tta_affine``: ``<test_dir>/tta_affine.json`` -- the seed, the options and the V forward matrices -- written by the rank that writes
    the run's output, as the corruption record is."""

    def __init__(self, record):
        super().__init__(record, 'tta_affine.json')


def _tta_affine(context, world):
    """``others.tta_affine: {samples: V, rotation: deg, scale: s, shift: px, flip: bool}`` (an rcu_amd extension, include/rcu_warp.h): test-time
    augmentation over V seeded affine transforms, the first the identity (steps.affine_tta_draw under the YAML file's ``seed``, 0 without one),
    composed with ``others.mc`` when that is set (V x T passes, with the weight-scaling pass), else alone in eval mode -- in place of the predict
    step, followed by MultiPredictionSummary -> (batch steps, the record of ``tta_affine.json``), or None without the key.  One process; not
    beside tta, agreement, mc_adaptive, density, laplace or knn (``_RULES``): a ValueError that names the key otherwise."""
    others = context.config.others
    if not hasattr(others, 'tta_affine'):
        return None
    _check_rules(others, world, 'tta_affine')
    value = others.tta_affine
    if not isinstance(value, dict):
        value = dict(vars(value)) if hasattr(value, '__dict__') else value
    if not isinstance(value, dict) or 'samples' not in value or set(value) - set(TTA_AFFINE_OPTIONS):
        raise ValueError('others.tta_affine must be a mapping with samples and any of rotation, scale, shift, flip, got {!r}'.format(value))
    flip = value.get('flip', False)
    if not isinstance(flip, bool):
        raise ValueError('others.tta_affine: flip must be true or false, got {!r}'.format(flip))
    mc = int(getattr(others, 'mc', 0) or 0)
    seed = 0 if context.config.seed is None else int(context.config.seed)
    try:
        step = steps.AffineTtaMcPredictStep(value['samples'], mc_steps=mc, seed=seed, rotation=value.get('rotation', 0.0),
                                            scale=value.get('scale', 0.0), shift=value.get('shift', 0.0), flip=flip,
                                            group_pixels=_other(context, 'group_pixels'), exact=bool(_other(context, 'exact', True)), ws_pass=mc > 0)
    except (TypeError, ValueError) as e:
        raise ValueError('others.tta_affine: {}'.format(e)) from None
    record = dict(step.options, samples=step.transforms, seed=seed, mc=mc, matrices=step.matrices.tolist())
    return [step, steps.MultiPredictionSummary()], record


def _default_plan(context, world, density_fit=None, laplace_step=None, knn_step=None, affine_steps=None):
    """The one decision of the default script: affine tta, density, k-NN, laplace, tta, adaptive, agreement, sharded mc, mc or plain -> (batch
    steps, the entries they add to the assembled subject, the per-subject hooks that write them)."""
    if affine_steps is not None:     # (the written maps keep their names)
        return affine_steps, (), []
    if density_fit is not None:      # one deterministic pass per batch: under a multi-process launch the run is rank 0's alone (_run)
        return [steps.DensityPredictStep(density_fit)], ('density',), [DensityWriteHook()]
    if knn_step is not None:         # (the same)
        return [knn_step], ('knn',), [KnnWriteHook()]
    if laplace_step is not None:     # (the same)
        return [laplace_step], ('laplace_std',), [LaplaceStdWriteHook()]
    others = context.config.others
    adaptive = _adaptive(context, world)
    agreement = adaptive is None and _agreement(context, world)      # (beside a schedule the key is off: _RULES)
    if hasattr(others, 'tta'):
        return _tta_steps(context, world), (), []
    if not hasattr(others, 'mc'):
        return [steps.SegmentationPredictStep(do_probs=True)], (), []
    # ``others.group_pixels`` / ``others.exact`` (rcu_amd extensions): the memory / reproducibility trade of the MC step.  Every stream lane of every
    # rank sizes its plan for n x min(group_pixels // (n H W), T) samples (canonical plans: 24 GB per lane for four passes of a 160-slice BraTS
    # batch) and ``exact`` keeps the statistics as exact float64 sums; a smaller ``group_pixels`` (or ``stream_lanes: 1``) shrinks the workspace,
    # ``exact: false`` halves the statistics and the reduce at the price of byte-identity across lanes, groups and world sizes.
    mc, options = others.mc, dict(lanes=_other(context, 'stream_lanes'), group_pixels=_other(context, 'group_pixels'))
    if adaptive is not None:      # (the written map files keep their names: the slice rows only feed adaptive.csv)
        return ([steps.McPredictStep(mc, seed=_adaptive_seed(context), adaptive=adaptive, **options), steps.MultiPredictionSummary(),
                 AdaptiveRowsStep(adaptive['check_at'])], ('adaptive',), [AdaptiveCsvHook(adaptive['check_at'], mc)])
    options.update(seed=_mask_seed(context, world), exact=bool(_other(context, 'exact', True)))
    if agreement:
        return ([steps.McPredictStep(mc, agreement=True, **options), steps.MultiPredictionSummary(), steps.SampleAgreementStep()], ('agreement',),
                [AgreementCsvHook(mc)])
    if world.world > 1:     # the T + 1 passes of every batch sharded over the ranks, one sum-reduce per batch (rcu_amd.distributed)
        return [rdist.ShardedMcPredictStep(mc, world, **options), steps.MultiPredictionSummary()], (), []
    return [steps.McPredictStep(mc, **options), steps.MultiPredictionSummary()], (), []


def _default_steps(context, world):
    return _default_plan(context, world)[0]


def _hooks(write_hook, extra=()):
    hooks = [loops.ConsoleTestLogHook(), loops.WriteTestMetricsCsvHook('metrics.csv'), write_hook] + list(extra)
    return loops.ReducedComposeTestLoopHook(hooks)


def _other_model_dir(context):
    others = context.config.others
    if not hasattr(others, 'model_dir') or not hasattr(others, 'test_at'):
        raise ValueError('missing "model_dir" or "test_at" entry in the configuration (others)')
    return others.model_dir


def _load_model_at(context, model_dir, provide_features=False):
    """The trained model of ``model_dir`` at ``others.test_at``, on the context's device, in eval mode."""
    mf = mgt.ModelFiles.from_model_dir(model_dir)
    model = mgt.load_model_from_parameters(mf.model_path())
    if provide_features:
        model.provide_features = True
    mgt.load_checkpoint(mgt.find_checkpoint_file(mf.weight_checkpoint_dir, context.config.others.test_at), model)
    return model.to(context.device).eval()


def _load_additional_models(context):
    """others.model_dir (list) + others.test_at -> extra ensemble members (brats_test_ensemble.py:37-57)."""
    model_dirs = _other_model_dir(context)
    model_dirs = [model_dirs] if isinstance(model_dirs, str) else list(model_dirs)
    models = []
    for i, model_dir in enumerate(model_dirs):
        logging.info('load additional model [{}/{}] {}'.format(i + 1, len(model_dirs), os.path.basename(model_dir)))
        models.append(_load_model_at(context, model_dir))
    return models


def _load_segmentation_model(context):
    """others.model_dir + others.test_at -> the trained segmentation U-Net with provide_features set
    (brats_test_auxiliary_feat.py:35-46)."""
    return _load_model_at(context, _other_model_dir(context), provide_features=True)


def _loop_options(context):
    """Test-loop options from the YAML file's ``others`` (rcu_amd extensions): ``coalesce_pixels`` -- merge loader batches up to that many
    pixels per step (loops.Test; DEFAULT since round 6: ``loops.Test.COALESCE_PIXELS``, one benchmark-sized BraTS volume -- the shipped
    ``batch_size: 32`` then runs as launches that fill the GPU, and, the seeded Dropout2d masks being keyed by the slice and not by the batch,
    the same YAML file writes the same files for any ``batch_size``; ``0`` switches it off: steps and hooks then see the loader's batches, as in
    the reference; two BraTS volumes, 7864320, keep the launches of an 8-GPU run at 640 samples) --, ``pipelined: false`` (the reference's
    callback order), ``max_inflight``, ``loader_timing: true`` (the loader thread logs where its time went)."""
    value = _other(context, 'coalesce_pixels')
    return dict(coalesce=loops.Test.COALESCE_PIXELS if value is None else int(value), pipelined=_other(context, 'pipelined'),
                max_inflight=_other(context, 'max_inflight'), loader_timing=bool(_other(context, 'loader_timing', False)))


def _context(device, config_file):
    """-> (context, world): under ``python -m torch.distributed.run`` every rank gets its own GPU (rcu_amd.distributed.world_from_env) and
    only rank 0 creates the test directory, logs, assembles, evaluates and writes."""
    world = rdist.world_from_env(device)
    context = loops.TorchTestContext(world.device)
    context.writes_output = world.is_root
    context.load_from_config(config_file)
    return context, world


def _nothing_to_shard(world):
    """A run of one deterministic forward pass per batch has nothing to shard over samples: under a multi-process launch it is rank 0's alone
    -> whether this rank leaves at once."""
    if world.world > 1 and not world.is_root:
        logging.info('rank {}: this configuration has one forward pass per batch, nothing to shard; rank 0 runs it'.format(world.rank))
        return True
    return False


def _run(context, dataset, test_steps, write_hook, entries, world=None, startup_hooks=(), subject_hooks=()):
    """``startup_hooks`` run on every rank; ``subject_hooks`` (per-subject writers such as AgreementCsvHook) on the root alone, behind the write hook."""
    world = world if world is not None else rdist.World()
    sharded = [s_ for s_ in test_steps if isinstance(s_, rdist._ShardedStepBase)]
    if not sharded and _nothing_to_shard(world):
        return context
    build = data_mod.BuildData(build_dataset=data_mod.BuildVolumeDataset() if dataset == 'brats' else data_mod.BuildIsicDataset())
    options = _loop_options(context)
    extra_hooks = list(startup_hooks) + list(subject_hooks)
    spec = _other(context, 'device_metrics')
    if spec and world.is_root:      # opt-in: the evaluation's metrics on the maps while they are in HBM (DeviceMetricsHook)
        store = {}
        test_steps = test_steps + [CollectOnDeviceStep(store)]
        extra_hooks.append(DeviceMetricsHook(dataset, spec, store))
    if world.is_root and bool(_other(context, 'device_confusion', True)):
        # the subjects' Dice counts ride with the batches (ConfusionOnDeviceStep; ``others.device_confusion: false`` keeps them at subject level)
        test_steps = test_steps + [ConfusionOnDeviceStep()]
        entries = None if entries is None else tuple(entries) + ('confusion',)
    if dataset != 'brats':
        test_steps = test_steps + [PrepareSubjectStep()]
    if not world.is_root:
        # a rank other than the root of a sharded run: the same loader and the same batch steps, nothing assembled, evaluated or written
        # (the same coalescing: every rank must see the root's batches -- their shapes size the collective, their indices rotate the jobs)
        test = loops.Test(test_steps, [], None, entries=(), coalesce=options['coalesce'], pipelined=options['pipelined'],
                          max_inflight=options['max_inflight'])
        hook = loops.ReducedComposeTestLoopHook(list(startup_hooks)) if startup_hooks else loops.TestLoopHook()
    elif dataset == 'brats':
        test = loops.Test(test_steps, [loops.ExtractSubjectInfoStep(), EvalSubjectStep()], loops.SubjectAssembler(),
                          entries=entries, **options)
        hook = _hooks(write_hook, extra_hooks)
    else:
        test = loops.Test(test_steps, [EvalSubjectStep(squeeze_labels=True, keep_prediction=True)],
                          loops.Subject2dAssembler(), entries=entries, **options)
        hook = _hooks(write_hook, extra_hooks)
    try:
        test(context, build, hook=hook)
    except BaseException:
        if world.world > 1 and sharded:
            # A rank that failed must NOT issue the closing collectives: the other ranks are still in their per-batch reduces, a barrier from
            # here would pair with one of those (mismatched collectives: RCCL hangs until its watchdog fires) and the traceback below would
            # never be printed.  Log it, tear this rank's communicator down so that the peers' pending collectives fail instead of waiting, and
            # let the exception end the process: a non-zero exit makes the launcher (torch.distributed.run) end the other ranks.
            logging.exception('rank {} of {}: the test loop failed; leaving without the closing barrier'.format(world.rank, world.world))
            _abandon_process_group()
        raise
    else:
        if world.world > 1 and sharded:      # (a run that is rank 0's alone has nobody to meet: the other ranks have left)
            import torch
            import torch.distributed as dist
            for s_ in sharded:
                s_.finish()
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            dist.barrier()           # no rank leaves (and frees what a collective still reads) before the root has the last batch
    return context


def _abandon_process_group(timeout_s=10.0):
    """Best effort, bounded in time: destroy this rank's process group from a helper thread (a communicator with collectives in flight may not
    come down at once; the exception that brought us here must not wait for it)."""
    import threading
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return

    def destroy():
        try:
            dist.destroy_process_group()
        except Exception:  # noqa: BLE001 - we are already failing; the original exception is the one to report
            pass

    t = threading.Thread(target=destroy, name='rcu-abandon-process-group', daemon=True)
    t.start()
    t.join(timeout_s)


def test_default(dataset, config_file=None, config_id=None, device='cuda'):
    context, world = _context(device, config_file or _config_path(dataset, config_id))
    _check_others(context, 'default', world)
    affine = _tta_affine(context, world)      # (refuses others.tta_affine beside the keys of its _RULES rows and under a multi-rank launch)
    density_fit = _density(context)      # (refuses others.density beside the keys that sample)
    knn = _knn(context)                  # (refuses others.knn beside them, beside others.density and beside others.laplace)
    laplace = _laplace(context)          # (refuses others.laplace beside them and beside others.density)
    corrupt_steps, corrupt_hooks = _corruption(context)
    test_steps, more_entries, subject_hooks = _default_plan(context, world, density_fit, None if laplace is None else laplace[0],
                                                            None if knn is None else knn[0], None if affine is None else affine[0])
    record_hooks = (([] if laplace is None else [LaplaceRecordHook(laplace[1])]) + ([] if knn is None else [KnnRecordHook(knn[1])]) +
                    ([] if affine is None else [TtaAffineRecordHook(affine[1])]))
    return _run(context, dataset, corrupt_steps + test_steps, WriteHook(link_inputs=dataset == 'isic'),
                ('probabilities',) + more_entries if dataset == 'brats' else None, world,
                startup_hooks=_temperature_hooks(context) + corrupt_hooks + record_hooks, subject_hooks=subject_hooks)


def test_ensemble(dataset, config_file=None, device='cuda'):
    context, world = _context(device, config_file or os.path.join(CONFIG_DIR, 'test_{}_ensemble.yaml'.format(dataset)))
    _check_others(context, 'ensemble', world)
    corrupt_steps, corrupt_hooks = _corruption(context)
    members = _load_additional_models(context)
    lanes = _other(context, 'stream_lanes')
    if world.world > 1:     # the K members of every batch sharded over the ranks (bin-dl/brats_test_ensemble.py:44-59 on N GPUs)
        test_steps = [rdist.ShardedEnsemblePredictionStep(members, world, lanes=lanes), steps.MultiPredictionSummary()]
    else:
        test_steps = [steps.EnsemblePredictionStep(members, lanes=lanes), steps.MultiPredictionSummary()]
    return _run(context, dataset, corrupt_steps + test_steps, WriteHook(link_inputs=dataset == 'isic'), None, world, startup_hooks=corrupt_hooks)


def test_aleatoric(dataset, config_file=None, device='cuda'):
    context, world = _context(device, config_file or os.path.join(CONFIG_DIR, 'test_{}_aleatoric.yaml'.format(dataset)))
    _check_others(context, 'aleatoric', world)
    corrupt_steps, corrupt_hooks = _corruption(context)
    return _run(context, dataset, corrupt_steps + _aleatoric_steps(context, world), WriteHook(with_sigma=True, link_inputs=dataset == 'isic'),
                None, world, startup_hooks=corrupt_hooks)


# ------------------------------------------------------------------------------- auxiliary networks
class AuxiliaryFeatPredictStep(steps.BatchStep):
    """bin-dl/brats_test_auxiliary_feat.py:64-82: segmentation network with provide_features, then the auxiliary
    PostNet (``context.model``) on its features; the features stay in the U-Net's workspace (no copy)."""

    def __init__(self, test_model):
        self.test_model = test_model

    def __call__(self, batch_context, task_context, context) -> None:
        if not isinstance(context, steps.Context):
            raise ValueError('expected type is "TorchTestContext" but object is of type "{}"'.format(type(context).__name__))
        batch_context.input['images'] = batch_context.input['images'].float().to(context.device)
        segm_logits = self.test_model(batch_context.input['images'])
        batch_context.output['segm_probabilities'] = steps.softmax(segm_logits)
        logits = context.model(self.test_model.features)
        batch_context.output['probabilities'] = steps.softmax(logits)


class AuxiliarySegmPredictStep(steps.BatchStep):
    """bin-dl/brats_test_auxiliary_segm.py:50-71: the auxiliary U-Net sees the images plus the segmentation to be
    judged (labels channel 1) and predicts where that segmentation is wrong."""

    def __init__(self, keep_labels=False):
        self.keep_labels = keep_labels       # isic_test_auxiliary_segm.py:80-81

    def __call__(self, batch_context, task_context, context) -> None:
        if not isinstance(context, steps.Context):
            raise ValueError('expected type is "TorchTestContext" but object is of type "{}"'.format(type(context).__name__))
        import torch
        batch_context.input['images'] = batch_context.input['images'].float().to(context.device)
        batch_context.input['labels'] = batch_context.input['labels'].long().to(context.device)
        pred = batch_context.input['labels'][:, 1]
        inpt = torch.cat([batch_context.input['images'], pred.unsqueeze(1).float()], dim=1)
        logits = context.model(inpt)
        batch_context.output['logits'] = logits
        batch_context.output['probabilities'] = steps.softmax(logits)
        batch_context.output['orig_prediction'] = pred.unsqueeze(1)
        if self.keep_labels:
            batch_context.output['labels'] = batch_context.input['labels']


class EvalAuxiliaryFeatStep(loops.SubjectStep):
    """Dice of the SEGMENTATION network's arg-max (brats_test_auxiliary_feat.py:85-99)."""

    def __init__(self, squeeze_labels=False):
        self.evaluate = ev.ComposeEvaluation([ev.DiceNumpy()])
        self.squeeze_labels = squeeze_labels

    def __call__(self, subject_context, task_context, context) -> None:
        probabilities = subject_context.subject_data['segm_probabilities']
        target = subject_context.subject_data['labels']
        if self.squeeze_labels:
            target = target.squeeze(-1)
        results = {}
        self.evaluate({'prediction': np.argmax(probabilities, axis=-1), 'probabilities': probabilities, 'target': target},
                      results)
        subject_context.metrics.update(results)


class EvalAuxiliarySegmStep(loops.SubjectStep):
    """Dice of "predicted wrong" against "is wrong" (brats_test_auxiliary_segm.py:74-91)."""

    def __init__(self, set_score=False):
        self.evaluate = ev.ComposeEvaluation([ev.DiceNumpy()])
        self.set_score = set_score

    def __call__(self, subject_context, task_context, context) -> None:
        probabilities = subject_context.subject_data['probabilities']
        labels = subject_context.subject_data['labels']
        results = {}
        self.evaluate({'prediction': np.argmax(probabilities, axis=-1), 'probabilities': probabilities,
                       'target': labels[..., 1] != labels[..., 0]}, results)
        subject_context.metrics.update(results)
        if self.set_score:
            subject_context.score = results['dice']


class WriteConfidenceHook(loops.TestLoopHook):
    """``{subject}_confidence.nii.gz`` (foreground output of the auxiliary network) + ``{subject}_prediction.nii.gz``
    (brats_test_auxiliary_feat.py:102-135, brats_test_auxiliary_segm.py:94-124; ISIC variants symlink the inputs)."""

    def __init__(self, prediction_entry, link=(), in_background=True):
        self.prediction_entry, self.link, self.in_background = prediction_entry, tuple(link), in_background

    def on_test_subject_end(self, subject_context, task_context, context):
        if not isinstance(context, loops.TorchTestContext):
            raise ValueError('expected type is "TorchTestContext" but object is of type "{}"'.format(type(context).__name__))
        data = subject_context.subject_data
        subject = data.get('subject', subject_context.subject_index)
        confidence = np.ascontiguousarray(data['probabilities'][..., 1], dtype=np.float32)
        if self.prediction_entry == 'segm_probabilities':
            prediction = np.argmax(data['segm_probabilities'], axis=-1).astype(np.uint8)
        else:
            prediction = np.squeeze(data['orig_prediction']).astype(np.uint8)
        props, test_dir = data.get('properties'), context.test_dir

        def work():
            nifti.write(os.path.join(test_dir, '{}_confidence.nii.gz'.format(subject)), confidence, props)
            nifti.write(os.path.join(test_dir, '{}_prediction.nii.gz'.format(subject)), prediction, props)

        nifti.do_work(work, in_background=self.in_background)
        if self.link:
            files = context.test_data.dataset.get_files_by_id(subject_context.subject_index)
            for key in self.link:
                src = os.path.abspath(files[key])
                dst = os.path.join(context.test_dir, os.path.basename(src))
                if not os.path.lexists(dst):
                    os.symlink(src, dst)

    def on_termination(self, context):
        nifti.join_all()


def _auxiliary(script, dataset, config_file, device, loop_of):
    """What the two auxiliary scripts share.  ``loop_of(context)`` -> (batch steps, subject steps, assembler, entries, write hook, further
    BuildData arguments) of the dataset: one deterministic forward pass per batch, so under a multi-process launch the run is rank 0's alone."""
    context, world = _context(device, config_file or os.path.join(CONFIG_DIR, 'test_{}_{}.yaml'.format(dataset, script)))
    _check_others(context, script, world)
    corrupt_steps, corrupt_hooks = _corruption(context)
    if _nothing_to_shard(world):
        return context
    batch_steps, subject_steps, assembler, entries, hook, build_options = loop_of(context)
    build = data_mod.BuildData(build_dataset=data_mod.BuildVolumeDataset() if dataset == 'brats' else data_mod.BuildIsicDataset(), **build_options)
    test = loops.Test(corrupt_steps + batch_steps, subject_steps, assembler, entries=entries)
    test(context, build, hook=_hooks(hook, corrupt_hooks))
    return context


def test_auxiliary_feat(dataset, config_file=None, device='cuda'):
    def loop_of(context):
        predict = AuxiliaryFeatPredictStep(_load_segmentation_model(context))
        if dataset == 'brats':
            return ([predict], [loops.ExtractSubjectInfoStep(), EvalAuxiliaryFeatStep()], loops.SubjectAssembler(),
                    ('probabilities', 'segm_probabilities'), WriteConfidenceHook('segm_probabilities'), {})
        return ([predict, PrepareSubjectStep()], [EvalAuxiliaryFeatStep(squeeze_labels=True)], loops.Subject2dAssembler(),
                ('probabilities', 'segm_probabilities', 'labels'), WriteConfidenceHook('segm_probabilities', link=('label_paths',)), {})

    return _auxiliary('auxiliary_feat', dataset, config_file, device, loop_of)


def test_auxiliary_segm(dataset, config_file=None, device='cuda'):
    def loop_of(context):
        if dataset == 'brats':
            return ([AuxiliarySegmPredictStep()], [loops.ExtractSubjectInfoStep(), EvalAuxiliarySegmStep()], loops.SubjectAssembler(),
                    ('probabilities', 'orig_prediction'), WriteConfidenceHook('orig_prediction'), {})
        if not hasattr(context.config.others, 'prediction_dir'):
            raise ValueError('"others.prediction_dir" is required in the config')
        return ([AuxiliarySegmPredictStep(keep_labels=True)], [EvalAuxiliarySegmStep(set_score=True)], loops.Subject2dAssembler(),
                ('probabilities', 'labels', 'orig_prediction'), WriteConfidenceHook('orig_prediction', link=('label_paths', 'image_paths')),
                dict(prediction_dir=context.config.others.prediction_dir))

    return _auxiliary('auxiliary_segm', dataset, config_file, device, loop_of)


# ------------------------------------------------------------------------------- temperature scaling (EXTENSION)
def _validation_batches(context, dataset, device):
    """(images, target) per loader batch of ``test_data`` -- the validation volumes, read as the test scripts read theirs -- with the target the
    evaluation binarises to (labels > 0, rechun/eval/analysis.py: target > 0), on the device."""
    loader = context.test_data.loader
    volumes = {}
    for batch in loader:
        images = batch['images'].float().to(device)
        images = images.contiguous()
        n, _, h, w = images.shape
        if dataset == 'brats':
            source = context.test_data.dataset
            pieces = []
            for si, k in zip(batch['subject_index'], batch['slice_index']):
                si, k = int(si), int(k)
                if si not in volumes:
                    volumes.clear()
                    labels = np.asarray(source.direct_extract(si, ('labels',))['labels'])
                    volumes[si] = torch.from_numpy(np.ascontiguousarray(labels.reshape(labels.shape[:3]) > 0).astype(np.uint8)).to(device)
                pieces.append(volumes[si][k])
            target = torch.stack(pieces)
        else:
            labels = batch['labels']
            labels = labels if torch.is_tensor(labels) else torch.as_tensor(np.asarray(labels))
            target = (labels.to(device).reshape(n, h, w) > 0).to(torch.uint8)
        yield images, target


def _fit_context(script, dataset, config_file, device, check_model):
    """What the fit scripts share up to the fit itself -> (context, seed) with the model loaded and checked (``check_model(model)`` raises), the run
    directory and its log set up, the generators seeded with the YAML ``seed`` (0 without one) and ``test_data`` built: one process, one loader."""
    if dataset not in ('brats', 'isic'):
        raise ValueError('chose "brats" or "isic" as dataset')
    context, world = _context(device, config_file)
    if world.world > 1:
        raise ValueError('the {} fit runs in one process; launch it without torch.distributed.run'.format(script[len('fit_'):]))
    _check_others(context, script, world)
    seed = 0 if context.config.seed is None else int(context.config.seed)
    context.load_from_checkpoint(context.get_test_at())
    check_model(context.model)
    context.setup_directory()
    context.setup_logging()
    context.do_seed(seed)
    context.load_test_data(data_mod.BuildData(build_dataset=data_mod.BuildVolumeDataset() if dataset == 'brats' else data_mod.BuildIsicDataset()))
    return context, seed


def _check_temperature_model(model):
    if not hasattr(model, 'set_temperature'):
        raise ValueError('the temperature fit needs a U-Net segmentation model')
    if model.sigma_out:
        raise ValueError('the temperature fit is not defined for a sigma_out model (its sigma is in logit units)')
    if model.nb_classes != 2:
        raise ValueError('the temperature fit scripts take binary models (nb_classes = 2), got {}'.format(model.nb_classes))


def fit_temperature(dataset, config_file, device='cuda'):
    """bin-dl/{brats,isic}_fit_temperature.py (EXTENSION): fit the temperature of a test configuration's model on the volumes its ``test_data``
    names -- the VALIDATION volumes -- by the NLL of the pass-averaged prediction (``others.mc`` passes with the YAML ``seed``, 0 without one,
    else one eval-mode pass), on all voxels, target labels > 0.  Writes ``temperature.json`` into the run directory and returns the fit;
    ``others.temperature: <that file>`` applies it in the default test scripts."""
    context, seed = _fit_context('fit_temperature', dataset, config_file, device, _check_temperature_model)
    mc = int(_other(context, 'mc', 0) or 0)
    fit = calibration.fit_temperature(context.model, _validation_batches(context, dataset, context.device), mc_steps=mc, seed=seed,
                                      group_pixels=_other(context, 'group_pixels'))
    record = dict(fit.as_dict(), model_dir=context.config.model_dir, test_at=context.config.test_at,
                  dataset=context.config.test_data.dataset, mc=mc)
    path = os.path.join(context.test_dir, 'temperature.json')
    with open(path, 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write('\n')
    logging.info('temperature %.6f (mean NLL %.6f at T = 1, %.6f at the best candidate, %d voxels, %d passes) -> %s', fit.temperature,
                 fit.mean_nll_at_1, fit.mean_nll_at_best_candidate, fit.voxels, fit.passes, path)
    print('temperature: {!r}'.format(fit.temperature))
    return fit


def fit_density(dataset, config_file, device='cuda'):
    """bin-dl/{brats,isic}_fit_density.py (EXTENSION): fit the class Gaussians of the feature-space density (rcu_amd.density) on the volumes a test
    configuration's ``test_data`` names -- the VALIDATION volumes, read as ``fit_temperature`` reads them -- with one eval-mode pass per batch,
    target labels > 0 (K = 2).  ``others.density_ridge`` (1e-6) and ``others.density_shared_covariance`` (false) are the fit's options.  Writes
    ``density.npz`` and a readable ``density.json`` into the run directory and returns the fit; ``others.density: <that .npz>`` applies it in the
    default test scripts."""
    context, _ = _fit_context('fit_density', dataset, config_file, device, density_mod._feature_channels)      # (refuses a model that is no U-Net)
    fit = density_mod.fit_density(context.model, _validation_batches(context, dataset, context.device),
                                  ridge=float(_other(context, 'density_ridge', 1e-6)),
                                  shared_covariance=bool(_other(context, 'density_shared_covariance', False)), nb_classes=2)
    path = os.path.join(context.test_dir, 'density.npz')
    density_mod.save_density(fit, path)
    record = dict(fit.as_dict(), model_dir=context.config.model_dir, test_at=context.config.test_at, dataset=context.config.test_data.dataset)
    with open(os.path.join(context.test_dir, 'density.json'), 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write('\n')
    logging.info('density fit: F = %d, K = %d, counts %s, %d voxels -> %s', fit.F, fit.K, [int(v) for v in fit.n], fit.voxels, path)
    print('density: {}'.format(path))
    return fit


_KNN_BANK_OPTIONS = {'per_class': 1024, 'normalize': True}


def _knn_bank_options(context):
    """``others.knn_bank: {per_class: 1024, normalize: true}`` -> the two options; anything else in it is refused by name."""
    value = _other(context, 'knn_bank', None)
    given = {} if value is None else (dict(value) if isinstance(value, dict) else dict(vars(value)))
    unknown = sorted(set(given) - set(_KNN_BANK_OPTIONS))
    if unknown:
        raise ValueError('others.knn_bank takes {}; got {}'.format(', '.join(sorted(_KNN_BANK_OPTIONS)), ', '.join(unknown)))
    options = dict(_KNN_BANK_OPTIONS, **given)
    per_class, normalize = options['per_class'], options['normalize']
    if isinstance(per_class, bool) or not isinstance(per_class, int) or not 1 <= 2 * per_class <= knn_mod.MAX_BANK:
        raise ValueError('others.knn_bank.per_class must be an integer in 1..{}, got {!r}'.format(knn_mod.MAX_BANK // 2, per_class))
    if not isinstance(normalize, bool):
        raise ValueError('others.knn_bank.normalize must be true or false, got {!r}'.format(normalize))
    return per_class, normalize


def fit_knn(dataset, config_file, device='cuda'):
    """bin-dl/{brats,isic}_fit_knn.py (EXTENSION): sample the bank of the nearest-neighbour feature uncertainty (rcu_amd.knn) on the volumes a test
    configuration's ``test_data`` names -- the VALIDATION volumes, read as ``fit_temperature`` reads them, the slices counted in loader order --
    with one eval-mode pass per batch, target labels > 0 (K = 2), under the YAML ``seed`` (0 without one).  ``others.knn_bank: {per_class: 1024,
    normalize: true}`` are the fit's options.  Writes ``knn.npz`` and a readable ``knn.json`` into the run directory and returns the bank;
    ``others.knn: <that .npz>`` applies it in the default test scripts."""
    context, seed = _fit_context('fit_knn', dataset, config_file, device, knn_mod.check_model)      # (no U-Net, more than 32 channels: refused)
    per_class, normalize = _knn_bank_options(context)
    bank = knn_mod.fit_knn(context.model, _validation_batches(context, dataset, context.device), per_class, seed, normalize=normalize, nb_classes=2)
    path = os.path.join(context.test_dir, 'knn.npz')
    knn_mod.save_knn(bank, path)
    record = dict(bank.as_dict(), model_dir=context.config.model_dir, test_at=context.config.test_at, dataset=context.config.test_data.dataset)
    with open(os.path.join(context.test_dir, 'knn.json'), 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write('\n')
    logging.info('k-NN bank: F = %d, M = %d, counts %s, normalize %s, seed %d -> %s', bank.F, bank.M, bank.counts(), bank.normalize, bank.seed, path)
    print('knn: {}'.format(path))
    return bank


def _image_batches(context, device):
    """The images of every loader batch of ``test_data`` on the device: no labels are read."""
    for batch in context.test_data.loader:
        yield batch['images'].float().to(device).contiguous()


def fit_laplace(dataset, config_file, device='cuda'):
    """bin-dl/{brats,isic}_fit_laplace.py (EXTENSION): fit the last-layer Laplace approximation (rcu_amd.laplace) on the volumes a test
    configuration's ``test_data`` names, with one eval-mode pass per batch; no labels are needed.  ``others.laplace_hessian_scale`` (1.0),
    ``others.laplace_prior_precision`` (1.0; a number > 0 or ``evidence``) and ``others.temperature`` (a number or a temperature.json: the model
    is fitted as it will run) are the fit's options.  Writes ``laplace.npz`` and a readable ``laplace.json`` into the run directory and returns
    the fit; ``others.laplace: <that .npz>`` applies it in the default test scripts."""
    context, _ = _fit_context('fit_laplace', dataset, config_file, device, laplace_mod.check_model)      # (no U-Net, sigma_out, C outside 2..4: refused)
    if hasattr(context.config.others, 'temperature'):
        context.model.set_temperature(calibration.load_temperature(context.config.others.temperature))
    fit = laplace_mod.fit_laplace(context.model, _image_batches(context, context.device),
                                  hessian_scale=_other(context, 'laplace_hessian_scale', 1.0),
                                  prior_precision=_other(context, 'laplace_prior_precision', 1.0))
    path = os.path.join(context.test_dir, 'laplace.npz')
    laplace_mod.save_laplace(fit, path)
    record = dict(fit.as_dict(), model_dir=context.config.model_dir, test_at=context.config.test_at, dataset=context.config.test_data.dataset,
                  prior_precision=_other(context, 'laplace_prior_precision', 1.0))
    with open(os.path.join(context.test_dir, 'laplace.json'), 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write('\n')
    logging.info('Laplace fit: F = %d, C = %d, tau %.6g, hessian_scale %.6g, temperature %.6g, %d voxels -> %s', fit.F, fit.C, fit.tau,
                 fit.hessian_scale, fit.temperature, fit.voxels, path)
    print('laplace: {}'.format(path))
    return fit


_AUXILIARY_FIT_OPTIONS = {'epochs': 1, 'lr': 1e-4, 'nb_convs': 3}


def _auxiliary_fit_options(context):
    """``others.auxiliary_fit: {epochs, lr: 1e-4, nb_convs: 3}`` -> the three options; anything else in it is refused by name."""
    value = _other(context, 'auxiliary_fit', None)
    given = {} if value is None else (dict(value) if isinstance(value, dict) else dict(vars(value)))
    unknown = sorted(set(given) - set(_AUXILIARY_FIT_OPTIONS))
    if unknown:
        raise ValueError('others.auxiliary_fit takes {}; got {}'.format(', '.join(sorted(_AUXILIARY_FIT_OPTIONS)), ', '.join(unknown)))
    options = dict(_AUXILIARY_FIT_OPTIONS, **given)
    epochs, lr, nb_convs = options['epochs'], options['lr'], options['nb_convs']
    if isinstance(epochs, bool) or not isinstance(epochs, int) or epochs < 1:
        raise ValueError('others.auxiliary_fit.epochs must be an integer >= 1, got {!r}'.format(epochs))
    if isinstance(nb_convs, bool) or not isinstance(nb_convs, int) or not 1 <= nb_convs <= auxiliary_mod.MAX_CONVS:
        raise ValueError('others.auxiliary_fit.nb_convs must be an integer in 1..{}, got {!r}'.format(auxiliary_mod.MAX_CONVS, nb_convs))
    try:
        lr = float(lr)
    except (TypeError, ValueError):
        raise ValueError('others.auxiliary_fit.lr must be a number > 0, got {!r}'.format(lr)) from None
    if not (np.isfinite(lr) and lr > 0):
        raise ValueError('others.auxiliary_fit.lr must be a number > 0, got {!r}'.format(lr))
    return epochs, lr, nb_convs


def _check_auxiliary_model(model):
    channels = density_mod._feature_channels(model)      # (refuses a model that is no U-Net)
    if channels > auxiliary_mod.MAX_FEATURES:
        raise ValueError('the auxiliary fit takes U-Nets of up to {} feature channels (start_filters), got {}'.format(auxiliary_mod.MAX_FEATURES, channels))


def fit_auxiliary_feat(dataset, config_file, device='cuda'):
    """bin-dl/{brats,isic}_fit_auxiliary_feat.py (EXTENSION; the reference's *_train_auxiliary_feat.py as a post-hoc fit): fit the auxiliary
    PostNet on the features of the frozen segmentation model the configuration's ``model_dir`` / ``test_at`` name, on the volumes its
    ``test_data`` names (``batch_size`` and ``shuffle`` honoured under the YAML ``seed``), target arg-max != (labels > 0), all-black slices
    dropped.  ``others.auxiliary_fit: {epochs, lr: 1e-4, nb_convs: 3}`` are the fit's options.  Writes into the run directory a PostNet model
    directory ``model_auxiliary_feat`` (a checkpoint per epoch, the last one also as ``best``), ``auxiliary_fit.json`` and ``auxiliary_fit.csv``
    (one row per epoch: steps, voxels, error fraction, mean loss) and returns the rows.  That directory as ``model_dir`` with the segmentation
    model under ``others.model_dir`` runs the ``*_test_auxiliary_feat.py`` scripts."""
    context, seed = _fit_context('fit_auxiliary_feat', dataset, config_file, device, _check_auxiliary_model)
    epochs, lr, nb_convs = _auxiliary_fit_options(context)
    params = dict(in_channels=int(context.model.start_filters), nb_classes=2, nb_convs=nb_convs)
    postnet = model_mod.PostNet(**params)
    files = mgt.ModelFiles(context.test_dir, 'auxiliary_feat')

    def save(epoch, net, row):
        state = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
        mgt.save_model(files, 'postnet', params, state, epoch=epoch, is_best=False)
        if epoch == epochs:
            mgt.save_model(files, 'postnet', params, state, epoch=epoch, is_best=True)
        logging.info('auxiliary fit: epoch %d, %d steps, %d voxels, error fraction %.6f, mean loss %.6f', epoch, row['steps'], row['voxels'],
                     row['error_fraction'], row['mean_loss'])

    rows = auxiliary_mod.fit_auxiliary_feat(context.model, postnet, lambda: _validation_batches(context, dataset, 'cpu'), epochs, lr=lr, seed=seed,
                                            skip_black=True, on_epoch=save)
    with open(os.path.join(context.test_dir, 'auxiliary_fit.csv'), 'w', newline='') as f:
        writer = csv.writer(f)
        writer.writerow(['epoch', 'steps', 'voxels', 'error_fraction', 'mean_loss'])
        for row in rows:
            writer.writerow([row['epoch'], row['steps'], row['voxels'], repr(row['error_fraction']), repr(row['mean_loss'])])
    record = dict(params, epochs=epochs, lr=lr, seed=seed, model_dir=context.config.model_dir, test_at=context.config.test_at,
                  dataset=context.config.test_data.dataset, postnet_model_dir=files.model_dir, rows=rows)
    with open(os.path.join(context.test_dir, 'auxiliary_fit.json'), 'w') as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write('\n')
    print('auxiliary_feat: {}'.format(files.model_dir))
    return rows


for _fn in (test_default, test_ensemble, test_aleatoric, test_auxiliary_feat, test_auxiliary_segm, fit_temperature, fit_density, fit_laplace,
            fit_auxiliary_feat, fit_knn):
    _fn.__test__ = False   # not pytest tests


def eval_uncertainty(dataset, run_dirs: dict, ground_truth_dir, base_dir, actions=('minmax', 'ece_dice', 'calib', 'bnf_ue'),
                     expected_subjects=None, fused=True, batch_subjects=8, timing=None, levels=1000, connectivity=26, bands=10, dice_fail=0.8,
                     calib_bins=10, mass_bins=10, recalibrate_from=None, merge_radius=0, min_lesion_voxels=0, match_iou=0.5, patch=(1, 4, 4),
                     patch_accuracy=500, rescale='minmax', quantiles=1000):
    """``run_dirs``: run id (baseline, baseline_mc, ..., aleatoric) -> prediction directory.  BraTS evaluates
    inside the T2 brain mask (``ece_details='foreground'``), ISIC on all pixels (eval_uncertainty.py:19-26).
    ``ground_truth_dir``: the BraTS tree of ``<subject>/<subject>_{t2,seg,...}.nii.gz`` or, for ISIC, the dataset
    prefix (``.../ISIC-2017_Test_v2``) whose ``_Data`` / ``_Part1_GroundTruth`` folders hold the jpg / png files."""
    if dataset not in ('brats', 'isic'):
        raise ValueError('chose "brats" or "isic" as dataset')
    if dataset == 'brats':
        gts = evalrun.collect_brats_ground_truth(ground_truth_dir)
        details = 'foreground'
    else:
        gts = evalrun.collect_isic_ground_truth(ground_truth_dir)
        details = ''
    entries = [evalrun.get_eval_data(run_id, path, gts, expected_subjects) for run_id, path in run_dirs.items()]
    # (levels: of the extension actions 'ue_curves' and 'components', connectivity: of 'components'; bands: of 'boundary'; dice_fail: of 'agreement'; calib_bins / mass_bins / recalibrate_from: of 'calib_curves', whose level histogram has `levels` levels too; merge_radius / min_lesion_voxels / match_iou: of 'lesions', which shares levels and connectivity with 'components'; patch / patch_accuracy: of 'patches', whose histogram has `levels` levels; fused / batch_subjects / timing: rcu_amd.evalrun.evaluate_runs -- one upload per subject shared by all actions, subjects batched per launch)
    evalrun.evaluate_runs(entries, list(actions), base_dir, details, fused=fused, batch_subjects=batch_subjects, timing=timing, levels=levels,
                          connectivity=connectivity, bands=bands, dice_fail=dice_fail, calib_bins=calib_bins, mass_bins=mass_bins,
                          recalibrate_from=recalibrate_from, merge_radius=merge_radius, min_lesion_voxels=min_lesion_voxels, match_iou=match_iou,
                          patch=patch, patch_accuracy=patch_accuracy, rescale=rescale, quantiles=quantiles)      # (rescale / quantiles: the rescale of sigma / density entries in the actions on the prepared uncertainty and the Q of the 'quantiles' action)
    return entries
