"""Evaluation-script surface: what ``bin-eval/eval_uncertainty.py`` of the reference does, on the GPU.

Mirrors
  CSV hooks            rechun/eval/hook.py:10-116 (WriteCsvHook, WriteBinsCsvHook, WriteSummaryCsvHook)
  file / run registry  rechun/eval/evaldata.py:8-103, common/data/collector.py:120-174, rechun/directories.py:56-71
  loader               rechun/eval/analysis.py:15-125 (probabilities / target>0 / prediction / T2 brain mask, cached)
  actions + driver     bin-eval/eval_uncertainty.py:13-244 (minmax, ece_dice, calib, bnf_ue); ue_curves, components, boundary, agreement, calib_curves, lesions and patches are extensions
so that the CSV files ``bin-analysis/*`` consumes keep their names, columns and row order.  The volumes
are read with rcu_amd.nifti, the per-voxel work (histograms, counts, entropy) runs through
rcu_amd.evaluation on the GPU; the ``bnf_ue`` action evaluates its 11 thresholds in ONE pass per subject
and fans the result out to the 11 per-threshold CSV files the reference writes.
"""
import abc
import csv
import glob
import os
import time

import numpy as np

from . import evaluation as ev
from . import nifti

# rechun/directories.py:56-71
ECE_FOREGROUND_NAME = 'ece_foreground'
ECE_NAME = 'ece'
CALIB_NAME = 'calibration'
UNCERTAINTY_NAME = 'uncertainty'
MINMAX_NAME = 'minmax'
CALIBRATION_PLACEHOLDER = 'eval_calibration_{}.csv'
UNCERTAINTY_PLACEHOLDER = 'eval_uncertainty_{}_th{}.csv'
ECE_PLACEHOLDER = 'eval_ece_{}.csv'
MINMAX_PLACEHOLDER = 'eval_summary_minmax_{}.csv'
# rcu_amd extension (the 'quantiles' action, the sibling of 'minmax'): the run's quantile table, in its own directory
QUANTILES_NAME = 'quantiles'
QUANTILES_PLACEHOLDER = 'eval_quantiles_{}.csv'
RESCALES = ('minmax', 'quantile')
# rcu_amd extension (the 'ue_curves' action), next to the per-threshold files in UNCERTAINTY_NAME
UE_CURVES_PLACEHOLDER = 'eval_ue_curves_{}.csv'
UE_CURVES_POOLED_PLACEHOLDER = 'eval_ue_curves_pooled_{}.csv'
UE_LEVELS_PLACEHOLDER = 'eval_ue_levels_{}.csv'
# rcu_amd extension (the 'calib_curves' action), next to the reliability bins in CALIB_NAME
CALIB_CURVES_PLACEHOLDER = 'eval_calib_curves_{}.csv'
CALIB_CURVES_POOLED_PLACEHOLDER = 'eval_calib_curves_pooled_{}.csv'
CALIB_LEVELS_PLACEHOLDER = 'eval_calib_levels_{}.csv'
CALIB_LEVELS_COLUMNS = ('level', 'threshold', 'n_neg', 'n_pos', 'mean_confidence', 'positive_fraction', 'isotonic')
# rcu_amd extension (the 'components' action), in UNCERTAINTY_NAME as well
COMPONENTS_PLACEHOLDER = 'eval_components_{}.csv'
COMPONENTS_POOLED_PLACEHOLDER = 'eval_components_pooled_{}.csv'
COMPONENT_LIST_PLACEHOLDER = 'eval_component_list_{}.csv'
# rcu_amd extension (the 'boundary' action), in UNCERTAINTY_NAME as well
BOUNDARY_PLACEHOLDER = 'eval_boundary_{}.csv'
BOUNDARY_POOLED_PLACEHOLDER = 'eval_boundary_pooled_{}.csv'
BOUNDARY_BANDS_PLACEHOLDER = 'eval_boundary_bands_{}.csv'
# rcu_amd extension (the 'patches' action), in UNCERTAINTY_NAME as well
PATCHES_PLACEHOLDER = 'eval_patches_{}.csv'
PATCHES_POOLED_PLACEHOLDER = 'eval_patches_pooled_{}.csv'
PATCH_LEVELS_PLACEHOLDER = 'eval_patch_levels_{}.csv'
PATCH_LEVELS_COLUMNS = ('level', 'threshold', 'accurate_fg', 'inaccurate', 'accurate_bg', 'pavpu', 'p_ac', 'p_ui')
# rcu_amd extension (the 'lesions' action), in UNCERTAINTY_NAME as well
LESIONS_PLACEHOLDER = 'eval_lesions_{}.csv'
LESIONS_POOLED_PLACEHOLDER = 'eval_lesions_pooled_{}.csv'
LESION_LIST_PLACEHOLDER = 'eval_lesion_list_{}.csv'
LESION_CURVE_PLACEHOLDER = 'eval_lesion_curve_{}.csv'

# rcu_amd extension (the 'agreement' action), in UNCERTAINTY_NAME as well; AGREEMENT_FILE is what the test script wrote into the run directory
AGREEMENT_PLACEHOLDER = 'eval_agreement_{}.csv'
AGREEMENT_POOLED_PLACEHOLDER = 'eval_agreement_pooled_{}.csv'
AGREEMENT_FILE = 'agreement.csv'
# score -> whether a HIGH value points at a failed segmentation (the agreement scores are low there, the volume spread is high)
AGREEMENT_SCORES = {'mean_pairwise_dice': False, 'min_pairwise_dice': False, 'pooled_pairwise_dice': False, 'iou_all': False, 'volume_cv': True}

CONFIDENCE_ENTRY = {'baseline': 'probabilities', 'baseline_mc': 'probabilities', 'center': 'probabilities',
                    'center_mc': 'probabilities', 'ensemble': 'probabilities', 'auxiliary_feat': 'confidence',
                    'auxiliary_segm': 'confidence', 'aleatoric': 'sigma'}   # evaldata.py:21-47
# rcu_amd extension: a default run under others.density -- its {subject}_density.nii.gz (the feature-space energy, rcu_amd.density) is unbounded
# like sigma and takes sigma's path through every action: the rescale_sigma rescale (global min-max through the minmax action), then an uncertainty
CONFIDENCE_ENTRY['density'] = 'density'
# rcu_amd extension: a default run under others.laplace, seen twice -- `laplace` reads its probabilities (the Laplace predictive: ece_dice, calib
# and calib_curves speak about it), `laplace_std` its {subject}_laplace_std.nii.gz (the std of the predicted class's logit), which takes sigma's path
CONFIDENCE_ENTRY['laplace'] = 'probabilities'
CONFIDENCE_ENTRY['laplace_std'] = 'laplace_std'
# rcu_amd extension: a default run under others.knn -- its {subject}_knn.nii.gz (the distance to the k-th nearest bank row, rcu_amd.knn) is unbounded
# like sigma and takes sigma's path
CONFIDENCE_ENTRY['knn'] = 'knn'


# ------------------------------------------------------------------------------------- CSV hooks
def write_table(path, header, rows):
    """A CSV file of one header row and ``rows``."""
    with open(path, 'w', newline='') as f:
        writer = csv.writer(f)
        writer.writerow(header)
        writer.writerows(rows)


class EvalHook:
    def on_run_start(self, run_id: str):
        pass

    def on_subject(self, results: dict, subject_name: str, run_id: str):
        pass

    def on_run_end(self, results_history: dict, run_id: str):
        pass


class ReducedComposeEvalHook(EvalHook):
    """Calls only the methods a member hook really overrides (common/trainloop/hooks.py:116-133)."""

    def __init__(self, hooks: list) -> None:
        for name in ('on_run_start', 'on_subject', 'on_run_end'):
            fns = [getattr(h, name) for h in hooks if getattr(type(h), name) is not getattr(EvalHook, name)]
            setattr(self, name, self._chain(fns))

    @staticmethod
    def _chain(fns):
        def call(*args, **kwargs):
            for fn in fns:
                fn(*args, **kwargs)
        return call


class WriteCsvHook(EvalHook):
    """One row per subject: ``test_id, subject_name, <entries>``; list-valued results are unfolded to
    ``key_<i>`` columns with zero-padded indices (hook.py:28-72)."""

    def __init__(self, file_path: str, entries=None) -> None:
        self.file_path = file_path
        self.rows = []
        self.entries = None if entries is None else list(entries)
        self.header = None

    @staticmethod
    def _unfold_results(results):
        flat = {}
        for key, value in results.items():
            if isinstance(value, np.ndarray):
                value = value.tolist()
            if isinstance(value, (list, tuple)):
                digits = len(str(len(value)))
                for i, v in enumerate(value):
                    flat['{}_{:0{}d}'.format(key, i, digits)] = v
            else:
                flat[key] = value
        return flat

    def on_subject(self, results: dict, subject_name: str, run_id: str):
        flat = self._unfold_results(results)
        if self.entries is None:
            self.entries = list(flat.keys())
        if self.header is None:
            self.header = ['test_id', 'subject_name'] + self.entries
        self.rows.append([run_id, subject_name] + [flat[e] for e in self.entries])

    def on_run_end(self, results_history: dict, run_id: str):
        write_table(self.file_path, self.header, self.rows)


class WriteBinsCsvHook(WriteCsvHook):
    """Re-expands the non-empty-bin arrays to all bins before unfolding (hook.py:75-93)."""

    def on_subject(self, results: dict, subject_name: str, run_id: str):
        non_zero = results['bins_non_zero']
        for key in ('bins_count', 'bins_avg_confidence', 'bins_positive_fraction'):
            full = np.zeros_like(non_zero, dtype=results[key].dtype)
            full[non_zero] = results[key]
            results[key] = full
        super().on_subject(results, subject_name, run_id)


class WriteSummaryCsvHook(EvalHook):
    """``confidence_entry, min, max`` over the whole run (hook.py:96-116)."""

    def __init__(self, file_path: str, entries=('min', 'max'), summary_fn=(np.min, np.max),
                 confidence_entry='probabilities') -> None:
        if len(entries) != len(summary_fn):
            raise ValueError('entries and summary_fn must be of same length')
        self.file_path = file_path
        self.entries = list(entries)
        self.summary_fn = list(summary_fn)
        self.confidence_entry = confidence_entry

    def on_run_end(self, results_history: dict, run_id: str):
        write_table(self.file_path, ['confidence_entry'] + self.entries,
                    [[self.confidence_entry] + [fn(results_history[e]) for e, fn in zip(self.entries, self.summary_fn)]])


def read_min_max(min_max_file: str):
    """rechun/eval/helper.py:50-55."""
    with open(min_max_file, 'r') as f:
        reader = csv.reader(f)
        next(reader)
        _, min_, max_ = next(reader)
    return float(min_), float(max_)


# ------------------------------------------------------------------------------ files and runs
class SubjectFiles:
    """subject id + {category: {entry: path}} (the part of pymia's SubjectFile the path uses)."""

    def __init__(self, subject, **categories):
        self.subject = subject
        self.categories = {k: dict(v) for k, v in categories.items()}


def collect_predictions(prediction_path, post_fixes, categories):
    """``**/<subject>_<postfix>.nii.gz`` under a prediction directory (collector.py:120-161)."""
    by_id = {}
    for pf in post_fixes:
        tail = '_{}.nii.gz'.format(pf)
        for path in glob.glob(os.path.join(prediction_path, '**', '*' + tail), recursive=True):
            by_id.setdefault(os.path.basename(path)[:-len(tail)], {})[pf] = path
    out = []
    for subject, files in by_id.items():
        if set(files) != set(post_fixes):
            raise AssertionError('id "{}" has not all required entries "({})"'.format(subject, list(post_fixes)))
        cats = {}
        for pf, cat in zip(post_fixes, categories):
            cats.setdefault(cat, {})[pf] = files[pf]
        out.append(SubjectFiles(subject, **cats))
    return out


def collect_brats_ground_truth(root_dir):
    """``**/<subject>/<subject>_{flair,t1,t2,t1ce,seg}.nii.gz`` (collector.py:17-71); subject = directory name."""
    out = []
    for flair in sorted(glob.glob(os.path.join(root_dir, '**', '*_flair.nii.gz'), recursive=True)):
        stem = flair[:-len('_flair.nii.gz')]
        images = {'flair': flair, 't1': stem + '_t1.nii.gz', 't2': stem + '_t2.nii.gz', 't1c': stem + '_t1ce.nii.gz'}
        labels = {'gt': stem + '_seg.nii.gz'} if os.path.exists(stem + '_seg.nii.gz') else {}
        out.append(SubjectFiles(os.path.basename(os.path.dirname(flair)), images=images, labels=labels))
    return out


def collect_isic_ground_truth(root_dir_with_prefix):
    """``<prefix>_Data/<id>.jpg`` + ``<prefix>_Part1_GroundTruth/<id>_segmentation.png`` (collector.py:75-120);
    subject = the first 12 characters of the file name."""
    by_id = {}
    for path in glob.glob(root_dir_with_prefix + '_Data/*') + glob.glob(root_dir_with_prefix + '_Part1_GroundTruth/*'):
        name = os.path.basename(path)
        if name.endswith('_segmentation.png'):
            by_id.setdefault(name[:12], {})['gt'] = path
        elif name.endswith('.jpg'):
            by_id.setdefault(name[:12], {})['image'] = path
    out = []
    for id_, files in sorted(by_id.items()):
        if 'gt' in files and 'image' in files:
            out.append(SubjectFiles(id_, images={'image': files['image']}, labels={'gt': files['gt']}))
    return out


def read_label_image(path, dtype=np.uint8):
    """NIfTI, or the png masks of ISIC (the reference reads both through ``sitk.ReadImage(path, sitkUInt8)``)."""
    if str(path).endswith(('.png', '.jpg')):
        from PIL import Image
        return np.array(Image.open(path).convert('L')).astype(dtype)
    return nifti.read(path, dtype)[0]


def combine(files_from, files_to):
    """collector.py:164-174: add the categories of ``files_from`` to the same subject in ``files_to``."""
    by_id = {sf.subject: sf for sf in files_from}
    for sf in files_to:
        for cat, entries in by_id[sf.subject].categories.items():
            sf.categories.setdefault(cat, {}).update(entries)
    return files_to


class EvalData:
    def __init__(self, id_, eval_path, confidence_entry='probabilities', subject_files=None) -> None:
        self.id_ = id_
        self.eval_path = eval_path
        self.confidence_entry = confidence_entry
        self.subject_files = subject_files if subject_files is not None else []


def get_eval_data(run_id, prediction_dir, ground_truth_files, expected_subjects=None):
    """One run: collect ``*_prediction`` + ``*_<confidence entry>`` files and join them with the ground truth."""
    entry = EvalData(run_id, prediction_dir, CONFIDENCE_ENTRY.get(run_id, 'probabilities'))
    preds = collect_predictions(prediction_dir, ['prediction', entry.confidence_entry], ['labels', 'misc'])
    preds = combine(ground_truth_files, preds)
    if expected_subjects is not None:
        assert set(expected_subjects) == set(sf.subject for sf in preds)
    entry.subject_files = sorted(preds, key=lambda sf: sf.subject)
    return entry


# -------------------------------------------------------------------------------------- loader
class Loader:
    """Per-subject cached reads (analysis.py:15-125)."""

    class Params:
        def __init__(self, misc_entry='probabilities', need_target=True, need_prediction=True, need_t2_mask=False,
                     need_gt_dist_and_boarder=False, need_prediction_dist_and_boarder=False):
            self.misc_entry = misc_entry
            self.need_target = need_target
            self.need_prediction = need_prediction
            self.need_t2_mask = need_t2_mask
            self.need_gt_dist_and_boarder = need_gt_dist_and_boarder
            self.need_prediction_dist_and_boarder = need_prediction_dist_and_boarder

    def __init__(self) -> None:
        self.cached = {}
        self.cached_subject = None

    def _get(self, key, fn):
        if key not in self.cached:
            self.cached[key] = fn()
        return self.cached[key].copy()

    def _get_dist_and_boarder(self, boarder_entry, dist_entry, read_label_map):
        """analysis.py:109-116: the border shell (1, 1) and the distance map of a label map, on the GPU, cached per subject.  -> (mask, distance)"""
        if boarder_entry not in self.cached or dist_entry not in self.cached:
            distance, mask = ev.boarder_mask(read_label_map().astype(bool), 1, 1)
            self.cached[boarder_entry] = mask
            self.cached[dist_entry] = distance
        return self.cached[boarder_entry].copy(), self.cached[dist_entry].copy()

    def get_data(self, sf: SubjectFiles, params):
        if sf.subject != self.cached_subject:
            self.cached.clear()
            self.cached_subject = sf.subject
        to_eval = {params.misc_entry: self._get(params.misc_entry,
                                                lambda: nifti.read(sf.categories['misc'][params.misc_entry])[0])}

        def read_target():       # labels 0..4 are binarised (analysis.py:88-89)
            return self._get('target', lambda: (read_label_image(sf.categories['labels']['gt']) > 0).astype(np.uint8))

        def read_prediction():
            return self._get('prediction', lambda: nifti.read(sf.categories['labels']['prediction'], np.uint8)[0])

        if params.need_target:
            to_eval['target'] = read_target()
        if params.need_prediction:
            to_eval['prediction'] = read_prediction()
        # analysis.py:54-64: the mask under *_boarder, the distance under *_distance
        if getattr(params, 'need_gt_dist_and_boarder', False):
            to_eval['target_boarder'], to_eval['target_distance'] = self._get_dist_and_boarder('target_boarder', 'target_distance', read_target)
        if getattr(params, 'need_prediction_dist_and_boarder', False):
            to_eval['prediction_boarder'], to_eval['prediction_distance'] = self._get_dist_and_boarder('prediction_boarder', 'prediction_distance',
                                                                                                   read_prediction)
        if params.need_t2_mask:
            to_eval['mask'] = self._get('mask', lambda: nifti.read(sf.categories['images']['t2'])[0] > 0)
        return to_eval


# ------------------------------------------------------------------------------------- actions
class EvalCase:
    def __init__(self, metric, hook, id_='') -> None:
        self.result_history = {}
        self.metric = metric
        self.hook = hook
        self.id_ = id_

    def record(self, results, subject_name, id_):
        self.hook.on_subject(results, subject_name, id_)
        for k, v in results.items():
            self.result_history.setdefault(k, []).append(v)

    def do_eval(self, to_eval, subject_name, id_):
        results = {}
        self.metric(to_eval, results)
        self.record(results, subject_name, id_)


class EvalAction(abc.ABC):
    """An action of the evaluation script.  The plain loop calls ``eval_subject``; what the fused loop (``_evaluate_fused``, the
    device-metrics hook) needs to serve the action from the one `evaluation.SubjectBatch.metrics` call of a batch is declared here too:
    ``scans``, ``fused_arguments`` and ``record_fused``."""

    scans = None              # the scans (names of ``want``) of `SubjectBatch.metrics` the action is recorded from; None: it cannot run fused
    runs_first = False        # whether it writes a file of the run that other actions of the same call read at set-up time ('minmax', 'quantiles')
    whole_run = False         # whether it walks the run itself (``eval_run``) instead of being handed one subject at a time
    need_mask = False         # whether it evaluates inside the T2 brain mask
    checks_range = True       # whether its preparation refuses maps outside [0, 1] (helper.add_background_probability)

    def __init__(self) -> None:
        self.load_params = None
        self.prepare = None
        self.eval_cases = []
        self.id_ = ''
        self.out_dir = None

    @abc.abstractmethod
    def setup_eval(self, eval_data: EvalData):
        pass

    def fused_arguments(self):
        """The keyword arguments of `SubjectBatch.metrics` this action fixes ('mask': whether the batch holds the brain mask)."""
        return {}

    def record_fused(self, res, slot, subject, n_dim):
        """Subject ``slot`` of a `SubjectBatch.metrics` result -> the rows ``eval_subject`` would have recorded."""

    def path(self, placeholder):
        return os.path.join(self.out_dir, placeholder.format(self.id_))

    def start_eval(self):
        print(self.id_ + ', '.join(c.id_ for c in self.eval_cases if c.id_ != ''))
        for case in self.eval_cases:
            case.hook.on_run_start(self.id_)

    def eval_subject(self, sf, loader):
        to_eval = loader.get_data(sf, self.load_params)
        if self.prepare:
            to_eval = self.prepare(to_eval)
        for case in self.eval_cases:
            case.do_eval(to_eval, sf.subject, self.id_)

    def eval_run(self, eval_data: EvalData):
        """The whole run at once, for an action that declares ``whole_run`` (between ``start_eval`` and ``finish_eval``)."""
        raise NotImplementedError

    def finish_eval(self):
        for case in self.eval_cases:
            case.hook.on_run_end(case.result_history, self.id_)


def _minmax_for(min_max_dir, run_id, rescale):
    if rescale != 'global':
        return None
    return read_min_max(os.path.join(min_max_dir, MINMAX_PLACEHOLDER.format(run_id)))


def quantiles_file(quantile_dir, run_id):
    return os.path.join(quantile_dir, QUANTILES_PLACEHOLDER.format(run_id))


def read_quantiles_for(quantile_dir, run_id, quantiles):
    """The table the 'quantiles' action wrote for this run, with the Q the call asks for; anything else is a ValueError naming file and flag."""
    path = quantiles_file(quantile_dir, run_id)
    if not os.path.exists(path):
        raise ValueError('--rescale quantile: {} is missing; run `--act quantiles` over run {} first (in this call or an earlier one)'.format(path, run_id))
    table = ev.load_quantiles(path)
    if table.Q != int(quantiles):
        raise ValueError('--rescale quantile: {} holds Q = {} boundaries, --quantiles asks for {}; run `--act quantiles --quantiles {}` again'
                         .format(path, table.Q, quantiles, quantiles))
    return table


class SaveQuantilesAction(EvalAction):
    """EXTENSION (the sibling of ``SaveMinMaxAction``): the exact quantile table of a 'sigma' / 'density' run (evaluation.quantile_table) over the
    voxels inside the T2 brain mask where the dataset evaluates inside one, over every voxel otherwise, written to
    ``<base_dir>/quantiles/eval_quantiles_<id>.csv``.  It reads the run once per radix pass (twice by default) and therefore walks the run itself;
    it never joins the fused probability loop.  On a probability-map or 'confidence' run it writes nothing and says so."""

    scans = None
    runs_first = True
    whole_run = True
    checks_range = False
    ENTRIES = ('sigma', 'density', 'laplace_std', 'knn')

    def __init__(self, quantile_dir, quantiles, need_mask):
        super().__init__()
        self.quantile_dir, self.quantiles, self.need_mask = quantile_dir, ev._check_quantiles(quantiles), bool(need_mask)
        self.entry = None

    def setup_eval(self, eval_data):
        self.id_ = eval_data.id_
        self.entry = eval_data.confidence_entry
        self.load_params = None       # (it reads its files itself, once per pass)

    def eval_subject(self, sf, loader):
        pass

    def eval_run(self, eval_data):
        if self.entry not in self.ENTRIES:
            print('quantiles: run {} holds a {} map in [0, 1], which is not rescaled: nothing written'.format(self.id_, self.entry))
            return
        if not eval_data.subject_files:
            raise ValueError('quantiles: run {} has no subjects'.format(self.id_))
        params = Loader.Params(self.entry, need_target=False, need_prediction=False, need_t2_mask=self.need_mask)
        files = eval_data.subject_files

        def volumes():
            reader = _ReadAhead(files, params, depth=4)
            try:
                for i, sf in enumerate(files):
                    data = reader.get(i)
                    yield sf.subject, data[self.entry], data.get('mask')
            finally:
                reader.close()

        start = time.time()
        table = ev.quantile_table(volumes, self.quantiles, population='mask' if self.need_mask else 'all')
        os.makedirs(self.quantile_dir, exist_ok=True)
        ev.save_quantiles(table, quantiles_file(self.quantile_dir, self.id_))
        print('quantiles: {} subjects, N = {}, Q = {} ({}s)'.format(len(files), table.N, table.Q, time.time() - start))


class SaveMinMaxAction(EvalAction):
    scans = ('minmax',)
    runs_first = True
    checks_range = False      # (it moves the confidence entry as it is)

    def __init__(self, min_max_dir: str) -> None:
        super().__init__()
        self.min_max_dir = min_max_dir
        os.makedirs(min_max_dir, exist_ok=True)

    def setup_eval(self, eval_data):
        self.id_ = eval_data.id_
        self.prepare = ev.MoveEntry(eval_data.confidence_entry, 'probabilities')
        self.load_params = Loader.Params(eval_data.confidence_entry)
        metric = ev.ComposeEvaluation([ev.LambdaEvaluation(lambda x: x.min(), ('probabilities',), 'min'),
                                       ev.LambdaEvaluation(lambda x: x.max(), ('probabilities',), 'max')])
        hook = WriteSummaryCsvHook(os.path.join(self.min_max_dir, MINMAX_PLACEHOLDER.format(self.id_)),
                                   confidence_entry=eval_data.confidence_entry)
        self.eval_cases = [EvalCase(metric, hook)]

    def record_fused(self, res, slot, subject, n_dim):
        self.eval_cases[0].record({'min': res['min'][slot], 'max': res['max'][slot]}, subject, self.id_)


def _confusion(res, slot):
    """tp, tn, fp, fn of a subject: the first four of the uncertainty-error counts at any threshold (the 'ue' scan)."""
    return tuple(int(v) for v in res['counts'][slot][0][:4])


class PreparedAction(EvalAction):
    """What the actions on a prepared confidence entry share: the preparation function (``get_probability_preparation`` or
    ``get_uncertainty_preparation``) with its rescale arguments, the output directory ``<base_dir>/<out_name>``, the mask flag, the
    preparation of a run (``setup_run`` is the subclass's part of ``setup_eval``), a subject's prepared entries, the usual file of one row
    per subject and the one-row file of a pooled result."""

    def __init__(self, preparation, out_name, need_mask, base_dir, rescale_confidence, rescale_sigma, min_max_dir):
        super().__init__()
        self.preparation, self.need_mask = preparation, need_mask
        self.rescale_confidence, self.rescale_sigma, self.min_max_dir = rescale_confidence, rescale_sigma, min_max_dir
        self.out_dir = os.path.join(base_dir, out_name)
        self.quantile_dir, self.quantiles = None, ev.QUANTILES      # (of rescale_sigma == 'quantile': get_actions sets them)
        os.makedirs(self.out_dir, exist_ok=True)

    def setup_eval(self, eval_data):
        rescale = self.rescale_confidence if eval_data.confidence_entry == 'confidence' else self.rescale_sigma
        if eval_data.confidence_entry == 'probabilities':
            mm = None
        elif rescale == 'quantile':      # the table takes the place of the (min, max) pair
            mm = read_quantiles_for(self.quantile_dir, eval_data.id_, self.quantiles)
        else:
            mm = _minmax_for(self.min_max_dir, eval_data.id_, rescale)
        self.prepare, self.id_ = self.preparation(eval_data.confidence_entry, eval_data.id_, self.rescale_confidence, self.rescale_sigma, mm)
        self.load_params = Loader.Params(eval_data.confidence_entry, need_t2_mask=self.need_mask)
        self.setup_run()

    @abc.abstractmethod
    def setup_run(self):
        """``eval_cases`` and whatever the run accumulates, once ``id_``, ``prepare`` and ``load_params`` are set."""

    def subject_rows(self, placeholder, keys):
        """The usual ``eval_cases``: one CSV file of one row per subject, filled through ``eval_cases[0].record``."""
        self.eval_cases = [EvalCase(None, WriteCsvHook(self.path(placeholder), entries=keys))]

    def prepared(self, sf, loader):
        to_eval = loader.get_data(sf, self.load_params)
        return self.prepare(to_eval) if self.prepare else to_eval

    def write_pooled_row(self, path, keys, row):
        write_table(path, ['test_id'] + list(keys), [[self.id_] + [row[k] for k in keys]])


class EceAction(PreparedAction):
    scans = ('ece', 'ue')

    def __init__(self, base_dir, details, rescale_confidence='subject', rescale_sigma='subject', min_max_dir=None):
        foreground = details == 'foreground'
        super().__init__(ev.get_probability_preparation, ECE_FOREGROUND_NAME if foreground else ECE_NAME, foreground, base_dir, rescale_confidence,
                         rescale_sigma, min_max_dir)

    def setup_run(self):
        metric = ev.ComposeEvaluation([ev.EceBinaryNumpy(threshold_range=None, with_mask=self.need_mask),
                                       ev.DiceNumpy(), ev.ConfusionMatrix()])
        hook = WriteCsvHook(self.path(ECE_PLACEHOLDER), entries=('ece', 'dice', 'tp', 'tn', 'fp', 'fn', 'n'))
        self.eval_cases = [EvalCase(metric, hook)]

    def fused_arguments(self):
        return {'mask': self.need_mask}

    def record_fused(self, res, slot, subject, n_dim):
        tp, tn, fp, fn = _confusion(res, slot)
        results = {'ece': ev.ece_from_histogram(*(h[slot] for h in res['hist']), n_dim=n_dim), 'dice': ev._dice(tp, fp, fn)}
        results.update(tp=tp, tn=tn, fp=fp, fn=fn, n=tp + tn + fp + fn)
        self.eval_cases[0].record(results, subject, self.id_)


class EceCalibrationAction(PreparedAction):
    scans = ('ece', 'ue')

    def __init__(self, base_dir, details='', rescale_confidence='subject', rescale_sigma='subject', min_max_dir=None):
        super().__init__(ev.get_probability_preparation, CALIB_NAME, details == 'foreground', base_dir, rescale_confidence, rescale_sigma, min_max_dir)

    def setup_run(self):
        metric = ev.ComposeEvaluation([ev.EceBinaryNumpy(threshold_range=None, return_bins=True,
                                                         with_mask=self.need_mask), ev.DiceNumpy()])
        self.eval_cases = [EvalCase(metric, WriteBinsCsvHook(self.path(CALIBRATION_PLACEHOLDER)))]

    def fused_arguments(self):
        return {'mask': self.need_mask}

    def record_fused(self, res, slot, subject, n_dim):
        tp, _, fp, fn = _confusion(res, slot)
        results = {}             # key order of EceBinaryNumpy(return_bins=True) + DiceNumpy: the bins, ece, dice
        results['ece'] = ev.ece_from_histogram(*(h[slot] for h in res['hist']), n_dim=n_dim, out_bins=results)
        results['dice'] = ev._dice(tp, fp, fn)
        self.eval_cases[0].record(results, subject, self.id_)


class UncertaintyAction(PreparedAction):
    """The actions on the prepared 'uncertainty' entry: files in ``<base_dir>/uncertainty``, no brain mask; and the check of ``levels``."""

    def __init__(self, base_dir, rescale_confidence='', rescale_sigma='global', min_max_dir=None):
        super().__init__(ev.get_uncertainty_preparation, UNCERTAINTY_NAME, False, base_dir, rescale_confidence, rescale_sigma, min_max_dir)

    @staticmethod
    def checked_levels(levels):
        if not 2 <= int(levels) <= ev._lib.RCU_UNC_HIST_MAX_LEVELS:
            raise ValueError('levels must be in 2..{}, got {}'.format(ev._lib.RCU_UNC_HIST_MAX_LEVELS, levels))
        return int(levels)


class CorrectionAction(UncertaintyAction):
    """11 CSV files (one per threshold) from one GPU pass per subject."""

    def __init__(self, thresholds, base_dir, rescale_confidence='', rescale_sigma='global', min_max_dir=None):
        super().__init__(base_dir, rescale_confidence, rescale_sigma, min_max_dir)
        self.thresholds = list(thresholds)

    @property
    def scans(self):         # fused only where the library's table of the reference's uncertain-voxel sets covers the thresholds
        return ('ue',) if ev.from_p_supported(self.thresholds) else None

    def fused_arguments(self):
        return {'thresholds': tuple(self.thresholds)}

    def setup_run(self):
        self.sweep = ev.UncertaintyAndCorrectionSweep(self.thresholds)
        self.eval_cases = []
        for thr in self.thresholds:
            thr_str = '{:.2f}'.format(thr).replace('.', '')
            hook = WriteCsvHook(os.path.join(self.out_dir, UNCERTAINTY_PLACEHOLDER.format(self.id_, thr_str)), None)
            self.eval_cases.append(EvalCase(None, hook))

    def eval_subject(self, sf, loader):
        results = {}
        self.sweep(self.prepared(sf, loader), results)
        for thr, case in zip(self.thresholds, self.eval_cases):
            case.record(results[thr], sf.subject, self.id_)

    def record_fused(self, res, slot, subject, n_dim):
        for t, case in enumerate(self.eval_cases):
            case.record(ev.correction_results(res['counts'][slot][t]), subject, self.id_)


class LevelHistogramAction(UncertaintyAction):
    """The body of ``UeCurvesAction`` and ``PatchesAction``: one integer histogram ``[ROWS, levels]`` per subject (``histogram`` in the plain
    loop, ``res[RESULT]`` in the fused one), ``metrics`` of it as the subject's row (``KEYS``), the histograms summed, and at the end the
    same metrics of the sum and the sum itself, one row per level.  ``FILES``: the placeholders of these three files."""

    RESULT = ROWS = KEYS = metrics = FILES = LEVELS_COLUMNS = None

    def __init__(self, levels, base_dir, rescale_confidence='', rescale_sigma='global', min_max_dir=None):
        self.levels = self.checked_levels(levels)
        super().__init__(base_dir, rescale_confidence, rescale_sigma, min_max_dir)
        self.pooled = None

    def fused_arguments(self):
        return {'levels': self.levels}

    def setup_run(self):
        self.subject_rows(self.FILES[0], self.KEYS)
        self.pooled = np.zeros((self.ROWS, self.levels), dtype=np.uint64)

    def record_histogram(self, hist, subject_name):
        """One subject's histogram ``[ROWS, levels]``: its metrics row, and its share of the pooled histogram."""
        self.eval_cases[0].record(self.metrics(hist), subject_name, self.id_)
        self.pooled += np.asarray(hist, dtype=np.uint64)

    def eval_subject(self, sf, loader):
        to_eval = self.prepared(sf, loader)
        self.record_histogram(self.histogram(to_eval['prediction'], to_eval['target'], to_eval['uncertainty']), sf.subject)

    def record_fused(self, res, slot, subject, n_dim):
        self.record_histogram(res[self.RESULT][slot], subject)

    def extra_levels_columns(self):
        """What the levels file holds per level behind ``level, threshold`` and the pooled integers."""
        return [[]] * self.levels

    def finish_eval(self):
        super().finish_eval()
        self.write_pooled_row(self.path(self.FILES[1]), self.KEYS, self.metrics(self.pooled))
        extra = self.extra_levels_columns()
        write_table(self.path(self.FILES[2]), self.LEVELS_COLUMNS,
                    ([level, level / self.levels] + [int(v) for v in self.pooled[:, level]] + extra[level] for level in range(self.levels)))


class UeCurvesAction(LevelHistogramAction):
    """EXTENSION (the reference has no such action): threshold-free uncertainty-error metrics from one level histogram per subject
    (evaluation.uncertainty_histogram / ue_curve_metrics), prepared exactly like ``CorrectionAction`` and, like it, without a brain mask.
    Files in ``<base_dir>/uncertainty``:
      eval_ue_curves_<id>.csv          one row per subject: n, n_errors, auroc, auprc, aurc, eaurc, ue_dice_max, ue_dice_max_threshold
      eval_ue_curves_pooled_<id>.csv   the same metrics of the SUM of the subjects' histograms (integers: whatever the batching or order)
      eval_ue_levels_<id>.csv          that pooled histogram, one row per level: level, threshold, tp, tn, fp, fn -- ``threshold`` = level /
                                       levels, the boundary below the level; the rows from level k on add up to the voxels with
                                       uncertainty > k / levels, so risk-coverage and uncertainty-error Dice curves need no second run"""

    scans = ('ue_hist',)
    RESULT, ROWS, KEYS, metrics = 'ue_hist', 4, ev.UE_CURVE_KEYS, staticmethod(ev.ue_curve_metrics)
    FILES = (UE_CURVES_PLACEHOLDER, UE_CURVES_POOLED_PLACEHOLDER, UE_LEVELS_PLACEHOLDER)
    LEVELS_COLUMNS = ('level', 'threshold', 'tp', 'tn', 'fp', 'fn')

    def histogram(self, prediction, target, uncertainty):
        return ev.uncertainty_histogram(prediction, target, uncertainty, self.levels)[0]


class PatchesAction(LevelHistogramAction):
    """EXTENSION (the reference has no such action): patch accuracy vs. patch uncertainty (Mukhoti & Gal, 2018) from one patch histogram per
    subject (evaluation.patch_histogram / pavpu_metrics) over a grid of non-overlapping windows of ``patch`` = (depth, height, width) voxels,
    a patch being accurate when more than ``accuracy_per_mille`` / 1000 of its voxels are.  Prepared exactly like ``UeCurvesAction`` -- any
    confidence entry, no brain mask.  Files in ``<base_dir>/uncertainty``:
      eval_patches_<id>.csv          one row per subject: the keys of evaluation.PAVPU_KEYS
      eval_patches_pooled_<id>.csv   the same metrics of the SUM of the subjects' histograms (integers: whatever the batching or order)
      eval_patch_levels_<id>.csv     that pooled histogram, one row per level: level, threshold = level / levels, the patches of the level
                                     that are accurate with foreground / inaccurate / accurate pure background, and PAvPU, p(accurate |
                                     certain) and p(uncertain | inaccurate) over all patches with "uncertain" := level >= this one (empty
                                     at level 0, where there is no threshold)"""

    scans = ('patches',)
    RESULT, ROWS, KEYS, metrics = 'patch_hist', 3, ev.PAVPU_KEYS, staticmethod(ev.pavpu_metrics)
    FILES = (PATCHES_PLACEHOLDER, PATCHES_POOLED_PLACEHOLDER, PATCH_LEVELS_PLACEHOLDER)
    LEVELS_COLUMNS = PATCH_LEVELS_COLUMNS

    def __init__(self, levels, patch, accuracy_per_mille, base_dir, rescale_confidence='', rescale_sigma='global', min_max_dir=None):
        self.levels = self.checked_levels(levels)
        self.patch, self.accuracy_per_mille = ev._check_patch(patch), ev._check_per_mille(accuracy_per_mille)
        super().__init__(levels, base_dir, rescale_confidence, rescale_sigma, min_max_dir)

    def fused_arguments(self):
        return {'levels': self.levels, 'patch': self.patch, 'accuracy_per_mille': self.accuracy_per_mille}

    def histogram(self, prediction, target, uncertainty):
        return ev.patch_histogram(prediction, target, uncertainty, patch=self.patch, levels=self.levels,
                                  accuracy_per_mille=self.accuracy_per_mille)[0]

    def extra_levels_columns(self):
        return [list(point or ('', '', '')) for point in ev.pavpu_curve(self.pooled)]


class RegionTablesAction(UncertaintyAction):
    """What ``ComponentsAction`` and ``LesionsAction`` share: ``levels`` and the check of ``connectivity``, a run's tables and the rows
    of its list file (one row per region: ``LIST_PLACEHOLDER``, ``LIST_HEADER``), next to the file of one row per subject."""

    SUBJECT_PLACEHOLDER = KEYS = LIST_PLACEHOLDER = LIST_HEADER = None

    def __init__(self, levels, connectivity, base_dir, rescale_confidence='', rescale_sigma='global', min_max_dir=None):
        self.levels, self.connectivity = self.checked_levels(levels), int(connectivity)
        if self.connectivity not in (6, 26):
            raise ValueError('connectivity must be 6 or 26, got {}'.format(connectivity))
        super().__init__(base_dir, rescale_confidence, rescale_sigma, min_max_dir)
        self.tables, self.list_rows = [], []

    def setup_run(self):
        self.subject_rows(self.SUBJECT_PLACEHOLDER, self.KEYS)
        self.tables, self.list_rows = [], []

    def write_list(self):
        write_table(self.path(self.LIST_PLACEHOLDER), self.LIST_HEADER, self.list_rows)


class ComponentsAction(RegionTablesAction):
    """EXTENSION (the reference has no such action): component-level uncertainty metrics from connected components labelled on the GPU
    (evaluation.component_table / component_metrics).  The uncertainty is prepared exactly like ``UeCurvesAction``'s -- the entropy of a
    probability map in registers, the rescaled map of a 'confidence' / 'sigma' run -- and there is no brain mask.  Files in
    ``<base_dir>/uncertainty``:
      eval_components_<id>.csv          one row per subject: the keys of evaluation.COMPONENT_METRIC_KEYS
      eval_components_pooled_<id>.csv   the same metrics of all subjects' tables together (whatever the batching or the subject order)
      eval_component_list_<id>.csv      one row per predicted component: subject, component (1..K in raster order of first voxels), root_index,
                                        voxels, target_voxels, mean_uncertainty, max_uncertainty, is_fp"""

    scans = ('components',)
    SUBJECT_PLACEHOLDER, KEYS, LIST_PLACEHOLDER = COMPONENTS_PLACEHOLDER, ev.COMPONENT_METRIC_KEYS, COMPONENT_LIST_PLACEHOLDER
    LIST_HEADER = ('subject', 'component', 'root_index', 'voxels', 'target_voxels', 'mean_uncertainty', 'max_uncertainty', 'is_fp')

    def fused_arguments(self):
        return {'connectivity': self.connectivity}

    def record_fused(self, res, slot, subject, n_dim):
        self.record_tables(*res['components'][slot], subject)

    def record_tables(self, pred_table, target_table, subject_name):
        """One subject's two tables: its metrics row, its components' rows, and its share of the pooled tables."""
        self.eval_cases[0].record(ev.component_metrics(pred_table, target_table, self.levels), subject_name, self.id_)
        for k, row in enumerate(pred_table):
            voxels, overlap = int(row['voxels']), int(row['other_voxels'])
            self.list_rows.append([subject_name, k + 1, int(row['root']), voxels, overlap, int(row['unc_sum']) / (voxels * ev.COMPONENT_UNC_ONE),
                                   int(row['unc_max']) / ev.COMPONENT_UNC_ONE, int(overlap == 0)])
        self.tables.append((pred_table, target_table))

    def eval_subject(self, sf, loader):
        to_eval = self.prepared(sf, loader)
        pr, tg = to_eval['prediction'], to_eval['target']
        self.record_tables(ev.component_table(pr, tg, to_eval['uncertainty'], self.connectivity)[0],
                           ev.component_table(tg, pr, None, self.connectivity)[0], sf.subject)

    def finish_eval(self):
        super().finish_eval()
        empty = np.zeros(0, dtype=ev.COMPONENT_DTYPE)
        pooled = ev.component_metrics(np.concatenate([empty] + [t[0] for t in self.tables]), np.concatenate([empty] + [t[1] for t in self.tables]),
                                      self.levels)
        self.write_pooled_row(self.path(COMPONENTS_POOLED_PLACEHOLDER), self.KEYS, pooled)
        self.write_list()


class LesionsAction(RegionTablesAction):
    """EXTENSION (the reference has no such action): lesion-wise metrics -- BraTS 2023's lesion-wise Dice, lesion F1, panoptic quality, a
    one-to-one matching and the filtering of predicted lesions by their uncertainty -- from the joint table of the predicted components and
    the target's lesions, made on the GPU (evaluation.lesion_tables / lesion_metrics).  The uncertainty is prepared exactly like
    ``ComponentsAction``'s, and there is no brain mask.  Files in ``<base_dir>/uncertainty``:
      eval_lesions_<id>.csv          one row per subject: the keys of evaluation.LESION_METRIC_KEYS
      eval_lesions_pooled_<id>.csv   the same metrics of all subjects' tables together (whatever the batching or the subject order)
      eval_lesion_list_<id>.csv      one row per kept lesion: subject and the keys of evaluation.LESION_LIST_KEYS
      eval_lesion_curve_<id>.csv     the pooled filtering curve, one row per threshold k / levels: level, threshold and the keys of
                                     evaluation.LESION_CURVE_KEYS with the components of mean uncertainty > threshold removed"""

    scans = ('lesions',)
    SUBJECT_PLACEHOLDER, KEYS, LIST_PLACEHOLDER = LESIONS_PLACEHOLDER, ev.LESION_METRIC_KEYS, LESION_LIST_PLACEHOLDER
    LIST_HEADER = ('subject',) + ev.LESION_LIST_KEYS

    def __init__(self, levels, connectivity, merge_radius, min_lesion_voxels, match_iou, base_dir, rescale_confidence='', rescale_sigma='global',
                 min_max_dir=None):
        super().__init__(levels, connectivity, base_dir, rescale_confidence, rescale_sigma, min_max_dir)
        self.merge_radius = ev._check_merge_radius(merge_radius)
        self.min_lesion_voxels, self.match_iou = int(min_lesion_voxels), float(match_iou)
        if self.min_lesion_voxels < 0:
            raise ValueError('min_lesion_voxels must be >= 0, got {}'.format(min_lesion_voxels))
        if not 0.5 <= self.match_iou < 1.0:
            raise ValueError('match_iou must be in [0.5, 1): only above an IoU of 0.5 is the matching one-to-one; got {}'.format(match_iou))

    def fused_arguments(self):
        return {'connectivity': self.connectivity, 'merge_radius': self.merge_radius}

    def record_fused(self, res, slot, subject, n_dim):
        self.record_tables(res['lesions'][slot], subject)

    def analysis(self, tables):
        return ev.lesion_analysis(tables, self.levels, self.match_iou, self.min_lesion_voxels)

    def record_tables(self, tables, subject_name):
        """One subject's ``lesion_tables`` triple: its metrics row, its lesions' rows, and its share of the pooled tables."""
        metrics, _, listed = self.analysis(tables)
        self.eval_cases[0].record(metrics, subject_name, self.id_)
        self.list_rows.extend([subject_name] + [row[k] for k in ev.LESION_LIST_KEYS] for row in listed[0])
        self.tables.append((subject_name, tables))

    def eval_subject(self, sf, loader):
        to_eval = self.prepared(sf, loader)
        self.record_tables(ev.lesion_tables(to_eval['prediction'], to_eval['target'], to_eval['uncertainty'], self.connectivity, self.merge_radius)[0],
                           sf.subject)

    def finish_eval(self):
        super().finish_eval()
        pooled, curve, _ = self.analysis([t for _, t in sorted(self.tables, key=lambda entry: entry[0])])
        self.write_pooled_row(self.path(LESIONS_POOLED_PLACEHOLDER), self.KEYS, pooled)
        self.write_list()
        write_table(self.path(LESION_CURVE_PLACEHOLDER), ['level', 'threshold'] + list(ev.LESION_CURVE_KEYS),
                    ([k, k / self.levels] + [row[key] for key in ev.LESION_CURVE_KEYS] for k, row in enumerate(curve)))


class BoundaryAction(UncertaintyAction):
    """EXTENSION (the reference prepares the border shell -- labelhelper.boarder_mask, analysis.py:54-64 -- but has no such action): where the
    errors and the uncertainty sit relative to the target's boundary, from exact distance transforms on the GPU (evaluation.boundary_table,
    surface_distance_histograms, boarder_mask).  The uncertainty is prepared exactly like ``UeCurvesAction``'s and ``ComponentsAction``'s,
    and there is no brain mask.  Files in ``<base_dir>/uncertainty``:
      eval_boundary_<id>.csv          one row per subject: evaluation.BOUNDARY_TABLE_KEYS, hd, hd95, assd, and the keys of
                                      evaluation.UE_CURVE_KEYS with the suffix _off_border: the level histogram of the voxels outside the
                                      target's border shell boarder_mask(target, 1, 1)
      eval_boundary_pooled_<id>.csv   the same metrics of the SUM of the subjects' tables and off-border histograms (integers: whatever the
                                      batching or the order; surface distances are per subject and do not pool)
      eval_boundary_bands_<id>.csv    the pooled table, one row per (side, band): side, band, voxels, errors, unc_sum, unc_err_sum and
                                      evaluation.BOUNDARY_BAND_KEYS"""

    scans = ('boundary',)
    SURFACE_KEYS = ('hd', 'hd95', 'assd')
    OFF_BORDER_KEYS = tuple(k + '_off_border' for k in ev.UE_CURVE_KEYS)
    SUBJECT_KEYS = ev.BOUNDARY_TABLE_KEYS + SURFACE_KEYS + OFF_BORDER_KEYS
    POOLED_KEYS = ev.BOUNDARY_TABLE_KEYS + OFF_BORDER_KEYS

    def __init__(self, levels, bands, base_dir, rescale_confidence='', rescale_sigma='global', min_max_dir=None):
        self.levels, self.bands = self.checked_levels(levels), int(bands)
        if not 1 <= self.bands <= ev._lib.RCU_BOUNDARY_MAX_BANDS:
            raise ValueError('bands must be in 1..{}, got {}'.format(ev._lib.RCU_BOUNDARY_MAX_BANDS, bands))
        super().__init__(base_dir, rescale_confidence, rescale_sigma, min_max_dir)
        self.pooled_table = self.pooled_hist = None

    def fused_arguments(self):
        return {'levels': self.levels, 'bands': self.bands}

    def record_fused(self, res, slot, subject, n_dim):
        self.record_boundary(*res['boundary'][slot], subject)

    def setup_run(self):
        self.subject_rows(BOUNDARY_PLACEHOLDER, self.SUBJECT_KEYS)
        self.pooled_table = np.zeros((2, self.bands + 1), dtype=ev.BOUNDARY_DTYPE)
        self.pooled_hist = np.zeros((4, self.levels), dtype=np.uint64)

    @staticmethod
    def _row(table, off_border_hist):
        metrics = ev.boundary_metrics(table)
        row = {k: metrics[k] for k in ev.BOUNDARY_TABLE_KEYS}
        curves = ev.ue_curve_metrics(off_border_hist)
        row.update({k + '_off_border': curves[k] for k in ev.UE_CURVE_KEYS})
        return row

    def record_boundary(self, table, surface_hist, off_border_hist, subject_name):
        """One subject's boundary table, surface histograms and off-border level histogram: its row, and its share of the pooled integers."""
        row = self._row(table, off_border_hist)
        surface = ev.surface_distance_metrics(surface_hist)
        row.update({k: surface[k] for k in self.SURFACE_KEYS})
        self.eval_cases[0].record({k: row[k] for k in self.SUBJECT_KEYS}, subject_name, self.id_)
        self.pooled_table = ev.add_boundary_tables([self.pooled_table, table])
        self.pooled_hist += np.asarray(off_border_hist, dtype=np.uint64)

    def eval_subject(self, sf, loader):
        to_eval = self.prepared(sf, loader)
        pr, tg, unc = to_eval['prediction'], to_eval['target'], to_eval['uncertainty']
        _, shell = ev.boarder_mask(tg, 1, 1)
        self.record_boundary(ev.boundary_table(pr, tg, unc, bands=self.bands)[0], ev.surface_distance_histograms(pr, tg)[0],
                             ev.uncertainty_histogram(pr, tg, unc, self.levels, mask=~shell)[0], sf.subject)

    def finish_eval(self):
        super().finish_eval()
        self.write_pooled_row(self.path(BOUNDARY_POOLED_PLACEHOLDER), self.POOLED_KEYS, self._row(self.pooled_table, self.pooled_hist))
        bands = ev.boundary_metrics(self.pooled_table)
        write_table(self.path(BOUNDARY_BANDS_PLACEHOLDER), ['side', 'band'] + list(ev.BOUNDARY_DTYPE.names) + list(ev.BOUNDARY_BAND_KEYS),
                    ([side, band] + [int(self.pooled_table[side, band][k]) for k in ev.BOUNDARY_DTYPE.names] +
                     [float(bands[k][side, band]) for k in ev.BOUNDARY_BAND_KEYS] for side in range(2) for band in range(self.bands + 1)))


def read_recalibration_map(path, levels):
    """The ``isotonic`` column of an ``eval_calib_levels_<id>.csv`` (another run's pooled level histogram, typically the validation run's) as a
    float64 [levels] map; a file of another number of levels is refused."""
    with open(path, newline='') as f:
        rows = list(csv.DictReader(f))
    if len(rows) != levels or [int(r['level']) for r in rows] != list(range(levels)):
        raise ValueError('{} holds {} levels, this evaluation uses {}: evaluate both runs with the same --levels'.format(path, len(rows), levels))
    return np.array([float(r['isotonic']) for r in rows], dtype=np.float64)


class CalibCurvesAction(PreparedAction):
    """EXTENSION (the reference's calibration measure is a 10-bin ECE): proper scoring rules, the Brier decomposition, equal-width /
    equal-mass / maximum / Kolmogorov-Smirnov calibration errors and a reliability curve from one calibration level histogram per subject
    (evaluation.calibration_levels / calibration_curve_metrics), prepared exactly like ``EceCalibrationAction`` -- every confidence entry,
    inside the brain mask with ``details == 'foreground'``.  Files in ``<base_dir>/calibration``:
      eval_calib_curves_<id>.csv          one row per subject: the keys of evaluation.CALIB_CURVE_KEYS
      eval_calib_curves_pooled_<id>.csv   the same metrics of the SUM of the subjects' integers (whatever the batching or the order)
      eval_calib_levels_<id>.csv          that pooled histogram, one row per level: level, threshold (the lower edge t_level, 0 for level 0),
                                          n_neg, n_pos, mean_confidence, positive_fraction (empty for an empty level), isotonic
                                          (evaluation.isotonic_levels: the monotone recalibration map fitted on this run)
    ``recalibrate_from``: such a levels file of ANOTHER run evaluated with the same ``levels``; its isotonic map adds the columns
    ``brier_recal``, ``nll_recal``, ``ece_recal`` to the two metrics files."""

    scans = ('calib_levels',)

    def __init__(self, levels, base_dir, details='', calib_bins=10, mass_bins=10, recalibrate_from=None, rescale_confidence='subject',
                 rescale_sigma='subject', min_max_dir=None):
        self.levels, self.calib_bins, self.mass_bins = int(levels), int(calib_bins), int(mass_bins)
        if not 2 <= self.levels <= ev._lib.RCU_CALIB_CURVE_MAX_LEVELS:
            raise ValueError('levels must be in 2..{}, got {}'.format(ev._lib.RCU_CALIB_CURVE_MAX_LEVELS, levels))
        if self.calib_bins < 1 or self.levels % self.calib_bins:
            raise ValueError('calib_bins = {} does not divide levels = {}'.format(calib_bins, levels))
        if self.mass_bins < 1:
            raise ValueError('mass_bins must be >= 1, got {}'.format(mass_bins))
        self.recalibration = None if recalibrate_from is None else read_recalibration_map(recalibrate_from, self.levels)
        self.keys = ev.CALIB_CURVE_KEYS + (ev.CALIB_RECAL_KEYS if self.recalibration is not None else ())
        super().__init__(ev.get_probability_preparation, CALIB_NAME, details == 'foreground', base_dir, rescale_confidence, rescale_sigma, min_max_dir)
        self.pooled_levels = self.pooled_totals = None

    def fused_arguments(self):
        return {'levels': self.levels, 'mask': self.need_mask}

    def record_fused(self, res, slot, subject, n_dim):
        self.record_levels(res['calib_levels'][slot], res['calib_totals'][slot], subject)

    def setup_run(self):
        self.subject_rows(CALIB_CURVES_PLACEHOLDER, self.keys)
        # Python integers: the pooled sum of Q(p) of a few hundred BraTS subjects can pass 2^63
        self.pooled_levels = np.zeros((3, self.levels), dtype=object)
        self.pooled_totals = np.zeros((2, 4), dtype=object)

    def metrics(self, levels, totals):
        return ev.calibration_curve_metrics(levels, totals, self.calib_bins, self.mass_bins, self.recalibration)

    def record_levels(self, levels, totals, subject_name):
        """One subject's level histogram ``[3, levels]`` and class totals ``[2, 4]``: its metrics row, and its share of the pooled integers."""
        self.eval_cases[0].record(self.metrics(levels, totals), subject_name, self.id_)
        self.pooled_levels += np.asarray(levels).astype(object)
        self.pooled_totals += np.asarray(totals).astype(object)

    def eval_subject(self, sf, loader):
        to_eval = self.prepared(sf, loader)
        levels, totals = ev.calibration_levels(to_eval['probabilities'], to_eval['target'], self.levels,
                                               mask=to_eval['mask'] if self.need_mask else None)
        self.record_levels(levels[0], totals[0], sf.subject)

    def finish_eval(self):
        super().finish_eval()
        self.write_pooled_row(self.path(CALIB_CURVES_POOLED_PLACEHOLDER), self.keys, self.metrics(self.pooled_levels, self.pooled_totals))
        thresholds = [0.0] + [float(t) for t in ev.calibration_thresholds(self.levels)]
        isotonic = ev.isotonic_levels(self.pooled_levels)
        rows = []
        for level in range(self.levels):
            n_neg, n_pos, conf = (int(v) for v in self.pooled_levels[:, level])
            n = n_neg + n_pos
            rows.append([level, thresholds[level], n_neg, n_pos, conf / (n << 32) if n else '', n_pos / n if n else '', float(isotonic[level])])
        write_table(self.path(CALIB_LEVELS_PLACEHOLDER), CALIB_LEVELS_COLUMNS, rows)


def read_agreement_csv(path):
    """``agreement.csv`` of a test run (scripts.AgreementCsvHook) -> {subject: {column: float}}."""
    if not os.path.isfile(path):
        raise FileNotFoundError('{} is missing: the agreement action reads what the default test scripts write with "others.agreement: true" '
                                '(next to others.mc) in the YAML file'.format(path))
    with open(path, newline='') as f:
        return {row['subject']: {k: float(v) for k, v in row.items() if k != 'subject'} for row in csv.DictReader(f)}


def agreement_pooled_rows(dice, scores, dice_fail):
    """Per score of ``scores`` ({name: values in subject order}): Pearson and Spearman correlation with ``dice`` and the AUROC of detecting
    ``dice < dice_fail`` by the score (evaluation.failure_auroc; NaN where undefined) -> rows (score, pearson, spearman, auroc, subjects, failed)."""
    dice = np.asarray(dice, dtype=np.float64)
    failed = dice < float(dice_fail)
    rows = []
    for name, values in scores.items():
        values = np.asarray(values, dtype=np.float64)
        rows.append([name, ev.pearson(values, dice), ev.spearman(values, dice), ev.failure_auroc(values, failed, AGREEMENT_SCORES.get(name, False)),
                     int(dice.size), int(failed.sum())])
    return rows


class AgreementAction(EvalAction):
    """EXTENSION (the reference has no such action): do the structure-wise uncertainties of the MC samples (``agreement.csv`` of the run, written
    by the default test scripts under ``others.agreement: true``) flag the failed segmentations?  Files in ``<base_dir>/uncertainty``:
      eval_agreement_<id>.csv          one row per subject: dice (prediction against ground truth), then the scores of agreement.csv
      eval_agreement_pooled_<id>.csv   one row per score: Pearson and Spearman correlation with Dice over the subjects, AUROC of detecting
                                       dice < ``dice_fail`` by the score (low agreement / high volume spread = failure; ties count half)"""

    scans = ('ue',)           # (its Dice comes from the confusion counts)

    def __init__(self, base_dir, dice_fail=0.8):
        super().__init__()
        self.dice_fail = float(dice_fail)
        self.out_dir = os.path.join(base_dir, UNCERTAINTY_NAME)
        os.makedirs(self.out_dir, exist_ok=True)
        self.table, self.dice, self.scores = {}, [], {}

    def setup_eval(self, eval_data):
        self.id_ = eval_data.id_
        self.prepare = None
        self.load_params = Loader.Params(eval_data.confidence_entry)
        self.table = read_agreement_csv(os.path.join(eval_data.eval_path, AGREEMENT_FILE))
        self.dice, self.scores = [], {k: [] for k in AGREEMENT_SCORES}
        self.eval_cases = [EvalCase(None, WriteCsvHook(self.path(AGREEMENT_PLACEHOLDER), entries=('dice',) + tuple(AGREEMENT_SCORES)))]

    def record_dice(self, dice, subject_name):
        row = self.table.get(str(subject_name))
        if row is None:
            raise ValueError('{} has no row for subject {}'.format(AGREEMENT_FILE, subject_name))
        results = {'dice': dice}
        results.update({k: row[k] for k in AGREEMENT_SCORES})
        self.eval_cases[0].record(results, subject_name, self.id_)
        self.dice.append(dice)
        for k in AGREEMENT_SCORES:
            self.scores[k].append(row[k])

    def eval_subject(self, sf, loader):
        to_eval = loader.get_data(sf, self.load_params)
        tp, _, fp, fn, _ = ev.confusion_matrx(to_eval['prediction'], to_eval['target'])
        self.record_dice(ev._dice(tp, fp, fn), sf.subject)

    def record_fused(self, res, slot, subject, n_dim):
        tp, _, fp, fn = _confusion(res, slot)
        self.record_dice(ev._dice(tp, fp, fn), subject)

    def finish_eval(self):
        super().finish_eval()
        write_table(self.path(AGREEMENT_POOLED_PLACEHOLDER),
                    ['test_id', 'score', 'pearson', 'spearman', 'auroc_dice_below_{}'.format(self.dice_fail), 'subjects', 'failed'],
                    ([self.id_] + row for row in agreement_pooled_rows(self.dice, self.scores, self.dice_fail)))


def get_actions(action_names, min_max_dir, base_dir, ece_details, levels=ev.UE_LEVELS, connectivity=26, bands=10, dice_fail=0.8, calib_bins=10,
                mass_bins=10, recalibrate_from=None, merge_radius=0, min_lesion_voxels=0, match_iou=0.5, patch=ev.PATCH_DEFAULT, patch_accuracy=500,
                rescale='minmax', quantiles=ev.QUANTILES):
    """bin-eval/eval_uncertainty.py:226-244, plus the extensions 'ue_curves' (``levels``: its number of uncertainty levels), 'components'
    (``connectivity`` 6 or 26; ``levels``: the threshold grid of its filtered Dice), 'boundary' (``bands``: its distance bands, 1..64;
    ``levels``: of its off-border level histogram) and 'calib_curves' (``levels``: of its calibration level histogram; ``calib_bins``: the
    equal-width bins of its ECE, a divisor of ``levels``; ``mass_bins``: of its equal-mass ECE; ``recalibrate_from``: the levels file of
    another run whose isotonic map is to be judged) and 'lesions' (``connectivity``, ``levels`` as 'components'; ``merge_radius``: target
    lesions closer than this Euclidean dilation are one lesion; ``min_lesion_voxels``: smaller lesions count as background; ``match_iou``:
    the IoU above which a component and a lesion match, in [0.5, 1)) and 'patches' (``patch``: the (depth, height, width) extents of its
    windows, each in 1..16; ``patch_accuracy``: a patch is accurate when more than this many per mille of its voxels are; ``levels``: of its
    patch histogram) and 'quantiles' (``quantiles``: the Q boundaries of the run's quantile table, written to ``<base_dir>/quantiles``).
    ``rescale`` = 'quantile': the actions on the prepared uncertainty -- 'bnf_ue', 'ue_curves', 'patches', 'components', 'lesions', 'boundary' --
    take the quantile rescale (evaluation.RescaleQuantile, files ``*_quantilerescale``) where they take the global min-max today ('sigma' and
    'density' entries); 'ece_dice', 'calib' and 'calib_curves' keep min-max (a rank-transformed uncertainty is uniform by construction and says
    nothing about calibration), probability-map runs and 'confidence' entries are untouched."""
    if rescale not in RESCALES:
        raise ValueError('rescale must be one of {}, got {!r}'.format(RESCALES, rescale))
    quantile_dir = os.path.join(base_dir, QUANTILES_NAME)
    uncertainty_rescale = ('subject', 'quantile' if rescale == 'quantile' else 'global', min_max_dir)
    rescale = ('subject', 'global', min_max_dir)
    table = {'minmax': lambda: SaveMinMaxAction(min_max_dir),
             'ece_dice': lambda: EceAction(base_dir, ece_details, *rescale),
             'calib': lambda: EceCalibrationAction(base_dir, ece_details, *rescale),
             'quantiles': lambda: SaveQuantilesAction(quantile_dir, quantiles, ece_details == 'foreground'),
             'bnf_ue': lambda: CorrectionAction(ev.UE_THRESHOLDS, base_dir, *uncertainty_rescale),
             'ue_curves': lambda: UeCurvesAction(levels, base_dir, *uncertainty_rescale),
             'patches': lambda: PatchesAction(levels, patch, patch_accuracy, base_dir, *uncertainty_rescale),
             'components': lambda: ComponentsAction(levels, connectivity, base_dir, *uncertainty_rescale),
             'lesions': lambda: LesionsAction(levels, connectivity, merge_radius, min_lesion_voxels, match_iou, base_dir, *uncertainty_rescale),
             'boundary': lambda: BoundaryAction(levels, bands, base_dir, *uncertainty_rescale),
             'agreement': lambda: AgreementAction(base_dir, dice_fail),      # (``dice_fail``: the Dice below which a segmentation counts as failed)
             'calib_curves': lambda: CalibCurvesAction(levels, base_dir, ece_details, calib_bins, mass_bins, recalibrate_from, *rescale)}
    actions = [table[name]() for name in action_names if name in table]
    for action in actions:
        if isinstance(action, PreparedAction):
            action.quantile_dir, action.quantiles = quantile_dir, ev._check_quantiles(quantiles)
    return actions


# ------------------------------------------------------------------------ the fused subject loop
class _ReadAhead:
    """The files of the coming subjects, read by a few threads while the current ones are evaluated (zlib releases the GIL: the .nii.gz
    streams really inflate side by side).  One task per FILE -- a subject's two to four files inflate side by side too, and the float32
    maps do not queue behind a neighbour's label images.  ``get(i)`` -> the ``to_eval`` dict of subject i (blocks until its files are in)."""

    def __init__(self, subject_files, params, depth, threads=None):
        import concurrent.futures
        if threads is None:       # gunzip is what the fused loop waits for (tools/eval_throughput.py): as many streams as the host can spare, at most 8
            threads = min(8, max(2, (os.cpu_count() or 4) // 2))
        self.subject_files, self.params, self.depth = subject_files, params, max(1, int(depth))
        self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=threads, thread_name_prefix='rcu-eval-read')
        self.futures = {}
        self.next = 0

    @staticmethod
    def _timed(fn, *args):
        t0 = time.perf_counter()
        return fn(*args), time.perf_counter() - t0

    def _tasks(self, sf):
        cats, p = sf.categories, self.params
        tasks = {p.misc_entry: (lambda path: nifti.read(path)[0], cats['misc'][p.misc_entry])}
        if p.need_target:
            tasks['target'] = (lambda path: (read_label_image(path) > 0).astype(np.uint8), cats['labels']['gt'])       # analysis.py:88-89
        if p.need_prediction:
            tasks['prediction'] = (lambda path: nifti.read(path, np.uint8)[0], cats['labels']['prediction'])
        if p.need_t2_mask:
            tasks['mask'] = (lambda path: nifti.read(path)[0] > 0, cats['images']['t2'])
        return tasks

    def _fill(self, upto):
        while self.next < min(upto, len(self.subject_files)):
            self.futures[self.next] = {key: self.pool.submit(self._timed, fn, path)
                                       for key, (fn, path) in self._tasks(self.subject_files[self.next]).items()}
            self.next += 1

    def get(self, i):
        self._fill(i + 1 + self.depth)
        entry = self.futures.pop(i)
        if isinstance(entry, _Done):
            return entry.result()
        out, read_s = {}, 0.0
        for key, future in entry.items():
            out[key], seconds = future.result()
            read_s += seconds
        out['_read_s'] = read_s
        return out

    def close(self):
        self.pool.shutdown(wait=False, cancel_futures=True)


class _LoaderAhead:
    """``Loader`` objects for the coming subjects of the reference-ordered loop, their caches filled by the reader threads: the union of what
    the run's actions will ask ``Loader.get_data`` for (one task per file, as ``_ReadAhead``)."""

    def __init__(self, subject_files, params_list, depth):
        # (the actions of a run share its confidence entry; an action that wants another one reads it itself: a cache miss in Loader)
        union = Loader.Params(params_list[0].misc_entry, need_target=False, need_prediction=False, need_t2_mask=False)
        for p in params_list:
            union.need_target |= bool(p.need_target)
            union.need_prediction |= bool(p.need_prediction)
            union.need_t2_mask |= bool(p.need_t2_mask)
            union.need_gt_dist_and_boarder |= bool(getattr(p, 'need_gt_dist_and_boarder', False))
            union.need_prediction_dist_and_boarder |= bool(getattr(p, 'need_prediction_dist_and_boarder', False))
        self.reader = _ReadAhead(subject_files, union, depth)
        self.subject_files = subject_files

    def get(self, i):
        sf = self.subject_files[i]
        loader = Loader()
        loader.cached_subject = sf.subject
        data = self.reader.get(i)
        data.pop('_read_s', None)
        loader.cached.update(data)
        return loader

    def close(self):
        self.reader.close()


SCANS = ('ece', 'minmax', 'ue', 'ue_hist', 'components', 'boundary', 'calib_levels', 'lesions', 'patches')      # the order of ``want``


def metrics_call(actions):
    """The one `evaluation.SubjectBatch.metrics` call that serves a list of actions on a probability-map run -> (its keyword arguments:
    ``want`` = the actions' scans and 'minmax', ``thresholds`` = (0.5,) unless an action fixes them, and whatever else the actions fix;
    whether the batch holds the brain mask; the arguments two actions fix differently -- with any, one call cannot serve them all)."""
    fixed, clashes = {}, set()
    for action in actions:
        for key, value in action.fused_arguments().items():
            if fixed.setdefault(key, value) != value:
                clashes.add(key)
    scans = {'minmax'}.union(*(action.scans or () for action in actions))
    fixed.pop('mask', None)       # (an argument of the batch, not of the call)
    fixed.setdefault('thresholds', (0.5,))
    return dict(fixed, want=[scan for scan in SCANS if scan in scans]), any(action.need_mask for action in actions), clashes


def _fusable(entry, actions):
    """The fused loop covers the runs whose confidence entry IS the probability map (baseline, baseline_mc, center, center_mc, ensemble:
    evaldata.py:21-47) -- no rescaling, no uncertainty-to-probability conversion -- when every action can be recorded from the scans of
    `SubjectBatch.metrics` and no two actions fix different values for one of its arguments: the batch holds one mask ('ece_dice', 'calib'
    and 'calib_curves' must agree on it), the level histograms of one call have one number of levels."""
    return entry.confidence_entry == 'probabilities' and all(a.scans is not None for a in actions) and not metrics_call(actions)[2]


def metrics_wanted(actions):
    """(`want` of evaluation.SubjectBatch.metrics, thresholds of the uncertainty-error counts, whether the batch holds a mask) for a list of
    actions on a probability-map run."""
    call, with_mask, _ = metrics_call(actions)
    return call['want'], call['thresholds'], with_mask


def record_subject(actions, subject, res, slot, n_dim):
    """Fan the metrics of subject ``slot`` of a `SubjectBatch.metrics` result out to the actions' CSV hooks -- the rows (keys, key order,
    value types) the per-action strategies of the reference-ordered loop produce."""
    mn, mx = res['min'][slot], res['max'][slot]
    # helper.add_background_probability's range check (rechun/eval/helper.py:8-12, 31-47), on the device's min / max
    if any(a.checks_range for a in actions):
        if mx > 1:
            raise ValueError('Found value larger than 1: "{}"'.format(mx))
        if mn < 0:
            raise ValueError('Found value smaller than 0: "{}"'.format(mn))
    for action in actions:
        action.record_fused(res, slot, subject, n_dim)


def _evaluate_fused(entry, actions, batch_subjects, timing):
    """All actions of a 'probabilities' run from ONE upload per subject and ONE launch per scan and batch of subjects: files read ahead by
    threads, subjects of equal size staged side by side in pinned memory, `evaluation.SubjectBatch.metrics` -- reliability histogram inside
    the mask (ece_dice and calib share it), the uncertainty-error counts of all thresholds from the probability map (their tp / tn / fp /
    fn are ece_dice's confusion matrix), min / max -- and the results fanned out to the actions' CSV hooks in subject order.  The rows are
    those of the per-action loop, byte for byte (tests/test_gpu_parity.py)."""
    call, want_mask, _ = metrics_call(actions)
    params = Loader.Params('probabilities', need_target=True, need_prediction=True, need_t2_mask=want_mask)
    files = entry.subject_files
    reader = _ReadAhead(files, params, depth=2 * batch_subjects)
    batches = {}          # voxels per subject -> SubjectBatch (datasets have one size; a mixed one gets a batch object per size)
    try:
        i = 0
        while i < len(files):
            t_start = time.perf_counter()
            first = reader.get(i)
            n_vox, n_dim = first['probabilities'].size, first['target'].ndim
            group = [(i, first)]
            while len(group) < batch_subjects and i + len(group) < len(files):
                nxt = reader.get(i + len(group))
                if nxt['probabilities'].size != n_vox:
                    reader.futures[i + len(group)] = _Done(nxt)       # another size: it opens the next batch
                    break
                group.append((i + len(group), nxt))
            t_read = time.perf_counter()
            batch = batches.get((n_vox, want_mask))
            if batch is None or batch.count < len(group):
                batch = batches[(n_vox, want_mask)] = ev.SubjectBatch(max(batch_subjects, len(group)), n_vox, with_mask=want_mask)
            batch.used = 0
            for slot, (_, d) in enumerate(group):
                batch.put(slot, d['probabilities'], d['prediction'], d['target'], d.get('mask'))
            t_stage = time.perf_counter()
            batch.upload()
            res = batch.metrics(**call)
            t_gpu = time.perf_counter()
            for slot, (k, d) in enumerate(group):
                record_subject(actions, files[k].subject, res, slot, n_dim)
            t_end = time.perf_counter()
            per = (t_end - t_start) / len(group)
            for k, d in group:
                print('[{}/{}] {} ({}s)'.format(k + 1, len(files), files[k].subject, per))
            if timing is not None:
                timing['subjects'] += len(group)
                timing['batches'] += 1
                timing['wait_for_files_s'] += t_read - t_start
                timing['read_thread_s'] += sum(d['_read_s'] for _, d in group)
                timing['stage_s'] += t_stage - t_read
                timing['upload_and_kernels_s'] += t_gpu - t_stage
                timing['csv_rows_s'] += t_end - t_gpu
            i += len(group)
    finally:
        reader.close()


class _Done:
    def __init__(self, value):
        self.value = value

    def result(self):
        return self.value


def evaluate_runs(eval_data_list, action_names, base_dir, ece_details='', fused=True, batch_subjects=8, timing=None, levels=ev.UE_LEVELS,
                  connectivity=26, bands=10, dice_fail=0.8, calib_bins=10, mass_bins=10, recalibrate_from=None, merge_radius=0, min_lesion_voxels=0,
                  match_iou=0.5, patch=ev.PATCH_DEFAULT, patch_accuracy=500, rescale='minmax', quantiles=ev.QUANTILES):
    """The subject loop of bin-eval/eval_uncertainty.py:13-50 for already collected runs.
    ``fused`` (default): runs whose confidence entry is the probability map go through ``_evaluate_fused`` -- one upload per subject shared by
    all actions, ``batch_subjects`` subjects per launch, files read ahead; the other runs (confidence / sigma entries: host-side
    rescaling recipes) and ``fused=False`` take the reference's subject-by-subject, action-by-action order.
    ``timing``: a dict that receives where the fused loop's time went (tools/eval_throughput.py); ``levels``: of the 'ue_curves' and
    'components' actions; ``connectivity``: of the 'components' action; ``bands``: of the 'boundary' action; ``calib_bins``, ``mass_bins``,
    ``recalibrate_from``: of the 'calib_curves' action; ``merge_radius``, ``min_lesion_voxels``, ``match_iou``: of the 'lesions' action, which
    shares ``levels`` and ``connectivity`` with 'components'; ``patch``, ``patch_accuracy``: of the 'patches' action; ``rescale``, ``quantiles``:
    the rescale of 'sigma' / 'density' entries in the actions on the prepared uncertainty and the Q of the 'quantiles' action (``get_actions``)."""
    actions = get_actions(action_names, os.path.join(base_dir, MINMAX_NAME), base_dir, ece_details, levels, connectivity, bands, dice_fail, calib_bins,
                          mass_bins, recalibrate_from, merge_radius, min_lesion_voxels, match_iou, patch, patch_accuracy, rescale, quantiles)
    for entry in eval_data_list:
        first = [a for a in actions if a.runs_first]
        rest = [a for a in actions if not a.runs_first]
        if entry.confidence_entry != 'probabilities' and first and rest:
            # the global and the quantile rescale of a confidence / sigma / density entry read the file the minmax / quantiles action writes for
            # this run, at set-up time: `--act minmax ue_curves` (`--act quantiles ue_curves --rescale quantile`) in ONE call runs the actions
            # that write such a file over the run first (a call without them reads an earlier call's file)
            _evaluate_entry(entry, first, fused, batch_subjects, timing)
            _evaluate_entry(entry, rest, fused, batch_subjects, timing)
        else:
            _evaluate_entry(entry, actions, fused, batch_subjects, timing)


def _evaluate_entry(entry, actions, fused, batch_subjects, timing):
    """One run through ``actions`` (evaluate_runs)."""
    for action in actions:
        action.setup_eval(entry)
    for action in actions:
        action.start_eval()
    whole = [a for a in actions if a.whole_run]
    if whole:       # actions that walk the run themselves ('quantiles': once per radix pass); the others go on as if these were not named
        for action in whole:
            action.eval_run(entry)
            action.finish_eval()
        actions = [a for a in actions if not a.whole_run]
        if not actions:
            return
    if fused and entry.subject_files and _fusable(entry, actions):
        if timing is not None:
            for key in ('subjects', 'batches', 'wait_for_files_s', 'read_thread_s', 'stage_s', 'upload_and_kernels_s', 'csv_rows_s'):
                timing.setdefault(key, 0)
        _evaluate_fused(entry, actions, max(1, int(batch_subjects)), timing)
        for action in actions:
            action.finish_eval()
        return
    # the reference's subject-by-subject, action-by-action order (eval_uncertainty.py:36-46); the files of the coming subjects are read by
    # the threads of _ReadAhead meanwhile, into the caches of the subjects' Loaders (what an action asks for first is there already)
    wanted = [a.load_params for a in actions if a.load_params is not None]
    ahead = _LoaderAhead(entry.subject_files, wanted, depth=4) if (wanted and len(entry.subject_files) > 1) else None
    try:
        for i, sf in enumerate(entry.subject_files):
            print('[{}/{}] {}'.format(i + 1, len(entry.subject_files), sf.subject), end=' ', flush=True)
            loader = ahead.get(i) if ahead is not None else Loader()
            start = time.time()
            for action in actions:
                action.eval_subject(sf, loader)
            print('({}s)'.format(time.time() - start))
    finally:
        if ahead is not None:
            ahead.close()
    for action in actions:
        action.finish_eval()
