#!/usr/bin/env python3
"""Evaluation driver with the reference's command line (bin-eval/eval_uncertainty.py:248-251): --ds --ids --act, nothing else
required.  The directories come from rcu_amd.directories, the mirror of the reference's rechun/directories.py whose
"required to be set" entries can be given in the environment (RCU_BRATS_ORIG_DATA_DIR, RCU_BRATS_BASELINE_MC_PREDICT, ...)
instead of by editing the module; --pred_dir / --gt_dir / --out_dir override them per call."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _int_in(lo, hi):
    """argparse type: an integer in lo..hi (anything else is a usage error)."""
    def parse(text):
        value = int(text)
        if not lo <= value <= hi:
            raise argparse.ArgumentTypeError('must be in {}..{}, got {}'.format(lo, hi, value))
        return value
    return parse


def make_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--ds', type=str, nargs='?', help='the dataset to evaluate the runs on')
    parser.add_argument('--ids', type=str, nargs='*', help='the ids of the runs to be evaluated (default: the reference\'s eight; rcu_amd only, when '
                        'named: density -- a default run under others.density, whose <subject>_density.nii.gz is rescaled like the aleatoric sigma, '
                        'run minmax first; laplace laplace_std -- a default run under others.laplace as a probabilities run on the predictive and as its '
                        '<subject>_laplace_std.nii.gz, rescaled like sigma; knn -- a default run under others.knn, whose <subject>_knn.nii.gz is rescaled like sigma)')
    parser.add_argument('--act', type=str, nargs='*', help='the names of the evaluation configuration: minmax, ece_dice, calib, bnf_ue (the default: '
                        'all four) and, rcu_amd only, ue_curves (threshold-free uncertainty-error metrics from a level histogram) components '
                        '(component-level metrics from connected components: false-positive detection by mean uncertainty, filtered Dice) and '
                        'boundary (errors and uncertainty by distance to the target\'s boundary, surface distances, metrics off the border shell), agreement '
                        '(the run\'s agreement.csv -- written under others.agreement: true -- against each subject\'s Dice: correlations, failure detection) and lesions '
                        '(lesion-wise Dice, lesion F1, panoptic quality and the filtering of predicted lesions by uncertainty, from the joint table of '
                        'predicted components and target lesions) and patches (patch accuracy vs. patch uncertainty of Mukhoti & Gal 2018 -- p(accurate | certain), '
                        'p(uncertain | inaccurate), PAvPU -- over a grid of non-overlapping windows, from a patch table made on the GPU) and quantiles '
                        '(the sibling of minmax for --rescale quantile: the exact quantile table of a sigma / density run, by radix selection on the GPU)')
    parser.add_argument('--pred_dir', type=str, default=None, help='root with one sub-directory per dataset and run id '
                        '(default: directories.PREDICT_DIR and the per-run *_PREDICT names)')
    parser.add_argument('--gt_dir', type=str, default=None, help='BraTS training tree / ISIC dataset prefix '
                        '(default: directories.BRATS_ORIG_DATA_DIR / ISIC_PREPROCESSED_TEST_DATA_DIR)')
    parser.add_argument('--out_dir', type=str, default=None, help='default: directories.EVAL_DIR')
    parser.add_argument('--batch_subjects', type=int, default=8, help='rcu_amd: subjects of a probability-map run evaluated per GPU launch')
    parser.add_argument('--levels', type=int, default=1000, help='rcu_amd: uncertainty levels of the ue_curves action and threshold grid of the '
                        'components and lesions actions and levels of the patch histogram of the patches action (2..4096)')
    parser.add_argument('--connectivity', type=int, default=26, choices=(6, 26), help='rcu_amd: neighbourhood of the components and lesions actions (2-D images: 4 / 8)')
    parser.add_argument('--merge_radius', type=int, default=0, help='rcu_amd: the lesions action counts target components closer than this Euclidean '
                        'dilation (in voxels) as one lesion; 0: the target\'s components')
    parser.add_argument('--min_lesion_voxels', type=int, default=0, help='rcu_amd: the lesions action treats target lesions with fewer voxels as background')
    parser.add_argument('--match_iou', type=float, default=0.5, help='rcu_amd: the lesions action matches a predicted component and a lesion whose IoU '
                        'is above this, in [0.5, 1)')
    parser.add_argument('--bands', type=int, default=10, help='rcu_amd: distance bands of the boundary action (1..64)')
    parser.add_argument('--dice_fail', type=float, default=0.8, help='rcu_amd: the agreement action counts a subject with Dice below this as a failed '
                        'segmentation')
    parser.add_argument('--calib_bins', type=int, default=10, help='rcu_amd: equal-width bins of the ECE / MCE of the calib_curves action (--act calib_curves: '
                        'Brier, NLL, Brier decomposition, equal-width / equal-mass / maximum / Kolmogorov-Smirnov calibration errors and a reliability '
                        'curve from a histogram of --levels levels); must divide --levels')
    parser.add_argument('--mass_bins', type=int, default=10, help='rcu_amd: equal-mass bins of the calib_curves action')
    parser.add_argument('--recalibrate_from', type=str, default=None, help='rcu_amd: an eval_calib_levels_<id>.csv of another run (the validation run, '
                        'evaluated with the same --levels): the calib_curves action also reports Brier, NLL and ECE under that run\'s isotonic map')
    parser.add_argument('--patch', type=_int_in(1, 16), default=4, help='rcu_amd: in-plane edge of the windows of the patches action, in voxels (1..16)')
    parser.add_argument('--patch_depth', type=_int_in(1, 16), default=1, help='rcu_amd: depth of the windows of the patches action in slices (1..16); the '
                        'default 1 gives windows on the slices a 2-D network saw, --patch_depth 4 with --patch 4 gives cubes')
    parser.add_argument('--patch_accuracy', type=_int_in(0, 999), default=500, help='rcu_amd: the patches action counts a window as accurate when more '
                        'than this many per mille of its voxels are predicted correctly (0..999)')
    parser.add_argument('--rescale', type=str, default='minmax', choices=('minmax', 'quantile'), help='rcu_amd: how the unbounded entries (the sigma of '
                        'an aleatoric run, the energy of a density run) reach [0, 1] in bnf_ue, ue_curves, patches, components, lesions and boundary. '
                        'minmax (the default): the reference\'s global min-max from the file of --act minmax, files *_globalrescale. quantile: the '
                        'rank transform of the run from the table of --act quantiles (run it first, or name it in the same call), files '
                        '*_quantilerescale: every level holds an equal share of the voxels, whatever the outliers. ece_dice, calib and calib_curves keep '
                        'min-max under either value (a rank-transformed uncertainty is uniform by construction and says nothing about calibration); '
                        'probability-map runs and confidence entries are untouched')
    parser.add_argument('--quantiles', type=_int_in(2, 4096), default=1000, help='rcu_amd: the Q boundaries of the table --act quantiles writes '
                        '(<out>/quantiles/eval_quantiles_<id>.csv: the exact k/Q quantiles of the run inside the T2 brain mask for BraTS, over all pixels '
                        'for ISIC) and --rescale quantile expects (2..4096); choose --levels equal to it and every level gets its share')
    parser.add_argument('--plain', action='store_true', help='rcu_amd: the reference\'s subject-by-subject, action-by-action loop for every run')
    return parser


if __name__ == '__main__':
    args = make_parser().parse_args()
    from rcu_amd import directories as dirs
    from rcu_amd import scripts
    ds = args.ds or 'brats'
    ids = args.ids or list(dirs.RUN_IDS)
    acts = args.act or ['minmax', 'ece_dice', 'calib', 'bnf_ue']
    print('\n**************************************')
    print('dataset: {}'.format(ds))
    print('to_evaluate: {}'.format(ids))
    print('eval_actions: {}'.format(acts))
    print('**************************************\n')
    if ds not in ('brats', 'isic'):
        raise ValueError('chose "brats" or "isic" as dataset')          # eval_uncertainty.py:27-28
    gt_dir = args.gt_dir or dirs.ground_truth_dir(ds)
    if not gt_dir:
        raise SystemExit('the ground-truth directory is not set: export RCU_BRATS_ORIG_DATA_DIR (the reference asks for the same '
                         'entry in rechun/directories.py:7) or pass --gt_dir')
    runs = {i: (os.path.join(args.pred_dir, ds, i) if args.pred_dir else dirs.prediction_dir(ds, i)) for i in ids}
    out_dir = os.path.join(args.out_dir, ds) if args.out_dir else dirs.eval_dir(ds)
    scripts.eval_uncertainty(ds, runs, gt_dir, out_dir, acts, fused=not args.plain, batch_subjects=args.batch_subjects,
                             levels=args.levels, connectivity=args.connectivity, bands=args.bands, dice_fail=args.dice_fail,
                             calib_bins=args.calib_bins, mass_bins=args.mass_bins, recalibrate_from=args.recalibrate_from,
                             merge_radius=args.merge_radius, min_lesion_voxels=args.min_lesion_voxels, match_iou=args.match_iou,
                             patch=(args.patch_depth, args.patch, args.patch), patch_accuracy=args.patch_accuracy,
                             rescale=args.rescale, quantiles=args.quantiles)
