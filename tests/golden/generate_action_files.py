"""Fixture G31: the bytes every evaluation action writes, pinned as SHA-256 digests (tests/golden/g31_action_files.json).

A `SubjectBatch.metrics` result for two subjects is put together from integers the repository already holds -- the level histograms of
G22, the component tables of G23, the boundary tables and surface distances of G24, the calibration levels of G26, the lesion tables of
G27, the patch tables of G28 (through ``patch_histogram_of_table``) -- plus hand-written min / max, reliability histograms and an
``agreement.csv``.  The actions are set up through ``get_actions``, fed through ``record_subject`` and finished; every file they wrote is
digested, ``metrics_wanted`` of the action list is recorded next to the digests.  Two sets: all eleven actions with 'foreground', and the
four actions of the reference script with '' as details.  No GPU; tests/test_action_files_cpu.py repeats the procedure and compares.

    python tests/golden/generate_action_files.py
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for path in (os.path.dirname(TESTS), TESTS):
    if path not in sys.path:
        sys.path.insert(0, path)

OUT = os.path.join(HERE, 'g31_action_files.json')
ALL_ACTIONS = ('minmax', 'ece_dice', 'calib', 'bnf_ue', 'ue_curves', 'components', 'boundary', 'agreement', 'calib_curves', 'lesions', 'patches')
REFERENCE_ACTIONS = ALL_ACTIONS[:4]
SETS = {'all': (ALL_ACTIONS, 'foreground'), 'reference': (REFERENCE_ACTIONS, '')}
PARAMETERS = dict(levels=64, connectivity=6, bands=3, dice_fail=0.8, calib_bins=8, mass_bins=5, merge_radius=2, min_lesion_voxels=0, match_iou=0.5,
                  patch=(1, 4, 4), patch_accuracy=500)
RUN_ID = 'baseline_mc'
# subject -> the case of each fixture it takes its integers from (G22 / G26, G23, G24, G27, G28); recorded in this order, which is sorted
SUBJECTS = {'Brats18_A_1': dict(voxels='a', components='d10', boundary='box', lesions='noise', patches='v0'),
            'Brats18_B_1': dict(voxels='b', components='d30', boundary='face', lesions='merge', patches='v1')}
AGREEMENT_CSV = ('subject,mean_pairwise_dice,min_pairwise_dice,pooled_pairwise_dice,iou_all,volume_cv\n'
                 'Brats18_A_1,0.9,0.8,0.91,0.7,0.05\n'
                 'Brats18_B_1,0.5,0.2,0.55,0.3,0.4\n')
# the reliability histogram of ten bins (count, sum of confidences, sum of positives) and min / max, by hand
RELIABILITY = {'Brats18_A_1': ([40, 0, 3, 5, 2, 1, 0, 4, 6, 30], [1.5, 0.0, 0.75, 1.75, 0.9, 0.55, 0.0, 3.0, 5.25, 29.0], [1, 0, 1, 1, 1, 1, 0, 3, 5, 29],
                               0.0, 1.0),
               'Brats18_B_1': ([12, 7, 0, 0, 9, 0, 0, 0, 1, 90], [0.25, 1.0, 0.0, 0.0, 4.0, 0.0, 0.0, 0.0, 0.85, 88.5], [0, 2, 0, 0, 4, 0, 0, 0, 1, 80],
                               0.015625, 0.984375)}


def subject_result(subject):
    """What `SubjectBatch.metrics` would return for a batch of this one subject (slot 0)."""
    from conftest import load_golden
    from rcu_amd import evaluation as ev
    import test_boundary_cpu
    import test_calib_curves_cpu
    import test_components_cpu
    import test_lesions_cpu
    import test_patches_cpu
    import test_ue_curves_cpu
    case, levels = SUBJECTS[subject], PARAMETERS['levels']
    g22, g23, g24, g26 = (load_golden(n) for n in ('g22_ue_curves', 'g23_components', 'g24_boundary', 'g26_calib_curves'))
    v = case['voxels']
    maps = g22[v + '_prediction'], g22[v + '_target'], g22[v + '_uncertainty']
    count, sum_conf, sum_pos, lo, hi = RELIABILITY[subject]
    calib_levels, calib_totals = test_calib_curves_cpu.numpy_calibration_levels(g26[v + '_p'], g26[v + '_target'], levels, g26[v + '_mask'])
    components = tuple(test_components_cpu.as_table(g23['{}_c6_{}_table'.format(case['components'], side)]) for side in ('pred', 'target'))
    b = case['boundary']
    boundary = (test_boundary_cpu.as_table(g24[b + '_table_r3']), test_boundary_cpu.histogram_of(g24[b + '_sq_p_to_t'], g24[b + '_sq_t_to_p']),
                test_ue_curves_cpu.numpy_histogram(*maps, levels, mask=g22[v + '_mask']))
    with np.load(test_patches_cpu.G28) as g28:
        patch_table = test_patches_cpu.fixture_table(g28, case['patches'], 1)
    return {'min': np.array([lo], dtype=np.float32), 'max': np.array([hi], dtype=np.float32),
            'hist': (np.array([count], dtype=np.int64), np.array([sum_conf], dtype=np.float64), np.array([sum_pos], dtype=np.int64)),
            'counts': g22[v + '_counts'][:1],
            'ue_hist': test_ue_curves_cpu.numpy_histogram(*maps, levels)[None],
            'components': [components],
            'boundary': [boundary],
            'calib_levels': calib_levels[None], 'calib_totals': test_calib_curves_cpu.with_nll(calib_totals)[None],
            'lesions': [test_lesions_cpu.fixture_tables(test_lesions_cpu.fixture(), case['lesions'], 6, 2)],
            'patch_hist': ev.patch_histogram_of_table(patch_table, levels, PARAMETERS['patch_accuracy'])[None]}


def digests(root):
    out = {}
    for folder, _, names in os.walk(root):
        for name in names:
            path = os.path.join(folder, name)
            with open(path, 'rb') as f:
                out[os.path.relpath(path, root).replace(os.sep, '/')] = hashlib.sha256(f.read()).hexdigest()
    return dict(sorted(out.items()))


def snapshot(work_dir):
    """-> {set name: {'metrics_wanted': [want, thresholds, want_mask], 'files': {relative path: sha256}}}, the files written under ``work_dir``."""
    from rcu_amd import evalrun
    run_dir = os.path.join(work_dir, 'run')
    os.makedirs(run_dir)
    with open(os.path.join(run_dir, evalrun.AGREEMENT_FILE), 'w') as f:
        f.write(AGREEMENT_CSV)
    results = {subject: subject_result(subject) for subject in SUBJECTS}
    out = {}
    for name, (action_names, details) in SETS.items():
        base = os.path.join(work_dir, name)
        actions = evalrun.get_actions(list(action_names), os.path.join(base, evalrun.MINMAX_NAME), base, details, **PARAMETERS)
        entry = evalrun.EvalData(RUN_ID, run_dir, 'probabilities')
        for action in actions:
            action.setup_eval(entry)
        for action in actions:
            action.start_eval()
        for subject in SUBJECTS:
            evalrun.record_subject(actions, subject, results[subject], 0, 3)
        for action in actions:
            action.finish_eval()
        want, thresholds, want_mask = evalrun.metrics_wanted(actions)
        out[name] = {'metrics_wanted': [list(want), [float(t) for t in thresholds], bool(want_mask)], 'files': digests(base)}
    return out


if __name__ == '__main__':
    with tempfile.TemporaryDirectory() as tmp:
        result = snapshot(tmp)
    with open(OUT, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote {}: {}'.format(OUT, {k: len(v['files']) for k, v in result.items()}))
