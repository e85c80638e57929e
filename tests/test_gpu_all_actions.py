"""All eleven evaluation actions in one run: the fused loop (one `SubjectBatch.metrics` call per batch, its arguments merged from the
actions by ``evalrun.metrics_call``) and the plain subject-by-subject loop must write the same files with the same bytes, on subjects of
one size and two shapes; and the device-metrics hook, which takes its call from the same helper, the bytes of the four default actions."""
import os
import types

import numpy as np
import pytest
import torch

from test_gpu_ue_curves import _all_csv

pytestmark = pytest.mark.gpu
ALL_ACTIONS = ['minmax', 'ece_dice', 'calib', 'bnf_ue', 'ue_curves', 'components', 'boundary', 'agreement', 'calib_curves', 'lesions', 'patches']
# the odd shape in the middle: the first batch of two holds both shapes
SHAPES = {'Brats18_A_1': (4, 16, 20), 'Brats18_B_1': (4, 20, 16), 'Brats18_C_1': (4, 16, 20)}


def _tree(tmp_path):
    """Per subject a probability map, its prediction, a target of two blobs and a T2 image under gt/HGG/ and run/, and the run's agreement.csv."""
    from rcu_amd import evalrun, nifti
    rng = np.random.RandomState(31)
    gt_root, run_dir = tmp_path / 'gt' / 'HGG', tmp_path / 'run'
    run_dir.mkdir()
    truth, agreement = {}, ['subject,' + ','.join(evalrun.AGREEMENT_SCORES)]
    for k, (sub, shape) in enumerate(SHAPES.items()):
        (gt_root / sub).mkdir(parents=True)
        seg = np.zeros(shape, dtype=np.uint8)
        seg[1:3, 2:7, 3 + k:9 + k] = 1
        seg[0:2, 10:14, 11:15] = 4
        p = np.clip(0.7 * (seg > 0) + 0.6 * rng.rand(*shape) - 0.15, 0.0, 1.0).astype(np.float32)
        p.reshape(-1)[:3] = [0.0, 1.0, 0.5]
        pred = (p > 0.5).astype(np.uint8)
        t2 = (rng.rand(*shape) * (rng.rand(*shape) > 0.3)).astype(np.float32)
        for mod, arr in (('flair', t2), ('t1', t2), ('t2', t2), ('t1ce', t2), ('seg', seg)):
            nifti.write(str(gt_root / sub / '{}_{}.nii.gz'.format(sub, mod)), arr)
        nifti.write(str(run_dir / '{}_probabilities.nii.gz'.format(sub)), p)
        nifti.write(str(run_dir / '{}_prediction.nii.gz'.format(sub)), pred)
        truth[sub] = (p, pred, seg)
        agreement.append('{},{}'.format(sub, ','.join(str(v) for v in np.round(rng.rand(len(evalrun.AGREEMENT_SCORES)), 3))))
    (run_dir / evalrun.AGREEMENT_FILE).write_text('\n'.join(agreement) + '\n')
    return str(tmp_path / 'gt'), str(run_dir), truth


def test_fused_and_plain_loops_write_the_same_bytes_for_all_actions_and_the_hook_for_the_default_four(tmp_path):
    from rcu_amd import evalrun, scripts
    assert torch.cuda.is_available()
    gt_dir, run_dir, truth = _tree(tmp_path)
    entry = evalrun.get_eval_data('baseline_mc', run_dir, evalrun.collect_brats_ground_truth(gt_dir), expected_subjects=list(SHAPES))
    arguments = dict(levels=64, calib_bins=8, bands=3, connectivity=6, merge_radius=1, patch=(2, 4, 4))
    fused_dir, plain_dir = str(tmp_path / 'eval_fused'), str(tmp_path / 'eval_plain')
    timing = {}
    evalrun.evaluate_runs([entry], ALL_ACTIONS, fused_dir, 'foreground', batch_subjects=2, timing=timing, **arguments)
    assert (timing['subjects'], timing['batches']) == (3, 2)          # it did take the fused loop: the two shapes in one batch, then one subject
    evalrun.evaluate_runs([entry], ALL_ACTIONS, plain_dir, 'foreground', fused=False, **arguments)
    fused, plain = _all_csv(fused_dir), _all_csv(plain_dir)
    assert sorted(fused) == sorted(plain) and len(fused) == 3 + 11 + 3 + 3 + 3 + 2 + 3 + 4 + 3
    for name in fused:
        assert fused[name] == plain[name], name

    # the hook on the same maps, resident on the device, with the dataset's labels as the target and no ground-truth tree: no mask
    default_dir, hook_dir = str(tmp_path / 'eval_default'), str(tmp_path / 'eval_hook')
    evalrun.evaluate_runs([entry], ALL_ACTIONS[:4], default_dir, '')
    dev = torch.device('cuda:0')
    store = {k: {'p': torch.from_numpy(p).to(dev), 'prediction': torch.from_numpy(pred).to(dev)} for k, (p, pred, _) in enumerate(truth.values())}
    hook = scripts.DeviceMetricsHook('brats', dict(run_id='baseline_mc', out_dir=hook_dir), store)
    context = types.SimpleNamespace(test_dir=str(tmp_path), config=types.SimpleNamespace(test_name='unused'))
    hook.on_test_start(None, context)
    for k, (sub, (_, _, seg)) in reversed(list(enumerate(truth.items()))):          # (the hook sorts the subjects itself)
        hook.on_test_subject_end(types.SimpleNamespace(subject_index=k, subject_data={'subject': sub, 'labels': seg}), None, context)
    hook.on_test_end(None, context)
    from_hook, from_files = _all_csv(hook_dir), _all_csv(default_dir)
    assert sorted(from_hook) == sorted(from_files) and len(from_hook) == 14
    for name in from_hook:
        assert from_hook[name] == from_files[name], name
