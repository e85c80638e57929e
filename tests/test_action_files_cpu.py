"""The files of all eleven evaluation actions against the snapshot tests/golden/g31_action_files.json (tests/golden/generate_action_files.py;
no GPU): a two-subject `SubjectBatch.metrics` result made of the integers of fixtures G22..G28, fanned out by ``evalrun.record_subject`` to
actions from ``evalrun.get_actions``, must give the recorded bytes -- every file name, column order and value format -- and the recorded
``metrics_wanted``.  And the fused loop is refused to action lists that do not agree on an argument of the one `metrics` call."""
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import generate_action_files as gen  # noqa: E402


def test_every_action_writes_the_recorded_bytes(tmp_path):
    with open(gen.OUT) as f:
        recorded = json.load(f)
    got = gen.snapshot(str(tmp_path))
    assert sorted(got) == sorted(recorded) == ['all', 'reference']
    for name in recorded:
        assert got[name]['metrics_wanted'] == recorded[name]['metrics_wanted'], name
        assert sorted(got[name]['files']) == sorted(recorded[name]['files']), name
        changed = [path for path, digest in recorded[name]['files'].items() if got[name]['files'][path] != digest]
        assert not changed, (name, changed)
    # the snapshot is of what it says: eleven actions' files, eleven threshold files among them, and the four reference actions' alone
    assert len(recorded['all']['files']) > len(recorded['reference']['files']) == 3 + 11
    assert recorded['all']['metrics_wanted'][0] == ['ece', 'minmax', 'ue', 'ue_hist', 'components', 'boundary', 'calib_levels', 'lesions', 'patches']
    assert recorded['all']['metrics_wanted'][2] and not recorded['reference']['metrics_wanted'][2]


def test_actions_that_disagree_on_a_metrics_argument_are_not_fused(tmp_path):
    from rcu_amd import evalrun
    base = str(tmp_path / 'eval')
    entry = evalrun.EvalData('baseline', 'unused', 'probabilities')
    for patch_levels, fusable in ((1000, False), (64, True)):
        actions = [evalrun.UeCurvesAction(64, base, 'subject', 'global', None),
                   evalrun.PatchesAction(patch_levels, (1, 4, 4), 500, base, 'subject', 'global', None)]
        for action in actions:
            action.setup_eval(entry)
        assert evalrun._fusable(entry, actions) == fusable
