"""What the seven script functions answer to the extension keys of ``others``, alone and in pairs, against the snapshot
tests/golden/g34_script_keys.json (tests/golden/generate_script_keys.py; no GPU), which was recorded before the keys moved into the one table
``scripts._OTHERS`` and is not regenerated: the matrix is replayed and must give the recorded file byte for byte.

One declared exception.  The table has one key order (tta, mc, temperature, agreement, mc_adaptive, logit_samples, corruption, density); the
two fit scripts used to ask for logit_samples before agreement and mc_adaptive.  In the four cases ``REORDERED`` -- each run without and with
``mc: 20``, as every case of the matrix -- a run that was refused for logit_samples is now refused for the other key of the pair, with that
script's recorded single-key message for it, byte for byte.  (With ``mc: 20`` the density fit refuses mc first, then as now: those runs are
not excepted.)  No other entry may differ."""
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import generate_script_keys as gen  # noqa: E402

REORDERED = [('fit_temperature', 'agreement', 'logit_samples'), ('fit_temperature', 'mc_adaptive', 'logit_samples'),
             ('fit_density', 'agreement', 'logit_samples'), ('fit_density', 'mc_adaptive', 'logit_samples')]


def test_every_script_answers_the_keys_as_recorded(tmp_path):
    with open(gen.OUT) as f:
        text = f.read()
    recorded = json.loads(text)
    got = gen.snapshot(str(tmp_path))
    excepted = 0
    for script, key, late in REORDERED:
        answers = recorded['scripts'][script]
        for prefix in ('', 'mc+'):
            case = '{}{}+{}'.format(prefix, key, late)
            if 'others.{} '.format(late) not in answers[case]:      # (not refused for logit_samples at the time: nothing to except)
                continue
            assert answers[case] == answers[prefix + late]
            assert 'others.{} '.format(key) in answers[prefix + key] and answers[prefix + key] != answers[case]
            assert got['scripts'][script][case] == answers[prefix + key], (script, case)
            got['scripts'][script][case] = answers[case]
            excepted += 1
    assert excepted == 6      # the four cases; the temperature fit takes mc, so both of its runs of a case ask for the keys in table order
    for part in recorded:      # (named differences first: a failure then says which case moved)
        for name in recorded[part]:
            assert got[part][name] == recorded[part][name], (part, name)
    assert gen.dumps(got) == text


def test_the_snapshot_is_of_what_it_says():
    with open(gen.OUT) as f:
        recorded = json.load(f)
    assert sorted(recorded) == ['default_steps', 'runs', 'scripts'] and sorted(recorded['scripts']) == sorted(gen.SCRIPTS)
    names = sorted(gen.cases())
    assert len(names) == 2 * (1 + 7 + 21) + len(gen.VARIANTS) + 2 * len(gen.MALFORMED)
    for script in gen.SCRIPTS:
        assert sorted(recorded['scripts'][script]) == names
    for script in gen.RECORDED_RUNS:
        accepted = sorted(name for name, outcome in recorded['scripts'][script].items() if outcome == 'accepted')
        assert sorted(recorded['runs'][script]) == accepted and accepted
    assert '/tmp' not in json.dumps(recorded) and '<TMP>' in json.dumps(recorded)
