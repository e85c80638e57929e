"""Fixture G34: what the seven script functions of rcu_amd.scripts answer to the extension keys of the YAML file's ``others``, alone and in
pairs (tests/golden/g34_script_keys.json).  Recorded once, before the keys moved into one table, and not regenerated since.

Every case is a BraTS YAML file whose ``test_dir`` and ``model_dir`` lie under a work directory and do not exist, run with ``device='cpu'`` in
one process.  The cases: every subset of size 0, 1 and 2 of {tta, temperature, agreement: true, mc_adaptive, logit_samples, density,
corruption}, each without and with ``mc: 20``; ``agreement: false`` and ``exact: false`` beside mc + mc_adaptive (and ``agreement: false`` alone
and beside density); a malformed value of every key that validates its value, without and with ``mc: 20``.

    'scripts'        script -> case -> the exception's class and message when it is raised while ``<work>/out`` does not exist (the work directory
                     written as <TMP>), else the word ``accepted``: what happens once the directory exists depends on data that is not there
    'runs'           test_default / test_aleatoric -> accepted case -> what the script hands to ``scripts._run`` (replaced by a recorder for
                     the call): the class names of the batch steps, the entries, the class names of the startup and the per-subject hooks
    'default_steps'  ``scripts._default_steps`` called directly, in one process and as rank 0 of 2 -> class names, or class and message

No GPU; tests/test_script_keys_cpu.py repeats the procedure and compares.

    python tests/golden/generate_script_keys.py
"""
import itertools
import json
import logging
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for path in (os.path.dirname(TESTS), TESTS):
    if path not in sys.path:
        sys.path.insert(0, path)

OUT = os.path.join(HERE, 'g34_script_keys.json')
SCRIPTS = ('test_default', 'test_ensemble', 'test_aleatoric', 'test_auxiliary_feat', 'test_auxiliary_segm', 'fit_temperature', 'fit_density')
RECORDED_RUNS = ('test_default', 'test_aleatoric')
YAML = """
config:
  test_name: brats_test_x
  test_dir: {work}/out
  model_dir: {work}/train/model_x
  seed: 20
  test_at: best
  others:
    model_dir: {model_dir}
    test_at: best
{others}meta:
  type: test-config
  version: 0
"""
# key -> its line in ``others`` ({work}: the work directory, where density.npz is written from fixture G32)
KEYS = {'tta': 'tta: [identity, flip_h]', 'temperature': 'temperature: 1.5', 'agreement': 'agreement: true',
        'mc_adaptive': 'mc_adaptive: {{check_at: [5, 10], tolerance: 0.01, max_unsettled: 0}}', 'logit_samples': 'logit_samples: 10',
        'density': 'density: {work}/density.npz', 'corruption': 'corruption: {{kind: gaussian_noise, severity: 3}}'}
MC = 'mc: 20'
VARIANTS = {'mc+mc_adaptive+agreement_false': [MC, KEYS['mc_adaptive'], 'agreement: false'],
            'mc+mc_adaptive+exact_false': [MC, KEYS['mc_adaptive'], 'exact: false'],
            'agreement_false': ['agreement: false'], 'density+agreement_false': [KEYS['density'], 'agreement: false']}
MALFORMED = {'temperature_negative': 'temperature: -2.0', 'temperature_no_file': 'temperature: {work}/none.json', 'agreement_no_bool': 'agreement: 3',
             'mc_adaptive_no_dict': 'mc_adaptive: [5, 10]', 'mc_adaptive_first_checkpoint': 'mc_adaptive: {{check_at: [1], tolerance: 0.01}}',
             'logit_samples_zero': 'logit_samples: 0', 'density_no_file': 'density: {work}/nothing.npz', 'density_no_path': 'density: 1.5',
             'corruption_kind': 'corruption: {{kind: fog, severity: 1}}', 'corruption_bare_name': 'corruption: gaussian_noise'}
# scripts._default_steps called directly: the ``others`` of the context
DIRECT = {'plain': dict(), 'mc': dict(mc=20), 'tta': dict(tta=['identity', 'flip_h']), 'mc+tta': dict(mc=20, tta=['identity', 'flip_h']),
          'mc+agreement': dict(mc=20, agreement=True), 'agreement': dict(agreement=True), 'tta+agreement': dict(tta=['identity'], agreement=True),
          'mc+mc_adaptive': dict(mc=20, mc_adaptive=dict(check_at=[5, 10], tolerance=0.01, max_unsettled=0)),
          'mc_adaptive': dict(mc_adaptive=dict(check_at=[5, 10], tolerance=0.01, max_unsettled=0))}


def cases():
    """-> {case name: the lines of ``others``}"""
    out = {}
    for size in (0, 1, 2):
        for subset in itertools.combinations(KEYS, size):
            for mc in (False, True):
                out['+'.join((('mc',) if mc else ()) + subset) or 'none'] = ([MC] if mc else []) + [KEYS[k] for k in subset]
    out.update(VARIANTS)
    for name, line in MALFORMED.items():
        out[name] = [line]
        out['mc+' + name] = [MC, line]
    return out


def _names(items):
    return [type(item).__name__ for item in items]


def _error(e, work_dir):
    return '{}: {}'.format(type(e).__name__, e).replace(work_dir, '<TMP>')


def _write_density(work_dir):
    import numpy as np
    from rcu_amd import density
    with np.load(os.path.join(HERE, 'g32_density.npz')) as g:
        density.save_density(density.fit_from_moments(g['n_32'], g['S_32'], g['G_32']), os.path.join(work_dir, 'density.npz'))


def run_case(script, lines, work_dir):
    """-> (outcome, what ``_run`` was handed or None)"""
    from rcu_amd import scripts
    out_dir, seen = os.path.join(work_dir, 'out'), {}
    model_dir = os.path.join(work_dir, 'train', 'model_x')
    path = os.path.join(work_dir, 'test_brats_x.yaml')
    with open(path, 'w') as f:
        f.write(YAML.format(work=work_dir, model_dir='[{}]'.format(model_dir) if script == 'test_ensemble' else model_dir,
                            others=''.join('    {}\n'.format(line.format(work=work_dir)) for line in lines)))

    def recorder(context, dataset, test_steps, write_hook, entries, world=None, startup_hooks=(), subject_hooks=()):
        seen.update(test_steps=_names(test_steps), entries=None if entries is None else list(entries), startup_hooks=_names(startup_hooks),
                    subject_hooks=_names(subject_hooks))
        return context

    real_run, handlers = scripts._run, list(logging.getLogger().handlers)
    if script in RECORDED_RUNS:
        scripts._run = recorder
    try:
        if script.startswith('fit_'):
            getattr(scripts, script)('brats', path, device='cpu')
        else:
            getattr(scripts, script)('brats', config_file=path, device='cpu')
        outcome = 'accepted'
    except Exception as e:  # noqa: BLE001 - the outcome is what is recorded
        outcome = 'accepted' if os.path.exists(out_dir) else _error(e, work_dir)
    finally:
        scripts._run = real_run
        for handler in [h for h in logging.getLogger().handlers if h not in handlers]:      # (the log file of a run that got as far as its directory)
            logging.getLogger().removeHandler(handler)
            handler.close()
        shutil.rmtree(out_dir, ignore_errors=True)
    return outcome, (seen if seen else None)


def direct_steps(others, world):
    from rcu_amd import config as cfg
    from rcu_amd import loops, scripts
    context = loops.TorchTestContext('cpu')
    context.config = cfg.TestConfiguration()
    context.config.seed = 20
    context.config.others = cfg.OtherParameters().from_dict(others)
    try:
        return _names(scripts._default_steps(context, world))
    except Exception as e:  # noqa: BLE001
        return '{}: {}'.format(type(e).__name__, e)


def snapshot(work_dir):
    from rcu_amd import distributed as rdist
    work_dir = os.path.realpath(work_dir)
    saved = {key: os.environ.pop(key) for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK') if key in os.environ}
    try:
        _write_density(work_dir)
        out = {'scripts': {}, 'runs': {script: {} for script in RECORDED_RUNS}, 'default_steps': {}}
        for script in SCRIPTS:
            out['scripts'][script] = {}
            for name, lines in cases().items():
                outcome, run = run_case(script, lines, work_dir)
                out['scripts'][script][name] = outcome
                if script in RECORDED_RUNS and outcome == 'accepted':
                    out['runs'][script][name] = run
        for name, others in DIRECT.items():
            out['default_steps'][name] = {'world_1': direct_steps(dict(others), rdist.World()),
                                          'rank_0_of_2': direct_steps(dict(others), rdist.World(rank=0, world=2))}
    finally:
        os.environ.update(saved)
    return out


def dumps(result):
    return json.dumps(result, indent=1, sort_keys=True) + '\n'


if __name__ == '__main__':
    if os.path.exists(OUT):
        sys.exit('{} exists: it was recorded before the keys moved into one table and is not regenerated'.format(OUT))
    with tempfile.TemporaryDirectory() as tmp:
        result = snapshot(tmp)
    with open(OUT, 'w') as f:
        f.write(dumps(result))
    print('wrote {}: {}'.format(OUT, {script: len(v) for script, v in result['scripts'].items()}))
