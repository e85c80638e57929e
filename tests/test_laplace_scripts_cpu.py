"""The script surface of the last-layer Laplace uncertainty without a GPU: the ``others.laplace`` key of the default test scripts with its
refusals and compositions, the scripts that do not take it, the fit scripts' entry points, and the ``laplace`` / ``laplace_std`` run types of the
evaluation.  (tests/test_script_keys_cpu.py keeps the recorded answers of every script to every key that existed before.)"""
import json
import os

import numpy as np
import pytest

import laplace_reference as ref
from test_density_scripts_cpu import _context, _yaml_with

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def fit_file(tmp_path, golden):
    from rcu_amd import laplace
    g = golden('g35_laplace')
    theta = np.concatenate([g['W_32_2'], g['w0_32_2'][:, None]], 1).astype(np.float64)
    fit = laplace.fit_from_moments(*ref.moments(g['psi_32_2'], g['p32_32_2']), theta, 0.5, 'evidence', voxels=192)
    path = str(tmp_path / 'laplace.npz')
    laplace.save_laplace(fit, path)
    return path, fit


def test_the_key_is_the_last_row_and_its_absence_changes_nothing(fit_file):
    from rcu_amd import distributed as rdist
    from rcu_amd import scripts, steps
    path, fit = fit_file
    assert scripts._OTHERS[-1].name == 'laplace' and [row.name for row in scripts._OTHERS].count('laplace') == 1
    assert scripts._laplace(_context(dict())) is None and scripts._laplace(_context(dict(mc=20))) is None
    assert scripts._laplace(_context(dict(laplace_link='sample', laplace_samples=4))) is None
    plain = scripts._default_steps(_context(dict()), rdist.World())
    assert [type(s) for s in plain] == [steps.SegmentationPredictStep] and plain[0].do_probs
    for others in (dict(laplace=path), dict(laplace=path, temperature=1.5), dict(laplace=path, corruption=[dict(kind='gaussian_noise', severity=5)]),
                   dict(laplace=path, agreement=False), dict(laplace=path, device_metrics=['ece_dice'])):
        step, record = scripts._laplace(_context(others))
        assert isinstance(step, steps.LaplacePredictStep) and step.fit.A.tobytes() == fit.A.tobytes() and (step.link, step.samples) == ('probit', 0)
        assert record == dict(fit.as_dict(), file=path, link='probit', samples=0, seed=20)
        json.dumps(record)
    step, record = scripts._laplace(_context(dict(laplace=path, laplace_link='sample', laplace_samples=16), seed=7))
    assert (step.link, step.samples, step.seed) == ('sample', 16, 7) and (record['link'], record['samples'], record['seed']) == ('sample', 16, 7)
    got_steps, entries, hooks = scripts._default_plan(_context(dict(laplace=path)), rdist.World(), None, step)
    assert got_steps == [step] and entries == ('laplace_std',) and [type(h) for h in hooks] == [scripts.LaplaceStdWriteHook]
    assert scripts.LaplaceStdWriteHook.ENTRY == 'laplace_std' and scripts.DensityWriteHook.ENTRY == 'density'


@pytest.mark.parametrize('key, value', [('mc', 20), ('tta', ['identity', 'flip_h']), ('agreement', True), ('mc_adaptive', dict(check_at=[5], tolerance=0.01)),
                                        ('logit_samples', 8), ('density', 'density.npz')])
def test_the_key_does_not_compose_with_the_sampling_keys_or_density(fit_file, key, value):
    from rcu_amd import scripts
    with pytest.raises(ValueError, match='others.laplace does not compose with others.{}'.format(key)):
        scripts._laplace(_context({'laplace': fit_file[0], key: value}))


def test_a_file_or_an_option_that_cannot_be_used_is_refused_by_key(tmp_path, fit_file):
    from rcu_amd import scripts
    with pytest.raises(ValueError, match='others.laplace.*cannot be read'):
        scripts._laplace(_context(dict(laplace=str(tmp_path / 'nothing.npz'))))
    with pytest.raises(ValueError, match='others.laplace must be the path'):
        scripts._laplace(_context(dict(laplace=1.5)))
    with pytest.raises(ValueError, match='others.laplace: link must be one of probit, sample'):
        scripts._laplace(_context(dict(laplace=fit_file[0], laplace_link='logit')))
    with pytest.raises(ValueError, match="others.laplace: link='sample' needs samples >= 1"):
        scripts._laplace(_context(dict(laplace=fit_file[0], laplace_link='sample')))


def test_default_script_refuses_before_it_touches_anything(tmp_path, monkeypatch, fit_file):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    path = _yaml_with(tmp_path, '    mc: 20\n    laplace: {}\n'.format(fit_file[0]))
    with pytest.raises(ValueError, match='others.laplace does not compose with others.mc'):
        scripts.test_default('brats', path, None, device='cpu')
    assert not (tmp_path / 'out').exists()


@pytest.mark.parametrize('script', ['test_ensemble', 'test_aleatoric', 'test_auxiliary_feat', 'test_auxiliary_segm', 'fit_temperature', 'fit_density',
                                    'fit_laplace'])
def test_other_scripts_refuse_the_key(tmp_path, monkeypatch, fit_file, script):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    path = _yaml_with(tmp_path, '    model_dir: [{}]\n    laplace: {}\n'.format(tmp_path / 'train' / 'model_x', fit_file[0]))
    with pytest.raises(ValueError, match='others.laplace.*the {} script does not take it'.format(script.replace('test_', ''))):
        if script.startswith('fit_'):
            getattr(scripts, script)('brats', str(path), device='cpu')
        else:
            getattr(scripts, script)('brats', config_file=str(path), device='cpu')
    assert not (tmp_path / 'out').exists()


@pytest.mark.parametrize('others, word', [('    mc: 20\n', 'others.mc: the Laplace fit is one eval-mode pass'), ('    tta: [identity]\n', 'others.tta: the Laplace fit'),
                                          ('    corruption: gaussian_noise\n', 'others.corruption'), ('    agreement: true\n', 'others.agreement'),
                                          ('    logit_samples: 4\n', 'others.logit_samples'), ('    density: d.npz\n', 'others.density'),
                                          ('    mc_adaptive: {check_at: [5], tolerance: 0.01}\n', 'others.mc_adaptive')])
def test_fit_script_refuses_the_keys_of_other_runs(tmp_path, monkeypatch, others, word):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    with pytest.raises(ValueError, match=word):
        scripts.fit_laplace('brats', _yaml_with(tmp_path, others), device='cpu')
    assert not (tmp_path / 'out').exists()
    with pytest.raises(ValueError, match='brats'):
        scripts.fit_laplace('other', 'x.yaml')


def test_fit_script_takes_the_temperature_key_and_runs_in_one_process(tmp_path, monkeypatch):
    from rcu_amd import distributed as rdist
    from rcu_amd import scripts
    assert 'fit_laplace' in scripts._TAKEN_BY['temperature'] and 'fit_density' not in scripts._TAKEN_BY['temperature']
    scripts._check_others(_context(dict(temperature=1.5, laplace_hessian_scale=0.1, laplace_prior_precision='evidence')), 'fit_laplace', rdist.World())
    monkeypatch.setattr(scripts, '_context', lambda device, config_file: (_context(dict()), rdist.World(rank=0, world=2)))
    with pytest.raises(ValueError, match='the laplace fit runs in one process'):
        scripts.fit_laplace('brats', 'unused.yaml', device='cpu')
    assert scripts.fit_laplace.__test__ is False


@pytest.mark.parametrize('dataset', ['brats', 'isic'])
def test_entry_points_wrap_the_fit(dataset):
    text = open(os.path.join(ROOT, 'bin-dl', '{}_fit_laplace.py'.format(dataset))).read()
    assert "scripts.fit_laplace('{}', args.config_file)".format(dataset) in text and "add_argument('-config_file'" in text
    like = open(os.path.join(ROOT, 'bin-dl', '{}_fit_density.py'.format(dataset))).read()
    assert text.count('\n') == like.count('\n') and 'density' not in text


def test_laplace_and_laplace_std_are_run_types_beside_the_references():
    from rcu_amd import directories as dirs
    from rcu_amd import evalrun
    from rcu_amd import evaluation as ev
    assert evalrun.CONFIDENCE_ENTRY['laplace'] == 'probabilities' and evalrun.CONFIDENCE_ENTRY['laplace_std'] == 'laplace_std'
    assert dirs.LAPLACE_RUN_IDS == ('laplace', 'laplace_std') and not set(dirs.LAPLACE_RUN_IDS) & set(dirs.RUN_IDS) and len(dirs.RUN_IDS) == 8
    assert dirs.prediction_dir('brats', 'laplace').endswith(os.path.join('predictions', 'brats', 'laplace'))
    assert dirs.prediction_dir('isic', 'laplace_std').endswith(os.path.join('predictions', 'isic', 'laplace_std'))
    with pytest.raises(ValueError, match="unknown run id 'laplace_var': the run types are baseline, .*density, laplace, laplace_std"):
        dirs.prediction_dir('brats', 'laplace_var')
    assert 'laplace_std' in evalrun.SaveQuantilesAction.ENTRIES and 'laplace' not in evalrun.SaveQuantilesAction.ENTRIES
    # laplace_std takes sigma's path: the same rescale (global min-max), then an uncertainty
    rng = np.random.default_rng(0)
    std = (np.abs(rng.standard_normal((3, 5, 7))) * 4 + 0.1).astype(np.float32)
    mm = (float(std.min()), float(std.max()))
    as_std, id_std = ev.get_uncertainty_preparation('laplace_std', 'laplace_std', rescale_sigma='global', min_max=mm)
    as_sigma, _ = ev.get_uncertainty_preparation('sigma', 'aleatoric', rescale_sigma='global', min_max=mm)
    assert id_std == 'laplace_std_globalrescale'
    a, b = as_std({'laplace_std': std.copy()})['uncertainty'], as_sigma({'sigma': std.copy()})['uncertainty']
    assert np.array_equal(a, b) and 0.0 <= float(a.min()) < 1e-3 and 1.0 - 1e-3 < float(a.max()) <= 1.0
    # laplace is a probabilities run: the entropy of the predictive, no rescale
    _, id_p = ev.get_uncertainty_preparation(evalrun.CONFIDENCE_ENTRY['laplace'], 'laplace', rescale_sigma='global', min_max=mm)
    assert id_p == 'laplace'
    import importlib.util
    spec = importlib.util.spec_from_file_location('eval_uncertainty_cli', os.path.join(ROOT, 'bin-eval', 'eval_uncertainty.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert 'laplace_std' in cli.make_parser().format_help()


@pytest.mark.parametrize('hook_name, key, entry', [('DensityWriteHook', 'density', 'density'), ('LaplaceStdWriteHook', 'laplace', 'laplace_std')])
def test_the_map_hooks_write_their_entry_under_its_name(tmp_path, hook_name, key, entry):
    """The density hook's file name, bytes and error text after it was given a KEY and an ENTRY, and the Laplace hook beside it."""
    import types
    from rcu_amd import nifti, scripts
    hook = getattr(scripts, hook_name)(in_background=False)
    assert (hook.KEY, hook.ENTRY) == (key, entry)
    values = np.arange(2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4, 1) / 7.0
    props = nifti.ImageProperties((4, 3, 2), (1.0, -2.0, 3.0), (1.0, 1.0, 2.5))
    context = types.SimpleNamespace(test_dir=str(tmp_path))
    subject = types.SimpleNamespace(subject_index=5, subject_data={'subject': 'S1', 'properties': props, entry: values, 'probabilities': values})
    hook.on_test_subject_end(subject, None, context)
    hook.on_termination(context)
    assert os.listdir(tmp_path) == ['S1_{}.nii.gz'.format(entry)]
    got, rprops = nifti.read(str(tmp_path / 'S1_{}.nii.gz'.format(entry)))
    assert got.dtype == np.float32 and rprops == props and got.tobytes() == values[..., 0].astype(np.float32).tobytes()
    with pytest.raises(ValueError, match='others.{}: subject 5 came without its {} map'.format(key, entry)):
        hook.on_test_subject_end(types.SimpleNamespace(subject_index=5, subject_data={'subject': 'S1'}), None, context)
    record = scripts.LaplaceRecordHook(dict(tau=2.0))
    record.end_startup(types.SimpleNamespace(test_dir=str(tmp_path), writes_output=True))
    assert json.load(open(tmp_path / 'laplace.json')) == {'tau': 2.0}
