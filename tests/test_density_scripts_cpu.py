"""The script surface of the feature-space density without a GPU: the ``others.density`` key of the default test scripts and its refusals, the
scripts that do not take it, the fit scripts' entry points, and the ``density`` run type of the evaluation."""
import os

import numpy as np
import pytest

from test_script_surface_cpu import _write_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _context(others, seed=20):
    from rcu_amd import config as cfg
    from rcu_amd import loops
    context = loops.TorchTestContext('cpu')
    context.config = cfg.TestConfiguration()
    context.config.seed = seed
    context.config.others = cfg.OtherParameters().from_dict(others)
    return context


@pytest.fixture()
def fit_file(tmp_path, golden):
    from rcu_amd import density
    g = golden('g32_density')
    fit = density.fit_from_moments(g['n_32'], g['S_32'], g['G_32'])
    path = str(tmp_path / 'density.npz')
    density.save_density(fit, path)
    return path, fit


def _yaml_with(tmp_path, others_text):
    path = _write_cfg(tmp_path)
    text = open(path).read()
    assert '  others:\n    mc: 20\n' in text
    with open(path, 'w') as f:
        f.write(text.replace('  others:\n    mc: 20\n', '  others:\n' + others_text))
    return path


def test_the_key_loads_the_fit_and_its_absence_changes_nothing(fit_file):
    from rcu_amd import density, scripts, steps
    from rcu_amd import distributed as rdist
    path, fit = fit_file
    assert scripts._density(_context(dict())) is None and scripts._density(_context(dict(mc=20))) is None
    plain = scripts._default_steps(_context(dict()), rdist.World())
    assert [type(s) for s in plain] == [steps.SegmentationPredictStep] and plain[0].do_probs
    for others in (dict(density=path), dict(density=path, temperature=1.5), dict(density=path, corruption=[dict(kind='gaussian_noise', severity=5)]),
                   dict(density=path, agreement=False)):
        got = scripts._density(_context(others))
        assert isinstance(got, density.DensityFit) and got.A.tobytes() == fit.A.tobytes() and got.k.tobytes() == fit.k.tobytes()
    step = steps.DensityPredictStep(fit)
    assert step.fit is fit
    hook = scripts.DensityWriteHook()
    assert type(hook).on_test_subject_end is not scripts.loops.TestLoopHook.on_test_subject_end


@pytest.mark.parametrize('key, value', [('mc', 20), ('tta', ['identity', 'flip_h']), ('agreement', True), ('mc_adaptive', dict(check_at=[5], tolerance=0.01)),
                                        ('logit_samples', 8)])
def test_the_key_does_not_compose_with_the_sampling_keys(fit_file, key, value):
    from rcu_amd import scripts
    with pytest.raises(ValueError, match='others.density') as e:
        scripts._density(_context({'density': fit_file[0], key: value}))
    assert 'others.{}'.format(key) in str(e.value)


def test_a_density_file_that_cannot_be_read_is_refused_by_key(tmp_path):
    from rcu_amd import scripts
    with pytest.raises(ValueError, match='others.density.*cannot be read'):
        scripts._density(_context(dict(density=str(tmp_path / 'nothing.npz'))))
    with pytest.raises(ValueError, match='others.density must be the path'):
        scripts._density(_context(dict(density=1.5)))


def test_default_script_refuses_before_it_touches_anything(tmp_path, monkeypatch, fit_file):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    path = _yaml_with(tmp_path, '    mc: 20\n    density: {}\n'.format(fit_file[0]))
    with pytest.raises(ValueError, match='others.density does not compose with others.mc'):
        scripts.test_default('brats', path, None, device='cpu')
    assert not (tmp_path / 'out').exists()


@pytest.mark.parametrize('script', ['test_ensemble', 'test_aleatoric', 'test_auxiliary_feat', 'test_auxiliary_segm', 'fit_temperature', 'fit_density'])
def test_other_scripts_refuse_the_key(tmp_path, monkeypatch, fit_file, script):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    path = _yaml_with(tmp_path, '    model_dir: [{}]\n    density: {}\n'.format(tmp_path / 'train' / 'model_x', fit_file[0]))
    with pytest.raises(ValueError, match='others.density.*the {} script does not take it'.format(script.replace('test_', ''))):
        if script.startswith('fit_'):
            getattr(scripts, script)('brats', str(path), device='cpu')
        else:
            getattr(scripts, script)('brats', config_file=str(path), device='cpu')
    assert not (tmp_path / 'out').exists()


@pytest.mark.parametrize('others, word', [('    mc: 20\n', 'others.mc'), ('    tta: [identity]\n', 'others.tta'), ('    temperature: 1.5\n', 'others.temperature'),
                                          ('    corruption: gaussian_noise\n', 'others.corruption'), ('    agreement: true\n', 'others.agreement'),
                                          ('    logit_samples: 4\n', 'others.logit_samples'),
                                          ('    mc_adaptive: {check_at: [5], tolerance: 0.01}\n', 'others.mc_adaptive')])
def test_fit_script_refuses_the_keys_the_temperature_fit_refuses(tmp_path, monkeypatch, others, word):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    with pytest.raises(ValueError, match=word):
        scripts.fit_density('brats', _yaml_with(tmp_path, others), device='cpu')
    assert not (tmp_path / 'out').exists()
    with pytest.raises(ValueError, match='brats'):
        scripts.fit_density('other', 'x.yaml')


def test_fit_script_runs_in_one_process(tmp_path, monkeypatch):
    from rcu_amd import distributed as rdist
    from rcu_amd import scripts
    monkeypatch.setattr(scripts, '_context', lambda device, config_file: (_context(dict()), rdist.World(rank=0, world=2)))
    with pytest.raises(ValueError, match='one process'):
        scripts.fit_density('brats', 'unused.yaml', device='cpu')
    assert scripts.fit_density.__test__ is False


@pytest.mark.parametrize('dataset', ['brats', 'isic'])
def test_entry_points_wrap_the_fit(dataset):
    text = open(os.path.join(ROOT, 'bin-dl', '{}_fit_density.py'.format(dataset))).read()
    assert "scripts.fit_density('{}', args.config_file)".format(dataset) in text and "add_argument('-config_file'" in text
    like = open(os.path.join(ROOT, 'bin-dl', '{}_fit_temperature.py'.format(dataset))).read()
    assert text.count('\n') == like.count('\n')


def test_density_is_a_run_type_beside_the_references():
    from rcu_amd import directories as dirs
    from rcu_amd import evalrun
    from rcu_amd import evaluation as ev
    assert evalrun.CONFIDENCE_ENTRY['density'] == 'density' and evalrun.CONFIDENCE_ENTRY['aleatoric'] == 'sigma'
    assert 'density' not in dirs.RUN_IDS and len(dirs.RUN_IDS) == 8 and dirs.EXTENSION_RUN_IDS == ('density',)
    assert dirs.prediction_dir('brats', 'density').endswith(os.path.join('predictions', 'brats', 'density'))
    # it takes sigma's path: the same rescale (global min-max), then an uncertainty -- and the same for the calibration actions
    rng = np.random.default_rng(0)
    energy = (rng.standard_normal((3, 5, 7)) * 40 + 60).astype(np.float32)
    mm = (float(energy.min()), float(energy.max()))
    as_density, id_density = ev.get_uncertainty_preparation('density', 'density', rescale_sigma='global', min_max=mm)
    as_sigma, id_sigma = ev.get_uncertainty_preparation('sigma', 'aleatoric', rescale_sigma='global', min_max=mm)
    assert (id_density, id_sigma) == ('density_globalrescale', 'aleatoric_globalrescale')
    a, b = as_density({'density': energy.copy()})['uncertainty'], as_sigma({'sigma': energy.copy()})['uncertainty']
    assert np.array_equal(a, b) and 0.0 <= float(a.min()) < 1e-3 and 1.0 - 1e-3 < float(a.max()) <= 1.0
    pa, ida = ev.get_probability_preparation('density', 'density', rescale_sigma='subject')
    pb, _ = ev.get_probability_preparation('sigma', 'aleatoric', rescale_sigma='subject')
    assert ida == 'density_rescale'
    prediction = (rng.random(energy.shape) < 0.4).astype(np.uint8)
    assert np.array_equal(pa({'density': energy.copy(), 'prediction': prediction})['probabilities'],
                          pb({'sigma': energy.copy(), 'prediction': prediction})['probabilities'])
