"""The quantile rescale without a GPU (include/rcu.h "Quantile rescale"): the integer-numpy reference against fixture G33
(tests/golden/generate_quantiles.py), the key's order, the host side of the selection (``evaluation.quantile_refine``) on numpy-made
histograms, the level counts, the CSV file, the (l + 0.5) / Q -> level identity, and the driver's flags and refusals."""
import csv
import importlib.util
import os

import numpy as np
import pytest

import quantile_reference as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ('normal', 'lognormal', 'ties', 'special', 'small', 'equal')
PLANS = ((16, 16), (12, 10, 10), (8, 8, 8, 8))


def case(g, name):
    return g[name + '_maps'], g.get(name + '_mask'), int(g[name + '_Q'])


@pytest.fixture(scope='module')
def g33(golden):
    return golden('g33_quantiles')


@pytest.mark.parametrize('name', CASES)
def test_reference_reproduces_the_fixture(g33, name):
    maps, mask, q = case(g33, name)
    n, ranks, keys = qr.table(qr.population_keys(maps, mask), q)
    assert n == int(g33[name + '_N']) and np.array_equal(ranks, g33[name + '_ranks']) and np.array_equal(keys, g33[name + '_keys'])
    assert keys.dtype == np.uint32 and np.all(np.diff(keys.astype(np.int64)) >= 0)
    levels = qr.levels(qr.key(maps.reshape(-1)), keys).reshape(maps.shape)
    assert np.array_equal(levels, g33[name + '_levels']) and levels.min() >= 0 and levels.max() <= q - 1
    rescaled = qr.rescaled(levels, q)
    assert rescaled.dtype == np.float32 and np.array_equal(rescaled.view(np.uint32), g33[name + '_rescaled'].view(np.uint32))
    assert 0 < rescaled.min() and rescaled.max() < 1


def test_the_fixture_holds_the_cases_the_issue_names(g33):
    assert g33['lognormal_maps'].max() == np.float32(1e6) and not g33['lognormal_mask'][2].any() and g33['lognormal_mask'][0].any()
    ties = g33['ties_maps']
    assert 0.8 < float((ties == np.float32(0.125)).mean()) < 0.9
    special = g33['special_maps'].reshape(-1)
    assert np.isinf(special).sum() >= 2 and np.signbit(special[special == 0]).any() and not np.signbit(special[special == 0]).all()
    assert ((np.abs(special) > 0) & (np.abs(special) < np.finfo(np.float32).tiny)).sum() >= 4 and (special < 0).any()
    assert int(g33['small_N']) < int(g33['small_Q']) and len(set(g33['equal_keys'].tolist())) == 1
    assert not any(np.isnan(g33[name + '_maps']).any() for name in CASES)


def test_key_is_monotone_over_the_special_values():
    from rcu_amd import evaluation as ev
    f = np.finfo(np.float32)
    denormal = np.array([1, 0x007fffff], np.uint32).view(np.float32)
    ordered = np.array([-np.inf, -f.max, -3.0, -1.0, -f.tiny, -denormal[1], -denormal[0], -0.0, 0.0, denormal[0], denormal[1], f.tiny, 1.0, 3.0, f.max,
                        np.inf], np.float32)
    for key in (qr.key, ev.float_key):
        k = key(ordered).astype(np.int64)
        step = np.diff(k)
        assert np.all(step >= 0) and list(np.flatnonzero(step == 0)) == [7]          # only -0.0 and +0.0 share a key
        assert k[0] == 0x007fffff and k[-1] == 0xff800000                              # ~bits(-inf), bits(+inf) | sign
        assert np.array_equal(ev.key_float(key(ordered)).view(np.uint32), np.where(ordered == 0, np.float32(0), ordered).view(np.uint32))
    rng = np.random.RandomState(1)
    x = rng.randint(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32).view(np.float32)
    x = x[~np.isnan(x)]
    assert np.array_equal(qr.key(x), ev.float_key(x))
    order = np.argsort(x, kind='stable')
    assert np.all(np.diff(qr.key(x[order]).astype(np.int64)) >= 0)


@pytest.mark.parametrize('plan', PLANS)
@pytest.mark.parametrize('name', CASES)
def test_quantile_refine_reproduces_the_fixture_tables(g33, name, plan):
    """The package's host step, fed with numpy-made histograms of each pass, ends on the fixture's boundary keys."""
    from rcu_amd import evaluation as ev
    maps, mask, q = case(g33, name)
    pop = qr.population_keys(maps, mask)
    ranks, slots, prefixes, shift = ev.quantile_ranks(pop.size, q), None, None, 32
    assert ranks == [int(r) for r in g33[name + '_ranks']]
    for bits in plan:
        shift -= bits
        hist = qr.key_hist(pop, prefixes or [], shift, bits)
        digits, ranks, prefixes, slots = ev.quantile_refine(hist, ranks, slots, prefixes)
        assert all(0 <= d < (1 << bits) for d in digits) and all(r >= 1 for r in ranks)
        assert prefixes == sorted(set(prefixes)) and len(prefixes) <= q - 1
        for d, r, s in zip(digits, ranks, slots):       # the rank inside the digit does not exceed what the digit holds
            assert prefixes[s] & ((1 << bits) - 1) == d
    assert shift == 0 and np.array_equal(np.array([prefixes[s] for s in slots], np.uint32), g33[name + '_keys'])


def test_quantile_refine_refuses_what_cannot_be():
    from rcu_amd import evaluation as ev
    hist = np.array([[2, 0, 3, 1]])
    assert ev.quantile_refine(hist, [1, 2, 3, 5, 6]) == ([0, 0, 2, 2, 3], [1, 2, 1, 3, 1], [0, 2, 3], [0, 0, 1, 1, 2])
    assert ev.quantile_refine(np.array([[0, 4], [1, 1]]), [4, 2], [0, 1], [5, 9])[2:] == ([11, 19], [0, 1])
    for bad in ([0], [7]):
        with pytest.raises(ValueError):
            ev.quantile_refine(hist, bad)
    with pytest.raises(ValueError):
        ev.quantile_refine(np.zeros((1, 3)), [1])
    for plan in ((16, 15), (17, 15), (32,), ()):
        with pytest.raises(ValueError):
            ev._check_plan(plan)
    for q in (1, 4097):
        with pytest.raises(ValueError):
            ev._check_quantiles(q)


@pytest.mark.parametrize('name', ('normal', 'lognormal'))
def test_levels_hold_the_rank_differences(g33, name):
    """Distinct values: level l holds exactly r_{l+1} - r_l population voxels (r_0 = 0, r_Q = N)."""
    maps, mask, q = case(g33, name)
    pop = qr.population_keys(maps, mask)
    assert np.unique(pop).size == pop.size
    counts = np.bincount(qr.levels(pop, g33[name + '_keys']), minlength=q)
    r = np.concatenate([[0], g33[name + '_ranks'], [pop.size]])
    assert np.array_equal(counts, np.diff(r)) and counts.sum() == pop.size


def test_csv_round_trip(g33, tmp_path):
    from rcu_amd import evaluation as ev
    for name, population in (('lognormal', 'mask'), ('special', 'mask'), ('equal', 'all')):
        table = ev.QuantileTable(int(g33[name + '_Q']), int(g33[name + '_N']), g33[name + '_keys'], g33[name + '_ranks'], population)
        path = str(tmp_path / 'eval_quantiles_{}.csv'.format(name))
        ev.save_quantiles(table, path)
        assert ev.load_quantiles(path) == table
        with open(path, newline='') as f:
            rows = list(csv.reader(f))
        assert rows[0] == ['k', 'rank', 'key', 'value'] and rows[1] == ['0', str(table.N), str(table.Q), population] and len(rows) == table.Q + 1
        for row, key in zip(rows[2:], table.keys):       # `value` is the float32's shortest text that reads back to the same bits
            assert int(row[2]) == int(key) and np.float32(row[3]).view(np.uint32) == ev.key_float(np.array([key]))[0].view(np.uint32)
    with open(str(tmp_path / 'other.csv'), 'w') as f:
        f.write('confidence_entry,min,max\nsigma,0,1\n')
    with pytest.raises(ValueError):
        ev.load_quantiles(str(tmp_path / 'other.csv'))


@pytest.mark.parametrize('q', (2, 7, 1000, 4096))
def test_rescaled_value_gives_back_its_level(q):
    level = np.arange(q)
    value = qr.rescaled(level, q)
    assert value.dtype == np.float32 and np.array_equal(qr.grid_level(value, q), level)
    # the float32 rounding error stays below 2^-24, against 0.5 / Q to the nearest threshold
    assert np.abs(value.astype(np.float64) - (level + 0.5) / q).max() < 2.0 ** -24 < 0.5 / q


def test_entry_points_check_their_arguments_without_a_gpu():
    import ctypes
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    so = _lib.load()
    p = ctypes.c_void_p(256)       # (never dereferenced: every call below is refused first)
    three = (ctypes.c_uint32 * 3)(1, 5, 9)

    def key_hist(maps=p, mask=None, n=100, volumes=1, prefixes=None, n_prefixes=0, shift=16, bits=16, hist=p, counts=p, ws=p):
        status = so.rcu_key_hist(maps, mask, n, volumes, prefixes, n_prefixes, shift, bits, hist, counts, ws, None)
        return status, so.rcu_last_error().decode()

    for kwargs, word in ((dict(bits=0), 'bits'), (dict(bits=17), 'bits'), (dict(shift=17), 'shift + bits'), (dict(shift=-1), 'shift'),
                         (dict(prefixes=(ctypes.c_uint32 * 3)(1, 9, 5), n_prefixes=3, shift=0), 'strictly increasing'),
                         (dict(prefixes=(ctypes.c_uint32 * 2)(4, 4), n_prefixes=2, shift=0), 'strictly increasing'),
                         (dict(prefixes=three, n_prefixes=4096, shift=0), 'n_prefixes'), (dict(n_prefixes=-1), 'n_prefixes'),
                         (dict(n_prefixes=3, shift=0), 'null prefixes_host'),
                         (dict(prefixes=(ctypes.c_uint32 * 1)(1 << 16), n_prefixes=1, shift=0), '32 - shift - bits'),
                         (dict(prefixes=three, n_prefixes=3, shift=16), 'only prefix'),
                         (dict(maps=None), 'null maps_dev'), (dict(hist=None), 'null hist_dev'), (dict(counts=None), 'null counts_dev'),
                         (dict(ws=None), 'null workspace_dev'), (dict(volumes=0), 'n_volumes'), (dict(volumes=65536), 'n_volumes'), (dict(n=0), 'n_per_volume')):
        status, message = key_hist(**kwargs)
        assert status == -1 and message.startswith('rcu_key_hist: ') and word in message, (kwargs, message)
    assert so.rcu_key_hist_set_blocks_per_workgroup(-1) == -1 and so.rcu_key_hist_set_blocks_per_workgroup(0) == 0
    assert so.rcu_key_hist_workspace_bytes(0) >= 4 and so.rcu_key_hist_workspace_bytes(4095) >= 4 * 4095 and so.rcu_key_hist_workspace_bytes(4096) == 0

    def apply(map_=p, n=10, bounds=three, q=4, out=p, ws=p):
        status = so.rcu_quantile_apply(map_, n, bounds, q, out, None, ws, None)
        return status, so.rcu_last_error().decode()

    for kwargs, word in ((dict(q=1), 'quantiles'), (dict(q=4097), 'quantiles'), (dict(bounds=None), 'null bounds_host'),
                         (dict(bounds=(ctypes.c_uint32 * 3)(1, 9, 5)), 'non-decreasing'), (dict(map_=None), 'null map_dev'), (dict(out=None), 'null out_dev'),
                         (dict(ws=None), 'null workspace_dev'), (dict(n=0), 'n must be')):
        status, message = apply(**kwargs)
        assert status == -1 and message.startswith('rcu_quantile_apply: ') and word in message, (kwargs, message)
    assert so.rcu_quantile_apply_workspace_bytes(4096) >= 4 * 4095 and so.rcu_quantile_apply_workspace_bytes(1) == 0


# ------------------------------------------------------------------------------------------- driver
def _parser():
    spec = importlib.util.spec_from_file_location('bin_eval_uncertainty', os.path.join(ROOT, 'bin-eval', 'eval_uncertainty.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.make_parser()


def test_parser_flags():
    parser = _parser()
    args = parser.parse_args([])
    assert (args.rescale, args.quantiles) == ('minmax', 1000)
    args = parser.parse_args(['--act', 'quantiles', 'ue_curves', '--rescale', 'quantile', '--quantiles', '64'])
    assert (args.act, args.rescale, args.quantiles) == (['quantiles', 'ue_curves'], 'quantile', 64)
    for bad in (['--rescale', 'rank'], ['--quantiles', '1'], ['--quantiles', '4097']):
        with pytest.raises(SystemExit):
            parser.parse_args(bad)
    text = parser.format_help()
    assert 'ece_dice, calib and calib_curves keep' in ' '.join(text.split())


def _write_minmax(base, run_id, entry):
    from rcu_amd import evalrun
    os.makedirs(os.path.join(base, evalrun.MINMAX_NAME), exist_ok=True)
    evalrun.write_table(os.path.join(base, evalrun.MINMAX_NAME, evalrun.MINMAX_PLACEHOLDER.format(run_id)), ['confidence_entry', 'min', 'max'],
                        [[entry, 0.0, 4.0]])


UNCERTAINTY_ACTIONS = ('bnf_ue', 'ue_curves', 'patches', 'components', 'lesions', 'boundary')
ALL_ACTIONS = ('minmax', 'ece_dice', 'calib') + UNCERTAINTY_ACTIONS + ('calib_curves',)


def _ids(base, run_id, entry, **kwargs):
    from rcu_amd import evalrun
    actions = evalrun.get_actions(list(ALL_ACTIONS), os.path.join(base, evalrun.MINMAX_NAME), base, 'foreground', **kwargs)
    assert len(actions) == len(ALL_ACTIONS)
    data = evalrun.EvalData(run_id, 'unused', entry)
    for action in actions:
        action.setup_eval(data)
    return {name: action.id_ for name, action in zip(ALL_ACTIONS, actions)}


def test_default_arguments_build_the_ids_they_built_before(tmp_path):
    base = str(tmp_path / 'eval')
    for run_id, entry, suffix in (('baseline_mc', 'probabilities', ''), ('aleatoric', 'sigma', '_globalrescale'), ('density', 'density', '_globalrescale'),
                                  ('auxiliary_feat', 'confidence', '_rescale')):
        _write_minmax(base, run_id, entry)
        ids = _ids(base, run_id, entry)
        assert ids.pop('minmax') == run_id
        assert ids == {name: run_id + suffix for name in ALL_ACTIONS[1:]}, run_id
        assert _ids(base, run_id, entry, rescale='minmax', quantiles=64) == dict(ids, minmax=run_id)


def test_quantile_rescale_reaches_the_uncertainty_actions_alone(g33, tmp_path):
    from rcu_amd import evalrun, evaluation as ev
    base = str(tmp_path / 'eval')
    os.makedirs(os.path.join(base, evalrun.QUANTILES_NAME))
    table = ev.QuantileTable(1000, int(g33['lognormal_N']), g33['lognormal_keys'], g33['lognormal_ranks'], 'mask')
    for run_id, entry in (('aleatoric', 'sigma'), ('density', 'density')):
        _write_minmax(base, run_id, entry)
        ev.save_quantiles(table, evalrun.quantiles_file(os.path.join(base, evalrun.QUANTILES_NAME), run_id))
        ids = _ids(base, run_id, entry, rescale='quantile')
        assert {ids[name] for name in UNCERTAINTY_ACTIONS} == {run_id + '_quantilerescale'}
        assert {ids[name] for name in ('ece_dice', 'calib', 'calib_curves')} == {run_id + '_globalrescale'} and ids['minmax'] == run_id
    # probability maps and confidence entries are untouched, and need no table
    for run_id, entry, suffix in (('baseline_mc', 'probabilities', ''), ('auxiliary_feat', 'confidence', '_rescale')):
        _write_minmax(base, run_id, entry)
        assert set(_ids(base, run_id, entry, rescale='quantile').values()) == {run_id, run_id + suffix}
    with pytest.raises(ValueError):
        evalrun.get_actions(['ue_curves'], base, base, '', rescale='rank')
    # the action itself: never fused, first in a call, the mask where the dataset evaluates inside one
    for details, need_mask in (('foreground', True), ('', False)):
        (action,) = evalrun.get_actions(['quantiles'], base, base, details, quantiles=64)
        assert isinstance(action, evalrun.SaveQuantilesAction) and action.scans is None and action.runs_first and action.whole_run
        assert (action.need_mask, action.quantiles) == (need_mask, 64)
    assert evalrun.SCANS == ('ece', 'minmax', 'ue', 'ue_hist', 'components', 'boundary', 'calib_levels', 'lesions', 'patches')
    assert evalrun.get_actions(['minmax'], base, base, '')[0].runs_first and not evalrun.get_actions(['ue_curves'], base, base, '')[0].runs_first


def test_missing_table_and_other_q_are_refused(g33, tmp_path):
    from rcu_amd import evalrun, evaluation as ev
    base = str(tmp_path / 'eval')
    data = evalrun.EvalData('density', 'unused', 'density')
    (action,) = evalrun.get_actions(['ue_curves'], os.path.join(base, 'minmax'), base, 'foreground', rescale='quantile')
    path = os.path.join(base, 'quantiles', 'eval_quantiles_density.csv')
    with pytest.raises(ValueError) as err:
        action.setup_eval(data)
    assert path in str(err.value) and '--rescale quantile' in str(err.value) and '--act quantiles' in str(err.value)
    os.makedirs(os.path.dirname(path))
    ev.save_quantiles(ev.QuantileTable(7, int(g33['special_N']), g33['special_keys'], g33['special_ranks'], 'mask'), path)
    with pytest.raises(ValueError) as err:
        action.setup_eval(data)
    assert path in str(err.value) and '--quantiles' in str(err.value) and 'Q = 7' in str(err.value)
    (action,) = evalrun.get_actions(['ue_curves'], os.path.join(base, 'minmax'), base, 'foreground', rescale='quantile', quantiles=7)
    action.setup_eval(data)
    assert action.id_ == 'density_quantilerescale' and isinstance(action.prepare.prepare_data_list[0], ev.RescaleQuantile)
    assert action.path(evalrun.UE_LEVELS_PLACEHOLDER).endswith(os.path.join('uncertainty', 'eval_ue_levels_density_quantilerescale.csv'))


def test_quantiles_on_a_probability_run_writes_nothing_and_says_so(tmp_path, capsys):
    from rcu_amd import evalrun
    base = str(tmp_path / 'eval')
    for run_id, entry in (('baseline_mc', 'probabilities'), ('auxiliary_feat', 'confidence')):
        evalrun.evaluate_runs([evalrun.EvalData(run_id, 'unused', entry)], ['quantiles'], base, 'foreground')
        assert 'nothing written' in capsys.readouterr().out
    assert not os.path.exists(os.path.join(base, 'quantiles')) or not os.listdir(os.path.join(base, 'quantiles'))


def test_device_metrics_refuses_the_action():
    from rcu_amd import scripts
    with pytest.raises(ValueError) as err:
        scripts.DeviceMetricsHook('brats', {'actions': ['minmax', 'quantiles']}, {})
    assert 'others.device_metrics' in str(err.value) and 'quantiles' in str(err.value)
    scripts.DeviceMetricsHook('brats', {'actions': ['minmax', 'ece_dice']}, {})
