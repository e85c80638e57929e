"""Test-time augmentation without a GPU: the C ABI (symbols, argument validation), the D4 table, the mask-key contract, the YAML surface and the
sharded job lists."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ('identity', 'flip_h', 'flip_v', 'rot180', 'transpose', 'rot90', 'rot270', 'anti_transpose')

# the numpy definition of each element on the last two axes (independent of rcu_amd.steps.tta_torch)
NUMPY_OPS = {
    'identity': lambda a: a,
    'flip_h': lambda a: np.flip(a, -1),
    'flip_v': lambda a: np.flip(a, -2),
    'rot180': lambda a: np.flip(a, (-2, -1)),
    'transpose': lambda a: np.swapaxes(a, -2, -1),
    'rot90': lambda a: np.rot90(a, 1, (-2, -1)),
    'rot270': lambda a: np.rot90(a, 3, (-2, -1)),
    'anti_transpose': lambda a: np.swapaxes(np.rot90(a, 2, (-2, -1)), -2, -1),
}


@pytest.fixture(scope='module')
def lib():
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    return _lib


def test_tta_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, 'include', 'rcu.h')).read()
    declared = set(re.findall(r'\b(rcu_[a-z0-9_]+)\s*\(', header))
    so = lib.load()
    for name in ('rcu_tta_transform', 'rcu_mc_fold_transformed'):
        assert name in declared and name in lib.SIGNATURES and hasattr(so, name), name
    codes = dict(re.findall(r'#define (RCU_TTA_[A-Z0-9_]+) (\d+)', header))
    assert [int(codes['RCU_TTA_' + n.upper()]) for n in NAMES] == list(range(8))
    assert tuple(lib.TTA_ELEMENTS) == NAMES


def test_tta_argument_validation_without_gpu(lib):
    so = lib.load()
    x, out = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)

    def refused(status, *words):
        assert status == -1        # RCU_ERR_INVALID
        msg = so.rcu_last_error()
        assert msg, 'no message'
        for w in words:
            assert w in msg, (w, msg)

    # element code out of range
    refused(so.rcu_tta_transform(x, 2, 4, 16, 16, 8, out, None), b'element')
    refused(so.rcu_tta_transform(x, 2, 4, 16, 16, -1, out, None), b'element')
    refused(so.rcu_mc_fold_transformed(x, out, 2, 16, 16, 2, 8, 9, None), b'element')
    # codes 4-7 need square planes, on both entry points
    for e in range(4, 8):
        refused(so.rcu_tta_transform(x, 2, 4, 192, 256, e, out, None), b'square', b'192 x 256')
        refused(so.rcu_mc_fold_transformed(x, out, 2, 192, 256, 2, 8, e, None), b'square')
    # out == x (and any overlap)
    refused(so.rcu_tta_transform(x, 2, 4, 16, 16, 1, x, None), b'overlap')
    refused(so.rcu_tta_transform(x, 2, 4, 16, 16, 1, ctypes.c_void_p((1 << 20) + 64), None), b'overlap')
    refused(so.rcu_mc_fold_transformed(x, x, 2, 16, 16, 2, 8, 1, None), b'overlap')
    # n = 0
    refused(so.rcu_tta_transform(x, 0, 4, 16, 16, 1, out, None), b'empty')
    refused(so.rcu_mc_fold_transformed(x, out, 0, 16, 16, 2, 8, 1, None), b'empty')
    # flags outside RCU_MC_MI | RCU_MC_VAR | RCU_MC_EXACT (RCU_MC_INPUT_PROBS has no meaning for a blob)
    for flags in (lib.RCU_MC_INPUT_PROBS, lib.RCU_MC_EXACT | lib.RCU_MC_INPUT_PROBS, 16, -1):
        refused(so.rcu_mc_fold_transformed(x, out, 2, 16, 16, 2, flags, 1, None), b'flags')
    # null pointers, class count
    refused(so.rcu_tta_transform(None, 2, 4, 16, 16, 1, out, None), b'null')
    refused(so.rcu_mc_fold_transformed(x, None, 2, 16, 16, 2, 8, 1, None), b'null')
    refused(so.rcu_mc_fold_transformed(x, out, 2, 16, 16, 9, 8, 1, None), b'nb_classes')


@pytest.mark.parametrize('shape', [(2, 3, 6, 6), (1, 2, 5, 5), (2, 3, 4, 7), (1, 1, 15, 17)])
def test_group_table_names_torch_ops_and_inverses(shape):
    from rcu_amd import steps
    rng = np.random.default_rng(1)
    a = rng.standard_normal(shape).astype(np.float32)
    x = torch.from_numpy(a)
    square = shape[-1] == shape[-2]
    for code, name in enumerate(NAMES):
        assert steps.tta_element(name) == code and steps.tta_element(code) == code and steps.TTA_ELEMENTS[code] == name
        assert steps.tta_swaps_axes(name) == (code >= 4)
        if code >= 4 and not square:
            continue
        gx = steps.tta_torch(x, name)
        assert np.array_equal(gx.numpy(), NUMPY_OPS[name](a)), name
        inv = steps.TTA_INVERSE[code]
        assert np.array_equal(steps.tta_torch(gx, inv).numpy(), a), name
        assert np.array_equal(NUMPY_OPS[NAMES[inv]](NUMPY_OPS[name](a)), a), name
    # the inverse table: involutions except rot90 <-> rot270
    assert [steps.TTA_INVERSE[c] for c in range(8)] == [0, 1, 2, 3, 4, 6, 5, 7]


def test_transform_names_are_validated():
    from rcu_amd import steps
    assert steps.tta_elements(['identity', 'flip_h', 3]) == (0, 1, 3)
    for bad in (['identity', 'flip'], ['flip_h', 'flip_h'], ['flip_h', 1], [], [8], [True]):
        with pytest.raises(ValueError):
            steps.tta_elements(bad)
    with pytest.raises(ValueError):
        steps.TtaMcPredictStep(['rot90', 'mirror'])
    with pytest.raises(ValueError):
        steps.TtaMcPredictStep(['rot90', 'rot90'])
    with pytest.raises(ValueError):
        steps.check_tta_shape((0, 1, 5), 192, 256)
    with pytest.raises(ValueError, match='rot90.*192 x 256'):
        steps.check_tta_shape(steps.tta_elements(['flip_h', 'rot90']), 192, 256)
    steps.check_tta_shape(steps.tta_elements(NAMES), 240, 240)
    steps.check_tta_shape((0, 1, 2, 3), 192, 256)
    # samples and the exact-sum bound
    assert steps.TtaMcPredictStep(['identity', 'flip_h'], mc_steps=5).samples == 10
    assert steps.TtaMcPredictStep(NAMES).samples == 8 and steps.TtaMcPredictStep(NAMES).exact
    assert not steps.TtaMcPredictStep(NAMES[:4], mc_steps=1024).exact and steps.TtaMcPredictStep(NAMES[:4], mc_steps=512).exact


def test_mask_keys_identity_is_plain_mc_and_all_keys_are_distinct():
    from rcu_amd import steps
    for seed in (0, 20, 123456789, 2 ** 40 + 7):
        for t in (1, 2, 17, 2048):
            assert steps.tta_pass_seed(seed, 'identity', t) == steps.pass_seed(seed, t)
            assert steps.tta_pass_seed(seed, 0, t) == steps.pass_seed(seed, t)
        keys = [steps.tta_pass_seed(seed, e, t) for e in NAMES for t in range(1, 2049)]
        assert len(set(keys)) == len(keys) == 8 * 2048
        assert all(0 <= k < 2 ** 63 - 1 for k in keys)


def _context(others, seed=20):
    from rcu_amd import config as cfg
    from rcu_amd import loops
    context = loops.TorchTestContext('cpu')
    context.config = cfg.TestConfiguration()
    context.config.seed = seed
    context.config.others = cfg.OtherParameters().from_dict(others)
    return context


def test_yaml_surface_builds_the_tta_steps(monkeypatch):
    from rcu_amd import distributed as rdist
    from rcu_amd import scripts, steps
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    world = rdist.world_from_env('cuda')
    # with mc: TTA x MC, the seed of the YAML file, the weight-scaling pass as the MC step runs it
    built = scripts._default_steps(_context(dict(mc=5, tta=['identity', 'flip_h', 'flip_v', 'rot180'], stream_lanes=1)), world)
    assert [type(s_) for s_ in built] == [steps.TtaMcPredictStep, steps.MultiPredictionSummary]
    assert (built[0].elements, built[0].mc_steps, built[0].seed, built[0].lanes, built[0].ws_pass, built[0].exact) == ((0, 1, 2, 3), 5, 20, 1, True, True)
    # without mc: TTA alone, eval mode, in place of SegmentationPredictStep
    built = scripts._default_steps(_context(dict(tta=['rot90', 'identity'])), world)
    assert [type(s_) for s_ in built] == [steps.TtaMcPredictStep, steps.MultiPredictionSummary]
    assert (built[0].elements, built[0].mc_steps, built[0].ws_pass) == ((5, 0), 0, False)
    # two ranks: the sharded form
    built = scripts._default_steps(_context(dict(mc=2, tta=['identity', 'flip_h'])), rdist.World(0, 2))
    assert [type(s_) for s_ in built] == [rdist.ShardedTtaMcPredictStep, steps.MultiPredictionSummary]
    assert (built[0].elements, built[0].mc_steps, built[0].seed) == ((0, 1), 2, 20)
    built = scripts._default_steps(_context(dict(tta=['identity', 'flip_h'])), rdist.World(1, 2))
    assert type(built[0]) is rdist.ShardedTtaMcPredictStep and built[0].mc_steps == 0
    # unknown and duplicate names
    for bad in (['identity', 'mirror'], ['flip_h', 'flip_h']):
        with pytest.raises(ValueError):
            scripts._default_steps(_context(dict(mc=5, tta=bad)), world)
        with pytest.raises(ValueError):
            scripts._default_steps(_context(dict(tta=bad)), world)
    # a config without the key builds what it built before
    assert [type(s_) for s_ in scripts._default_steps(_context(dict(mc=20)), world)] == [steps.McPredictStep, steps.MultiPredictionSummary]
    assert [type(s_) for s_ in scripts._default_steps(_context({}), world)] == [steps.SegmentationPredictStep]
    assert [type(s_) for s_ in scripts._default_steps(_context(dict(mc=2)), rdist.World(0, 2))] == [rdist.ShardedMcPredictStep,
                                                                                                     steps.MultiPredictionSummary]


YAML = """
config:
  test_name: brats_test_x
  test_dir: {test_dir}
  model_dir: {model_dir}
  seed: 20
  test_at: best
  others:
    model_dir: [{model_dir}]
    tta: [identity, flip_h]
meta:
  type: test-config
  version: 0
"""


@pytest.mark.parametrize('script', ['test_ensemble', 'test_aleatoric', 'test_auxiliary_feat', 'test_auxiliary_segm'])
def test_other_scripts_refuse_the_tta_key(tmp_path, monkeypatch, script):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    path = tmp_path / 'test_brats_x.yaml'
    path.write_text(YAML.format(test_dir=tmp_path / 'out', model_dir=tmp_path / 'train' / 'model_x'))
    with pytest.raises(ValueError, match='others.tta'):
        getattr(scripts, script)('brats', config_file=str(path), device='cpu')
    assert not (tmp_path / 'out').exists()


@pytest.mark.parametrize('world', [1, 2, 8])
@pytest.mark.parametrize('mc', [0, 3, 5])
def test_sharded_job_lists_cover_every_transform_pass_once(world, mc):
    from rcu_amd import distributed as rdist
    transforms = ['identity', 'flip_h', 'flip_v', 'rot180']
    for ws_pass in (True, False):
        runners = [rdist.ShardedTtaMcRunner(None, transforms, mc, ws_pass=ws_pass, rank=r, world=world, seed=20) for r in range(world)]
        per = max(mc, 1)
        expected = ([('ws',)] if ws_pass else []) + [(e, t) for e in (0, 1, 2, 3) for t in range(1, per + 1)]
        for step in range(5):
            held = []
            for r, runner in enumerate(runners):
                for j in runner.jobs_of(step, r):
                    held.append(('ws',) if j == 0 else runner.job_pair(j))
            assert sorted(held, key=repr) == sorted(expected, key=repr), (world, mc, step)
            assert len(held) == len(set(held))
        assert runners[0].mc_steps == 4 * per and runners[0].jobs_per_step == 4 * per + (1 if ws_pass else 0)
    with pytest.raises(ValueError):
        rdist.ShardedTtaMcPredictStep(transforms, rdist.World(0, 2), mc_steps=2, seed=None)
    rdist.ShardedTtaMcPredictStep(transforms, rdist.World(0, 2), mc_steps=0, seed=None)
