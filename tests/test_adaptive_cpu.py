"""Adaptive MC dropout (include/rcu.h "Adaptive MC") without a device: the threshold arithmetic, the schedule's limits and bookkeeping, the
group-size cap, the YAML surface and its refusals, the C declarations, and the numpy restatement of tests/adaptive_reference.py on a
hand-made blob."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import adaptive_reference as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('rcu_mc_slice_scores', 'rcu_dropout_masks_indexed', 'rcu_mc_merge_slices', 'rcu_mc_finalize_counts')


# ------------------------------------------------------------------------------------------------ thr_q
@pytest.mark.parametrize('eps', [0.0, 2.0 ** -20, 0.01, 0.5])
def test_threshold_is_the_exact_ceiling(eps):
    from rcu_amd import steps
    for t in (2, 3, 5, 7, 10, 19, 2047):
        exact = Fraction(1.0 - eps) * t * 2 ** 40           # the float64 value of 1.0 - eps, as a rational
        want = exact.numerator // exact.denominator + (1 if exact.numerator % exact.denominator else 0)
        assert steps.adaptive_threshold(eps, t) == want == ar.thr_q(eps, t)
        assert want - 1 < exact <= want
        assert isinstance(steps.adaptive_threshold(eps, t), int)
    assert steps.adaptive_threshold(0.0, 5) == 5 * 2 ** 40 and steps.adaptive_threshold(0.5, 4) == 2 * 2 ** 40
    assert steps.adaptive_threshold(2.0 ** -20, 2) == 2 ** 41 - 2 ** 21


def test_threshold_where_the_product_is_not_a_float64():
    """(1 - 0.01) * 3 is not representable: the float64 product rounds, the rational ceiling does not."""
    from rcu_amd import steps
    one_minus = 1.0 - 0.01
    exact = Fraction(one_minus) * 3
    assert Fraction(one_minus * 3) != exact                  # the float64 multiplication rounds here
    assert (exact * 2 ** 40).denominator != 1                # and the scaled product is no integer: the ceiling is a real step up
    q = steps.adaptive_threshold(0.01, 3)
    assert Fraction(q - 1, 2 ** 40) < exact <= Fraction(q, 2 ** 40)
    # a voxel whose leading sum is (q - 1) * 2^-40 has a mean below 1 - eps, one at q * 2^-40 reaches it
    assert Fraction(q - 1, 3 * 2 ** 40) < Fraction(one_minus) <= Fraction(q, 3 * 2 ** 40)


# ------------------------------------------------------------------------------------------------ the schedule
def test_schedule_validation_names_the_limit():
    from rcu_amd import steps
    ok = steps.check_adaptive(dict(check_at=[5, 10], tolerance=0.01), 20)
    assert ok == dict(check_at=[5, 10], tolerance=0.01, max_unsettled=0)
    assert steps.check_adaptive(dict(check_at=(2, 3, 4, 5), tolerance=0, max_unsettled=3), 6)['max_unsettled'] == 3
    bad = [(dict(check_at=[1, 5], tolerance=0.1), 'first checkpoint'), (dict(check_at=[5, 20], tolerance=0.1), 'below mc_steps'),
           (dict(check_at=[5, 5], tolerance=0.1), 'increasing'), (dict(check_at=[10, 5], tolerance=0.1), 'increasing'),
           (dict(check_at=[2, 3, 4, 5, 6], tolerance=0.1), 'checkpoints'), (dict(check_at=[], tolerance=0.1), 'checkpoints'),
           (dict(check_at=[5], tolerance=1.0), 'tolerance'), (dict(check_at=[5], tolerance=-0.1), 'tolerance'),
           (dict(check_at=[5]), 'tolerance'), (dict(tolerance=0.1), 'check_at'), (dict(check_at=[5], tolerance=0.1, max_unsettled=-1), 'max_unsettled'),
           (dict(check_at=[5.5], tolerance=0.1), 'check_at'), (dict(check_at=[5], tolerance=0.1, bogus=1), 'bogus'), ([5, 10], 'dict')]
    for schedule, word in bad:
        with pytest.raises(ValueError, match=word):
            steps.check_adaptive(schedule, 20)


def test_the_step_names_what_the_adaptive_path_is_missing():
    from rcu_amd import steps
    schedule = dict(check_at=[2, 4], tolerance=0.01)
    step = steps.McPredictStep(6, seed=3, adaptive=schedule)
    assert step.adaptive == dict(check_at=[2, 4], tolerance=0.01, max_unsettled=0) and step.exact
    assert steps.McPredictStep(6, masks=[None] * 6, adaptive=schedule).adaptive is not None      # injected masks stand in for the seed
    assert steps.McPredictStep(6).adaptive is None
    for kw, word in ((dict(seed=3, exact=False), 'exact'), (dict(), 'seed'), (dict(seed=3, materialize=True), 'materialize'),
                     (dict(seed=3, agreement=True), 'agreement')):
        with pytest.raises(ValueError, match=word):
            steps.McPredictStep(6, adaptive=schedule, **kw)
    with pytest.raises(ValueError, match='exact'):
        steps.McPredictStep(4096, seed=3, adaptive=dict(check_at=[2], tolerance=0.01))
    # a model that is no rcu_amd UNet has no fused path
    import torch
    context = steps.TorchTestContext('cpu', model=torch.nn.Identity())
    with pytest.raises(ValueError, match='UNet'):
        step(steps.BatchContext({'images': torch.zeros(1, 4, 32, 32)}, 0), None, context)


def test_active_lists_compose_over_two_checkpoints():
    from rcu_amd import steps
    # 6 slices, T = 6, checkpoints 2 and 4: slices 1 and 4 retire at 2, slices 0 and 5 at 4, slices 2 and 3 run to 6
    plan = {0: {1, 4}, 1: {0, 5}}
    counts, spans = ar.schedule(6, [2, 4], 6, lambda k, t, active: [i in plan[k] for i in active])
    assert [list(s) for s in spans] == [[0, 1, 2, 3, 4, 5], [0, 2, 3, 5], [2, 3]]
    assert counts.tolist() == [4, 2, 6, 6, 2, 4] and counts.dtype == np.int32
    assert steps.adaptive_counts(6, [2, 4], 6, [list(s) for s in spans]) == counts.tolist()
    # everything retires at the first checkpoint: one span, the step ends there
    counts, spans = ar.schedule(3, [2, 4], 6, lambda k, t, active: [True] * len(active))
    assert counts.tolist() == [2, 2, 2] and len(spans) == 1 and steps.adaptive_counts(3, [2, 4], 6, [[0, 1, 2]]) == [2, 2, 2]
    # nothing retires: every span is the whole batch
    counts, spans = ar.schedule(3, [2, 4], 6, lambda k, t, active: [False] * len(active))
    assert counts.tolist() == [6, 6, 6] and [list(s) for s in spans] == [[0, 1, 2]] * 3
    assert steps.adaptive_counts(3, [2, 4], 6, [[0, 1, 2]] * 3) == [6, 6, 6]
    # the last slice leaves at the second checkpoint
    counts, spans = ar.schedule(2, [2, 4], 6, lambda k, t, active: [k == 1 or i == 0 for i in active])
    assert counts.tolist() == [2, 4] and [list(s) for s in spans] == [[0, 1], [1]]


def test_compact_groups_never_exceed_the_reserved_plan():
    from rcu_amd import steps

    class Model:
        @staticmethod
        def max_group_samples(h, w):
            return 10 ** 9
    pixels = steps.McPredictStep.GROUP_PIXELS
    n, h, w, total = 160, 192, 128, 20
    group = steps.pass_group_size(Model, n, h, w, pixels)
    assert group == 4
    plan_samples = n * min(group, total)                       # what reserve_canonical_plans sizes the plan for
    for m in (1, 7, 40, 80, 159, 160):
        g = steps.compact_group_size(Model, m, h, w, pixels, plan_samples)
        assert g >= 1 and m * g <= plan_samples
        assert g <= steps.pass_group_size(Model, m, h, w, pixels)
    assert steps.compact_group_size(Model, 80, h, w, pixels, plan_samples) == 8      # the same 640 samples, twice the passes
    assert steps.compact_group_size(Model, 160, h, w, pixels, plan_samples) == 4
    # a plan reserved for fewer samples than group_pixels would allow (T below the group size) caps the compact launch
    assert steps.compact_group_size(Model, 40, h, w, pixels, 160 * 2) == 8 and steps.pass_group_size(Model, 40, h, w, pixels) == 16
    assert steps.compact_group_size(Model, 300, h, w, pixels, 160) == 1


# ------------------------------------------------------------------------------------------------ the YAML surface
def _context(others, seed=20):
    from rcu_amd import config as cfg
    from rcu_amd import loops
    context = loops.TorchTestContext('cpu')
    context.config = cfg.TestConfiguration()
    context.config.seed = seed
    context.config.others = cfg.OtherParameters().from_dict(others)
    return context


SCHEDULE = dict(check_at=[5, 10], tolerance=0.01, max_unsettled=0)


def test_the_key_builds_the_adaptive_steps_and_its_absence_the_steps_of_before():
    from rcu_amd import distributed as rdist
    from rcu_amd import scripts, steps
    world = rdist.World()
    mc, summary, rows = scripts._default_steps(_context(dict(mc=20, mc_adaptive=dict(SCHEDULE), stream_lanes=1)), world)
    assert type(mc) is steps.McPredictStep and mc.adaptive == SCHEDULE and (mc.mc_steps, mc.seed, mc.lanes, mc.exact) == (20, 20, 1, True)
    assert type(summary) is steps.MultiPredictionSummary and type(rows) is scripts.AdaptiveRowsStep and rows.check_at == [5, 10]
    plain = scripts._default_steps(_context(dict(mc=20)), world)
    assert [type(s) for s in plain] == [steps.McPredictStep, steps.MultiPredictionSummary] and plain[0].adaptive is None
    # it composes with temperature, corruption and device_metrics: none of them is looked at here
    built = scripts._default_steps(_context(dict(mc=20, mc_adaptive=dict(SCHEDULE), temperature=1.5, corruption='gaussian_noise', device_metrics=True)), world)
    assert built[0].adaptive == SCHEDULE


def test_default_script_refusals_name_the_key():
    from rcu_amd import distributed as rdist
    from rcu_amd import scripts
    world = rdist.World()
    refused = [(dict(mc=20, mc_adaptive=dict(SCHEDULE), tta=['identity', 'flip_h']), 'tta'), (dict(mc_adaptive=dict(SCHEDULE), tta=['identity']), 'tta'),
               (dict(mc=20, mc_adaptive=dict(SCHEDULE), agreement=True), 'agreement'), (dict(mc=20, mc_adaptive=dict(SCHEDULE), exact=False), 'exact'),
               (dict(mc_adaptive=dict(SCHEDULE)), 'others.mc'), (dict(mc=10, mc_adaptive=dict(SCHEDULE)), 'mc_steps'),
               (dict(mc=20, mc_adaptive=dict(check_at=[1], tolerance=0.01)), 'first checkpoint'), (dict(mc=20, mc_adaptive=[5, 10]), 'dict')]
    for others, word in refused:
        with pytest.raises(ValueError, match='others.mc_adaptive') as e:
            scripts._default_steps(_context(others), world)
        assert word in str(e.value), (others, str(e.value))
    with pytest.raises(ValueError, match='others.mc_adaptive'):
        scripts._default_steps(_context(dict(mc=20, mc_adaptive=dict(SCHEDULE))), rdist.World(rank=0, world=2))
    with pytest.raises(ValueError, match='seed'):
        scripts._default_steps(_context(dict(mc=20, mc_adaptive=dict(SCHEDULE)), seed=None), world)


YAML = """
config:
  test_name: brats_test_x
  test_dir: {test_dir}
  model_dir: {model_dir}
  seed: 20
  test_at: best
  others:
    model_dir: [{model_dir}]
    mc: 20
    mc_adaptive: {{check_at: [5, 10], tolerance: 0.01, max_unsettled: 0}}
meta:
  type: test-config
  version: 0
"""


@pytest.mark.parametrize('script', ['test_ensemble', 'test_aleatoric', 'test_auxiliary_feat', 'test_auxiliary_segm', 'fit_temperature'])
def test_other_scripts_refuse_the_key(tmp_path, monkeypatch, script):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    path = tmp_path / 'test_brats_x.yaml'
    path.write_text(YAML.format(test_dir=tmp_path / 'out', model_dir=tmp_path / 'train' / 'model_x'))
    with pytest.raises(ValueError, match='others.mc_adaptive'):
        if script == 'fit_temperature':
            scripts.fit_temperature('brats', str(path), device='cpu')
        else:
            getattr(scripts, script)('brats', config_file=str(path), device='cpu')
    assert not (tmp_path / 'out').exists()


def test_adaptive_csv_row_adds_up():
    from rcu_amd import scripts
    q = 2 ** 40
    # [passes, margin_q at checkpoint 5, margin_q at checkpoint 10]: two slices retired at 5, one at 10, two ran to 20
    rows = [[5, 5 * q, -1], [5, 5 * q - 10, -1], [10, 4 * q, 10 * q - 4], [20, 3 * q, 7 * q], [20, 2 * q, 9 * q]]
    row = scripts.adaptive_csv_row(rows, [5, 10], 20)
    assert row[:5] == [5, 2, 1, 60, 100]
    assert row[1] * 15 + row[2] * 10 == row[4] - row[3]                    # the saved passes
    assert row[5] == min((5 * q - 10) / (5.0 * q), (10 * q - 4) / (10.0 * q)) and row[6] == (2 * q) / (5.0 * q)
    assert scripts.adaptive_csv_row([[20, q, q]], [5, 10], 20) == [1, 0, 0, 20, 20, '', 0.1]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_four_entry_points_are_declared_for_c99(tmp_path):
    header = open(os.path.join(ROOT, 'include', 'rcu.h')).read()
    assert 'Adaptive MC' in header
    declared = set(re.findall(r'\b(rcu_[a-z0-9_]+)\s*\(', header))
    assert set(SYMBOLS) <= declared
    from rcu_amd import _lib
    assert set(SYMBOLS) <= set(_lib.SIGNATURES) and _lib.RCU_ADAPTIVE_MAX_CHECKPOINTS == 4
    src = tmp_path / 'adaptive.c'
    src.write_text('\n'.join([
        '#include <stdio.h>', '#include "rcu.h"',
        'int (*scores)(const void*, size_t, size_t, int, int, int64_t, uint32_t*, int64_t*, void*) = rcu_mc_slice_scores;',
        'int (*masks)(const uint64_t*, int, int, const int64_t*, const int32_t*, const float*, int, float*, void*) = rcu_dropout_masks_indexed;',
        'int (*merge)(const void*, size_t, void*, size_t, size_t, int, int, const int32_t*, void*) = rcu_mc_merge_slices;',
        'int (*fin)(const void*, size_t, size_t, int, const int32_t*, int, float*, float*, float*, float*, void*) = rcu_mc_finalize_counts;',
        'int main(void) { printf("%d\\n", RCU_ADAPTIVE_MAX_CHECKPOINTS); return 0; }']) + '\n')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-c', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'adaptive.o')])


def test_arguments_are_checked_before_the_device_is_touched():
    import ctypes
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    so = _lib.load()
    p = ctypes.c_void_p(256)
    assert so.rcu_mc_slice_scores(p, 5, 279, 2, _lib.RCU_MC_MI, 1 << 40, p, p, None) == -1 and b'RCU_MC_EXACT' in so.rcu_last_error()
    assert so.rcu_mc_slice_scores(p, 5, 279, 2, 0, 1 << 40, p, p, None) == -1
    assert so.rcu_mc_slice_scores(None, 5, 279, 2, _lib.RCU_MC_EXACT, 1 << 40, p, p, None) == -1
    assert so.rcu_mc_slice_scores(p, 5, 279, 9, _lib.RCU_MC_EXACT, 1 << 40, p, p, None) == -1
    assert so.rcu_mc_slice_scores(p, 5, 279, 2, _lib.RCU_MC_EXACT, -1, p, p, None) == -1 and b'thr_q' in so.rcu_last_error()
    assert so.rcu_mc_slice_scores(p, 0, 279, 2, _lib.RCU_MC_EXACT, 1, p, p, None) == -1
    seeds, ch, keep = (ctypes.c_uint64 * 2)(1, 2), (ctypes.c_int32 * 2)(8, 8), (ctypes.c_float * 2)(0.9, 0.9)
    assert so.rcu_dropout_masks_indexed(seeds, 2, 1, None, ch, keep, 2, p, None) == -1
    assert so.rcu_dropout_masks_indexed(seeds, 0, 1, p, ch, keep, 2, p, None) == -1
    assert so.rcu_dropout_masks_indexed(seeds, 2, 1, p, ch, keep, 41, p, None) == -1 and b'n_sites' in so.rcu_last_error()
    assert so.rcu_dropout_masks_indexed(seeds, 2, 1 << 27, p, ch, keep, 2, p, None) == -1 and b'2^31' in so.rcu_last_error()
    q = ctypes.c_void_p(1 << 20)
    assert so.rcu_mc_merge_slices(p, 2, q, 5, 279, 2, _lib.RCU_MC_EXACT, None, None) == -1
    assert so.rcu_mc_merge_slices(p, 2, p, 5, 279, 2, _lib.RCU_MC_EXACT, p, None) == -1 and b'overlap' in so.rcu_last_error()
    assert so.rcu_mc_merge_slices(p, 2, q, 5, 279, 2, 16, p, None) == -1 and b'flags' in so.rcu_last_error()
    assert so.rcu_mc_merge_slices(p, 0, q, 5, 279, 2, _lib.RCU_MC_EXACT, p, None) == -1
    assert so.rcu_mc_finalize_counts(p, 5, 279, 2, None, _lib.RCU_MC_EXACT, None, None, None, None, None) == -1
    assert so.rcu_mc_finalize_counts(p, 5, 279, 2, p, _lib.RCU_MC_EXACT, None, None, p, None, None) == -1 and b'RCU_MC_MI' in so.rcu_last_error()
    assert so.rcu_mc_finalize_counts(p, 5, 279, 2, p, _lib.RCU_MC_EXACT, None, None, None, p, None) == -1 and b'RCU_MC_VAR' in so.rcu_last_error()


# ------------------------------------------------------------------------------------------------ the numpy restatement
def test_reference_scores_and_per_slice_finalise_on_a_hand_made_blob():
    q = 2.0 ** -40
    eps, t = 0.01, 3
    thr = ar.thr_q(eps, t)
    # 2 slices of 3 voxels, C = 2, flags EXACT | MI: planes [S_0, S_1, sum H]
    planes = np.zeros((3, 2, 3))
    planes[0, 0] = [3.0, thr * q, (thr - 1) * q]            # slice 0: saturated, exactly on the threshold, one quantum below it
    planes[1, 0] = 3.0 - planes[0, 0]
    planes[0, 1] = [0.25, 1.5, 0.0]                        # slice 1: the leading class is class 1 at voxels 0 and 2
    planes[1, 1] = [2.75, 1.5, 3.0]
    planes[2] = [[0.0, 0.1, 0.2], [0.3, 0.6, 0.0]]
    unsettled, margin = ar.slice_scores(planes, 2, thr)
    assert unsettled.tolist() == [1, 2] and unsettled.dtype == np.uint32
    assert margin.tolist() == [thr - 1, 3 * 2 ** 39] and margin.dtype == np.int64
    assert ar.retired(unsettled).tolist() == [False, False] and ar.retired(unsettled, 1).tolist() == [True, False]
    assert ar.slice_scores(planes, 2, thr - 1)[0].tolist() == [0, 2]
    with pytest.raises(AssertionError):
        ar.leading_q(planes + q / 2, 2)
    # per-slice finalise: slice 0 over 3 passes, slice 1 over 6 (its sums doubled): the same means
    planes[:, 1] *= 2
    out = ar.finalise_counts(planes, 2, [3, 6], ar.EXACT | ar.MI)
    assert out['probabilities'].shape == (2, 2, 3) and out['entropy'].shape == (2, 1, 3)
    assert np.array_equal(out['probabilities'][0, 0], planes[0, 0] / 3) and np.array_equal(out['probabilities'][1, 1], planes[1, 1] / 6)
    assert np.allclose(out['probabilities'].sum(axis=1), 1.0)
    assert out['entropy'][0, 0, 0] == 0.0 and out['entropy'][1, 0, 1] == pytest.approx(np.log(2))
    assert np.allclose(out['mutual_info'][1, 0], out['entropy'][1, 0] - planes[2, 1] / 6)
    # merge: rows land where the index says, a negative entry is skipped, the rest keeps every bit
    dst = np.arange(3 * 4 * 3, dtype=np.float64).reshape(3, 4, 3) * q
    before = dst.copy()
    src = np.ones((3, 3, 3)) * q
    ar.merge_slices(dst, src, [3, -1, 0])
    assert np.array_equal(dst[:, 3], before[:, 3] + q) and np.array_equal(dst[:, 0], before[:, 0] + q)
    assert np.array_equal(dst[:, 1:3], before[:, 1:3])
