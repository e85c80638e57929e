"""MC sample agreement without a GPU: the host arithmetic of evaluation.agreement_metrics against a brute-force computation from explicit
boolean samples, the identities of the integer tables, Spearman's correlation, the pooled CSV of the 'agreement' evaluation action, the C
ABI (symbols, argument validation before the device is touched), the vote bit of a pass under pass groups and lanes, and the scripts and
steps that must refuse the key."""
import csv
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('rcu_unet_forward_accumulate_votes', 'rcu_mc_votes', 'rcu_agreement_tables')


def tables_from_samples(samples):
    """Boolean samples ``[T, V]`` -> (hist ``[T + 1]``, pairs ``[T, T]``) by the definitions of include/rcu.h."""
    samples = np.asarray(samples, dtype=bool)
    t = samples.shape[0]
    hist = np.bincount(samples.sum(axis=0), minlength=t + 1).astype(np.int64)
    s = samples.astype(np.int64)
    return hist, s @ s.T


def brute_force_metrics(samples):
    """The table of ISSUE / evaluation.agreement_metrics, from the sets themselves (no tables)."""
    samples = np.asarray(samples, dtype=bool)
    t = samples.shape[0]
    sizes = [int(a.sum()) for a in samples]
    dices, inter_total = [], 0
    for i, j in itertools.combinations(range(t), 2):
        inter = int((samples[i] & samples[j]).sum())
        inter_total += inter
        dices.append(2.0 * inter / (sizes[i] + sizes[j]) if sizes[i] + sizes[j] else 1.0)
    union, inter_all = int(samples.any(axis=0).sum()), int(samples.all(axis=0).sum())
    mean = sum(sizes) / t
    var = sum((v - mean) ** 2 for v in sizes) / t
    return {'passes': t, 'mean_pairwise_dice': sum(dices) / len(dices), 'min_pairwise_dice': min(dices),
            'pooled_pairwise_dice': 2.0 * inter_total / ((t - 1) * sum(sizes)) if sum(sizes) else 1.0,
            'iou_all': inter_all / union if union else 1.0, 'volume_mean': mean, 'volume_cv': math.sqrt(var) / mean if mean else 0.0,
            'union': union, 'intersection': inter_all}


def _cases():
    rng = np.random.RandomState(11)
    for t in (2, 5, 20):
        yield 't{}_random'.format(t), rng.rand(t, 500) < 0.4
        blob = rng.rand(t, 500) < 0.9
        blob[:, 200:] = False                                  # most voxels background, a core most passes agree on
        yield 't{}_blob'.format(t), blob
        some_empty = rng.rand(t, 300) < 0.5
        some_empty[::2] = False                                # every second sample is empty (pairs of two empty samples: T >= 3)
        yield 't{}_some_empty'.format(t), some_empty
        yield 't{}_all_empty'.format(t), np.zeros((t, 64), dtype=bool)


@pytest.mark.parametrize('name,samples', list(_cases()), ids=[n for n, _ in _cases()])
def test_agreement_metrics_equal_the_brute_force_definitions(name, samples):
    from rcu_amd import evaluation as ev
    hist, pairs = tables_from_samples(samples)
    got, ref = ev.agreement_metrics(hist, pairs), brute_force_metrics(samples)
    assert tuple(got) == ev.AGREEMENT_KEYS and set(ref) == set(got)
    for k in ev.AGREEMENT_KEYS:
        assert abs(got[k] - ref[k]) <= 1e-12, (k, got[k], ref[k])
    for k in ('passes', 'union', 'intersection'):
        assert isinstance(got[k], int) and got[k] == ref[k]
    # the packed upper triangle (what a slice row carries) gives the same
    t = samples.shape[0]
    packed = pairs[np.triu_indices(t)]
    assert np.array_equal(ev.unpack_pairs(packed, t), pairs)
    assert ev.agreement_metrics(hist, packed) == got
    if name.endswith('all_empty'):
        assert (got['mean_pairwise_dice'], got['min_pairwise_dice'], got['pooled_pairwise_dice'], got['iou_all']) == (1.0, 1.0, 1.0, 1.0)
        assert (got['volume_mean'], got['volume_cv'], got['union'], got['intersection']) == (0.0, 0.0, 0, 0)


@pytest.mark.parametrize('t', [2, 5, 20, 33, 64])
def test_table_identities(t):
    """sum_{i<j} I_ij == sum_c C(c, 2) hist[c]  and  sum_i n_i == sum_c c hist[c]: both count (voxel, pair) and (voxel, pass) incidences."""
    from rcu_amd import evaluation as ev
    samples = np.random.RandomState(t).rand(t, 777) < 0.3
    hist, pairs = tables_from_samples(samples)
    c = np.arange(t + 1, dtype=np.int64)
    assert int(np.triu(pairs, 1).sum()) == int((c * (c - 1) // 2 * hist).sum())
    assert int(np.trace(pairs)) == int((c * hist).sum())
    assert int(hist.sum()) == samples.shape[1]
    assert ev.agreement_row_length(t) == hist.size + t * (t + 1) // 2
    # tables of slices add up to the table of the subject
    parts = [tables_from_samples(samples[:, a:b]) for a, b in ((0, 100), (100, 101), (101, 777))]
    assert np.array_equal(sum(p[0] for p in parts), hist) and np.array_equal(sum(p[1] for p in parts), pairs)


def test_agreement_metrics_refuses_mismatched_tables():
    from rcu_amd import evaluation as ev
    with pytest.raises(ValueError):
        ev.agreement_metrics(np.zeros(4), np.zeros((2, 2)))
    with pytest.raises(ValueError):
        ev.agreement_metrics(np.zeros(1), np.zeros((0, 0)))


def test_spearman_is_scipys_with_ties():
    stats = pytest.importorskip('scipy.stats')
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(5)
    for n in (2, 3, 10, 57):
        a = rng.randint(0, 5, n).astype(np.float64)          # many ties
        b = a * 0.5 + rng.randint(0, 3, n)
        ref = stats.spearmanr(a, b)[0]
        got = ev.spearman(a, b)
        assert (math.isnan(got) and math.isnan(ref)) or abs(got - ref) < 1e-12, (n, got, ref)
        assert abs(ev.pearson(a, b) - stats.pearsonr(a, b)[0]) < 1e-12 or np.std(a) == 0 or np.std(b) == 0
    assert np.array_equal(ev.average_ranks([3.0, 1.0, 3.0, 2.0, 3.0]), [4.0, 1.0, 4.0, 2.0, 4.0])
    assert math.isnan(ev.spearman([1.0, 1.0, 1.0], [1.0, 2.0, 3.0])) and math.isnan(ev.spearman([1.0], [2.0]))
    assert ev.spearman([1, 2, 3, 4], [10, 20, 30, 500]) == pytest.approx(1.0, abs=1e-15)


def test_average_ranks_and_failure_auroc_by_hand():
    from rcu_amd import evaluation as ev
    # scores low where the segmentation failed: perfect detection
    assert ev.failure_auroc([0.2, 0.3, 0.9, 0.8], [True, True, False, False], higher_is_worse=False) == 1.0
    assert ev.failure_auroc([0.2, 0.3, 0.9, 0.8], [True, True, False, False], higher_is_worse=True) == 0.0
    # one tie between a failed and a good subject counts half: pairs (f, g): (0.5, 0.5) tie, (0.5, 0.9) ok, (0.1, 0.5) ok, (0.1, 0.9) ok
    assert ev.failure_auroc([0.5, 0.1, 0.5, 0.9], [True, True, False, False], higher_is_worse=False) == 3.5 / 4
    assert math.isnan(ev.failure_auroc([0.5, 0.1], [False, False], higher_is_worse=False))


AGREEMENT_CSV = """subject,passes,mean_pairwise_dice,min_pairwise_dice,pooled_pairwise_dice,iou_all,volume_mean,volume_cv,union,intersection,volume_1,volume_2
s0,2,0.9,0.9,0.9,0.8,100.0,0.01,110,90,99,101
s1,2,0.5,0.5,0.5,0.3,50.0,0.30,80,20,35,65
s2,2,0.7,0.7,0.7,0.5,70.0,0.10,90,50,63,77
s3,2,0.95,0.95,0.95,0.9,10.0,0.02,11,9,10,10
"""


def test_pooled_csv_of_a_hand_made_agreement_csv(tmp_path):
    from rcu_amd import evalrun
    run = tmp_path / 'run'
    run.mkdir()
    (run / 'agreement.csv').write_text(AGREEMENT_CSV)
    dice = {'s0': 0.92, 's1': 0.40, 's2': 0.75, 's3': 0.85}
    action = evalrun.AgreementAction(str(tmp_path / 'eval'), dice_fail=0.8)
    action.setup_eval(evalrun.EvalData('baseline_mc', str(run)))
    action.start_eval()
    for subject in sorted(dice):
        action.record_dice(dice[subject], subject)
    action.finish_eval()
    rows = list(csv.DictReader(open(str(tmp_path / 'eval' / 'uncertainty' / 'eval_agreement_baseline_mc.csv'))))
    assert [r['subject_name'] for r in rows] == ['s0', 's1', 's2', 's3'] and [float(r['dice']) for r in rows] == [0.92, 0.40, 0.75, 0.85]
    assert list(rows[0])[:3] == ['test_id', 'subject_name', 'dice'] and list(rows[0])[3:] == list(evalrun.AGREEMENT_SCORES)
    assert float(rows[1]['iou_all']) == 0.3 and float(rows[3]['volume_cv']) == 0.02
    pooled = {r['score']: r for r in csv.DictReader(open(str(tmp_path / 'eval' / 'uncertainty' / 'eval_agreement_pooled_baseline_mc.csv')))}
    assert set(pooled) == set(evalrun.AGREEMENT_SCORES)
    d = np.array([0.92, 0.40, 0.75, 0.85])
    m = np.array([0.9, 0.5, 0.7, 0.95])
    row = pooled['mean_pairwise_dice']
    assert abs(float(row['pearson']) - np.corrcoef(m, d)[0, 1]) < 1e-12
    assert abs(float(row['spearman']) - 0.8) < 1e-12            # ranks 3 1 2 4 against 4 1 2 3: 1 - 6 * 2 / (4 * 15)
    # failed: s1, s2 (dice < 0.8); their scores 0.5, 0.7 are below those of s0, s3: every (failed, good) pair is ranked right
    assert float(row['auroc_dice_below_0.8']) == 1.0 and (row['subjects'], row['failed'], row['test_id']) == ('4', '2', 'baseline_mc')
    assert float(pooled['volume_cv']['auroc_dice_below_0.8']) == 1.0 and float(pooled['volume_cv']['spearman']) < 0
    # a subject the CSV does not know, and a run without the file (the message names the YAML key)
    with pytest.raises(ValueError, match='s9'):
        action.record_dice(0.5, 's9')
    empty = tmp_path / 'other'
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match='others.agreement'):
        evalrun.AgreementAction(str(tmp_path / 'eval2')).setup_eval(evalrun.EvalData('baseline_mc', str(empty)))
    assert [type(a) for a in evalrun.get_actions(['agreement'], str(tmp_path / 'mm'), str(tmp_path / 'eval3'), '', dice_fail=0.6)] == \
        [evalrun.AgreementAction]


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.fixture(scope='module')
def lib():
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    return _lib


def test_agreement_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, 'include', 'rcu.h')).read()
    declared = set(re.findall(r'\b(rcu_[a-z0-9_]+)\s*\(', header))
    so = lib.load()
    for name in NAMES:
        assert name in declared and name in lib.SIGNATURES and hasattr(so, name), name
    assert '#define RCU_VOTES_MAX_PASSES 64' in header and lib.RCU_VOTES_MAX_PASSES == 64


def _refused(so, status, *words):
    assert status == -1        # RCU_ERR_INVALID
    msg = so.rcu_last_error()
    for w in words:
        assert w in msg, (w, msg)


def test_standalone_argument_validation_without_gpu(lib):
    so = lib.load()
    vol, plane, hist, pairs = (ctypes.c_void_p(v) for v in (1 << 20, 1 << 30, 1 << 31, 1 << 32))

    def votes(i=vol, n=2, hw=64, c=2, flags=lib.RCU_MC_INPUT_PROBS, p=plane, words=1, bit=0):
        return so.rcu_mc_votes(i, n, hw, c, flags, p, words, bit, None)

    def tables(p=plane, words=1, n=1000, vols=3, passes=20, h=hist, pr=pairs):
        return so.rcu_agreement_tables(p, words, n, vols, passes, h, pr, None)

    _refused(so, votes(i=None), b'null')
    _refused(so, votes(p=None), b'null')
    for words in (0, 3, -1):
        _refused(so, votes(words=words), b'n_words')
        _refused(so, tables(words=words), b'n_words')
    for words, bit in ((1, -1), (1, 32), (2, 64), (2, -5)):
        _refused(so, votes(words=words, bit=bit), b'bit')
    for c in (0, 9, -1):
        _refused(so, votes(c=c), b'nb_classes')
    assert votes(n=0) == 0 and votes(hw=0) == 0           # nothing to do: not an error, nothing launched
    _refused(so, tables(p=None), b'null')
    _refused(so, tables(h=None), b'null')
    _refused(so, tables(pr=None), b'null')
    for words, passes in ((1, 0), (1, 33), (2, 65), (1, -2)):
        _refused(so, tables(words=words, passes=passes), b'passes')
    _refused(so, tables(n=0), b'n_per_volume')
    _refused(so, tables(n=(1 << 31) - 1), b'n_per_volume')
    _refused(so, tables(vols=0), b'n_volumes')
    _refused(so, tables(vols=65536), b'n_volumes')
    _refused(so, tables(n=1 << 30, vols=4), b'2^32')


def test_forward_argument_validation_without_gpu(lib):
    so = lib.load()
    x, stats, plane = (ctypes.c_void_p(v) for v in (1 << 20, 1 << 30, 1 << 31))
    bits = (ctypes.c_int32 * 4)(0, 1, 2, 3)

    def fwd(h, xx=x, n=2, passes=4, st=stats, p=plane, words=1, b=bits):
        return so.rcu_unet_forward_accumulate_votes(h, xx, n, passes, None, st, lib.RCU_MC_EXACT, p, words, b, None)

    desc = lib.UnetDesc(nb_classes=2, in_channels=4, depth=2, start_filters=8, has_dropout=1, dropout_center=-1, sigma_out=0, bn=1, height=32,
                        width=32, max_batch=8, residual=0, provide_features=0)
    h = ctypes.c_void_p()
    assert so.rcu_unet_plan(ctypes.byref(desc), None, ctypes.byref(h)) == 0
    try:
        _refused(so, fwd(h, xx=None), b'null')
        _refused(so, fwd(h, st=None), b'null')
        _refused(so, fwd(h, p=None), b'null')
        _refused(so, fwd(h, b=None), b'null')
        _refused(so, fwd(h, words=0), b'n_words')
        _refused(so, fwd(h, words=3), b'n_words')
        _refused(so, fwd(h, b=(ctypes.c_int32 * 4)(0, 1, 32, 3)), b'bit 32')
        _refused(so, fwd(h, b=(ctypes.c_int32 * 4)(0, -1, 2, 3)), b'bit -1')
        _refused(so, fwd(h, words=2, b=(ctypes.c_int32 * 4)(31, 32, 63, 64)), b'bit 64')
        _refused(so, fwd(h, n=3), b'max_batch')        # 3 x 4 > 8
        _refused(so, fwd(h, passes=0), b'max_batch')
    finally:
        so.rcu_unet_destroy(h)
    _refused(so, fwd(None), b'null handle')


# ------------------------------------------------------------------------------------------------ bits, steps, scripts
def test_the_bit_of_a_pass_does_not_depend_on_groups_or_lanes():
    from rcu_amd import steps
    assert [steps.vote_bit(j) for j in (1, 32, 33, 64)] == [0, 31, 32, 63]
    for bad in (0, 65, -1):                                 # the weight-scaling pass (job 0) casts no vote
        with pytest.raises(ValueError):
            steps.vote_bit(bad)
    for t, group, lanes in ((5, 4, 1), (5, 4, 2), (20, 4, 2), (33, 3, 1), (33, 4, 2), (64, 5, 3), (64, 64, 1)):
        plan = steps.launch_plan([0] + list(range(1, t + 1)), (0,), t, group, lanes)
        assert plan[0] == ('ws', 0, 0, (0,))
        seen = {}
        for kind, lane, element, jobs in plan[1:]:
            assert kind == 'passes' and element == 0 and 0 <= lane < lanes and 1 <= len(jobs) <= group
            for j in jobs:
                assert j not in seen
                seen[j] = (steps.vote_bit(j) // 32, steps.vote_bit(j) % 32, lane)
        assert sorted(seen) == list(range(1, t + 1))
        assert all(seen[j][:2] == ((j - 1) // 32, (j - 1) % 32) for j in seen)
        assert len({v[:2] for v in seen.values()}) == t          # every pass its own bit
    # the plan that makes the head launch split at the word boundary: a group with passes 31, 32, 33
    plan = steps.launch_plan(list(range(1, 34)), (0,), 33, 3, 1)
    assert (31, 32, 33) in [jobs for _, _, _, jobs in plan]


def test_steps_validate_agreement():
    from rcu_amd import distributed as rdist
    from rcu_amd import steps
    for bad in (0, 1, 65, 2.0, '20', True, None):
        with pytest.raises(ValueError, match='agreement'):
            steps.McPredictStep(bad, agreement=True)
    assert steps.McPredictStep(2, agreement=True).agreement and steps.McPredictStep(64, agreement=True).agreement
    assert steps.McPredictStep(1).agreement is False and steps.McPredictStep(100).agreement is False
    with pytest.raises(ValueError, match='agreement'):
        rdist.ShardedMcPredictStep(20, rdist.World(rank=0, world=2), seed=3, agreement=True)
    assert rdist.ShardedMcPredictStep(20, rdist.World(rank=0, world=2), seed=3).mc_steps == 20
    with pytest.raises(ValueError):
        steps.SampleVotes(1, 4, 4, 65, 'cpu')
    with pytest.raises(ValueError):
        steps.sample_votes(np.zeros((2, 1, 2, 4, 4)))


def _context(others, seed=20):
    from rcu_amd import config as cfg
    from rcu_amd import loops
    context = loops.TorchTestContext('cpu')
    context.config = cfg.TestConfiguration()
    context.config.seed = seed
    context.config.others = cfg.OtherParameters().from_dict(others)
    return context


def test_default_steps_follow_the_yaml():
    from rcu_amd import distributed as rdist
    from rcu_amd import scripts, steps
    world = rdist.World()
    mc, summary, agreement = scripts._default_steps(_context(dict(mc=20, agreement=True)), world)
    assert type(mc) is steps.McPredictStep and mc.agreement and mc.mc_steps == 20 and mc.seed == 20
    assert type(summary) is steps.MultiPredictionSummary and type(agreement) is steps.SampleAgreementStep
    # false, or absent: the steps of before
    for others in (dict(mc=20, agreement=False), dict(mc=20)):
        mc, summary = scripts._default_steps(_context(others), world)
        assert type(mc) is steps.McPredictStep and mc.agreement is False
    (plain,) = scripts._default_steps(_context(dict(agreement=False)), world)
    assert type(plain) is steps.SegmentationPredictStep
    for others in (dict(agreement=True), dict(mc=20, agreement=True, tta=['identity', 'flip_h']), dict(agreement=True, tta=['identity']),
                   dict(mc=1, agreement=True), dict(mc=65, agreement=True), dict(mc=20, agreement='yes'), dict(mc=20, agreement=1)):
        with pytest.raises(ValueError, match='agreement'):
            scripts._default_steps(_context(others), world)
    with pytest.raises(ValueError, match='others.agreement'):
        scripts._default_steps(_context(dict(mc=20, agreement=True)), rdist.World(rank=0, world=2))


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
    agreement: true
meta:
  type: test-config
  version: 0
"""


@pytest.mark.parametrize('script', ['test_ensemble', 'test_aleatoric', 'test_auxiliary_feat', 'test_auxiliary_segm'])
def test_other_scripts_refuse_the_agreement_key(tmp_path, monkeypatch, script):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    path = tmp_path / 'test_brats_x.yaml'
    path.write_text(YAML.format(test_dir=tmp_path / 'out', model_dir=tmp_path / 'train' / 'model_x'))
    with pytest.raises(ValueError, match='others.agreement'):
        getattr(scripts, script)('brats', config_file=str(path), device='cpu')
    assert not (tmp_path / 'out').exists()


def test_fit_script_and_tta_run_refuse_the_agreement_key(tmp_path, monkeypatch):
    from rcu_amd import scripts
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)
    path = tmp_path / 'fit.yaml'
    path.write_text(YAML.format(test_dir=tmp_path / 'out', model_dir=tmp_path / 'train' / 'model_x'))
    with pytest.raises(ValueError, match='others.agreement'):
        scripts.fit_temperature('brats', str(path), device='cpu')
    tta = tmp_path / 'tta.yaml'
    tta.write_text(YAML.format(test_dir=tmp_path / 'out', model_dir=tmp_path / 'train' / 'model_x').replace('    mc: 20\n', '    mc: 20\n    tta: [identity]\n'))
    with pytest.raises(ValueError, match='others.agreement'):
        scripts.test_default('brats', config_file=str(tta), device='cpu')
    assert not (tmp_path / 'out').exists()
