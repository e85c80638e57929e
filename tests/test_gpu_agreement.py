"""MC sample agreement on the GPU: the pair-count kernel against numpy, the vote kernels against torch's arg-max, the fused MC step with
votes against the replayed passes (pass groups, lanes, word boundary, batching, padded level 0), the script surface and the evaluation
action.  Everything is an integer or a bit: exact equality throughout."""
import csv
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
PARAMS = dict(nb_classes=2, in_channels=4, depth=4, start_filters=32, dropout=0.05)
DEV = 'cuda:0'


# ------------------------------------------------------------------------------------------------ references
def numpy_tables(plane, passes, n_volumes):
    """uint32 plane ``[n_words, V]`` -> (hist ``[vol, T + 1]``, pairs ``[vol, T, T]``) by the definitions of include/rcu.h."""
    plane = np.asarray(plane).view(np.uint32).reshape(plane.shape[0], n_volumes, -1)
    bits = np.stack([(plane[j // 32] >> np.uint32(j % 32)) & np.uint32(1) for j in range(passes)], axis=-1).astype(np.int64)    # [vol, n, T]
    hist = np.stack([np.bincount(b.sum(axis=1), minlength=passes + 1) for b in bits]).astype(np.int64)
    pairs = np.einsum('vni,vnj->vij', bits, bits)
    return hist, pairs


def pack_votes(fg):
    """bool ``[T, ...]`` -> int32 ``[n_words, ...]``: sample t in bit t % 32 of word t // 32."""
    fg = np.asarray(fg, dtype=bool)
    words = np.zeros(((fg.shape[0] + 31) // 32,) + fg.shape[1:], dtype=np.uint32)
    for t in range(fg.shape[0]):
        words[t // 32] |= fg[t].astype(np.uint32) << np.uint32(t % 32)
    return words.view(np.int32)


def votes_of_stack(multi):
    """``[T, N, C, H, W]`` probabilities -> the packed plane torch's arg-max gives (first maximum: ties go to the lower class)."""
    return pack_votes((multi.argmax(dim=2) != 0).cpu().numpy())


# ------------------------------------------------------------------------------------------------ 1. rcu_agreement_tables
def _planes(rng, n_words, n_volumes, n):
    total = n_volumes * n
    last_wave = np.zeros((n_words, total), dtype=np.uint32)
    tail = n - (n // 64) * 64 or 64                                   # the last (partial) wave of every volume
    for v in range(n_volumes):
        last_wave[:, (v + 1) * n - tail:(v + 1) * n] = rng.randint(0, 1 << 32, (n_words, tail), dtype=np.uint64).astype(np.uint32)
    return {'zero': np.zeros((n_words, total), dtype=np.uint32),
            'ones': np.full((n_words, total), 0xFFFFFFFF, dtype=np.uint32),      # (bits at or above T are garbage: they must not count)
            'random': rng.randint(0, 1 << 32, (n_words, total), dtype=np.uint64).astype(np.uint32),
            'last_wave': last_wave}


@pytest.mark.parametrize('n_volumes,n', [(3, 1000), (1, 63), (3, 1001)], ids=['3x1000', '1x63', '3x1001'])
@pytest.mark.parametrize('passes', [2, 20, 32, 33, 64])
def test_agreement_tables_equal_numpy(passes, n_volumes, n):
    """Volume ends inside a wave (1000 = 15 waves + 40; 1001: unaligned volumes, the scalar loads), a volume smaller than a wave, the word
    boundary and both words; all-zero (the skip), all-ones with garbage above T, random, and votes in the last partial wave only."""
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(passes * 7 + n)
    n_words = (passes + 31) // 32
    for name, plane in _planes(rng, n_words, n_volumes, n).items():
        hist, pairs = ev.agreement_tables(plane, passes, n_volumes)
        ref_hist, ref_pairs = numpy_tables(plane, passes, n_volumes)
        assert hist.dtype == np.int64 and pairs.dtype == np.int64 and pairs.shape == (n_volumes, passes, passes), name
        assert np.array_equal(hist, ref_hist), (name, hist, ref_hist)
        assert np.array_equal(pairs, ref_pairs), name
        assert np.array_equal(pairs, pairs.transpose(0, 2, 1)) and int(hist.sum()) == n_volumes * n


def test_agreement_tables_many_groups_per_wave():
    """8 volumes of 200,000 voxels: 32 workgroups per volume, 782 groups of 256 voxels for their 512 waves -- the grid-stride loop and its
    load of the next group; a blob-like plane (most groups skip) and a random one.  The tables of the volumes add up to the whole's."""
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(3)
    n_volumes, n, passes = 8, 200000, 20
    random = rng.randint(0, 1 << 32, (1, n_volumes * n), dtype=np.uint64).astype(np.uint32)
    blob = np.zeros_like(random)
    for v in range(n_volumes):
        blob[0, v * n + 50000:v * n + 54000] = 0xFFFFF
        blob[0, v * n + 54000:v * n + 56000] = random[0, :2000]
    for plane in (random, blob):
        hist, pairs = ev.agreement_tables(plane, passes, n_volumes)
        ref_hist, ref_pairs = numpy_tables(plane, passes, n_volumes)
        assert np.array_equal(hist, ref_hist) and np.array_equal(pairs, ref_pairs)
        whole_hist, whole_pairs = ev.agreement_tables(plane, passes, 1)
        assert np.array_equal(whole_hist[0], hist.sum(axis=0)) and np.array_equal(whole_pairs[0], pairs.sum(axis=0))


# ------------------------------------------------------------------------------------------------ 2. rcu_mc_votes
@pytest.mark.parametrize('shape', [(2, 2, 32, 32), (1, 3, 8, 40)], ids=['2x2x32x32', '1x3x8x40'])
def test_mc_votes_equal_torch_argmax(shape):
    """Probabilities and logits, exact ties (to the lower class), bits 0, 31, 32 and 63; the neighbouring bits stay as they were."""
    from rcu_amd import _lib
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(sum(shape))
    # logits on a grid of quarters: plenty of exact ties, and distinct logits stay distinct through the softmax
    logits = (torch.randint(-4, 5, shape, generator=gen).float() / 4).to(DEV)
    probs = torch.rand(shape, generator=gen).to(DEV)
    probs[:, :, :2] = 0.25                                             # rows where all classes tie: background
    probs[:, 0, 2] = probs[:, c - 1, 2]                                # class 0 ties with the last class
    if c > 2:
        probs[:, 1, 3] = probs[:, 2, 3] = 2.0                          # classes 1 and 2 tie above class 0: foreground
    so = _lib.load()
    for volume, flags in ((probs, _lib.RCU_MC_INPUT_PROBS), (logits, 0)):
        ref = (volume.argmax(dim=1) != 0).cpu().numpy()
        assert 0 < ref.sum() < ref.size
        for bit in (0, 31, 32, 63):
            before = torch.randint(-2 ** 31, 2 ** 31, (2, n, h, w), generator=gen, dtype=torch.int64).to(torch.int32)
            word, mask = bit // 32, np.uint32(1 << (bit % 32))
            before[word] &= ~int(mask) if mask < 2 ** 31 else 0x7FFFFFFF          # the pass's own bit starts clear
            plane = before.to(DEV)
            _lib.check(so.rcu_mc_votes(_lib.ptr(volume), n, h * w, c, flags, _lib.ptr(plane), 2, bit, _lib.current_stream()))
            got, was = plane.cpu().numpy().view(np.uint32), before.numpy().view(np.uint32)
            assert np.array_equal((got[word] & mask) != 0, ref), (bit, flags)
            assert np.array_equal(got[word] & ~mask, was[word] & ~mask) and np.array_equal(got[1 - word], was[1 - word])
        # a one-word plane: the same bits through the Python surface
        if flags:
            from rcu_amd import steps
            votes = steps.sample_votes(torch.stack([volume, volume.flip(0), volume]))
            assert votes.passes == 3 and votes.n_words == 1
            assert np.array_equal(votes.plane.cpu().numpy(), votes_of_stack(torch.stack([volume, volume.flip(0), volume])))


# ------------------------------------------------------------------------------------------------ 3. / 4. the fused step
def balanced_state(state, params, x):
    """``state`` with the classifier's foreground bias moved so that the eval-mode decision boundary runs through the middle of x's voxels
    (the median logit difference becomes 0): the synthetic weights alone call every voxel foreground in every pass, and samples that all
    agree test nothing."""
    from rcu_amd.model import UNet
    model = UNet(**params)
    model.load_state_dict(state)
    logits = model.to(DEV)(x.to(DEV))
    logits = logits[0] if isinstance(logits, tuple) else logits
    shift = float((logits[:, 1] - logits[:, 0]).median())
    out = dict(state)
    bias = out['conv_cls.1.bias'].clone()
    bias[1] -= shift
    out['conv_cls.1.bias'] = bias
    return out


@pytest.fixture(scope='module')
def x_small():
    return torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(20))


@pytest.fixture(scope='module')
def unet(x_small):
    from oracle import unet_oracle as uo
    from rcu_amd.model import UNet
    model = UNet(**PARAMS)
    model.load_state_dict(balanced_state(uo.synthetic_state(20, **PARAMS), PARAMS, x_small))
    return model.to(DEV)


def _run_step(model, x, passes, sample_offset=0, **kw):
    from rcu_amd import steps
    bc = steps.BatchContext({'images': x.clone()}, 0, sample_offset=sample_offset)
    ctx = steps.TorchTestContext(DEV, model)
    steps.McPredictStep(passes, seed=20, **kw)(bc, None, ctx)
    multi = bc.output['multi_probabilities']
    steps.MultiPredictionSummary()(bc, None, ctx)
    return bc, multi


_reference_cache = {}


def _reference(model, x, passes, key):
    """Once per (input, T): the plain step's outputs (agreement=False) and the votes of its replayed passes."""
    if key not in _reference_cache:
        bc, stats = _run_step(model, x, passes)
        _reference_cache[key] = (bc.output['probabilities'].clone(), bc.output['entropy'].clone(), votes_of_stack(stats.as_tensor()))
    return _reference_cache[key]


def _check_against_reference(model, x, passes, key, sample_offset=0, **kw):
    probabilities, entropy, ref_votes = _reference(model, x, passes, key)
    bc, _ = _run_step(model, x, passes, sample_offset, agreement=True, **kw)
    votes = bc.output['sample_votes']
    assert votes.passes == passes and votes.plane.dtype == torch.int32 and tuple(votes.plane.shape) == ((passes + 31) // 32,) + tuple(ref_votes.shape[1:])
    got = votes.plane.cpu().numpy()
    assert np.array_equal(got, ref_votes), (kw, int((got != ref_votes).sum()))
    assert torch.equal(bc.output['probabilities'], probabilities) and torch.equal(bc.output['entropy'], entropy), kw
    return bc


@pytest.mark.parametrize('lanes', [1, 2])
@pytest.mark.parametrize('group', [1, 2, 3, 4])
@pytest.mark.parametrize('passes', [5, 33])
def test_fused_votes_equal_the_replayed_passes(unet, x_small, passes, group, lanes):
    """Votes == arg-max of ``stats.as_tensor()`` bit for bit, whatever the pass groups (1, 2, 3 and 4 passes per launch; 33 passes in groups
    of 3 put passes 31, 32, 33 -- both words -- into one launch) and lanes; the statistics' outputs are those of ``agreement=False``."""
    from rcu_amd import steps
    n, _, h, w = x_small.shape
    # the launches this run makes (what McPredictStep._fused plans): the group size is not capped, and the sizes meant to occur do
    assert steps.pass_group_size(unet, n, h, w, group * n * h * w) == group
    launches = [jobs for kind, _, _, jobs in steps.launch_plan(list(range(passes + 1)), (0,), passes, group, min(lanes, passes)) if kind == 'passes']
    assert sorted(j for jobs in launches for j in jobs) == list(range(1, passes + 1)) and max(len(jobs) for jobs in launches) <= group
    if lanes == 1:
        assert {len(jobs) for jobs in launches} == {group, passes % group} - {0}          # 5: 1 | 2 + 1 | 3 + 2 | 4 + 1 passes per launch
    if (passes, group, lanes) == (33, 3, 1):
        assert (31, 32, 33) in launches          # one launch over both words: the head launch splits on the host
    ref_votes = _reference(unet, x_small, passes, ('small', passes))[2]
    assert 0 < (ref_votes != 0).sum() and len(np.unique(ref_votes)) > 2          # the samples differ: something to get wrong
    _check_against_reference(unet, x_small, passes, ('small', passes), group_pixels=group * n * h * w, lanes=lanes)


@pytest.mark.parametrize('passes', [5, 33])
def test_materialized_votes_and_agreement_rows(unet, x_small, passes):
    from rcu_amd import evaluation as ev
    from rcu_amd import steps
    bc = _check_against_reference(unet, x_small, passes, ('small', passes), materialize=True)
    # the step behind the summary: one row per slice, hist then the upper triangle; sample_votes is consumed
    ref_votes = _reference(unet, x_small, passes, ('small', passes))[2]
    steps.SampleAgreementStep()(bc, None, None)
    rows = bc.output['agreement'].cpu().numpy()
    assert 'sample_votes' not in bc.output and rows.dtype == np.int64 and rows.shape == (2, ev.agreement_row_length(passes))
    hist, pairs = numpy_tables(ref_votes.reshape(ref_votes.shape[0], -1), passes, 2)
    assert np.array_equal(rows[:, :passes + 1], hist)
    assert np.array_equal(ev.unpack_pairs(rows[:, passes + 1:], passes), pairs)


def test_votes_do_not_depend_on_the_batch(unet, x_small):
    """Batch of 2 against two batches of 1 (``sample_offset``): bits are a function of (seed, slice, pass)."""
    ref_votes = _reference(unet, x_small, 5, ('small', 5))[2]
    for i in range(2):
        bc, _ = _run_step(unet, x_small[i:i + 1], 5, sample_offset=i, agreement=True)
        assert np.array_equal(bc.output['sample_votes'].plane.cpu().numpy(), ref_votes[:, i:i + 1]), i


def test_votes_on_a_padded_level_zero(unet):
    """One 240 x 240 slice: level 0 is allocated larger than the image and the head reads that tensor."""
    x = torch.randn(1, 4, 240, 240, generator=torch.Generator().manual_seed(21))
    assert len(np.unique(_reference(unet, x, 3, ('slice240', 3))[2])) > 2          # the samples differ here too
    for lanes in (1, 2):
        _check_against_reference(unet, x, 3, ('slice240', 3), lanes=lanes)


def test_replay_recipe_keeps_working(unet, x_small):
    """The statistics of an agreement step still replay: MultiPredictionSummary asking for more than the step tracked."""
    from rcu_amd import steps
    bc = steps.BatchContext({'images': x_small.clone()}, 0, sample_offset=0)
    ctx = steps.TorchTestContext(DEV, unet)
    steps.McPredictStep(5, seed=20, agreement=True)(bc, None, ctx)
    steps.MultiPredictionSummary(do_mi=True)(bc, None, ctx)
    ref = steps.BatchContext({'images': x_small.clone()}, 0, sample_offset=0)
    steps.McPredictStep(5, seed=20, do_mi=True)(ref, None, ctx)
    steps.MultiPredictionSummary(do_mi=True)(ref, None, ctx)
    assert torch.equal(bc.output['mutual_info'], ref.output['mutual_info']) and torch.equal(bc.output['probabilities'], ref.output['probabilities'])
    assert np.array_equal(bc.output['sample_votes'].plane.cpu().numpy(), _reference(unet, x_small, 5, ('small', 5))[2])


# ------------------------------------------------------------------------------------------------ 5. / 6. scripts and the evaluation action
MC = 6


@pytest.fixture(scope='module')
def script_runs(tmp_path_factory):
    from rcu_amd import scripts
    from test_gpu_scripts import _files, _setup, _with_others
    tmp_path = tmp_path_factory.mktemp('agreement_scripts')
    cfg, vols, states, params = _setup(tmp_path, mc=MC)
    # the checkpoint again, with a decision boundary that runs through the volumes (balanced_state): samples that disagree
    from rcu_amd import management as mgt
    first = torch.from_numpy(vols[sorted(vols)[0]][0]).permute(0, 3, 1, 2).contiguous()
    states = [balanced_state(states[0], params, first)]
    mgt.save_model(mgt.ModelFiles(str(tmp_path / 'train_20'), 'm20'), 'unet', params, states[0], epoch=2)

    def run(suffix, batch_size=None, **others):
        path = _with_others(cfg, suffix, **others)
        if batch_size is not None:
            text = open(path).read()
            assert 'batch_size: 4' in text
            with open(path, 'w') as f:
                f.write(text.replace('batch_size: 4', 'batch_size: {}'.format(batch_size)))
        ctx = scripts.test_default('brats', path, None)
        written = {os.path.basename(f): open(f, 'rb').read() for f in glob.glob(os.path.join(ctx.test_dir, '*'))
                   if os.path.isfile(f) and os.path.basename(f) not in ('config.yaml', 'log.txt')}
        return ctx, written

    runs = {'plain': run('plain'), 'agreement': run('agreement', agreement=True), 'b2': run('b2', batch_size=2, agreement=True),
            'b8': run('b8', batch_size=8, agreement=True), 'loader_batches': run('loader_batches', agreement=True, coalesce_pixels=0)}
    assert set(_files(runs['plain'][0])) <= set(runs['plain'][1])
    return tmp_path, vols, states, params, runs


def test_script_writes_agreement_csv_and_nothing_else_changes(script_runs):
    from rcu_amd import evaluation as ev
    from rcu_amd import steps
    from rcu_amd.model import UNet
    tmp_path, vols, states, params, runs = script_runs
    plain, agreement = runs['plain'][1], runs['agreement'][1]
    assert 'agreement.csv' not in plain and 'metrics.csv' in plain and sum(k.endswith('.nii.gz') for k in plain) == 2 * len(vols)
    assert set(agreement) == set(plain) | {'agreement.csv'}
    for name in plain:                                                  # every other written file, byte for byte
        assert agreement[name] == plain[name], name
    for other in ('b2', 'b8', 'loader_batches'):
        assert runs[other][1]['agreement.csv'] == agreement['agreement.csv'], other
        assert all(runs[other][1][name] == plain[name] for name in plain), other
    rows = list(csv.DictReader(agreement['agreement.csv'].decode().splitlines()))
    assert [r['subject'] for r in rows] == sorted(vols)
    assert list(rows[0]) == ['subject'] + list(ev.AGREEMENT_KEYS) + ['volume_{}'.format(i + 1) for i in range(MC)]
    # the metrics recomputed from a materialised run of the same passes: the YAML's seed, the slices' global indices
    model = UNet(**params)
    model.load_state_dict(states[0])
    model.to(DEV)
    offset = 0
    for row, name in zip(rows, sorted(vols)):
        x = torch.from_numpy(vols[name][0]).permute(0, 3, 1, 2).contiguous()
        bc = steps.BatchContext({'images': x}, 0, sample_offset=offset)
        steps.McPredictStep(MC, seed=20, materialize=True)(bc, None, steps.TorchTestContext(DEV, model))
        offset += x.shape[0]
        plane = votes_of_stack(bc.output['multi_probabilities'])
        hist, pairs = numpy_tables(plane.reshape(plane.shape[0], -1), MC, 1)
        ref = ev.agreement_metrics(hist[0], pairs[0])
        assert ref['union'] > ref['intersection'] >= 0 and 0 < ref['mean_pairwise_dice'] < 1        # the samples do differ
        for k in ev.AGREEMENT_KEYS:
            assert float(row[k]) == ref[k], (name, k, row[k], ref[k])
        assert [int(row['volume_{}'.format(i + 1)]) for i in range(MC)] == [int(pairs[0][i, i]) for i in range(MC)]


def test_agreement_action_writes_its_files_and_leaves_the_others(script_runs):
    from rcu_amd import evalrun, nifti, scripts
    tmp_path, vols, _, _, runs = script_runs
    gt = tmp_path / 'gt' / 'HGG'
    for name, (images, labels, props) in vols.items():
        (gt / name).mkdir(parents=True)
        for mod, arr in (('flair', images[..., 0]), ('t1', images[..., 1]), ('t2', images[..., 2]), ('t1ce', images[..., 3]), ('seg', labels * 4)):
            nifti.write(str(gt / name / '{}_{}.nii.gz'.format(name, mod)), arr, props)
    run_dir = runs['agreement'][0].test_dir

    def evaluate(out, actions, **kw):
        scripts.eval_uncertainty('brats', {'baseline_mc': run_dir}, str(tmp_path / 'gt'), str(tmp_path / out), actions=actions, **kw)
        return {os.path.relpath(f, str(tmp_path / out)): open(f, 'rb').read() for f in glob.glob(str(tmp_path / out / '**' / '*.csv'), recursive=True)}

    base = evaluate('eval_base', ('minmax', 'ece_dice', 'bnf_ue'))
    with_agreement = evaluate('eval_agreement', ('minmax', 'ece_dice', 'bnf_ue', 'agreement'), dice_fail=0.5)
    new = {os.path.join('uncertainty', 'eval_agreement_baseline_mc.csv'), os.path.join('uncertainty', 'eval_agreement_pooled_baseline_mc.csv')}
    assert set(with_agreement) == set(base) | new
    assert all(with_agreement[k] == base[k] for k in base)
    alone_plain = evaluate('eval_alone', ('agreement',), dice_fail=0.5, fused=False)           # the subject-by-subject loop: the same rows
    assert set(alone_plain) == new and all(alone_plain[k] == with_agreement[k] for k in new)
    rows = list(csv.DictReader(with_agreement[os.path.join('uncertainty', 'eval_agreement_baseline_mc.csv')].decode().splitlines()))
    metrics = {r['subject']: r for r in csv.DictReader(runs['agreement'][1]['metrics.csv'].decode().splitlines())}
    table = {r['subject']: r for r in csv.DictReader(runs['agreement'][1]['agreement.csv'].decode().splitlines())}
    assert [r['subject_name'] for r in rows] == sorted(vols)
    for r in rows:
        assert float(r['dice']) == float(metrics[r['subject_name']]['dice'])
        assert all(float(r[k]) == float(table[r['subject_name']][k]) for k in evalrun.AGREEMENT_SCORES)
    pooled = list(csv.DictReader(with_agreement[os.path.join('uncertainty', 'eval_agreement_pooled_baseline_mc.csv')].decode().splitlines()))
    assert [r['score'] for r in pooled] == list(evalrun.AGREEMENT_SCORES) and all(r['subjects'] == str(len(vols)) for r in pooled)
    assert 'auroc_dice_below_0.5' in pooled[0]
    # a run without agreement.csv: the message names the YAML key
    with pytest.raises(FileNotFoundError, match='others.agreement'):
        scripts.eval_uncertainty('brats', {'baseline_mc': runs['plain'][0].test_dir}, str(tmp_path / 'gt'), str(tmp_path / 'eval_missing'),
                                 actions=('agreement',))
