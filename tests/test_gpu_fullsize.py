"""Parity at BASELINE.json's full sizes and at the shapes real data has (VERDICT r01 weak points 1-2).

* The 160-slice BraTS launch (4 x 160 x 192 x 128): the work-item arithmetic that only triggers at N = 160 (tile ids by
  reciprocal multiplication, 256-workgroup grids streaming over thousands of tiles).  The first / middle / last slices of the
  160-slice launch are compared bit for bit with an 8-slice launch of the same slices (slices are independent and every
  kernel sums in a fixed order) and with the oracle; the fused forward + softmax + accumulate path likewise with injected masks.
* Native BraTS 240 x 240 slices (levels 240/120/60/30/15: no whole Winograd tile below the first level -> padded levels, round 6:
  csrc/rcu_plan.hip plan_unet), the reference's real ISIC size 192 x 256 (scripts/prepare_isic_data.py:29-30) and
  3 x 256 x 256, full width, against the oracle, asserting which kernel every layer got.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOGIT_TOL = 2e-6
PROB_TOL = 1e-4
PARAMS = dict(nb_classes=2, in_channels=4, depth=4, start_filters=32, dropout=0.05)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda')


def _model(params, state, dev):
    from rcu_amd.model import UNet
    m = UNet(**params)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    return m.to(dev)


def _maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


@pytest.mark.timeout(900)
def test_160_slice_launch_vs_8_slice_launch_and_oracle(dev):
    from oracle import summary_oracle as so
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    st = uo.synthetic_state(31, **PARAMS)
    g = torch.Generator().manual_seed(9)
    n, h, w = 160, 192, 128
    x = torch.randn(n, 4, h, w, generator=g)
    _, sites = uo.unet_plan(**PARAMS)
    T = 3
    mask_sets = [uo.sample_masks(sites, n, 0.3, g) for _ in range(T)]
    sel = np.r_[0:8, 76:84, 152:160]                           # first, middle and last eight slices
    groups = [sel[0:8], sel[8:16], sel[16:24]]
    big = _model(PARAMS, st, dev)
    small = _model(PARAMS, st, dev)
    xd = x.to(dev)
    assert big.layer_table(h, w, n)[1]['kernel'] == small.layer_table(h, w, 8)[1]['kernel']

    # eval pass and one stochastic pass: logits of the 160-slice launch
    for mk in (None, mask_sets[0]):
        out = big(xd, mk).cpu().numpy()
        for rows in groups:
            mk8 = None if mk is None else [m[rows] for m in mk]
            out8 = small(xd[rows], mk8).cpu().numpy()
            assert np.array_equal(out[rows], out8), 'a slice depends on the batch it is launched in'
            ref = uo.unet_forward(st, x[rows], mk8, **PARAMS).numpy()
            assert _maxdiff(out[rows], ref) < LOGIT_TOL

    # the fused path of the timed bench: T passes accumulated into the statistics, float32 and float64 (variance) blobs
    for do_var in (False, True):
        stats = steps.McStatistics(n, 2, h, w, dev, do_mi=True, do_var=do_var)
        for mk in mask_sets:
            big.forward_accumulate(xd, stats, mk)
        summary = stats.finalize(True, do_var)
        for rows in groups:
            s8 = steps.McStatistics(8, 2, h, w, dev, do_mi=True, do_var=do_var)
            for mk in mask_sets:
                small.forward_accumulate(xd[rows], s8, [m[rows] for m in mk])
            sum8 = s8.finalize(True, do_var)
            for key in summary:
                assert torch.equal(summary[key][rows], sum8[key]), key
            multi = torch.stack([torch.softmax(uo.unet_forward(st, x[rows], [m[rows] for m in mk], **PARAMS), 1) for mk in mask_sets])
            ref = so.multi_prediction_summary(multi, True, do_var)
            for key in summary:
                assert _maxdiff(summary[key][rows].cpu().numpy(), ref[key].numpy()) < PROB_TOL, key


@pytest.mark.timeout(900)
@pytest.mark.parametrize('cin,n,h,w', [(4, 5, 240, 240), (3, 2, 192, 256), (3, 2, 256, 256)])
def test_real_data_shapes_full_width_vs_oracle(dev, cin, n, h, w):
    from oracle import unet_oracle as uo
    params = dict(PARAMS, in_channels=cin)
    st = uo.synthetic_state(33, **params)
    g = torch.Generator().manual_seed(10)
    x = torch.rand(n, cin, h, w, generator=g) if cin == 3 else torch.randn(n, cin, h, w, generator=g)
    _, sites = uo.unet_plan(**params)
    masks = uo.sample_masks(sites, n, 0.3, g)
    m = _model(params, st, dev)
    rows = m.layer_table(h, w, n)
    assert len(rows) == 23                                       # 19 conv units (conv_cls.0 last) + 4 up-convolutions
    # kernel selection (csrc/rcu_plan.hip, pick_config): which family every layer got at this shape
    kernels = [r['kernel'] for r in rows]
    # the first unit on its own kernel (whole 8x32 tiles), every other layer on a Winograd kernel -- at 240x240 (levels 240 / 120 / 60 / 30 / 15) and
    # at 192x256's 12x16 bottom level through levels ALLOCATED with whole-tile extents (rcu_unet_options.pad_levels; rounds 1-5: >= 16 of the 23
    # layers of a 240x240 slice ran the direct kernels)
    assert kernels[0].startswith('conv3x3_first'), kernels
    assert sum('winograd' in k for k in kernels[1:]) == 22, kernels
    grids = {(r['height'], r['width'], r['grid_height'], r['grid_width']) for r in rows if not r['upsample']}
    if (h, w) == (240, 240):
        assert {(120, 120, 128, 128), (60, 60, 64, 64), (30, 30, 32, 32), (15, 15, 16, 16)} <= grids, grids
    elif (h, w) == (192, 256):
        assert (12, 16, 16, 16) in grids and (192, 256, 192, 256) in grids, grids
    else:
        assert all(g[:2] == g[2:] for g in grids), grids
    for mk in (None, masks):
        ref = uo.unet_forward(st, x, mk, **params).numpy()
        out = m(x.to(dev), mk).cpu().numpy()
        assert _maxdiff(out, ref) < LOGIT_TOL
        assert _maxdiff(torch.softmax(torch.from_numpy(out), 1).numpy(), torch.softmax(torch.from_numpy(ref), 1).numpy()) < PROB_TOL


@pytest.mark.timeout(900)
def test_pass_pair_of_the_full_volume_is_bit_identical_to_single_passes(dev):
    """The headline path runs the MC passes of a 160-slice volume four (round 2-3: two) per launch (640 samples: the 48x32 / 24x16 / 12x8
    levels then fill their last round of workgroups; every tensor still below 2 GB): rcu_unet_forward_accumulate_passes at N = 160 must give
    exactly the statistics of single-pass launches under the same masks -- in pairs and in fours -- through McPredictStep too (its default
    GROUP_PIXELS takes four passes per launch; its default two stream lanes change the summation order only)."""
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    st = uo.synthetic_state(35, **PARAMS)
    g = torch.Generator().manual_seed(12)
    n, h, w = 160, 192, 128
    x = torch.randn(n, 4, h, w, generator=g).to(dev)
    _, sites = uo.unet_plan(**PARAMS)
    mask_sets = [uo.sample_masks(sites, n, 0.3, g) for _ in range(8)]
    model = _model(PARAMS, st, dev)
    # ONE plan for single passes, pairs and fours, as the predict steps make it (steps.reserve_canonical_plans): which kernel a layer gets depends
    # on the batch its plan is sized for -- the 12x8 level runs F(4x4,3x3) in a 640-sample plan and F(2x2,3x3) in a 160-sample one -- and a
    # pass's bits are a property of the plan
    model.reserve(h, w, 4 * n)
    single = steps.McStatistics(n, 2, h, w, dev, do_mi=True)
    for ms in mask_sets:
        model.forward_accumulate(x, single, ms)
    paired = steps.McStatistics(n, 2, h, w, dev, do_mi=True)
    for k in range(0, 8, 2):
        model.forward_accumulate(x, paired, mask_sets[k:k + 2], passes=2)
    assert torch.equal(single.blob, paired.blob)
    fours = steps.McStatistics(n, 2, h, w, dev, do_mi=True)
    model.forward_accumulate(x, fours, mask_sets[:4], passes=4)
    model.forward_accumulate(x, fours, mask_sets[4:], passes=4)
    assert torch.equal(single.blob, fours.blob)
    # ... and exactly the statistics of the standalone head kernel behind conv_cls.0's plain epilogue: at this size every workgroup of the fused
    # F(4x4,3x3) head kernel walks 60 tiles, its waves drifting apart between the chunk barriers -- the wave-local LDS hand-over of the head
    # (csrc/rcu_wino4.hip, wino4_epilogue_head) must not depend on that
    assert [r['kernel'] for r in model.layer_table(h, w, 4 * n) if r['head_fusable']] == ['conv3x3_winograd4<T32x32,N32,K8>']
    model.set_fuse_head(False)
    unfused = steps.McStatistics(n, 2, h, w, dev, do_mi=True)
    model.forward_accumulate(x, unfused, mask_sets[:4], passes=4)
    model.forward_accumulate(x, unfused, mask_sets[4:], passes=4)
    model.set_fuse_head(True)
    assert torch.equal(fours.blob, unfused.blob)
    # no layer of the 640-sample plan has left the Winograd kernels (an up-convolution reads the LOW-resolution grid: 1.0 GB, not 3 GB)
    assert not [r['kernel'] for r in model.layer_table(h, w, 4 * n) if 'igemm' in r['kernel']]
    assert steps.pass_group_size(model, n, h, w, steps.McPredictStep.GROUP_PIXELS) == 4
    assert steps.balanced_groups(8, 4, 2) == [4, 4]
    ctx = steps.TorchTestContext('cuda', model)
    outs = []
    for group_pixels, lanes in ((0, 1), (None, 1), (None, 2), (None, 2)):
        bc = steps.BatchContext({'images': x}, 0)
        steps.McPredictStep(8, do_mi=True, masks=mask_sets, group_pixels=group_pixels, lanes=lanes)(bc, None, ctx)
        steps.MultiPredictionSummary(do_mi=True)(bc, None, ctx)
        outs.append(bc.output)
    for key in ('probabilities', 'entropy', 'mutual_info', 'ws_probabilities'):
        assert torch.equal(outs[0][key], outs[1][key]), key          # one stream: pairs == single passes, bit for bit
        # two stream lanes (the default): each lane sums its own passes and the sums are added -- float32 summation order -- and the
        # assignment of launches to lanes is fixed, so a second run gives the same bits
        assert float((outs[2][key] - outs[1][key]).abs().max()) < 1e-6, key
        assert torch.equal(outs[2][key], outs[3][key]), key


@pytest.mark.timeout(900)
@pytest.mark.parametrize('cin,n,h,w', [(4, 3, 100, 100), (3, 2, 150, 200), (4, 2, 40, 32), (3, 1, 77, 51)])
def test_centre_pad_shapes_full_width_vs_oracle(dev, cin, n, h, w):
    """Sizes that 2^depth does not divide: max-pool floors (unet.py:94), the up-convolution comes out smaller than the skip tensor and
    is zero-padded around its centre before the concatenation (unet.py:110-116).  Full width, against the oracle, masks injected;
    a smaller batch on the same plan gives the same bits (the padded border is written once, at plan creation)."""
    from oracle import unet_oracle as uo
    params = dict(PARAMS, in_channels=cin)
    st = uo.synthetic_state(37, **params)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(n, cin, h, w, generator=g)
    _, sites = uo.unet_plan(**params)
    masks = uo.sample_masks(sites, n, 0.3, g)
    m = _model(params, st, dev)
    rows = m.layer_table(h, w, n)
    assert any(r['upsample'] and (r['height'] % 2 or r['width'] % 2) for r in rows)       # at least one padded up-convolution
    for mk in (None, masks):
        ref = uo.unet_forward(st, x, mk, **params).numpy()
        out = m(x.to(dev), mk).cpu().numpy()
        assert out.shape == ref.shape
        assert _maxdiff(out, ref) < LOGIT_TOL
    if n > 1:
        assert np.array_equal(m(x[:1].to(dev), [mk[:1] for mk in masks]).cpu().numpy(), out[:1])


def _split_masks(model, flat, n, rows):
    """Concatenated device mask tensor [site][n][C_site] -> per-site [len(rows), C_site] CPU tensors."""
    out, off = [], 0
    for _, c in model.dropout_sites():
        out.append(flat[off:off + n * c].view(n, c)[rows].cpu())
        off += n * c
    return out


@pytest.mark.timeout(1200)
def test_ensemble_of_ten_members_on_the_full_volume(dev):
    """BASELINE configs[3] at full size on one GPU: K = 10 members over the 160-slice volume through the runner the bench uses
    (ShardedEnsembleRunner, two stream lanes, one launch per member).  Eight slices against the oracle's ten forwards; the 160-slice
    launches bit-identical to 8-slice launches of the same slices (one lane); lanes and member order change the float32 summation
    order only; same bits run after run; the step seam (EnsemblePredictionStep) gives the runner's result."""
    from oracle import summary_oracle as so
    from oracle import unet_oracle as uo
    from rcu_amd import distributed as rdist
    from rcu_amd import steps
    K = 10
    n, h, w = 160, 192, 128
    states = [uo.synthetic_state(50 + k, **PARAMS) for k in range(K)]
    members = [_model(PARAMS, st, dev) for st in states]
    g = torch.Generator().manual_seed(21)
    x = torch.randn(n, 4, h, w, generator=g)
    xd = x.to(dev)
    sel = np.r_[0:3, 78:81, 158:160]
    two = rdist.ShardedEnsembleRunner(members, lanes=2)
    out = two.step(xd, 0)
    assert two.forwards_run == K and set(out) == {'probabilities', 'entropy'}
    again = two.step(xd, 1)
    for key in out:
        assert torch.equal(out[key], again[key]), key                       # fixed launch -> lane assignment: same bits
    one = rdist.ShardedEnsembleRunner(members, lanes=1).step(xd, 0)
    rev = rdist.ShardedEnsembleRunner(members[::-1], lanes=1).step(xd, 0)
    for key in out:
        assert float((out[key] - one[key]).abs().max()) < 1e-6, key
        assert float((rev[key] - one[key]).abs().max()) < 1e-6, key
    small = rdist.ShardedEnsembleRunner([_model(PARAMS, st, dev) for st in states], lanes=1).step(xd[sel], 0)
    for key in out:
        assert torch.equal(one[key][sel], small[key]), key                  # a slice does not depend on the batch it runs in
    multi = so.ensemble_probabilities([lambda xx, m, st=st: uo.unet_forward(st, xx, m, **PARAMS) for st in states], x[sel])
    ref = so.multi_prediction_summary(multi)
    for key in ('probabilities', 'entropy'):
        assert _maxdiff(out[key][sel].cpu().numpy(), ref[key].numpy()) < PROB_TOL, key
    bc = steps.BatchContext({'images': x}, 0)
    ctx = steps.TorchTestContext('cuda', members[0])
    steps.EnsemblePredictionStep(members[1:])(bc, None, ctx)
    steps.MultiPredictionSummary()(bc, None, ctx)
    for key in ('probabilities', 'entropy'):
        assert torch.equal(bc.output[key], out[key]), key
    p = out['probabilities']
    assert float((p.sum(1) - 1).abs().max()) < 1e-6 and float(out['entropy'].min()) >= 0 and float(out['entropy'].max()) <= np.log(2) + 1e-6


@pytest.mark.timeout(1200)
def test_sigma_head_mc50_on_the_full_volume(dev):
    """BASELINE configs[4] at full size on one GPU: sigma-head U-Net, T = 50 stochastic passes + the weight-scaling pass over the
    160-slice volume through ShardedAleatoricMcRunner (pass pairs, two stream lanes, masks drawn per (seed, volume, pass)).  Four
    slices against the composed oracle (the reference's pieces: customsteps.py:16-39, brats_test_aleatoric.py:57-73) under the very
    masks the runner drew; pass pairs == single passes bit for bit (one lane); lanes within float32 summation order; same seed, same
    bits."""
    from oracle import summary_oracle as so
    from oracle import unet_oracle as uo
    from rcu_amd import distributed as rdist
    params = dict(PARAMS, sigma_out=True)
    st = uo.synthetic_state(61, **params)
    T = 50
    n, h, w = 160, 192, 128
    model = _model(params, st, dev)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(n, 4, h, w, generator=g)
    xd = x.to(dev)
    sel = np.array([0, 79, 80, 159])
    runner = rdist.ShardedAleatoricMcRunner(model, T, seed=7, lanes=2, pass_group=2)
    out = runner.step(xd, 3)
    assert runner.forwards_run == T + 1
    assert set(out) == {'probabilities', 'entropy', 'sigma', 'ws_probabilities', 'ws_sigma'}
    again = rdist.ShardedAleatoricMcRunner(model, T, seed=7, lanes=2, pass_group=2).step(xd, 3)
    pairs = rdist.ShardedAleatoricMcRunner(model, T, seed=7, lanes=1, pass_group=2).step(xd, 3)
    singles = rdist.ShardedAleatoricMcRunner(model, T, seed=7, lanes=1, pass_group=1).step(xd, 3)
    other = rdist.ShardedAleatoricMcRunner(model, T, seed=8, lanes=2, pass_group=2).step(xd, 3)
    for key in out:
        assert torch.equal(out[key], again[key]), key
        assert torch.equal(pairs[key], singles[key]), key
        assert float((out[key] - pairs[key]).abs().max()) < 1e-5 * max(1.0, float(pairs[key].abs().max())), key
    assert float((out['probabilities'] - other['probabilities']).abs().max()) > 1e-5          # the seed matters
    assert torch.equal(out['ws_probabilities'], other['ws_probabilities'])                     # ... but not for the deterministic pass
    # the composed oracle on four slices under the runner's masks
    rows = torch.as_tensor(sel)
    mask_sets = [_split_masks(model, runner.masks_of(xd, 3, j), n, rows) for j in range(1, T + 1)]
    xs = x[sel]
    lg0, raw0 = uo.unet_forward(st, xs, None, **params)
    passes = [uo.unet_forward(st, xs, mk, **params) for mk in mask_sets]
    multi = torch.stack([torch.softmax(lg, 1) for lg, _ in passes])
    ref = so.multi_prediction_summary(multi)
    sigma_ref = torch.stack([raw.abs() for _, raw in passes]).mean(0)
    assert _maxdiff(out['probabilities'][sel].cpu().numpy(), ref['probabilities'].numpy()) < PROB_TOL
    assert _maxdiff(out['entropy'][sel].cpu().numpy(), ref['entropy'].numpy()) < PROB_TOL
    assert _maxdiff(out['ws_probabilities'][sel].cpu().numpy(), torch.softmax(lg0, 1).numpy()) < PROB_TOL
    scale = max(1.0, float(sigma_ref.max()))
    assert _maxdiff(out['sigma'][sel].cpu().numpy(), sigma_ref.numpy()) < PROB_TOL * scale
    assert _maxdiff(out['ws_sigma'][sel].cpu().numpy(), raw0.abs().numpy()) < PROB_TOL * scale
    assert float(out['sigma'].min()) >= 0


@pytest.mark.timeout(1200)
def test_isic_batch32_mc20_through_the_runner(dev):
    """BASELINE configs[1] at full size: 32 images of 3 x 256 x 256, T = 20 MC-dropout passes + the weight-scaling pass through
    ShardedMcRunner as `bench.py --workload isic` runs it (pass triples, two stream lanes, masks per (seed, volume, pass)).  Two images
    against the oracle's 21 forwards under the runner's masks; pass groups == single passes bit for bit (one lane); lanes within
    float32 summation order; same seed, same bits; all 32 images of the batch launch bit-identical to a 2-image launch."""
    from oracle import summary_oracle as so
    from oracle import unet_oracle as uo
    from rcu_amd import distributed as rdist
    from rcu_amd import steps
    params = dict(nb_classes=2, in_channels=3, depth=4, start_filters=32, dropout=0.05)
    st = uo.synthetic_state(71, **params)
    T, n, h, w = 20, 32, 256, 256
    model = _model(params, st, dev)
    g = torch.Generator().manual_seed(23)
    x = torch.rand(n, 3, h, w, generator=g)
    xd = x.to(dev)
    group = steps.pass_group_size(model, n, h, w, steps.McPredictStep.GROUP_PIXELS)
    assert group == 7                                # 224 samples: 1.88 GB for the widest tensor; two lanes run 7 7 | 3 3
    sel = np.array([0, 31])
    runner = rdist.ShardedMcRunner(model, T, seed=9, lanes=2, pass_group=group)
    out = runner.step(xd, 2)
    assert runner.forwards_run == T + 1 and set(out) == {'probabilities', 'entropy', 'ws_probabilities'}
    again = rdist.ShardedMcRunner(model, T, seed=9, lanes=2, pass_group=group).step(xd, 2)
    triples = rdist.ShardedMcRunner(model, T, seed=9, lanes=1, pass_group=group).step(xd, 2)
    singles = rdist.ShardedMcRunner(model, T, seed=9, lanes=1, pass_group=1).step(xd, 2)
    for key in out:
        assert torch.equal(out[key], again[key]), key
        assert torch.equal(triples[key], singles[key]), key
        assert float((out[key] - triples[key]).abs().max()) < 1e-6, key
    rows = torch.as_tensor(sel)
    mask_sets = [_split_masks(model, runner.masks_of(xd, 2, j), n, rows) for j in range(1, T + 1)]
    small = rdist.ShardedMcRunner(model, T, lanes=1, pass_group=1).step(xd[sel], 2, mask_sets=mask_sets)
    for key in out:
        assert torch.equal(singles[key][sel], small[key]), key          # an image does not depend on the batch it runs in
    ws, multi = so.mc_probabilities(lambda xx, mk: uo.unet_forward(st, xx, mk, **params), x[sel], mask_sets)
    ref = so.multi_prediction_summary(multi)
    assert _maxdiff(out['probabilities'][sel].cpu().numpy(), ref['probabilities'].numpy()) < PROB_TOL
    assert _maxdiff(out['entropy'][sel].cpu().numpy(), ref['entropy'].numpy()) < PROB_TOL
    assert _maxdiff(out['ws_probabilities'][sel].cpu().numpy(), ws.numpy()) < PROB_TOL


@pytest.mark.timeout(1200)
def test_brats_mc20_on_the_full_volume(dev):
    """BASELINE configs[2] at its own T (config/test_brats_baseline_mc.yaml:9: mc 20): the 160-slice volume, T = 20 MC-dropout passes + the
    weight-scaling pass through ShardedMcRunner exactly as `bench.py` runs it -- pass groups from steps.pass_group_size (4 passes = 640
    samples per launch), steps.balanced_groups over two stream lanes (4 4 | 4 4 | 2 2), masks drawn per (seed, volume, pass), exact
    statistics -- and through the step seam (McPredictStep + MultiPredictionSummary under the same seed).  Four slices against the oracle's
    21 forwards under the runner's masks -- mean + entropy, and with every output tracked (mutual information + variance) --; and, because
    the sums are exact and the plans canonical: groups of four == pairs == single passes, two lanes == one lane, runner == step seam, all
    bit for bit; same seed, same bits; a slice does not depend on the batch it runs in."""
    from oracle import summary_oracle as so
    from oracle import unet_oracle as uo
    from rcu_amd import distributed as rdist
    from rcu_amd import steps
    st = uo.synthetic_state(81, **PARAMS)
    T, n, h, w = 20, 160, 192, 128
    model = _model(PARAMS, st, dev)
    g = torch.Generator().manual_seed(24)
    x = torch.randn(n, 4, h, w, generator=g)
    xd = x.to(dev)
    sel = np.array([0, 79, 80, 159])
    group = steps.pass_group_size(model, n, h, w, steps.McPredictStep.GROUP_PIXELS)
    assert group == 4 and steps.balanced_groups(T, group, 2) == [4, 4, 4, 4, 2, 2]          # what bench.py runs
    runner = rdist.ShardedMcRunner(model, T, seed=11, lanes=2, pass_group=group)
    out = runner.step(xd, 5)
    assert runner.forwards_run == T + 1 and set(out) == {'probabilities', 'entropy', 'ws_probabilities'}
    again = rdist.ShardedMcRunner(model, T, seed=11, lanes=2, pass_group=group).step(xd, 5)
    one_lane = rdist.ShardedMcRunner(model, T, seed=11, lanes=1, pass_group=group).step(xd, 5)
    pairs = rdist.ShardedMcRunner(model, T, seed=11, lanes=2, pass_group=2).step(xd, 5)
    singles = rdist.ShardedMcRunner(model, T, seed=11, lanes=1, pass_group=1).step(xd, 5)
    other = rdist.ShardedMcRunner(model, T, seed=12, lanes=2, pass_group=group).step(xd, 5)
    for key in out:
        for name, res in (('again', again), ('one lane', one_lane), ('pairs', pairs), ('singles', singles)):
            assert torch.equal(out[key], res[key]), (key, name)
    assert float((out['probabilities'] - other['probabilities']).abs().max()) > 1e-5          # the seed matters
    assert torch.equal(out['ws_probabilities'], other['ws_probabilities'])                     # ... but not for the deterministic pass
    rows = torch.as_tensor(sel)
    mask_sets = [_split_masks(model, runner.masks_of(xd, 5, j), n, rows) for j in range(1, T + 1)]
    small = rdist.ShardedMcRunner(model, T, lanes=1, pass_group=1).step(xd[sel], 5, mask_sets=mask_sets)
    for key in out:
        assert torch.equal(singles[key][sel], small[key]), key
    ws, multi = so.mc_probabilities(lambda xx, mk: uo.unet_forward(st, xx, mk, **PARAMS), x[sel], mask_sets)
    ref = so.multi_prediction_summary(multi, True, True)
    for key in ('probabilities', 'entropy'):
        assert _maxdiff(out[key][sel].cpu().numpy(), ref[key].numpy()) < PROB_TOL, key
    assert _maxdiff(out['ws_probabilities'][sel].cpu().numpy(), ws.numpy()) < PROB_TOL
    # every output (what `bench.py`'s all_outputs record times): the same passes into the S = 5 statistics
    full = rdist.ShardedMcRunner(model, T, seed=11, lanes=2, pass_group=group, do_mi=True, do_var=True).step(xd, 5)
    assert set(full) == {'probabilities', 'entropy', 'mutual_info', 'variance', 'ws_probabilities'}
    for key in ('probabilities', 'entropy', 'mutual_info', 'variance'):
        assert _maxdiff(full[key][sel].cpu().numpy(), ref[key].numpy()) < PROB_TOL, key
    assert float(full["variance"].min()) >= 0 and float(full['mutual_info'].min()) > -1e-6
    assert torch.equal(full['probabilities'], out['probabilities']) and torch.equal(full['entropy'], out['entropy'])   # the same exact sums
    # the step seam on the same volume under the same seed (the scripts pass the YAML seed): the runner's bits, stochastic outputs included
    bc = steps.BatchContext({'images': x}, 5)
    ctx = steps.TorchTestContext('cuda', model)
    steps.McPredictStep(T, seed=11)(bc, None, ctx)
    steps.MultiPredictionSummary()(bc, None, ctx)
    for key in ('probabilities', 'entropy', 'ws_probabilities'):
        assert torch.equal(bc.output[key], out[key]), key
    # without a seed the step draws from the device generator: another valid summary of 20 passes
    torch.manual_seed(3)
    bc = steps.BatchContext({'images': x}, 0)
    steps.McPredictStep(T)(bc, None, ctx)
    steps.MultiPredictionSummary()(bc, None, ctx)
    assert torch.equal(bc.output['ws_probabilities'], out['ws_probabilities'])
    p = bc.output['probabilities']
    assert float((p.sum(1) - 1).abs().max()) < 1e-6 and 0 < float((p - out['probabilities']).abs().max()) < 0.5
    assert float(bc.output['entropy'].min()) >= 0 and float(bc.output['entropy'].max()) <= np.log(2) + 1e-6


@pytest.mark.timeout(900)
def test_ensemble_members_share_one_activation_workspace(dev):
    """Members 2..K of an ensemble borrow the activation workspace of the first (rcu_unet_create_with's donor, include/rcu.h; the K
    resident models of bin-dl/brats_test_ensemble.py:44-57 differ in 35 MB of packed weights): a borrower owns < 50 MB at 160 slices,
    the owner the 6 GB; outputs carry the bits of members with workspaces of their own; destroying the owner first is safe."""
    import gc
    from oracle import unet_oracle as uo
    from rcu_amd import distributed as rdist
    K, n, h, w = 4, 160, 192, 128
    states = [uo.synthetic_state(90 + k, **PARAMS) for k in range(K)]
    g = torch.Generator().manual_seed(25)
    xd = torch.randn(n, 4, h, w, generator=g).to(dev)
    own = [_model(PARAMS, st, dev) for st in states]
    ref = rdist.ShardedEnsembleRunner(own, lanes=2, share_workspace=False).step(xd, 0)
    assert all(m._donor is None for m in own)
    own_bytes = [m.workspace_bytes(h, w, n, lane=i % 2) for i, m in enumerate(own)]      # member i runs on lane i mod 2
    assert min(own_bytes) > 5e9
    del own
    gc.collect()
    torch.cuda.empty_cache()
    shared = [_model(PARAMS, st, dev) for st in states]
    runner = rdist.ShardedEnsembleRunner(shared, lanes=2)
    out = runner.step(xd, 0)
    for key in ref:
        assert torch.equal(out[key], ref[key]), key
    assert all(m._donor is shared[0] for m in shared[1:])
    for i, m in enumerate(shared[1:], start=1):
        assert m.workspace_bytes(h, w, n, lane=i % 2) <= 150e6, i      # packed weights of the plan sized for 160 slices: 138 MB (Winograd tiles; 36 positions at the 12x8 level since round 5)
    assert shared[0].workspace_bytes(h, w, n) > 5e9
    # the workspace outlives its owner while a borrower still uses it: the borrower's plan of lane 1, called through the C ABI after
    # every plan of the owner has been destroyed
    from rcu_amd import _lib, steps
    borrower = shared[1]
    handle = next(v[0] for k, v in borrower._handles.items() if k[:3] == (h, w, 1))
    shared[0]._release()
    st1 = steps.McStatistics(n, 2, h, w, dev)
    _lib.check(_lib.load().rcu_unet_forward_accumulate(handle, _lib.ptr(xd), n, None, _lib.ptr(st1.blob), 0, _lib.current_stream()))
    st2 = steps.McStatistics(n, 2, h, w, dev)
    fresh = _model(PARAMS, states[1], dev)
    fresh.forward_accumulate(xd, st2)
    torch.cuda.synchronize()
    assert torch.equal(st1.blob, st2.blob)


@pytest.mark.timeout(1500)
def test_native_brats_volume_mc20_on_padded_levels(dev):
    """The reference's REAL BraTS volume -- 155 slices of 4 x 240 x 240 (scripts/create_brats18_dataset.py:53-72 never crops;
    config/test_brats_baseline_mc.yaml:30-31 slices the volume) -- at the config's own T = 20, through ShardedMcRunner as
    `bench.py --workload brats-native` runs it: one pass of 155 slices per launch (every tensor below 2 GB), two stream lanes, seeded masks,
    exact statistics; every layer on a Winograd kernel over padded levels (csrc/rcu_plan.hip plan_unet; rounds 1-5: >= 16 of 23
    layers on the direct kernels).  Three slices against the oracle's 21 forwards under the runner's masks; two lanes == one lane and the
    same seed gives the same bits (exact sums); a slice does not depend on the batch it runs in."""
    from oracle import summary_oracle as so
    from oracle import unet_oracle as uo
    from rcu_amd import distributed as rdist
    from rcu_amd import steps
    st = uo.synthetic_state(91, **PARAMS)
    T, n, h, w = 20, 155, 240, 240
    model = _model(PARAMS, st, dev)
    g = torch.Generator().manual_seed(26)
    x = torch.randn(n, 4, h, w, generator=g)
    xd = x.to(dev)
    sel = np.array([0, 77, 154])
    group = steps.pass_group_size(model, n, h, w, steps.McPredictStep.GROUP_PIXELS)
    assert group == 1
    rows_ = model.layer_table(h, w, n)
    assert sum('winograd' in r['kernel'] for r in rows_) == 22 and not any('igemm' in r['kernel'] for r in rows_)
    runner = rdist.ShardedMcRunner(model, T, seed=13, lanes=2, pass_group=group)
    out = runner.step(xd, 4)
    assert runner.forwards_run == T + 1 and set(out) == {'probabilities', 'entropy', 'ws_probabilities'}
    again = rdist.ShardedMcRunner(model, T, seed=13, lanes=2, pass_group=group).step(xd, 4)
    one_lane = rdist.ShardedMcRunner(model, T, seed=13, lanes=1, pass_group=group).step(xd, 4)
    for key in out:
        assert torch.equal(out[key], again[key]) and torch.equal(out[key], one_lane[key]), key
    rows = torch.as_tensor(sel)
    mask_sets = [_split_masks(model, runner.masks_of(xd, 4, j), n, rows) for j in range(1, T + 1)]
    small = rdist.ShardedMcRunner(model, T, lanes=1, pass_group=1).step(xd[sel], 4, mask_sets=mask_sets)
    for key in out:
        assert torch.equal(out[key][sel], small[key]), key
    ws, multi = so.mc_probabilities(lambda xx, mk: uo.unet_forward(st, xx, mk, **PARAMS), x[sel], mask_sets)
    ref = so.multi_prediction_summary(multi)
    for key in ('probabilities', 'entropy'):
        assert _maxdiff(out[key][sel].cpu().numpy(), ref[key].numpy()) < PROB_TOL, key
    assert _maxdiff(out['ws_probabilities'][sel].cpu().numpy(), ws.numpy()) < PROB_TOL
    # the step seam on a loader-sized batch of the same volume (64 slices: two batches of the shipped batch_size 32, coalesced)
    bc = steps.BatchContext({'images': x[:64]}, 0, sample_offset=4 * n)
    ctx = steps.TorchTestContext('cuda', model)
    steps.McPredictStep(T, seed=13)(bc, None, ctx)
    steps.MultiPredictionSummary()(bc, None, ctx)
    # (the same slices, the same global indices, the same seed: the same MC samples -- through another plan, so to float32 summation order)
    assert float((bc.output['probabilities'] - out['probabilities'][:64]).abs().max()) < 2e-6
