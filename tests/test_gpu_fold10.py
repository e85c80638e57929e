"""The folded F(4x4,3x3) tile of the 12x8 level with TEN slices per work item (csrc/rcu_wino4.hip, the FOLD geometry): 60 of a workgroup's 64
tile slots hold tiles, a slice's six tiles no longer line up with the waves or with a lane's four accumulator rows, so the slice -- Dropout2d
factor, store offset -- is per tile.  Model: depth 2 on 48 x 32 inputs, i.e. a 12 x 8 bottom level with 64 -> 128 -> 128 channels (8 and 16 Cin
chunks) under conv_winograd4 = 2, which takes the folded kernel whatever the batch.  Batches: 1 and 6 (partial groups), 9, 10, 11 (one short of,
exactly and one past a group), 21 (two full groups and a slice: every lane pattern, the one that straddles two slices with a real and with an
absent second slice).  And once on 44 x 28 inputs, whose 11 x 7 bottom level is allocated 12 x 8: the kernel's form for padded levels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOGIT_TOL = 2e-6      # the bounds of tests/test_gpu_parity.py for this family (test_unet_full_width_vs_oracle)
PROB_TOL = 1e-4
PARAMS = dict(nb_classes=2, in_channels=4, depth=2, start_filters=32, dropout=0.05)
H, W, NMAX = 48, 32, 21
BATCHES = [1, 6, 9, 10, 11, 21]
FOLDED = 'conv3x3_winograd4<S8T12x8,N32,K8>'
SEED, FIRST = 77, 1000


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda')


def _model(state, dev, **attrs):
    from rcu_amd.model import UNet
    m = UNet(**PARAMS)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    m.plan_options = dict(conv_winograd4=2)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m.to(dev)


@pytest.fixture(scope='module')
def case(dev):
    """State, input, the oracle's eval logits of all 21 slices, and every slice's seeded-mask forward run ALONE -- each computed once."""
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    state = uo.synthetic_state(31, **PARAMS)
    x = torch.randn(NMAX, 4, H, W, generator=torch.Generator().manual_seed(9))
    ref = uo.unet_forward(state, x, None, **PARAMS).numpy()
    m = _model(state, dev)
    steps.set_dropout_mode(m, True)
    alone = torch.cat([m(x[i:i + 1].to(dev), m.seeded_masks(1, dev, [SEED], FIRST + i)) for i in range(NMAX)]).cpu().numpy()
    steps.set_dropout_mode(m, False)
    return dict(state=state, x=x, ref=ref, alone=alone, model=m)


def _bottom_rows(rows):
    return [r for r in rows if not r['upsample'] and (r['height'], r['width']) == (12, 8)]


@pytest.mark.parametrize('n', BATCHES)
def test_folded_tile_vs_oracle_and_single_slices(dev, case, n):
    from rcu_amd import steps
    m, x = case['model'], case['x'][:n].to(dev)
    # (c) the kernel under test runs both units of the bottom level
    bottom = _bottom_rows(m.layer_table(H, W, n))
    assert len(bottom) == 2 and [(r['cin'], r['cout']) for r in bottom] == [(64, 128), (128, 128)]
    assert all(r['kernel'] == FOLDED for r in bottom), [r['kernel'] for r in bottom]
    # (a) eval forward against the oracle
    out = m(x).cpu().numpy()
    d = float(np.max(np.abs(out.astype(np.float64) - case['ref'][:n])))
    dp = float(np.max(np.abs(torch.softmax(torch.from_numpy(out), 1).numpy().astype(np.float64) -
                             torch.softmax(torch.from_numpy(case['ref'][:n]), 1).numpy())))
    print('n = {}: max |dlogit| {:.3e}, max |dp| {:.3e}'.format(n, d, dp))
    assert d < LOGIT_TOL and dp < PROB_TOL
    # (b) masks keyed by the global slice index: every slice of the batch is the bits of the slice run alone
    steps.set_dropout_mode(m, True)
    try:
        mc = m(x, m.seeded_masks(n, dev, [SEED], FIRST)).cpu().numpy()
    finally:
        steps.set_dropout_mode(m, False)
    wrong = [i for i in range(n) if not np.array_equal(mc[i], case['alone'][i])]
    assert not wrong, wrong
    assert not np.array_equal(mc, out)          # the factors did something


def test_folded_tile_on_a_padded_level(dev, case):
    """44 x 28 inputs: the bottom level is 11 x 7, allocated 12 x 8 (rcu_unet_options.pad_levels) -- the kernel's ConvArgs::part form, whose limits
    of the real image are per tile in this geometry too.  The padding must stay zero (the up-convolution and the second unit read it as the conv's
    zero padding), so a store beyond row 10 or column 6 of any slice shows against the oracle.  13 slices: a full group and a partial one."""
    from oracle import unet_oracle as uo
    n, h, w = 13, 44, 28
    m = case['model']
    bottom = [r for r in m.layer_table(h, w, n) if not r['upsample'] and (r['height'], r['width']) == (11, 7)]
    assert len(bottom) == 2 and all(r['kernel'] == FOLDED and (r['grid_height'], r['grid_width']) == (12, 8) for r in bottom)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(n, 4, h, w, generator=g)
    _, sites = uo.unet_plan(**PARAMS)
    masks = uo.sample_masks(sites, n, 0.3, g)
    for mk in (None, masks):
        ref = uo.unet_forward(case['state'], x, mk, **PARAMS).numpy()
        out = m(x.to(dev), mk).cpu().numpy()
        d = float(np.max(np.abs(out.astype(np.float64) - ref)))
        print('padded level, masks {}: max |dlogit| {:.3e}'.format(mk is not None, d))
        assert d < LOGIT_TOL
        again = m(x.to(dev), mk).cpu().numpy()          # a second forward on the same workspace: the padding is still zero
        assert np.array_equal(again, out)
        part = m(x[:4].to(dev), None if mk is None else [v[:4] for v in mk]).cpu().numpy()
        assert np.array_equal(part, out[:4])


@pytest.mark.parametrize('n', BATCHES)
def test_nothing_is_stored_behind_the_last_real_slice(dev, case, n):
    """(d) Idle slots and absent slices store nothing.  The activation tensors of a plan are not handed out, so the slack is read through its
    consumers: a plan sized for 32 slices is filled by a forward of 32; a forward of n slices of OTHER data follows; then the layers behind the
    bottom level run once more on all 32 slices (rcu_unet_run_layer: a layer on the workspace's current contents).  The feature tensor (the input
    of conv_cls.0, provide_features) of the slices n .. 31 must be the bits of the first forward: it is a function of the bottom level's output
    and of the skip tensors of exactly those slices, so a store of the n-slice forward behind slice n - 1 of any of them changes it."""
    big = 32
    m = _model(case['state'], dev, provide_features=True)
    m.reserve(H, W, big)
    g = torch.Generator().manual_seed(10)
    x32 = torch.randn(big, 4, H, W, generator=g).to(dev)
    m(x32)
    before = m.features.clone()
    rows = m.layer_table(H, W, big)
    bottom = _bottom_rows(rows)
    assert len(bottom) == 2 and all(r['kernel'] == FOLDED for r in bottom)
    cls = [r['index'] for r in rows if r['name'].startswith('conv_cls.0')][0]
    m(3.0 * torch.randn(n, 4, H, W, generator=g).to(dev))
    small = m.features.clone()
    assert not torch.equal(small, before[:n])
    for layer in range(bottom[-1]['index'] + 1, cls):
        m.run_layer(H, W, big, layer)
    after = m._features_view(m._handle(H, W, big), big, H, W, dev)
    torch.cuda.synchronize()
    assert torch.equal(after[n:], before[n:])
    assert torch.equal(after[:n], small)        # and the n slices in front are still the second forward's
