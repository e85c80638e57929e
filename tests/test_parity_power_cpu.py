"""The power of the whole-net parity tests, measured on the oracle alone (no GPU): tests/parity_power.py plants the faults a kernel of a deep
level could have -- an element that was not stored, a column of a slice that was lost, a slice that got another slice's Dropout2d factor --
into one layer's output and reports how far the logits move.  A parity test whose bound is above that distance cannot see the fault."""
import pytest
import torch

import parity_power as pp
from plan_rows import plan_rows
from oracle import unet_oracle as uo

LOGIT_TOL = 2e-6      # the bound of the parity tests that run synthetic_state nets (tests/test_gpu_parity.py)
POWER = 10.0          # every mutation must move the logits by at least this many times the bound of tests/test_gpu_deep_levels.py


@pytest.fixture(scope='module', autouse=True)
def _threads():
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, 8))
    yield
    torch.set_num_threads(before)


@pytest.mark.parametrize('extra', [dict(), dict(residual=True), dict(sigma_out=True), dict(dropout_center=1)])
def test_oracle_hooks_number_the_layers_as_the_planner_and_resume_bit_exactly(extra):
    """unet_forward's ``tap`` and ``dtype`` on a small net: the tap sees every conv unit and up-convolution under the index and name of its row
    in rcu_unet_layer_info; an identity tap and the default dtype change no bit; a forward resumed behind layer k from a recorded one is the
    full forward with the same mutation, bit for bit; float64 is float64 throughout and a rounding error away from float32."""
    params = dict(nb_classes=3, in_channels=2, depth=2, start_filters=8, dropout=0.2, **extra)
    state = uo.synthetic_state(3, **params)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 2, 22, 24, generator=g)      # 22 -> 11 -> 5: the centre pad on the way up
    plan, sites = uo.unet_plan(**params)
    masks = uo.sample_masks(sites, 2, 0.3, g)
    first = lambda r: r[0] if isinstance(r, tuple) else r      # noqa: E731  (logits of a (logits, sigma) pair)
    plain = uo.unet_forward(state, x, masks, **params)
    seen = {}

    def record(index, op, tensor):
        seen.setdefault(index, []).append((op['key'], tensor))
        return tensor
    taped = uo.unet_forward(state, x, masks, tap=record, **params)
    assert torch.equal(first(taped), first(plain)) and first(plain).dtype == torch.float32
    # the planner's rows (no device): same indices, same names; the rows the tap does not see are the residual 1x1 convs
    names = [r['name'] for r in plan_rows(22, 24, 2, nb_classes=3, in_channels=2, depth=2, start_filters=8, dropout_center=extra.get('dropout_center', -1),
                                          sigma_out=extra.get('sigma_out', False), residual=extra.get('residual', False))]
    for index, calls in seen.items():
        key = calls[0][0]
        assert names[index] == (key[:-len('.conv2d_batch_relu')] + '.conv2d_batch_relu.conv' if key.endswith('.conv2d_batch_relu') else key), (index, key)
        assert len(calls) == (2 if key.startswith('conv_cls.0') and extra.get('sigma_out') else 1)      # conv_sigma.0 shares the row of its twin
    assert sorted(set(range(len(names))) - set(seen)) == [i for i, nm in enumerate(names) if nm.endswith('.residual')]
    assert [op['index'] for op in plan if op['kind'] == 'res_add'] == [i for i, nm in enumerate(names) if nm.endswith('.residual')]
    # resume: a mutated forward from the recorded prefix == the mutated forward computed in full
    for layer in sorted(seen)[:-1]:
        def mutate(index, op, tensor):
            return tensor * 1.5 if index == layer else tensor
        full = first(uo.unet_forward(state, x, masks, tap=mutate, **params))
        assert not torch.equal(full, first(plain))

        def resumed(index, op, tensor):
            return mutate(index, op, tensor)
        resumed.resume = lambda index, op: seen[index][0][1] if index < layer else None
        assert torch.equal(first(uo.unet_forward(state, x, masks, tap=resumed, **params)), full), layer
    wide = first(uo.unet_forward(state, x, masks, dtype=torch.float64, **params))
    assert wide.dtype == torch.float64
    assert 0.0 < float((wide - first(plain)).abs().max()) < 1e-5 * float(wide.abs().max())


def _traces(state, x, masks, params):
    """Eval-mode traces of the first and the last slice and the first slice's trace under masks."""
    last = x.shape[0] - 1
    return (pp.Trace(state, x[:1], None, params), pp.Trace(state, x[last:], None, params),
            pp.Trace(state, x[:1], [m[:1] for m in masks], params))


def _responses(traces, layer, site):
    first, last, masked = traces
    out = {'lost element (0, 0)': (pp.lost_element(first, layer), first.range),
           'lost element (h-1, w-1) of the last slice': (pp.lost_element(last, layer, far=True), last.range),
           'lost column': (pp.lost_column(first, layer), first.range)}
    if site is not None:
        out['wrong factor'] = (pp.wrong_factor(masked, layer, site), masked.range)
        out['stray factor'] = (pp.stray_factor(first, layer), first.range)
    return out


@pytest.mark.timeout(300)
@pytest.mark.parametrize('name', sorted(pp.CASES))
def test_every_mutation_of_a_deep_layer_moves_the_logits_ten_bounds(name):
    """Every case of tests/test_gpu_deep_levels.py, every layer of a level of 48 x 32 pixels or fewer and one full-resolution layer
    (down_convs.0's second unit, whose only way to the logits is the longest skip): each mutation that applies moves some logit by at least
    10 x the bound that test allows on this case.  The slices are the first and the last of the case's batch."""
    case = pp.CASES[name]
    state, x, masks = pp.make_case(name)
    _, _, h, w = case['shape']
    traces = _traces(state, x, masks, case['params'])
    rows = pp.layers(case['params'], h, w)
    chosen = [r for r in rows if pp.is_deep(r[2], r[3]) or r[1].startswith('down_convs.0.block.block.1')]
    assert len(chosen) >= 8 and any(not pp.is_deep(r[2], r[3]) for r in chosen)
    weak = []
    for index, key, lh, lw, site in chosen:
        for what, (moved, logit_range) in _responses(traces, index, site).items():
            ratio = moved / pp.bound(logit_range)
            print('{} {:2d} {:<44} {:3d}x{:<3d} {:<42} {:.2e} = {:7.0f} x bound'.format(name, index, key, lh, lw, what, moved, ratio))
            if not ratio >= POWER:
                weak.append((index, key, what, moved, ratio))
    assert not weak, weak


@pytest.mark.timeout(300)
def test_synthetic_state_weights_are_blind_at_the_two_deepest_levels():
    """Why tests/test_gpu_deep_levels.py does not use synthetic_state.  On the net of test_winograd_kernels_vs_direct_and_oracle
    (synthetic_state(21), depth 4, 32 filters, 4 x 192 x 128; logit range 0.13) the faults planted at the 24x16 and 12x8 levels move the logits
    by less than the LOGIT_TOL = 2e-6 those tests compare within.  Measured max |dlogit|, one slice:

        layer (output)                      lost element      lost      wrong factor   stray factor
                                          (0,0)   (h-1,w-1)   column    0 <-> 1/keep   1 -> 1/keep
        down_convs.2.block.block.0  48x32  1.5e-6   1.2e-6    1.3e-5      4.9e-5         5.4e-6
        down_convs.3.block.block.0  24x16  1.0e-7   9.7e-8    7.2e-7      1.0e-6         3.8e-7
        down_convs.3.block.block.1  24x16  3.4e-7   2.3e-7    1.8e-6      2.8e-6         9.2e-7
        bottom_convs.block.0        12x8   9.3e-8   1.0e-7    9.8e-7      2.7e-7         2.0e-7
        bottom_convs.block.1        12x8   3.3e-7   3.5e-7    1.7e-6      3.1e-7         3.9e-7
        up_convs.0.upconv.1         24x16  7.8e-8   1.1e-7    1.2e-6        --           3.1e-7
        up_convs.0.block.block.0    24x16  1.1e-6   1.0e-6    1.0e-5      2.8e-6         2.7e-6
        up_convs.0.block.block.1    24x16  3.1e-6   2.6e-6    3.5e-5      4.3e-5         7.3e-6
        conv_cls.0                 192x128 3.0e-2   3.6e-2    9.7e-2      1.9e-2         1.8e-2

    Asserted for down_convs.3, bottom_convs and up_convs.0.upconv.1: a lost element and a stray factor stay below LOGIT_TOL, a lost column too,
    and no mutation -- the flipped factor of the channel with the LARGEST mean activation included, 2.8e-6 at worst -- comes near the 10 x bound
    that the test above demands of the sensitive_state cases, where the same faults answer at 75 x the bound and more.  Do not fold the
    deep-level tests back onto these weights."""
    state = uo.synthetic_state(21, **pp.WIDE)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 4, 192, 128, generator=g)
    _, sites = uo.unet_plan(**pp.WIDE)
    masks = uo.sample_masks(sites, 1, pp.MASK_P, g)
    traces = _traces(state, x, masks, pp.WIDE)
    rows = [r for r in pp.layers(pp.WIDE, 192, 128) if r[1].startswith(('down_convs.3.', 'bottom_convs.', 'up_convs.0.upconv'))]
    assert [(r[2], r[3]) for r in rows] == [(24, 16), (24, 16), (12, 8), (12, 8), (24, 16)]
    for index, key, lh, lw, site in rows:
        got = {what: moved for what, (moved, _) in _responses(traces, index, site).items()}
        print('{:<44} '.format(key) + '  '.join('{} {:.2e}'.format(k, v) for k, v in got.items()))
        for what, moved in got.items():
            assert 0.0 < moved < POWER * LOGIT_TOL, (key, what, moved)
            if what != 'wrong factor':
                assert moved < LOGIT_TOL, (key, what, moved)
