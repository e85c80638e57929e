"""Whole-net parity on weights that see the deep levels.  The parity tests on synthetic_state nets compare logits within 2e-6, and a fault at the
24x16 or 12x8 level of the depth-4 net -- a lost element, a lost column, a slice with another slice's Dropout2d factor -- moves them by less
(tests/test_parity_power_cpu.py holds the table).  Here every case runs on uo.sensitive_state weights (BatchNorm affines x 2.5), on which each of
those faults moves the logits by at least 75 x the bound at every layer of a level of 48x32 and below; the cases (tests/parity_power.py, CASES)
are the smallest shapes that reach the eight- and ten-slice work items, the four-slice tile, the padded levels of the reference's real shapes,
the up-convolutions that read them and the residual blocks.  Run on the GPU box: ``python -m pytest tests/test_gpu_deep_levels.py -m gpu``; the
one test without the mark needs the library but no device."""
import numpy as np
import pytest
import torch

import parity_power as pp
from plan_rows import plan_rows

# Logits within pp.bound = 2e-5 of the oracle's logit range (the project's bound for weights with BatchNorm gains, golden G18, whose measured
# worst is 8.4e-6), against the float32 oracle and against the float64 one.  The float32 oracle is 6.5e-7 .. 2.6e-6 of the range from the
# float64 one on these cases, so the bound is about 10 x the reference's own rounding, and it is 118 x below the weakest planted fault (75 x
# on the residual case E, which runs BatchNorm gain 2.0).  Measured max |dlogit| / logit range on an MI355X, worst plan of each case, against
# the float32 / float64 oracle; logit range eval / masks; worst |dp|:
#   A  eval 4.5e-6 / 4.3e-6 (conv_winograd4=2)   masks 4.9e-6 / 5.0e-6 (conv_winograd=0)   range 1.1 / 15.9   |dp| 1.9e-5
#   B  eval 3.5e-6 / 2.9e-6 (default)            masks 6.1e-6 / 5.7e-6 (pad_levels=0)      range 2.0 /  9.2   |dp| 1.7e-5
#   C  eval 3.1e-6 / 3.0e-6                      masks 4.6e-6 / 4.7e-6                     range 1.9 /  5.7   |dp| 8.5e-6
#   D  eval 4.6e-6 / 4.5e-6                      masks 3.0e-6 / 2.8e-6                     range 1.3 / 18.1   |dp| 1.5e-5
#   E  eval 3.1e-6 / 3.2e-6                      masks 3.5e-6 / 3.2e-6                     range 1.3 /  6.9   |dp| 4.8e-6
# The distances to the float64 oracle are those to the float32 one: what is measured is the kernels' float32 summation, not the reference's.
# Reproduce with ``python tools/stress_margin.py A B C D E``, or run this file with -s: every distance is printed before it is asserted.
PROB_TOL = 1e-4

C4_T32x32, C4_S2T16x32, C4_S8T8x16 = 'conv3x3_winograd4<T32x32,N32,K8>', 'conv3x3_winograd4<S2T16x32,N32,K8>', 'conv3x3_winograd4<S8T8x16,N32,K8>'
C4_S8T12x8, C4_S4T8x32 = 'conv3x3_winograd4<S8T12x8,N32,K8>', 'conv3x3_winograd4<S4T8x32,N32,K8>'
C2_T16x16, C2_T16x32 = 'conv3x3_winograd<T16x16,N64,K8>', 'conv3x3_winograd<T16x32,N32,K8>'
C2_S2T8x16, C2_S8T4x8 = 'conv3x3_winograd<S2T8x16,N64,K8>', 'conv3x3_winograd<S8T4x8,N64,K8>'
U2_T16x16, U2_T16x32 = 'upconv_winograd<T16x16,N64,K8>', 'upconv_winograd<T16x32,N32,K8>'
U2_S2T8x16, U2_S8T4x8 = 'upconv_winograd<S2T8x16,N64,K8>', 'upconv_winograd<S8T4x8,N64,K8>'
U4_T32x32, U4_S2T16x32, U4_S8T8x16 = 'upconv_winograd4<T32x32,N32,K8>', 'upconv_winograd4<S2T16x32,N32,K8>', 'upconv_winograd4<S8T8x16,N32,K8>'
FIRST = 'conv3x3_first<T8x32,K36>'
CD_T16x16, CD_T16x16_N32 = 'conv3x3_igemm<T16x16,N64,K8,db>', 'conv3x3_igemm<T16x16,N32,K8,db>'
CD_T8x16, CD_T8x16_N32 = 'conv3x3_igemm<T8x16,N64,K8,db>', 'conv3x3_igemm<T8x16,N32,K8>'
CD_S2T8x16, CD_S2T12x8 = 'conv3x3_igemm<S2T8x16,N64,K8,db>', 'conv3x3_igemm<S2T12x8,N64,K8,db>'
UD_T8x16, UD_T8x16_N32 = 'upconv_subpixel_igemm<T8x16,N64,K8,db>', 'upconv_subpixel_igemm<T8x16,N32,K8,db>'
UD_T16x16_N32, UD_S2T12x8 = 'upconv_subpixel_igemm<T16x16,N32,K8,db>', 'upconv_subpixel_igemm<S2T12x8,N64,K8,db>'

# Every Winograd instantiation the tests of this project name (test_gpu_parity.py, test_gpu_upconv4.py, test_gpu_fold10.py, test_abi_cpu.py)
# -- which is every one the libraries have: all of them must have run in a case below.
NAMED = {C4_T32x32, C4_S2T16x32, C4_S8T8x16, C4_S8T12x8, C4_S4T8x32, C2_T16x16, C2_T16x32, C2_S2T8x16, C2_S8T4x8,
         U2_T16x16, U2_T16x32, U2_S2T8x16, U2_S8T4x8, U4_T32x32, U4_S2T16x32, U4_S8T8x16}

# (case, plan) -> the kernel of every layer of a level of 48x32 pixels and below, in plan order (down levels, bottom level, then up-convolution
# + two units per up level; with residual blocks the 1x1 conv, which reports its block's first kernel, sits between the two units), and the set
# of kernels of the levels above.  Read from rcu_unet_plan for the cases' batch sizes.
_A_DEFAULT = 2 * [C4_S2T16x32] + 2 * [C4_S8T8x16] + 2 * [C2_S8T4x8] + [U2_S8T4x8] + 2 * [C4_S8T8x16] + [U2_S2T8x16] + 2 * [C4_S2T16x32]
_A_FOLD = 2 * [C4_S2T16x32] + 2 * [C4_S8T8x16] + 2 * [C4_S8T12x8] + [U2_S8T4x8] + 2 * [C4_S8T8x16] + [U2_S2T8x16] + 2 * [C4_S2T16x32]
_B_PADDED = 2 * [C4_T32x32] + 2 * [C4_S8T8x16] + [U2_T16x16] + 2 * [C4_T32x32]          # 30x30 on 32x32, 15x15 on 16x16
_B_REST = {FIRST, C4_S2T16x32, C4_T32x32, C2_T16x32, U2_T16x16, U2_T16x32}
_C_DEEP = 2 * [C4_S4T8x32] + 2 * [C4_S8T8x16] + [U2_T16x16] + 2 * [C4_S4T8x32]           # 24x32; 12x16 on 16x16
_C_REST = {FIRST, C4_S2T16x32, C4_T32x32, U2_S2T8x16, U2_T16x16, U2_T16x32}
_D_DEEP = 2 * [C4_S2T16x32] + 2 * [C4_S4T8x32] + [U2_S2T8x16] + 2 * [C4_S2T16x32]        # 16x64; 8x32
_SHIPPED_REST = {FIRST, C4_T32x32, U2_T16x16, U2_T16x32}
EXPECTED = {
    ('A', 'default'): dict(deep=_A_DEFAULT, rest=_SHIPPED_REST),
    ('A', 'conv_winograd4=2'): dict(deep=_A_FOLD, rest=_SHIPPED_REST),
    ('A', 'conv_winograd4=0'): dict(deep=2 * [C2_T16x16] + 2 * [C2_S2T8x16] + 2 * [C2_S8T4x8] + [U2_S8T4x8] + 2 * [C2_S2T8x16] + [U2_S2T8x16] + 2 * [C2_T16x16],
                                    rest={FIRST, C2_T16x16, C2_T16x32, U2_T16x16, U2_T16x32}),
    ('A', 'conv_winograd=0'): dict(deep=2 * [CD_T16x16] + 2 * [CD_T8x16] + 2 * [CD_S2T12x8] + [UD_S2T12x8] + 2 * [CD_T8x16] + [UD_T8x16] + 2 * [CD_T16x16],
                                   rest={FIRST, CD_T16x16_N32, CD_T16x16, UD_T16x16_N32, UD_T8x16}),
    ('A', 'conv_winograd4=2,upconv_winograd4=2'): dict(deep=2 * [C4_S2T16x32] + 2 * [C4_S8T8x16] + 2 * [C4_S8T12x8] + [U4_S8T8x16] + 2 * [C4_S8T8x16] +
                                                       [U4_S2T16x32] + 2 * [C4_S2T16x32], rest={FIRST, C4_T32x32, U4_T32x32}),
    ('A', 'act_layout=1'): dict(deep=_A_DEFAULT, rest=_SHIPPED_REST),
    ('A', 'head_winograd4=0'): dict(deep=_A_DEFAULT, rest=_SHIPPED_REST | {C2_T16x32}),
    ('B', 'default'): dict(deep=_B_PADDED, rest=_B_REST),
    ('B', 'conv_winograd4=2'): dict(deep=_B_PADDED, rest=_B_REST),
    ('B', 'pad_levels=0'): dict(deep=4 * [CD_T8x16] + [UD_T8x16] + 2 * [CD_T8x16], rest={CD_T16x16_N32, CD_T8x16_N32, CD_T8x16, UD_T8x16_N32, UD_T8x16}),
    ('C', 'default'): dict(deep=_C_DEEP, rest=_C_REST),
    ('C', 'conv_winograd4=2'): dict(deep=_C_DEEP, rest=_C_REST),
    ('D', 'default'): dict(deep=_D_DEEP, rest=_SHIPPED_REST),
    ('D', 'conv_winograd4=2'): dict(deep=_D_DEEP, rest=_SHIPPED_REST),
    ('E', 'default'): dict(deep=2 * [C4_S2T16x32] + [CD_T16x16] + 2 * [C4_S8T8x16] + [CD_S2T8x16] + 2 * [C2_S8T4x8] + [CD_S2T12x8] + [U2_S8T4x8] +
                           2 * [C4_S8T8x16] + [CD_S2T8x16] + [U2_S2T8x16] + 2 * [C4_S2T16x32] + [CD_T16x16],
                           rest={FIRST, CD_T16x16_N32, CD_T16x16, C4_T32x32, U2_T16x16, U2_T16x32}),
}


def _plan_id(options):
    return ','.join('{}={}'.format(k, v) for k, v in sorted(options.items())) or 'default'


RUNS = [(name, _plan_id(options)) for name in sorted(pp.CASES) for options in pp.CASES[name]['plans']]
OPTIONS = {(name, _plan_id(options)): options for name in pp.CASES for options in pp.CASES[name]['plans']}


def _split(rows):
    """Layer rows (height / width: the layer's output) -> (kernels of the levels of 48x32 pixels and below, set of kernels of the levels above)."""
    return ([r['kernel'] for r in rows if pp.is_deep(r['height'], r['width'])], {r['kernel'] for r in rows if not pp.is_deep(r['height'], r['width'])})


def test_expected_kernels_are_the_planners_and_cover_every_winograd_instantiation():
    """No device: rcu_unet_plan on each case's shape, batch and options gives the literals above, and over all cases every Winograd instantiation
    that the suite names appears in a plan that test_deep_levels_vs_oracle runs."""
    assert set(EXPECTED) == set(RUNS)
    seen = set()
    for name, plan in RUNS:
        case = pp.CASES[name]
        n, _, h, w = case['shape']
        p = case['params']
        deep, rest = _split(plan_rows(h, w, n, OPTIONS[name, plan], nb_classes=p['nb_classes'], in_channels=p['in_channels'], depth=p['depth'],
                                      start_filters=p['start_filters'], residual=p.get('residual', False)))
        assert deep == EXPECTED[name, plan]['deep'], (name, plan, deep)
        assert rest == EXPECTED[name, plan]['rest'], (name, plan, sorted(rest))
        seen.update(deep, rest)
    assert NAMED <= seen, sorted(NAMED - seen)
    assert not {k for k in seen if 'winograd' in k} - NAMED      # and the suite names every one a plan can hold


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda')


_REFS = {}


@pytest.fixture
def ref(request):
    """A case's state, input, masks and the oracle's logits in float32 and float64, eval mode and under the masks: computed once per case, by
    the first plan that asks, and never written to."""
    from oracle import unet_oracle as uo
    name = request.param
    if name not in _REFS:
        state, x, masks = pp.make_case(name)
        params = pp.CASES[name]['params']
        refs = {}
        for tag, mk in (('eval', None), ('masks', masks)):
            refs[tag] = (uo.unet_forward(state, x, mk, **params).numpy(), uo.unet_forward(state, x, mk, dtype=torch.float64, **params).numpy())
            assert refs[tag][1].dtype == np.float64
        _REFS[name] = dict(name=name, state=state, x=x, masks=masks, refs=refs)
    return _REFS[name]


def _maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


def _softmax(a):
    return torch.softmax(torch.from_numpy(np.asarray(a, dtype=np.float64)), 1).numpy()


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize('ref,plan', RUNS, indirect=['ref'])
def test_deep_levels_vs_oracle(dev, ref, plan):
    from rcu_amd.model import UNet
    name = ref['name']
    case = pp.CASES[name]
    n, _, h, w = case['shape']
    m = UNet(**case['params'])
    m.load_state_dict({k: torch.as_tensor(v) for k, v in ref['state'].items()})
    m.plan_options = dict(OPTIONS[name, plan])
    m = m.to(dev)
    deep, rest = _split(m.layer_table(h, w, n))
    assert deep == EXPECTED[name, plan]['deep'], deep
    assert rest == EXPECTED[name, plan]['rest'], sorted(rest)
    xd = ref['x'].to(dev)
    for tag, mk in (('eval', None), ('masks', ref['masks'])):
        ref32, ref64 = ref['refs'][tag]
        scale = float(np.abs(ref32).max())
        out_d = m(xd, mk)
        out = out_d.cpu().numpy()
        d32, d64, dp = _maxdiff(out, ref32), _maxdiff(out, ref64), _maxdiff(_softmax(out), _softmax(ref32))
        print('{} {} {}: range {:.3f}, |dlogit| / range {:.2e} (float32 oracle) {:.2e} (float64 oracle), oracle32 - oracle64 {:.2e}; bound {:.0e}; |dp| {:.2e}'
              .format(name, plan, tag, scale, d32 / scale, d64 / scale, _maxdiff(ref32, ref64) / scale, pp.REL_TOL, dp))
        assert d32 < pp.bound(scale), (tag, d32 / scale)
        assert d64 < pp.bound(scale), (tag, d64 / scale)
        assert dp < PROB_TOL and _maxdiff(_softmax(out), _softmax(ref64)) < PROB_TOL, tag
        # ragged prefixes of the batch on the same plan: slices are independent, so the first rows of the full run, bit for bit
        for k in case['prefixes']:
            part = m(xd[:k], None if mk is None else [v[:k] for v in mk])
            assert torch.equal(part, out_d[:k]), (tag, k)
        if name == 'B':
            # the padding of the allocated levels holds zeros that no kernel writes: after forwards of OTHER, large-valued data on the same
            # workspace (the full batch, and a prefix that leaves the last slice's planes as they were) the same input gives the same bits
            g = torch.Generator().manual_seed(7)
            for k in (n, n - 1):
                m((50.0 * torch.randn(k, case['shape'][1], h, w, generator=g)).to(dev), None if mk is None else [v[:k] for v in mk])
            assert torch.equal(m(xd, mk), out_d), tag
