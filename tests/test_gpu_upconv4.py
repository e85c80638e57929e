"""The 25-product F(4x4,3x3) up-convolutions (csrc/rcu_wino4_up.hip, plan option upconv_winograd4) against the oracle and against the sub-pixel
F(2x2,2x2) kernels they replace.  Run on the GPU box: ``python -m pytest tests -m gpu``."""
import numpy as np
import pytest
import torch

from conftest import golden_params

pytestmark = pytest.mark.gpu

LOGIT_TOL = 2e-6      # as tests/test_gpu_parity.py
PROB_TOL = 1e-4
NEW = {'upconv_winograd4<T32x32,N32,K8>', 'upconv_winograd4<S2T16x32,N32,K8>', 'upconv_winograd4<S8T8x16,N32,K8>'}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda')


def _model(params, state, dev, **plan_options):
    from rcu_amd.model import UNet
    m = UNet(**params)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    m.plan_options = dict(plan_options)
    return m.to(dev)


def _maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


def _softmax(a):
    return torch.softmax(torch.from_numpy(a), 1).numpy()


def test_upconv4_vs_oracle_and_subpixel_kernels(dev):
    """The BraTS architecture at 192x128 with 8 slices under upconv_winograd4=2: tiles that touch every image border, interior tile seams in both
    directions on the T32x32 levels, the two-slice and eight-slice work items.  With masks and without: against the oracle, against the
    option-0 plan (below 2e-5), and ragged batches of 3 and 5 slices bit-equal to the first rows of the 8-slice run."""
    from oracle import unet_oracle as uo
    params = dict(nb_classes=2, in_channels=4, depth=4, start_filters=32, dropout=0.05)
    st = uo.synthetic_state(21, **params)
    g = torch.Generator().manual_seed(6)
    n, h, w = 8, 192, 128
    x = torch.randn(n, 4, h, w, generator=g)
    _, sites = uo.unet_plan(**params)
    masks = uo.sample_masks(sites, n, 0.3, g)
    m_new, m_old = _model(params, st, dev, upconv_winograd4=2), _model(params, st, dev, upconv_winograd4=0)
    up_new = [row['kernel'] for row in m_new.layer_table(h, w, n) if 'upconv' in row['name']]
    assert up_new == ['upconv_winograd4<S8T8x16,N32,K8>', 'upconv_winograd4<S2T16x32,N32,K8>', 'upconv_winograd4<T32x32,N32,K8>',
                      'upconv_winograd4<T32x32,N32,K8>']
    assert not any('winograd4' in row['kernel'] for row in m_old.layer_table(h, w, n) if 'upconv' in row['name'])
    for mk in (masks, None):
        ref = uo.unet_forward(st, x, mk, **params).numpy()
        out = m_new(x.to(dev), mk).cpu().numpy()
        old = m_old(x.to(dev), mk).cpu().numpy()
        print('masks {}: new vs oracle {:.3e}, old vs oracle {:.3e}, new vs old {:.3e}'.format(mk is not None, _maxdiff(out, ref), _maxdiff(old, ref),
                                                                                            _maxdiff(out, old)))
        assert _maxdiff(out, ref) < LOGIT_TOL
        assert _maxdiff(_softmax(out), _softmax(ref)) < PROB_TOL
        assert _maxdiff(out, old) < 2e-5
        for k in (3, 5):
            out_k = m_new(x[:k].to(dev), None if mk is None else [s[:k] for s in mk]).cpu().numpy()
            assert np.array_equal(out_k, out[:k]), k


def test_upconv4_stress_fixture(golden, dev):
    """Reference golden G18 (BatchNorm affines x 2.5, classifier x 0.5: interior activations of 1e2..1e3, logits of +-20) under upconv_winograd4=2,
    within the tolerances of tests/test_gpu_parity.py's stress test."""
    from oracle import unet_oracle as uo
    REL = 2e-5
    g = golden('g18_unet_stress')
    p = golden_params(g)
    st = uo.stress_state(uo.reference_init_state(int(g['seed']), bn_seed=int(g['seed']) + 1000, **p), float(g['bn_gain']), float(g['head_gain']))
    x = torch.as_tensor(g['x'])
    n, _, h, w = x.shape
    _, sites = uo.unet_plan(**p)
    stride = int(g['stride'])
    m = _model(p, st, dev, upconv_winograd4=2)
    assert NEW <= {row['kernel'] for row in m.layer_table(h, w, n)}
    for tag, mk in [('eval', None)] + [('mc{}'.format(t), [g['mask{}_{}'.format(t, s)] for s in range(len(sites))]) for t in range(3)]:
        ref = uo.unet_forward(st, x, mk, **p).numpy()
        scale = float(np.abs(ref).max())
        out = m(x.to(dev), mk).cpu().numpy()
        dp = _maxdiff(_softmax(out), _softmax(ref))
        print('{}: |dlogit| / range {:.3e} (bound {:.0e}), |dp| {:.3e} (bound {:.0e})'.format(tag, _maxdiff(out, ref) / scale, REL, dp, PROB_TOL))
        assert _maxdiff(out, ref) < REL * scale, tag
        assert _maxdiff(out.reshape(-1)[::stride], g['logits_{}_strided'.format(tag)]) < REL * scale, tag
        assert dp < PROB_TOL, tag


def test_upconv4_single_tile_level(dev):
    """A depth-2, 32-filter net at 64x64 with 2 slices: the 32x32 output level consists of exactly one T32x32 tile -- no seam, all four borders in
    one tile -- and the 64x64 level of 2 x 2 tiles."""
    from oracle import unet_oracle as uo
    params = dict(nb_classes=2, in_channels=4, depth=2, start_filters=32, dropout=0.05)
    st = uo.synthetic_state(5, **params)
    x = torch.randn(2, 4, 64, 64, generator=torch.Generator().manual_seed(9))
    m = _model(params, st, dev, upconv_winograd4=2)
    ups = [(row['height'], row['kernel']) for row in m.layer_table(64, 64, 2) if 'upconv' in row['name']]
    assert ups == [(32, 'upconv_winograd4<T32x32,N32,K8>'), (64, 'upconv_winograd4<T32x32,N32,K8>')]
    ref = uo.unet_forward(st, x, None, **params).numpy()
    out = m(x.to(dev)).cpu().numpy()
    print('single tile: vs oracle {:.3e}'.format(_maxdiff(out, ref)))
    assert _maxdiff(out, ref) < LOGIT_TOL
