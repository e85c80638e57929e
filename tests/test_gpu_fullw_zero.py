"""The full-width F(4x4,3x3) tiles (csrc/rcu_wino4.hip, Wino4Tile<..., FULLW>: S8T8x16, the folded S8T12x8, S4T8x32) read the zero padding left and
right of the image from a region of LDS that holds zeros for the whole kernel: the lanes of the first and last tile column point their outer
patch column there.  A read that does not land on zeros -- a region that is not cleared, that a chunk's LDS-DMA or an epilogue writes, an address
outside it -- adds a multiple of whatever lies there to the border tiles.

Inputs: border columns (first and last, every channel) of about 1e3, interior of about 0.1, so the activations a wrong halo read would pick up --
the border column itself is the nearest -- are 1e4 times the interior's, and the kernels run on the smallest nets whose plans hold them:
  * S8T8x16: depth 1 on 8 x 16 slices, 8 slices: 32->32, the two-source 64->32 and 32->32 at one tile per slice group; and 2059 slices -- 258 slice
    groups for the kernel's 256 persistent workgroups, so two of them walk a second tile on the zeros the first one left (and the last group is
    ragged: three slices),
  * the folded tile: depth 2 on 48 x 32 slices under conv_winograd4 = 2 with 10 and 11 slices (eleven leave a second tile with one slice); the
    24 x 16 level above it runs S8T8x16 with three tile rows per slice,
  * S4T8x32: depth 1 on 8 x 32 slices, 4 slices.
Bound: the oracle's logits within 2e-5 of their range, the bound tests/test_gpu_parity.py sets for activations of this magnitude
(test_unet_stress_golden_wide_activations_and_logits); the probabilities within its PROB_TOL.  The logits of these inputs span 4 to 37, the
columns away from the border about a third of that; measured, the kernels stay within 1.6e-6 of the range.  The existing tests claim no bit identity
between the Winograd and the direct families, so none is asserted here; the slices of a batch are independent, which is asserted bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REL = 2e-5            # of the logits' range: tests/test_gpu_parity.py, the stress case
PROB_TOL = 1e-4
S8T8x16, FOLDED, S4T8x32 = 'conv3x3_winograd4<S8T8x16,N32,K8>', 'conv3x3_winograd4<S8T12x8,N32,K8>', 'conv3x3_winograd4<S4T8x32,N32,K8>'

# name -> depth, height, width, slices, kernel -> the (cin, cout, two-source) of the layers it must run
CASES = {
    's8t8x16': (1, 8, 16, 8, {S8T8x16: [(32, 32, 0), (64, 32, 1), (32, 32, 0)]}),
    's8t8x16-second-tile': (1, 8, 16, 2059, {S8T8x16: [(32, 32, 0), (64, 32, 1), (32, 32, 0)]}),
    'fold-10': (2, 48, 32, 10, {FOLDED: [(64, 128, 0), (128, 128, 0)], S8T8x16: [(32, 64, 0), (64, 64, 0), (128, 64, 1), (64, 64, 0)]}),
    'fold-11': (2, 48, 32, 11, {FOLDED: [(64, 128, 0), (128, 128, 0)], S8T8x16: [(32, 64, 0), (64, 64, 0), (128, 64, 1), (64, 64, 0)]}),
    's4t8x32': (1, 8, 32, 4, {S4T8x32: [(32, 32, 0), (64, 32, 1), (32, 32, 0)]}),
}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda')


def _maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


def _input(n, h, w, g):
    x = 0.1 * torch.randn(n, 4, h, w, generator=g)
    x[..., 0] = 1e3 * (1.0 + 0.1 * torch.randn(n, 4, h, generator=g))
    x[..., -1] = -1e3 * (1.0 + 0.1 * torch.randn(n, 4, h, generator=g))
    return x


@pytest.mark.parametrize('name', sorted(CASES))
def test_full_width_tiles_read_zeros_beside_the_image(dev, name):
    from oracle import unet_oracle as uo
    from rcu_amd.model import UNet
    depth, h, w, n, expected = CASES[name]
    params = dict(nb_classes=2, in_channels=4, depth=depth, start_filters=32, dropout=0.05)
    st = uo.synthetic_state(41, **params)
    m = UNet(**params)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in st.items()})
    m.plan_options = dict(conv_winograd4=2)
    m = m.to(dev)
    rows = m.layer_table(h, w, n)
    for kernel, layers in expected.items():
        assert [(r['cin'], r['cout'], r['dual_source']) for r in rows if r['kernel'] == kernel] == layers, kernel
    g = torch.Generator().manual_seed(17)
    x = _input(n, h, w, g)
    _, sites = uo.unet_plan(**params)
    masks = uo.sample_masks(sites, n, 0.3, g)
    for tag, mk in (('eval', None), ('masks', masks)):
        ref = uo.unet_forward(st, x, mk, **params).numpy()
        scale = float(ref.max() - ref.min())
        out = m(x.to(dev), mk).cpu().numpy()
        d = _maxdiff(out, ref)
        dp = _maxdiff(torch.softmax(torch.from_numpy(out), 1).numpy(), torch.softmax(torch.from_numpy(ref), 1).numpy())
        print('{} {}: logit range {:.3e}, max |dlogit| {:.3e} = {:.2e} of it, max |dp| {:.3e}'.format(name, tag, scale, d, d / scale, dp))
        assert scale > 1.0          # the border columns reach the logits
        assert d < REL * scale and dp < PROB_TOL, tag
        # a second forward on the same plan, and a ragged prefix of the batch: the same bits
        assert np.array_equal(m(x.to(dev), mk).cpu().numpy(), out)
        k = max(n - 3, 1)
        part = m(x[:k].to(dev), None if mk is None else [v[:k] for v in mk]).cpu().numpy()
        assert np.array_equal(part, out[:k])
