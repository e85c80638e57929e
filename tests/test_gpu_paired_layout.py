"""The pixel-pair ("paired") activation layout on the GPU (csrc/rcu_wino4_geom.h; act_layout = 0 pairs the tensors that only F(4x4,3x3) kernels
touch).  A layout is an addressing choice: the logits have the same bits under act_layout 0 (paired), 2 (channel-blocked) and 1 (channels-last).

Shapes, both under conv_winograd4 = 2 and upconv_winograd4 = 2 so that all five conv tiles and all three up-convolution tiles run:
  (i)  the BraTS architecture (depth 4, 32 filters) on 192 x 128 with 11 slices: an odd batch -- a half-empty S2T16x32 tile, a partly filled
       folded tile;
  (ii) depth 2, 32 filters, 64 x 64 with 3 slices: 2 x 2 T32x32 tiles per image -- interior tile borders and all four image borders;
  and depth 1 on 8 x 32 with 5 slices for the S4T8x32 tile, which neither of the two plans holds.
Inputs tell neighbouring columns apart (a swapped pixel pair, a pair read one column off): odd columns scaled by 1e3, even ones by 0.1, the border
columns and rows distinct (the idea of tests/test_gpu_fullw_zero.py).  Bounds against the oracle: that file's -- 2e-5 of the logit range, 1e-4 on
the probabilities."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REL = 2e-5
PROB_TOL = 1e-4
PAIRED = 2
CONV_TILES = ['conv3x3_winograd4<{},N32,K8>'.format(t) for t in ('T32x32', 'S2T16x32', 'S8T8x16', 'S8T12x8')]
UP_TILES = ['upconv_winograd4<{},N32,K8>'.format(t) for t in ('T32x32', 'S2T16x32', 'S8T8x16')]
# name -> depth, height, width, slices, the kernels that must run on paired tensors
CASES = {
    'brats-11': (4, 192, 128, 11, CONV_TILES[1:] + UP_TILES[1:]),
    'd2-64x64-3': (2, 64, 64, 3, [CONV_TILES[0], UP_TILES[0]]),
    's4t8x32-5': (1, 8, 32, 5, ['conv3x3_winograd4<S4T8x32,N32,K8>']),      # the fifth conv tile: a ragged second slice group
}
OPTIONS = dict(conv_winograd4=2, upconv_winograd4=2)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda')


def _input(n, h, w, g):
    x = torch.randn(n, 4, h, w, generator=g)
    x[..., 0::2] *= 0.1
    x[..., 1::2] *= 1e3
    x[..., 0] = 3e3 * (1.0 + 0.1 * torch.randn(n, 4, h, generator=g))
    x[..., -1] = -3e3 * (1.0 + 0.1 * torch.randn(n, 4, h, generator=g))
    x[..., 0, :] += 500.0
    x[..., -1, :] -= 500.0
    return x


def _model(params, state, dev, act_layout):
    from rcu_amd.model import UNet
    m = UNet(**params)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    m.plan_options = dict(OPTIONS, act_layout=act_layout)
    return m.to(dev)


@pytest.fixture(scope='module')
def runs(dev):
    """name -> everything the tests compare, computed once"""
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    out = {}
    for name, (depth, h, w, n, _) in CASES.items():
        params = dict(nb_classes=2, in_channels=4, depth=depth, start_filters=32, dropout=0.05)
        st = uo.synthetic_state(43, **params)
        g = torch.Generator().manual_seed(23)
        x = _input(n, h, w, g)
        _, sites = uo.unet_plan(**params)
        mask_sets = [uo.sample_masks(sites, n, 0.3, g) for _ in range(4)]
        r = dict(params=params, x=x, ref={'eval': uo.unet_forward(st, x, None, **params).numpy(),
                                          'masks': uo.unet_forward(st, x, mask_sets[0], **params).numpy()})
        for layout in (0, 2, 1):
            m = _model(params, st, dev, layout)
            r['rows', layout] = m.layer_table(h, w, n)
            r['layouts', layout] = m.layer_layouts(h, w, n)
            r['eval', layout] = m(x.to(dev), None).cpu().numpy()
            r['masks', layout] = m(x.to(dev), mask_sets[0]).cpu().numpy()
            if layout == 1:
                continue
            # the statistics of a pass group of 4 and of four single passes, with the head fused into conv_cls.0 and with head_kernel behind it
            for fused in (True, False):
                m.set_fuse_head(fused)
                group = steps.McStatistics(n, 2, h, w, dev, do_mi=True)
                m.forward_accumulate(x.to(dev), group, masks=mask_sets, passes=4)
                single = steps.McStatistics(n, 2, h, w, dev, do_mi=True)
                for ms in mask_sets:
                    m.forward_accumulate(x.to(dev), single, masks=ms)
                r['group', layout, fused] = group.blob.cpu().numpy().copy()
                r['single', layout, fused] = single.blob.cpu().numpy().copy()
            m.set_fuse_head(True)
        out[name] = r
    return out


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_tile_runs_on_paired_tensors(runs, name):
    r, expected = runs[name], CASES[name][4]
    rows, layouts = r['rows', 0], r['layouts', 0]
    for kernel in expected:
        hits = [lay for row, lay in zip(rows, layouts) if row['kernel'] == kernel]
        assert hits, kernel
        # it has read a paired tensor and written one (the 8 x 32 net has no unit that does both: its pooled level is not this kernel's)
        assert any(lay[0] == PAIRED for lay in hits) and any(lay[2] == PAIRED for lay in hits), (kernel, hits)
    print(name, [(row['kernel'], lay) for row, lay in zip(rows, layouts)])
    if name != 's4t8x32-5':
        assert rows[-1]['head_fusable'] and layouts[-1][0] == PAIRED      # the fused head reads a paired tensor
    assert [row['kernel'] for row in rows] == [row['kernel'] for row in r['rows', 2]] == [row['kernel'] for row in r['rows', 1]]
    assert all(PAIRED not in lay for lay in r['layouts', 2] + r['layouts', 1])


@pytest.mark.parametrize('name', sorted(CASES))
def test_paired_layout_gives_the_bits_of_blocked_and_channels_last(runs, name):
    r = runs[name]
    for tag in ('eval', 'masks'):
        ref = r['ref'][tag]
        scale = float(ref.max() - ref.min())
        d = float(np.max(np.abs(r[tag, 0].astype(np.float64) - ref)))
        dp = float(np.max(np.abs(torch.softmax(torch.from_numpy(r[tag, 0]), 1).numpy().astype(np.float64) -
                                 torch.softmax(torch.from_numpy(ref), 1).numpy())))
        print('{} {}: logit range {:.3e}, max |dlogit| {:.3e} = {:.2e} of it, max |dp| {:.3e}'.format(name, tag, scale, d, d / scale, dp))
        assert np.array_equal(r[tag, 0], r[tag, 2]), tag
        assert np.array_equal(r[tag, 0], r[tag, 1]), tag
        assert scale > 1.0
        assert d < REL * scale and dp < PROB_TOL, tag


@pytest.mark.parametrize('name', sorted(CASES))
def test_fused_head_and_pass_groups_on_paired_tensors(runs, name):
    r = runs[name]
    # the fused head on a paired input == head_kernel behind the plain kernel, bit for bit; a pass group of 4 == four single passes
    assert np.array_equal(r['group', 0, True], r['group', 0, False])
    assert np.array_equal(r['group', 0, True], r['single', 0, True])
    assert np.array_equal(r['single', 0, True], r['single', 0, False])
    # ... and the bits of the blocked layout
    assert np.array_equal(r['group', 0, True], r['group', 2, True])
