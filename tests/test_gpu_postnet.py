"""PostNet on the GPU (csrc/rcu_postnet.hip) beyond the three tests of test_gpu_parity.py: every width and class count under eval and under
Dropout2d masks at shapes whose waves straddle images, against the float64 chain of tests/postnet_reference.py within its derived bound; the
bit-for-bit contracts (a voxel's logits are a function of its features, its image's mask rows and the weights alone: not of its position in
the call, of the padding channels, or of the pitch); bn = 0 through the C ABI; the limits of the LDS image.  PostNet above the grid cap is
in tests/test_gpu_capped_launches.py.

The derived bound is a worst case in every layer (|W'| e_l): at three hidden convs it is 10^2 .. 10^3 times what either implementation does
(the float32 torch oracle uses 0.0001 of it, tests/test_capped_launches_cpu.py).  So the flat 2e-5 that test_gpu_parity.py holds PostNet to
against the float32 oracle is asserted beside it, here against the float64 chain.

Largest fraction of the derived bound used on the MI355X (every test prints its own): 0.094 (32 channels, no hidden conv, hw = 126); per width
32 / 40 / 48 / 64 / 96 channels 0.094 / 0.088 / 0.055 / 0.059 / 0.029; at three hidden convs 0.001 and less.  Largest distance from the float64
chain over all cases 2.5e-7 (96 channels above the cap, masked)."""
import ctypes

import numpy as np
import pytest
import torch

import postnet_reference as pr

pytestmark = pytest.mark.gpu
FLAT_TOL = 2e-5      # test_gpu_parity.py::test_postnet_full_width_vs_oracle


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda')


def _post(state, channels, classes, nb_convs, dev):
    from rcu_amd.model import PostNet
    post = PostNet(channels, classes, nb_convs=nb_convs).to(dev)
    post.load_state_dict(state)
    return post


def check_against_the_chain(got, logits, bound, tag, extra_bound=None):
    """|got - float64 chain| <= the derived bound entry by entry, and <= 2e-5; -> the largest fraction of the bound used."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == logits.shape and np.isfinite(got).all(), tag
    total = bound if extra_bound is None else bound + extra_bound
    used = pr.fraction_used(got, logits, total)
    flat = float(np.abs(got - logits).max())
    print('postnet {}: largest fraction of the bound used {:.4f}, largest distance {:.2e}'.format(tag, used, flat))
    assert used <= 1.0, (tag, used)
    assert flat <= FLAT_TOL, (tag, flat)
    return used


def _nhwc(x, pitch, dev, fill=None, seed=3, lead=0):
    """x [n, C, h, w] -> (the [n, C, h, w] view of a channels-last device buffer at ``pitch`` floats per voxel, ``lead`` images into its
    allocation; the buffer).  Channels C .. pitch - 1 hold zeros, or ``fill`` * standard normal draws."""
    n, c, h, w = x.shape
    if fill is None:
        buf = torch.zeros(lead + n, h, w, pitch)
    else:
        buf = torch.randn(lead + n, h, w, pitch, generator=torch.Generator().manual_seed(seed)) * fill
    buf[lead:, ..., :c] = torch.from_numpy(x).permute(0, 2, 3, 1)
    buf = buf.to(dev)
    view = buf[lead:, ..., :c].permute(0, 3, 1, 2)
    assert view.data_ptr() % 16 == 0 and view.stride(1) == 1 and view.stride(3) == pitch
    return view, buf


# ------------------------------------------------------------------------------------------ mask seams and widths
@pytest.mark.timeout(300)
@pytest.mark.parametrize('channels', pr.SEAM_CHANNELS)
@pytest.mark.parametrize('shape', pr.SEAM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_every_width_under_eval_and_masks_against_the_float64_chain(dev, shape, channels):
    worst = 0.0
    for classes in pr.SEAM_CLASSES:
        for nb_convs in pr.SEAM_CONVS:
            state, x, masks = pr.seam_case(shape, channels, classes, nb_convs)
            post = _post(state, channels, classes, nb_convs, dev)
            xd = torch.from_numpy(x).to(dev)
            tag = (shape, channels, classes, nb_convs)
            logits, bound = pr.forward(state, x, nb_convs)
            plain = post(xd).cpu().numpy()
            worst = max(worst, check_against_the_chain(plain, logits, bound, tag + ('eval',)))
            if masks is None:
                continue
            assert not masks[0][0].any() and (masks[-1][-1] == 1).all()
            m_logits, m_bound = pr.forward(state, x, nb_convs, masks)
            worst = max(worst, check_against_the_chain(post(xd, masks).cpu().numpy(), m_logits, m_bound, tag + ('masked',)))
            # all-ones masks are eval mode in exact arithmetic; the two LDS images (b_all | b_conv, b_shift) round differently, so the
            # contract is the sum of both bounds around the one float64 value, not equal bits
            ones = [np.ones_like(m) for m in masks]
            o_logits, o_bound = pr.forward(state, x, nb_convs, ones)
            assert float(np.abs(o_logits - logits).max()) < 1e-12
            by_ones = post(xd, ones).cpu().numpy()
            check_against_the_chain(by_ones, o_logits, o_bound, tag + ('ones',))
            assert (np.abs(by_ones.astype(np.float64) - plain.astype(np.float64)) <= bound + o_bound).all(), tag
    print('postnet {} C={}: largest fraction of the bound used over the classes and depths {:.4f}'.format(shape, channels, worst))


# ------------------------------------------------------------------------------------------ bit contracts
@pytest.mark.timeout(300)
@pytest.mark.parametrize('masked', [False, True], ids=['eval', 'masked'])
@pytest.mark.parametrize('channels', [32, 40, 64, 72, 96])
def test_logits_of_a_voxel_do_not_depend_on_the_call(dev, channels, masked):
    """Images 1..3 of five, alone and inside the larger call (hw = 35 and 126: an image starts at no multiple of the 32 voxels a wave takes),
    the mask rows staying with their images; then the same three images read in place one image into the larger allocation."""
    classes, nb_convs = 3, 2
    cp = (channels + 31) // 32 * 32
    for h, w in ((5, 7), (9, 14)):
        state, x, _ = pr.seam_case((5, h, w), channels, classes, nb_convs)
        masks = pr.draw_masks(5, channels, nb_convs, 0.3, torch.Generator().manual_seed(channels + h)) if masked else None
        post = _post(state, channels, classes, nb_convs, dev)
        sub = None if masks is None else [m[1:4] for m in masks]
        whole = post(torch.from_numpy(x).to(dev), masks)
        alone = post(torch.from_numpy(x[1:4]).to(dev), sub)
        logits, bound = pr.forward(state, x[1:4], nb_convs, sub)
        check_against_the_chain(alone.cpu().numpy(), logits, bound, (channels, h, w, masked))
        assert torch.equal(whole[1:4], alone), (h, w)
        view, _buf = _nhwc(x, cp, dev)
        assert torch.equal(post(view[1:4], sub), alone), (h, w, 'at its offset in a larger allocation')


@pytest.mark.timeout(300)
@pytest.mark.parametrize('masked', [False, True], ids=['eval', 'masked'])
@pytest.mark.parametrize('channels', [32, 40, 48, 64, 72, 96])
def test_logits_do_not_depend_on_the_padding_channels_or_the_pitch(dev, channels, masked):
    """include/rcu.h, rcu_postnet_forward: the padding channels up to the next multiple of 32 may hold any finite values (their weights are
    zero, and 0 * finite = 0 exactly); channels from that multiple on are never read."""
    classes, nb_convs, shape = 2, 3, (3, 5, 7)
    cp = (channels + 31) // 32 * 32
    state, x, masks = pr.seam_case(shape, channels, classes, nb_convs)
    masks = masks if masked else None
    post = _post(state, channels, classes, nb_convs, dev)
    want = post(torch.from_numpy(x).to(dev), masks)                      # the generic NCHW path: a zero-padded copy at pitch cp
    logits, bound = pr.forward(state, x, nb_convs, masks)
    check_against_the_chain(want.cpu().numpy(), logits, bound, (channels, masked))
    for pitch in (cp, cp + 4, 128):
        for fill in (None, 1.0e3):
            view, buf = _nhwc(x, pitch, dev, fill=fill, seed=pitch)
            if fill is not None and pitch > channels:
                assert float(buf[..., channels:].abs().max()) > 1e3
            assert torch.equal(post(view, masks), want), (pitch, fill)
    with pytest.raises(Exception):      # a pitch that is no multiple of 4 is refused by the C entry point, not read
        from rcu_amd import _lib
        out = torch.empty(3, classes, 5, 7, device=dev)
        _lib.check(_lib.load().rcu_postnet_forward(post._handle(), _lib.ptr(buf), cp + 2, 3, 35, None, _lib.ptr(out), _lib.current_stream()))


# ------------------------------------------------------------------------------------------ bn = 0 through the C ABI
def _create(channels, classes, nb_convs, bn):
    from rcu_amd import _lib
    handle = ctypes.c_void_p()
    _lib.check(_lib.load().rcu_postnet_create(channels, classes, nb_convs, bn, ctypes.byref(handle)))
    return handle


def _load(handle, state, keys):
    from rcu_amd import _lib
    for key in keys:
        host = torch.as_tensor(state[key]).to(torch.float32).contiguous()
        _lib.check(_lib.load().rcu_postnet_load_weight(handle, key.encode(), ctypes.c_void_p(host.data_ptr()), host.numel()))
    _lib.check(_lib.load().rcu_postnet_finalize_weights(handle))


def _forward(handle, x, classes, masks, dev):
    from rcu_amd import _lib
    n, c, h, w = x.shape
    view, buf = _nhwc(x, (c + 31) // 32 * 32, dev)
    md = None if masks is None else torch.from_numpy(np.concatenate([m.reshape(-1) for m in masks]).astype(np.float32)).to(dev)
    out = torch.full((n, classes, h, w), float('nan'), device=dev)
    _lib.check(_lib.load().rcu_postnet_forward(handle, _lib.ptr(buf), buf.shape[-1], n, h * w, _lib.ptr(md), _lib.ptr(out), _lib.current_stream()))
    return out


@pytest.mark.timeout(300)
def test_without_batchnorm_through_the_c_abi(dev):
    from rcu_amd import _lib
    channels, classes, nb_convs, shape = 32, 2, 2, (3, 5, 7)
    state, x, masks = pr.seam_case(shape, channels, classes, nb_convs)
    conv_keys = [k for k in state if '.bn.' not in k]
    bn_keys = [k for k in state if '.bn.' in k and not k.endswith('num_batches_tracked')]
    handle = _create(channels, classes, nb_convs, 0)
    try:
        _load(handle, state, conv_keys)
        got = {}
        for tag, m in (('eval', None), ('masked', masks)):
            logits, bound = pr.forward(state, x, nb_convs, m, bn=False)
            with_bn = pr.forward(state, x, nb_convs, m)[0]
            assert float(np.abs(with_bn - logits).max()) > 1e-2, 'BatchNorm was meant to matter'
            got[tag] = _forward(handle, x, classes, m, dev)
            check_against_the_chain(got[tag].cpu().numpy(), logits, bound, ('bn=0', tag))
        _load(handle, state, bn_keys + conv_keys)          # BatchNorm tensors beside the convs: bn = 0 does not read them
        for tag, m in (('eval', None), ('masked', masks)):
            assert torch.equal(_forward(handle, x, classes, m, dev), got[tag]), tag
    finally:
        _lib.load().rcu_postnet_destroy(handle)
    # with bn = 1 the same handle type needs them
    handle = _create(channels, classes, nb_convs, 1)
    try:
        with pytest.raises(_lib.RcuError, match='missing weight tensor'):
            _load(handle, state, conv_keys)
    finally:
        _lib.load().rcu_postnet_destroy(handle)


# ------------------------------------------------------------------------------------------ limits
@pytest.mark.timeout(300)
def test_the_limits_of_the_lds_image(dev):
    from rcu_amd import _lib
    from rcu_amd.model import PostNet
    with pytest.raises(_lib.RcuError, match='160 KB'):
        _create(96, 2, 4, 1)                                # 5 layers x 37,632 B; (96, 2, 3) runs in tests/test_gpu_capped_launches.py
    with pytest.raises(_lib.RcuError, match='at most 11 hidden convs'):
        _create(32, 2, 12, 1)
    with pytest.raises(_lib.RcuError):
        PostNet(32, 2, nb_convs=12).to(dev)(torch.zeros(1, 32, 5, 7, device=dev))
    state, x, masks = pr.seam_case((3, 5, 7), 32, 2, 11)   # the deepest chain: 12 layers, 52 KB of LDS
    post = _post(state, 32, 2, 11, dev)
    for tag, m in (('eval', None), ('masked', masks)):
        logits, bound = pr.forward(state, x, 11, m)
        check_against_the_chain(post(torch.from_numpy(x).to(dev), m).cpu().numpy(), logits, bound, ('nb_convs=11', tag))
