"""Last-layer Laplace on the GPU (include/rcu.h "Last-layer Laplace"): the moments kernel and the predictive kernel against the float64 reference
with the bounds of their float32 arithmetic, their bit-for-bit contracts (a slice's rows / a voxel's outputs are functions of that slice / voxel
alone), the classifier tap, the fit and the predict step on a synthetic U-Net.

Largest fractions of the bounds used on the MI355X (every test prints its own): moments 0.023, s2 (through std^2) 0.163, std 0.163, probabilities 0.067
-- above the predict kernel's grid cap 0.087, 0.087, 0.067; head_features 5.5e-7 of the oracle's range against 2e-6 (README, "Last-layer Laplace")."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import laplace_reference as ref
from test_gpu_step_seam import P_TOL      # the tolerance the project applies to its float32 softmax kernel

pytestmark = pytest.mark.gpu
SHAPES = ((24, 24), (32, 32), (40, 64), (64, 64))      # F / channel pitch
CLASSES = (2, 3, 4)
FEATURE_TOL = 2e-6      # tests/test_gpu_parity.py: LOGIT_TOL, here of the range of the oracle's activations


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda')


def _at_pitch(psi, pitch, seed=1):
    """[..., F] -> float32 [..., pitch] with finite garbage planted in the padding channels."""
    out = (np.random.default_rng(seed).standard_normal(psi.shape[:-1] + (pitch,)) * 1.0e3).astype(np.float32)
    out[..., :psi.shape[-1]] = psi
    return out


def _float32_softmax(z):
    z = z.astype(np.float32)
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _problem(F, C, n=3, hw=279):
    """Seeded features (non-negative, correlated, channel 2 dead), a classifier, and float32 probabilities with a saturated voxel per slice."""
    rng = np.random.default_rng(1000 * F + 10 * C + hw % 7)
    mix = rng.normal(0.0, 1.0, (F, F)) / np.sqrt(F) + np.diag(rng.uniform(0.3, 1.2, F))
    psi = np.maximum(rng.normal(0.2, 1.0, (n, hw, F)) @ mix.T, 0.0).astype(np.float32)
    psi[..., 2] = 0.0
    W = (rng.normal(0.0, 1.5, (C, F)) / np.sqrt(F)).astype(np.float32)
    w0 = rng.normal(0.0, 0.5, C).astype(np.float32)
    z = (psi.astype(np.float64) @ W.astype(np.float64).T + w0).astype(np.float32)
    z[:, 3] = 0.0
    z[:, 3, C - 1] = 150.0           # float32 softmax: exactly 1 and 0
    return psi, W, w0, z, _float32_softmax(z)


@functools.lru_cache(maxsize=None)
def _fit(F, C):
    from rcu_amd import laplace
    psi, W, w0, z, p = _problem(F, C)
    theta = np.concatenate([W, w0[:, None]], 1).astype(np.float64)
    return laplace.fit_from_moments(*ref.moments(psi, p), theta, 0.5, 2.0)


# ------------------------------------------------------------------------------------------------------------------ moments
def _moments(x, pitch, F, probs, n, hw, C, dev):
    """rcu_laplace_moments on device tensors (any views: their data_ptr is what the kernel gets) -> numpy (w, S, G)."""
    from rcu_amd import _lib
    lib = _lib.load()
    P = C * (C + 1) // 2
    w = torch.full((n, P), float('nan'), device=dev, dtype=torch.float64)
    S = torch.full((n, P, F), float('nan'), device=dev, dtype=torch.float64)
    G = torch.full((n, P, F, F), float('nan'), device=dev, dtype=torch.float64)
    nbytes = lib.rcu_laplace_moments_workspace_bytes(n, hw, F, C)
    assert nbytes % 256 == 0      # (0: a shape the call below refuses)
    ws = torch.full((max(nbytes, 256) // 8,), float('nan'), device=dev, dtype=torch.float64)
    _lib.check(lib.rcu_laplace_moments(ctypes.c_void_p(x.data_ptr()), pitch, F, ctypes.c_void_p(probs.data_ptr()), n, hw, C, _lib.ptr(w), _lib.ptr(S),
                                       _lib.ptr(G), _lib.ptr(ws), _lib.current_stream()))
    return w.cpu().numpy(), S.cpu().numpy(), G.cpu().numpy()


def _nchw(p):
    """[n, hw, C] -> contiguous [n, C, hw]"""
    return np.ascontiguousarray(np.swapaxes(p, 1, 2))


@pytest.mark.parametrize('C', CLASSES)
@pytest.mark.parametrize('F, pitch', SHAPES)
@pytest.mark.parametrize('hw', [279, 1024, 1087, 2 * 1024 + 1])
def test_moments_against_the_reference(dev, hw, F, pitch, C):
    psi, _, _, _, p = _problem(F, C, 3, hw)
    want = ref.moments(psi, p)
    bounds = ref.moment_bounds(psi, p)
    got = _moments(torch.from_numpy(_at_pitch(psi, pitch)).to(dev), pitch, F, torch.from_numpy(_nchw(p)).to(dev), 3, hw, C, dev)
    used = 0.0
    for name, g, r, b in zip('wSG', got, want, bounds):
        assert np.isfinite(g).all(), name
        err = np.abs(g - r)
        used = max(used, float((err[b > 0] / b[b > 0]).max()))
        assert (err <= b).all(), (name, float((err - b).max()))
    assert np.array_equal(got[2], np.swapaxes(got[2], 2, 3))          # both triangles, the same bits
    assert not got[1][:, :, 2].any() and not got[2][:, :, 2].any()      # the dead channel
    print('moments hw={} F={}/{} C={}: largest fraction of the bound used {:.4f}'.format(hw, F, pitch, C, used))


@pytest.mark.parametrize('F, pitch, C, hw', [(40, 64, 4, 1087), (32, 32, 2, 2 * 1024 + 1), (64, 64, 3, 279), (24, 32, 3, 1024)])
def test_moments_of_a_slice_do_not_depend_on_the_batch_the_padding_or_the_stream(dev, F, pitch, C, hw):
    psi, _, _, _, p = _problem(F, C, 3, hw)
    x = torch.from_numpy(_at_pitch(psi, pitch)).to(dev)
    y = torch.from_numpy(_nchw(p)).to(dev)
    abc = _moments(x, pitch, F, y, 3, hw, C, dev)
    # slices [c, a], other garbage in the channels >= F, on another stream
    ca_x = torch.from_numpy(_at_pitch(psi[[2, 0]], pitch, seed=7)).to(dev)
    ca_y = torch.from_numpy(_nchw(p[[2, 0]])).to(dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ca = _moments(ca_x, pitch, F, ca_y, 2, hw, C, dev)
    side.synchronize()
    alone = _moments(x[1], pitch, F, y[1], 1, hw, C, dev)
    for full, swapped, one in zip(abc, ca, alone):
        assert full[2].tobytes() == swapped[0].tobytes() and full[0].tobytes() == swapped[1].tobytes()
        assert full[1].tobytes() == one[0].tobytes()


def test_moments_arguments_are_checked_before_the_device_is_touched(dev):
    from rcu_amd import _lib
    psi, _, _, _, p = _problem(32, 2)
    x = torch.from_numpy(_at_pitch(psi, 32)).to(dev)
    y = torch.from_numpy(_nchw(p)).to(dev)
    for args, msg in (((x, 32, 65, y, 3, 279, 2), 'F must be in 1..64'), ((x, 30, 30, y, 3, 279, 2), 'multiple of 4'),
                      ((x, 28, 32, y, 3, 279, 2), 'channel_pitch must be >= F'), ((x, 32, 32, y, 3, 279, 5), 'nb_classes must be in 2..4'),
                      ((x, 32, 32, y, 3, 279, 1), 'nb_classes must be in 2..4'), ((x.reshape(-1)[1:], 32, 32, y, 2, 279, 2), '16-byte aligned')):
        with pytest.raises(_lib.RcuError, match=msg):
            _moments(*args, dev)
    assert _lib.load().rcu_laplace_moments_workspace_bytes(3, 279, 32, 5) == 0


# --------------------------------------------------------------------------------------------------------------- predictive
def _predict(x, pitch, F, logits, n, hw, fit, dev, std=True, std_pred=True, prediction=True):
    from rcu_amd import _lib
    a, b, kappa = fit.device_parameters(dev)
    C = fit.C
    out = {'p': torch.full((n, C, hw), float('nan'), device=dev)}
    if std:
        out['std'] = torch.full((n, C, hw), float('nan'), device=dev)
    if std_pred:
        out['std_pred'] = torch.full((n, hw), float('nan'), device=dev)
    if prediction:
        out['prediction'] = torch.full((n, hw), 255, device=dev, dtype=torch.uint8)
    _lib.check(_lib.load().rcu_laplace_predict(ctypes.c_void_p(x.data_ptr()), pitch, F, ctypes.c_void_p(logits.data_ptr()), n, hw, C, _lib.ptr(a),
                                               _lib.ptr(b), _lib.ptr(kappa), _lib.ptr(out['p']), _lib.ptr(out.get('std')), _lib.ptr(out.get('std_pred')),
                                               _lib.ptr(out.get('prediction')), _lib.current_stream()))
    return {k: v.cpu().numpy() for k, v in out.items()}


def _voxels(F, C, nvox):
    """nvox voxels of the problem's kind, a few pushed far off the data so that large variances are met too -> psi [nvox, F], z [nvox, C]"""
    psi, _, _, z, _ = _problem(F, C, 3, 4161)
    psi, z = psi.reshape(-1, F)[:nvox].copy(), z.reshape(-1, C)[:nvox].copy()
    psi[5::23] *= 30.0
    z[11::29] *= 8.0
    return psi, z


def _check_predictive(got, fit, psi, z, n, hw, tag):
    """got: the kernel's NCHW outputs of n slices of hw voxels; psi [n * hw, F], z [n * hw, C]."""
    C = fit.C
    a32, b32, k32 = fit.float32_parameters()
    want = ref.predictive(a32, b32, k32, psi, z)
    b_s2 = ref.s2_bounds(a32, b32, k32, psi)
    b_std = ref.std_bounds(b_s2, want['s2'])
    tol_p = ref.p_tolerance(ref.zt_bounds(b_s2, want, z), P_TOL)
    flat = {k: (np.swapaxes(v, 1, 2).reshape(n * hw, C) if v.ndim == 3 else v.reshape(n * hw)) for k, v in got.items()}
    assert all(np.isfinite(v).all() for v in flat.values()), tag
    e_std = np.abs(flat['std'] - want['std'])
    e_s2 = np.abs(flat['std'].astype(np.float64) ** 2 - want['s2'])          # s2 itself is not an output: through std^2, the issue's bound ...
    b_sq = ref.s2_through_std_bounds(b_s2, want['s2'])                       # ... plus the one rounding of the root
    e_p = np.abs(flat['p'] - want['p'])
    used = (float((e_s2 / b_sq).max()), float((e_std / b_std).max()), float((e_p / tol_p).max()))
    print('predictive {}: largest fraction of the bound used s2 {:.4f}, std {:.4f}, p {:.4f}'.format(tag, *used))
    assert (e_std <= b_std).all() and (e_s2 <= b_sq).all() and (e_p <= tol_p).all(), (tag, used)
    # the prediction is the first maximum of the probabilities the kernel wrote, std_pred the std of that class
    assert np.array_equal(flat['prediction'], flat['p'].argmax(1))
    assert flat['std_pred'].tobytes() == flat['std'][np.arange(n * hw), flat['prediction']].tobytes()
    return used


@pytest.mark.parametrize('C', CLASSES)
@pytest.mark.parametrize('F, pitch', SHAPES)
@pytest.mark.parametrize('n, hw', [(1, 1), (1, 63), (1, 65), (7, 1783)])      # 7 x 1783 = 12,481 voxels
def test_predictive_against_the_reference(dev, n, hw, F, pitch, C):
    fit = _fit(F, C)
    psi, z = _voxels(F, C, n * hw)
    x = torch.from_numpy(_at_pitch(psi, pitch)).to(dev)
    logits = torch.from_numpy(_nchw(z.reshape(n, hw, C))).to(dev)
    got = _predict(x, pitch, F, logits, n, hw, fit, dev)
    _check_predictive(got, fit, psi, z, n, hw, 'n={} hw={} F={}/{} C={}'.format(n, hw, F, pitch, C))
    assert np.abs(got['p'].sum(1) - 1.0).max() < 4 * P_TOL


CAPPED_SHAPE = (3, 457, 401)      # tests/capped_launches.py: hw = 183,257 = 32 * 5726 + 25


@pytest.mark.parametrize('F, pitch, C', [(32, 32, 2), (24, 24, 4), (64, 64, 2), (40, 64, 4)])
def test_predictive_above_the_grid_cap(dev, F, pitch, C):
    """launch_predict caps the grid at 2048 workgroups x 4 waves x 32 voxels = 262,144 voxels per round; every production batch is walked by the
    cur / nxt prefetch loop behind it.  3 x 457 x 401 = 549,771 voxels are 17,181 groups for 8,192 waves: every wave takes a second group, 797 a
    third, and the last group holds 11 voxels.  Against the float64 reference within the bounds, and bit for bit against the same voxels run as
    one-image calls (5,727 groups: one trip, no prefetch beyond it)."""
    n, h, w = CAPPED_SHAPE
    hw = h * w
    assert (n * hw + 31) // 32 > 2 * 2048 * 4 and hw <= 2048 * 4 * 32 and (n * hw) % 32 == 11
    fit = _fit(F, C)
    base_psi, base_z = _voxels(F, C, 12481)
    psi = np.resize(base_psi, (n * hw, F)).copy()
    z = np.resize(base_z, (n * hw, C)).copy()
    psi[7::31] *= 2.0            # (12,481 = 7 x 1783: every repetition is perturbed at other voxels)
    z[3::37] *= -1.5
    x = torch.from_numpy(_at_pitch(psi, pitch)).to(dev).reshape(n, hw, pitch)
    logits = torch.from_numpy(_nchw(z.reshape(n, hw, C))).to(dev)
    whole = _predict(x, pitch, F, logits, n, hw, fit, dev)
    used = np.zeros(3)
    for i in range(n):
        rows = slice(i * hw, (i + 1) * hw)
        used = np.maximum(used, _check_predictive({k: v[i:i + 1] for k, v in whole.items()}, fit, psi[rows], z[rows], 1, hw,
                                                  'above the cap, image {} F={}/{} C={}'.format(i, F, pitch, C)))
        piece = _predict(x[i], pitch, F, logits[i], 1, hw, fit, dev)
        for key in whole:
            assert whole[key][i:i + 1].tobytes() == piece[key].tobytes(), (key, i)
    print('predictive above the cap F={}/{} C={}: largest fraction of the bound used s2 {:.4f}, std {:.4f}, p {:.4f}'.format(F, pitch, C, *used))


@pytest.mark.parametrize('F, pitch, C', [(24, 24, 3), (32, 32, 2), (40, 64, 4), (64, 64, 2), (13, 16, 3)])
def test_outputs_of_a_voxel_do_not_depend_on_the_call(dev, F, pitch, C):
    if F == 13:      # no multiple of 4: the last float4 of a voxel is cut
        from rcu_amd import laplace
        psi0, W, w0, _, p0 = _problem(24, C)
        theta = np.concatenate([W[:, :13], w0[:, None]], 1).astype(np.float64)
        fit = laplace.fit_from_moments(*ref.moments(psi0[..., :13], p0), theta, 1.0, 1.0)
        psi, z = _voxels(24, C, 601)
        psi = np.ascontiguousarray(psi[:, :13])
    else:
        fit = _fit(F, C)
        psi, z = _voxels(F, C, 601)
    hw = 601
    base = _predict(torch.from_numpy(_at_pitch(psi, pitch)).to(dev), pitch, F, torch.from_numpy(_nchw(z[None])).to(dev), 1, hw, fit, dev)
    _check_predictive(base, fit, psi, z, 1, hw, 'base F={} C={}'.format(F, C))
    # a permutation of the voxels (with other garbage in the padding) permutes the outputs bit for bit
    perm = np.random.default_rng(F).permutation(hw)
    moved = _predict(torch.from_numpy(_at_pitch(psi[perm], pitch, seed=9)).to(dev), pitch, F, torch.from_numpy(_nchw(z[perm][None])).to(dev), 1, hw,
                     fit, dev)
    for key in base:
        assert np.take(base[key], perm, axis=-1).tobytes() == moved[key].tobytes(), key
    # the same voxels as 3 slices of 200 and one voxel short: another n, hw and tail
    cut = _predict(torch.from_numpy(_at_pitch(psi[:600], pitch)).to(dev), pitch, F,
                   torch.from_numpy(_nchw(z[:600].reshape(3, 200, C))).to(dev), 3, 200, fit, dev)
    assert np.swapaxes(cut['p'], 0, 1).reshape(C, 600).tobytes() == np.ascontiguousarray(base['p'][0][:, :600]).tobytes()
    assert cut['std_pred'].reshape(600).tobytes() == base['std_pred'][0, :600].tobytes()
    # NULL optional outputs change no other output's bits
    x, logits = torch.from_numpy(_at_pitch(psi, pitch)).to(dev), torch.from_numpy(_nchw(z[None])).to(dev)
    for flags in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        some = _predict(x, pitch, F, logits, 1, hw, fit, dev, *flags)
        assert sorted(some) == sorted(['p'] + [k for k, on in zip(('std', 'std_pred', 'prediction'), flags) if on])
        for key in some:
            assert some[key].tobytes() == base[key].tobytes(), (flags, key)


@pytest.mark.parametrize('C', CLASSES)
def test_prediction_is_the_first_maximum_on_planted_ties(dev, C):
    from rcu_amd import laplace
    F, hw = 32, 97
    fit = _fit(F, C)
    # every class with the parameters of class 0: equal logits then give equal probabilities, bit for bit
    tied = laplace.LaplaceFit(fit.H, fit.Sigma, np.stack([fit.A[0]] * C), np.stack([fit.b[0]] * C), np.stack([fit.kappa[0]] * C), 1.0, 1.0, 1.0, 0)
    psi, z = _voxels(F, C, hw)
    rng = np.random.default_rng(C)
    z = rng.normal(0, 1, (hw, C)).astype(np.float32)
    want = np.zeros(hw, np.int64)
    for v in range(hw):
        k = v % (C + 1)
        if k < C:      # classes k .. C-1 tie at the top
            z[v, k:] = z[v].max() + 1.0
            want[v] = k
        else:          # all different
            want[v] = int(z[v].argmax())
    got = _predict(torch.from_numpy(psi).to(dev), 32, F, torch.from_numpy(_nchw(z[None])).to(dev), 1, hw, tied, dev)
    assert np.array_equal(got['prediction'][0], want)
    top = got['p'][0].max(0)
    assert all((got['p'][0][k:, v] == top[v]).all() for v in range(hw) for k in [v % (C + 1)] if k < C), 'the ties were meant to survive'


def test_predict_arguments_are_checked_before_the_device_is_touched(dev):
    from rcu_amd import _lib, laplace
    fit = _fit(32, 2)
    psi, z = _voxels(32, 2, 64)
    x, logits = torch.from_numpy(psi).to(dev), torch.from_numpy(_nchw(z[None])).to(dev)
    for args, msg in (((x, 32, 65, logits, 1, 64), 'F must be in 1..64'), ((x, 34, 32, logits, 1, 64), 'multiple of 4'),
                      ((x.reshape(-1)[2:], 32, 32, logits, 1, 62), '16-byte aligned')):
        with pytest.raises(_lib.RcuError, match=msg):
            _predict(*args, fit, dev)
    a, b, kappa = fit.device_parameters(dev)
    status = _lib.load().rcu_laplace_predict(_lib.ptr(x), 32, 32, _lib.ptr(logits), 0, 64, 2, _lib.ptr(a), _lib.ptr(b), _lib.ptr(kappa),
                                             _lib.ptr(torch.empty_like(logits)), None, None, None, _lib.current_stream())
    assert status == _lib.RCU_ERR_INVALID and 'n must be in' in _lib.load().rcu_last_error().decode()
    feats = x.reshape(1, 8, 8, 32).permute(0, 3, 1, 2)
    with pytest.raises(ValueError, match='the fit has F = 32, C = 2'):
        laplace.predict(fit, feats, torch.zeros(1, 3, 8, 8, device=dev))
    with pytest.raises(ValueError, match='logits must be'):
        laplace.predict(fit, feats, torch.zeros(1, 2, 8, 9, device=dev))
    out = laplace.predict(fit, feats, logits.reshape(1, 2, 8, 8))
    raw = _predict(x, 32, 32, logits, 1, 64, fit, dev)
    assert out['probabilities'].cpu().numpy().tobytes() == raw['p'].tobytes() and tuple(out['std_pred'].shape) == (1, 1, 8, 8)
    assert out['std_pred'].cpu().numpy().tobytes() == raw['std_pred'].tobytes() and out['prediction'].cpu().numpy().tobytes() == raw['prediction'].tobytes()


# ---------------------------------------------------------------------------------------------------------------------- tap
PARAMS = dict(nb_classes=2, in_channels=4, depth=2, start_filters=32, dropout=0.05)      # the smallest U-Net of tests/test_gpu_density.py


def _unet(dev, seed=11, **over):
    from oracle import unet_oracle as uo
    from rcu_amd.model import UNet
    params = dict(PARAMS, **over)
    state = uo.synthetic_state(seed, **params)
    m = UNet(**params)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    return m.to(dev).eval(), state, params


@pytest.mark.parametrize('shape', [(32, 32), (40, 24)])      # (40 x 24: level 0 is allocated with whole tiles, the head tensor is compact all the same)
@pytest.mark.parametrize('classes', [2, 3])
def test_head_features_are_the_oracles_and_the_logits_keep_their_bits(dev, shape, classes):
    from oracle import unet_oracle as uo
    from rcu_amd import _lib
    h, w = shape
    m, state, params = _unet(dev, nb_classes=classes)
    x = torch.randn(3, 4, h, w, generator=torch.Generator().manual_seed(h))
    seen = {}

    def tap(index, op, tensor):
        if op['key'].startswith('conv_cls.0'):
            seen['psi'] = tensor
        return tensor
    uo.unet_forward(state, x, tap=tap, **params)
    plain = m(x.to(dev))
    assert m.head_features is None
    handle = m._handle(h, w, 3)
    ptr, ch, pitch = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()

    def state_error():
        status = _lib.load().rcu_unet_head_features(handle, ctypes.byref(ptr), ctypes.byref(ch), ctypes.byref(pitch))
        return status, _lib.load().rcu_last_error().decode()
    if classes == 2:      # the shipped shape: that forward fused the classifier into conv_cls.0
        status, text = state_error()
        assert status == _lib.RCU_ERR_STATE and 'fused the classifier' in text, (status, text)
    m.provide_head_features = True
    tapped = m(x.to(dev))
    assert tapped.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    feats = m.head_features
    assert tuple(feats.shape) == (3, 32, h, w) and m.fuse_head is True
    want = seen['psi']
    spread = float(want.max() - want.min())
    worst = float((feats.cpu() - want).abs().max())
    print('head_features {}x{} C={}: {:.3e} of the range {:.3f} (bound {:.0e})'.format(h, w, classes, worst / spread, spread, FEATURE_TOL))
    assert worst <= FEATURE_TOL * spread
    assert state_error()[0] == 0 and (ch.value, pitch.value) == (32, feats.permute(0, 2, 3, 1).stride(2))
    # the logits are the classifier on the tapped tensor
    again = torch.nn.functional.conv2d(feats, torch.as_tensor(state['conv_cls.1.weight']).to(dev), torch.as_tensor(state['conv_cls.1.bias']).to(dev))
    assert float((again - tapped).abs().max()) < 1e-5
    m.provide_head_features = False
    after = m(x.to(dev))
    assert after.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes() and m.head_features is None
    if classes == 2:
        assert state_error()[0] == _lib.RCU_ERR_STATE


def test_head_features_state_errors(dev):
    from rcu_amd import _lib
    lib = _lib.load()
    ptr = ctypes.c_void_p()
    m, _, _ = _unet(dev)
    fresh = m._handle(32, 32, 2)
    assert lib.rcu_unet_head_features(fresh, ctypes.byref(ptr), None, None) == _lib.RCU_ERR_STATE      # no forward yet
    assert lib.rcu_unet_head_features(None, ctypes.byref(ptr), None, None) == _lib.RCU_ERR_INVALID
    s, _, _ = _unet(dev, sigma_out=True)
    x = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(1)).to(dev)
    s(x)      # a sigma_out forward takes the separate head kernel, and is refused all the same
    assert lib.rcu_unet_head_features(s._handle(32, 32, 2), ctypes.byref(ptr), None, None) == _lib.RCU_ERR_STATE
    assert 'sigma_out' in lib.rcu_last_error().decode()
    s.provide_head_features = True
    with pytest.raises(ValueError, match='sigma_out'):
        s(x)


# ------------------------------------------------------------------------------------------------------------- step and fit
def _fit_bits(fit):
    return [getattr(fit, name).tobytes() for name in ('H', 'Sigma', 'A', 'b', 'kappa')] + [fit.tau, fit.voxels]


@pytest.mark.parametrize('shape, classes', [((32, 32), 2), ((40, 24), 2), ((32, 32), 3)])
def test_fit_and_step_on_a_synthetic_unet(dev, shape, classes):
    from rcu_amd import laplace, steps
    h, w = shape
    m, state, _ = _unet(dev, nb_classes=classes)
    images = torch.randn(6, 4, h, w, generator=torch.Generator().manual_seed(h + w)).to(dev)
    fits = []
    for cuts in ((6,), (4, 2), (1, 5)):
        edges = np.cumsum((0,) + cuts)
        fits.append(laplace.fit_laplace(m, [(images[a:b],) for a, b in zip(edges[:-1], edges[1:])], hessian_scale=0.1, prior_precision='evidence'))
        assert m.provide_head_features is False and not m.mc_active()
    backwards = laplace.fit_laplace(m, [images[3:].flip(0), images[:3]], hessian_scale=0.1, prior_precision='evidence')
    assert _fit_bits(fits[0]) == _fit_bits(fits[1]) == _fit_bits(fits[2]) == _fit_bits(backwards)
    fit = fits[0]
    assert (fit.F, fit.C, fit.voxels, fit.hessian_scale, fit.temperature) == (32, classes, 6 * h * w, 0.1, 1.0)

    ctx = steps.TorchTestContext('cuda', m)
    bc = steps.BatchContext({'images': images.cpu().clone()}, 0, 0)
    steps.LaplacePredictStep(fit)(bc, None, ctx)
    feats = m.head_features.cpu()           # the host round trip, before any other forward
    assert m.provide_head_features is False
    plain = steps.BatchContext({'images': images.cpu().clone()}, 0, 0)
    steps.SegmentationPredictStep(do_probs=True)(plain, None, ctx)
    logits = plain.output['logits']
    assert bc.output['logits'].cpu().numpy().tobytes() == logits.cpu().numpy().tobytes()
    std = bc.output['laplace_std']
    assert tuple(std.shape) == (6, 1, h, w) and std.dtype == torch.float32 and tuple(bc.output['probabilities'].shape) == (6, classes, h, w)
    # against predict on the materialised tensors, and those against the reference
    out = laplace.predict(fit, feats.to(dev), logits)
    assert out['probabilities'].cpu().numpy().tobytes() == bc.output['probabilities'].cpu().numpy().tobytes()
    assert out['std_pred'].cpu().numpy().tobytes() == std.cpu().numpy().tobytes()
    psi = feats.permute(0, 2, 3, 1).reshape(-1, 32).numpy()
    z = logits.permute(0, 2, 3, 1).reshape(-1, classes).cpu().numpy()
    got = {'p': out['probabilities'].reshape(6, classes, h * w).cpu().numpy(), 'std': out['std'].reshape(6, classes, h * w).cpu().numpy(),
           'std_pred': out['std_pred'].reshape(6, h * w).cpu().numpy(), 'prediction': out['prediction'].reshape(6, h * w).cpu().numpy()}
    _check_predictive(got, fit, psi, z, 6, h * w, 'step {}x{} C={}'.format(h, w, classes))
    p_model = plain.output['probabilities']
    assert not torch.equal(out['probabilities'], p_model), 'the predictive was meant to differ from the softmax'
    # the fit against the float64 reference on the same tensors (the moments are within their float32 bound: a loose check here)
    theta = np.concatenate([state['conv_cls.1.weight'].reshape(classes, 32), state['conv_cls.1.bias'].reshape(classes, 1)], 1).astype(np.float64)
    p32 = p_model.permute(0, 2, 3, 1).reshape(6, h * w, classes).cpu().numpy()
    theirs = ref.fit(*ref.moments(psi.reshape(6, h * w, 32), p32), theta, 0.1, 'evidence')
    assert theirs['tau'] == fit.tau
    np.testing.assert_allclose(fit.H, theirs['H'], rtol=0, atol=1e-4 * np.abs(theirs['H']).max())

    # link='sample': sample_logits of (z, std) under the aleatoric key, whatever the batching
    sampled = steps.BatchContext({'images': images.cpu().clone()}, 0, 0)
    steps.LaplacePredictStep(fit, link='sample', samples=8, seed=5)(sampled, None, ctx)
    want = steps.sample_logits(logits, out['std'], 8, steps.pass_seed(5, 0), 0)
    assert sampled.output['probabilities'].cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert sampled.output['logits'].cpu().numpy().tobytes() == logits.cpu().numpy().tobytes()
    halves = []
    for index, (a, b) in enumerate(((0, 4), (4, 6))):
        part = steps.BatchContext({'images': images[a:b].cpu().clone()}, index, a)
        steps.LaplacePredictStep(fit, link='sample', samples=8, seed=5)(part, None, ctx)
        halves.append(part.output)
    for key in ('probabilities', 'laplace_std'):
        assert torch.cat([o[key] for o in halves]).cpu().numpy().tobytes() == sampled.output[key].cpu().numpy().tobytes(), key

    # refusals on the device side
    with pytest.raises(ValueError, match='start_filters = 8'):
        steps.LaplacePredictStep(fit)(steps.BatchContext({'images': images.cpu()}, 0, 0), None, steps.TorchTestContext('cuda', _unet(dev, start_filters=8)[0]))
    m.set_temperature(2.0)
    with pytest.raises(ValueError, match='made at temperature 1.0, the model runs at 2.0'):
        steps.LaplacePredictStep(fit)(steps.BatchContext({'images': images.cpu()}, 0, 0), None, ctx)
    scaled = laplace.fit_laplace(m, [images])
    assert scaled.temperature == 2.0 and not np.array_equal(scaled.H, fit.H)
    m.set_temperature(1.0)


# ------------------------------------------------------------------------------------------------------------------ scripts
def _nii(ctx):
    import glob
    import os
    return {os.path.basename(f): open(f, 'rb').read() for f in sorted(glob.glob(os.path.join(ctx.test_dir, '*.nii.gz')))}


def test_fit_script_then_the_default_script_then_the_evaluation(tmp_path):
    import csv
    import glob
    import json
    import os
    import test_gpu_scripts as tgs
    from rcu_amd import laplace, nifti, scripts, steps
    from rcu_amd.model import UNet
    cfg, vols, states, params = tgs._setup(tmp_path)
    fit = scripts.fit_laplace('brats', tgs._with_others(cfg, 'fit', laplace_hessian_scale=0.05, laplace_prior_precision='evidence'))
    fit_dir = glob.glob(str(tmp_path / 'out_fit' / '*'))[0]
    npz = os.path.join(fit_dir, 'laplace.npz')
    doc = json.load(open(os.path.join(fit_dir, 'laplace.json')))
    assert (doc['F'], doc['C'], doc['hessian_scale'], doc['temperature'], doc['test_at'], doc['prior_precision']) == (32, 2, 0.05, 1.0, 'best', 'evidence')
    assert doc['voxels'] == sum(v[1].size for v in vols.values()) == fit.voxels and doc['tau'] == fit.tau and doc['model_dir']
    assert _fit_bits(laplace.load_laplace(npz)) == _fit_bits(fit)

    without = scripts.test_default('brats', tgs._with_others(cfg, 'plain'), None)
    with_key = scripts.test_default('brats', tgs._with_others(cfg, 'laplace', laplace=npz), None)
    a, b = _nii(without), _nii(with_key)
    assert len(a) == 2 * len(vols) and sorted(b) == sorted(list(a) + ['{}_laplace_std.nii.gz'.format(name) for name in vols])
    assert not os.path.exists(os.path.join(without.test_dir, 'laplace.json'))
    assert sorted(os.listdir(without.test_dir)) == sorted(f for f in os.listdir(with_key.test_dir) if 'laplace' not in f)
    record = json.load(open(os.path.join(with_key.test_dir, 'laplace.json')))
    assert record == dict(fit.as_dict(), file=npz, link='probit', samples=0, seed=record['seed'])
    # the files hold the step's predictive and its map
    m = UNet(**params)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in states[0].items()})
    m = m.to('cuda').eval()
    for name, (images, _, props) in vols.items():
        bc = steps.BatchContext({'images': torch.from_numpy(images).permute(0, 3, 1, 2).contiguous()}, 0, 0)
        steps.LaplacePredictStep(fit)(bc, None, steps.TorchTestContext('cuda', m))
        got, rprops = nifti.read(os.path.join(with_key.test_dir, name + '_laplace_std.nii.gz'))
        assert got.dtype == np.float32 and rprops == props and got.tobytes() == bc.output['laplace_std'][:, 0].cpu().numpy().tobytes()
        pred, fg = steps.prediction_and_foreground(bc.output['probabilities'])
        p_file, _ = nifti.read(os.path.join(with_key.test_dir, name + '_probabilities.nii.gz'))
        pred_file, _ = nifti.read(os.path.join(with_key.test_dir, name + '_prediction.nii.gz'))
        assert np.array_equal(p_file, fg.cpu().numpy().astype(p_file.dtype)) and np.array_equal(pred_file, pred.cpu().numpy())
        assert a[name + '_probabilities.nii.gz'] != b[name + '_probabilities.nii.gz'], 'the predictive was meant to differ from the softmax'
        # ... and the run without the key holds the default step's softmax and arg-max, as before the key existed
        plain = steps.BatchContext({'images': torch.from_numpy(images).permute(0, 3, 1, 2).contiguous()}, 0, 0)
        steps.SegmentationPredictStep(do_probs=True)(plain, None, steps.TorchTestContext('cuda', m))
        pred0, fg0 = steps.prediction_and_foreground(plain.output['probabilities'])
        p0_file, props0 = nifti.read(os.path.join(without.test_dir, name + '_probabilities.nii.gz'))
        pred0_file, _ = nifti.read(os.path.join(without.test_dir, name + '_prediction.nii.gz'))
        assert props0 == props and p0_file.dtype == np.float32 and p0_file.tobytes() == fg0.cpu().numpy().tobytes()
        assert pred0_file.dtype == np.uint8 and pred0_file.tobytes() == pred0.cpu().numpy().tobytes()

    # byte-identical files for another batch_size
    text = open(cfg).read()
    assert 'batch_size: 4' in text
    cfg_one = str(tmp_path / 'test_cfg_one.yaml')
    with open(cfg_one, 'w') as f:
        f.write(text.replace('batch_size: 4', 'batch_size: 1'))
    one = scripts.test_default('brats', tgs._with_others(cfg_one, 'laplace_b1', laplace=npz), None)
    assert _nii(one) == b
    assert open(os.path.join(one.test_dir, 'metrics.csv'), 'rb').read() == open(os.path.join(with_key.test_dir, 'metrics.csv'), 'rb').read()

    # composed: the sample link under a corruption and the device metrics -- the run completes and writes the same file names
    shifted = scripts.test_default('brats', tgs._with_others(cfg, 'shift', laplace=npz, laplace_link='sample', laplace_samples=4,
                                                             corruption=[dict(kind='gaussian_noise', severity=5)]), None)
    c = _nii(shifted)
    assert sorted(c) == sorted(b) and all(np.isfinite(nifti.read(os.path.join(shifted.test_dir, n + '_laplace_std.nii.gz'))[0]).all() for n in vols)
    assert json.load(open(os.path.join(shifted.test_dir, 'laplace.json')))['link'] == 'sample'
    # a fit made at another temperature is refused by the run, one made at the run's temperature is taken
    with pytest.raises(ValueError, match='made at temperature 1.0, the model runs at 1.5'):
        scripts.test_default('brats', tgs._with_others(cfg, 'wrong_t', laplace=npz, temperature=1.5), None)
    fit_t = scripts.fit_laplace('brats', tgs._with_others(cfg, 'fit_t', temperature=1.5))
    assert fit_t.temperature == 1.5
    npz_t = os.path.join(glob.glob(str(tmp_path / 'out_fit_t' / '*'))[0], 'laplace.npz')
    scaled = scripts.test_default('brats', tgs._with_others(cfg, 'right_t', laplace=npz_t, temperature=1.5), None)
    assert sorted(_nii(scaled)) == sorted(b)

    # the evaluation on the run as the types `laplace` and `laplace_std`
    gt = tmp_path / 'gt' / 'HGG'
    for name, (images, labels, props) in vols.items():
        (gt / name).mkdir(parents=True)
        for mod, arr in (('flair', images[..., 0]), ('t1', images[..., 1]), ('t2', images[..., 2]), ('t1ce', images[..., 3]), ('seg', labels * 4)):
            nifti.write(str(gt / name / '{}_{}.nii.gz'.format(name, mod)), arr, props)
    scripts.eval_uncertainty('brats', {'laplace': with_key.test_dir, 'laplace_std': with_key.test_dir}, str(tmp_path / 'gt'), str(tmp_path / 'eval'),
                             actions=('minmax', 'ece_dice', 'ue_curves'), expected_subjects=list(vols))
    written = glob.glob(str(tmp_path / 'eval' / '**' / '*.csv'), recursive=True)
    names = [os.path.basename(f) for f in written]
    assert any('minmax' in f and 'laplace_std' in f for f in names) and sum('laplace_std' in f for f in names) >= 2, names
    assert sum('laplace' in f and 'laplace_std' not in f for f in names) >= 2, names
    numbers = 0
    for f in written:
        for row in csv.reader(open(f)):
            for cell in row:
                try:
                    value = float(cell)
                except ValueError:
                    continue
                numbers += 1
                assert np.isfinite(value), (f, row)
    assert numbers > 20
