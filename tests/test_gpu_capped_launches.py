"""The grid-capped kernels beyond their caps (tests/capped_launches.py has the table and its arithmetic): at every shape here some wave or
workgroup walks a second and a third item, the last item is partial and items straddle image boundaries.  Every case asserts
  (a) the whole call against the float64 reference of the operation, within the tolerance the kernel's own test file uses, and
  (b) the whole call bit for bit against the same voxels run as one-trip pieces (one image each) on the same plan, weights and masks:
      a voxel's result is a function of that voxel's inputs alone.
The caps are the shipped ones; nothing here lowers them.

Fractions of the bounds used on the MI355X at 549,771 voxels (every test prints its own): density d2 0.018 / 0.006 / 0.008 and energy 0.015 /
0.001 / 0.003 at F = 32 / 45 / 64 (test_gpu_density.py's small shapes: 0.028 and 0.026); PostNet's derived bound 0.0011 and less at three hidden
convs, its largest distance from the float64 chain 2.5e-7 (bound 2e-5); head logits 3.2e-7 (bound 2e-6); temperature terms 0.043 of their tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import capped_launches as cl
import postnet_reference as pr
import quantile_reference as qr
import step_seam_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda')


@pytest.fixture(scope='module')
def g32(golden):
    return golden('g32_density')


# ------------------------------------------------------------------------------------------------------------------- PostNet
def _post(state, channels, classes, nb_convs, dev):
    from rcu_amd.model import PostNet
    post = PostNet(channels, classes, nb_convs=nb_convs).to(dev)
    post.load_state_dict(state)
    return post


@pytest.mark.timeout(300)
@pytest.mark.parametrize('masked', [False, True], ids=['eval', 'masked'])
@pytest.mark.parametrize('case', cl.POSTNET_CASES, ids=lambda c: '-'.join(map(str, c)))
def test_postnet_above_the_cap(dev, case, masked):
    import test_gpu_postnet as tp
    channels, classes, nb_convs = case
    n, h, w = cl.POSTNET_SHAPE
    state, x, masks = cl.postnet_capped_case(channels, classes, nb_convs, masked)
    post = _post(state, channels, classes, nb_convs, dev)
    xd = torch.from_numpy(x).to(dev)
    whole = post(xd, masks)
    logits, bound = pr.forward(state, x, nb_convs, masks)
    tp.check_against_the_chain(whole.cpu().numpy(), logits, bound, (case, masked, 'above the cap'))
    for i in range(n):      # one image is below the cap: every wave takes one group
        piece = post(xd[i:i + 1], None if masks is None else [m[i:i + 1] for m in masks])
        assert torch.equal(whole[i:i + 1], piece), (case, masked, i)
    if case == cl.POSTNET_CASES[0] and not masked:
        # read in place through a strided view: 32 of 64 floats per voxel, the other 32 are beyond 32 * cb and are never read
        buf = torch.randn(n, h, w, 64, generator=torch.Generator().manual_seed(11)) * 1.0e3
        buf[..., :32] = torch.from_numpy(x).permute(0, 2, 3, 1)
        view = buf.to(dev)[..., :32].permute(0, 3, 1, 2)
        assert view.stride(3) == 64 and not view.is_contiguous()
        assert torch.equal(post(view), whole)


@pytest.mark.timeout(600)
def test_feature_tap_and_postnet_above_the_cap(dev):
    """bin-dl/*_test_auxiliary_feat.py on a batch above the cap: a full-width U-Net with provide_features at 240 x 240 (padded levels, the
    compact feature copy) and PostNet on model.features in place and through the generic NCHW path."""
    from oracle import unet_oracle as uo
    from rcu_amd.model import PostNet, UNet
    params = dict(nb_classes=2, in_channels=4, depth=4, start_filters=32, dropout=0.05, provide_features=True)
    n, h, w = 5, 240, 240
    assert n * h * w > cl.ROWS['postnet'].walkers * cl.ROWS['postnet'].item
    state = uo.synthetic_state(41, **params)
    model = UNet(**params)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    model = model.to(dev).eval()
    x = torch.randn(n, 4, h, w, generator=torch.Generator().manual_seed(42))
    _, feats_ref = uo.unet_forward(state, x, None, return_features=True, **params)
    post_state = uo.postnet_synthetic_state(43, 32, 2)
    want = uo.postnet_forward(post_state, feats_ref).numpy()
    post = PostNet(32, 2).to(dev)
    post.load_state_dict(post_state)
    model(x.to(dev))
    feats = model.features
    assert tuple(feats.shape) == (n, 32, h, w) and not feats.is_contiguous()
    in_place = post(feats)
    generic = post(feats.contiguous())
    for tag, got in (('in place', in_place), ('generic', generic)):
        d = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        print('feature tap + PostNet {}: {:.3e} (bound 2e-05)'.format(tag, d))
        assert d < 2e-5, (tag, d)
    assert torch.equal(in_place, generic)


# ------------------------------------------------------------------------------------------------------------------- density energy
def _tiled_voxels(g32, F, nvox):
    """The G32 voxels, tiled to nvox, with the perturbations of test_gpu_density._probe_voxels over the whole length (936 is no multiple
    of 23 or 31: every repetition is perturbed at other voxels)."""
    if F in (32, 64):
        base = g32['phi_{}'.format(F)].reshape(-1, F)
        dead = int(g32['dead_channel'])
    else:
        base = np.ascontiguousarray(g32['phi_64'][..., 4:4 + F].reshape(-1, F))
        dead = int(g32['dead_channel']) - 4
    phi = np.resize(base, (nvox, F)).copy()
    phi[5::23] *= 3.0
    if 0 <= dead < F:
        phi[7::31, dead] += 0.01
    return phi


@pytest.mark.timeout(600)
@pytest.mark.parametrize('F, K, pitch', cl.DENSITY_CASES)
def test_density_energy_above_the_cap(dev, g32, F, K, pitch):
    import density_reference as dref
    import test_gpu_density as tgd
    from rcu_amd import density
    row = cl.ROWS['density_energy']
    nvox, hw = row.work, row.hw
    if F in (32, 64):
        fit = tgd._fit(g32, F, K)
    else:
        fit = density.fit_from_moments(*dref.moments(g32['phi_64'][..., 4:4 + F], tgd._labels(g32, K), K))
    phi = _tiled_voxels(g32, F, nvox)
    x = torch.from_numpy(tgd._at_pitch(phi, pitch)).to(dev)
    e, d2 = tgd._energy(x, pitch, F, nvox, fit, dev)
    tgd._check_energy(e, d2, fit, phi, 'above the cap: nvox={} F={} K={}'.format(nvox, F, K))
    for i in range(row.n_images):
        pe, pd2 = tgd._energy(x[i * hw:], pitch, F, hw, fit, dev)
        assert pe.tobytes() == e[i * hw:(i + 1) * hw].tobytes() and pd2.tobytes() == d2[i * hw:(i + 1) * hw].tobytes(), i
    without, _ = tgd._energy(x, pitch, F, nvox, fit, dev, with_d2=False)
    assert without.tobytes() == e.tobytes()


# ------------------------------------------------------------------------------------------------------------------- temperature
@pytest.mark.timeout(600)
@pytest.mark.parametrize('masked', [False, True], ids=['all', 'mask'])
@pytest.mark.parametrize('p, c', cl.TEMPERATURE_CASES)
def test_temperature_sweep_above_the_cap(dev, p, c, masked):
    import test_gpu_temperature as tt
    from rcu_amd import calibration as cal
    n, hw = cl.TEMPERATURE_SHAPE
    z, y = tt._case(p, c, n=n, hw=hw)
    z[:, 2, :, hw - 96:] = z[:, 0, :, :96]                    # the saturated block again, in the tiles of the third trip
    mask = (np.random.RandomState(5).rand(*y.shape) < 0.6) if masked else None
    keep = np.ones(y.shape, bool) if mask is None else mask
    sweep = tt._sweep(z.reshape(p, n, c, hw), y, mask, dev)
    sums = sweep.sums()
    assert len(sums) == len(cal.CANDIDATES) == 97 and sweep.voxels == int(keep.sum())
    for k in cl.TEMPERATURE_CANDIDATES:
        beta = np.float32(1.0 / cal.CANDIDATES[k])
        terms = tt._terms(z, y, beta, mask, dev)
        want = tt.oracle_terms(z, y, float(beta))
        err = np.abs(terms.astype(np.float64) - want)
        ok = (err <= 1e-5 * np.abs(want)) | (err <= 2.0 ** -20)
        print('temperature P={} C={} k={}: largest error / tolerance {:.3f}'.format(
            p, c, k, float((err[keep] / np.maximum(1e-5 * np.abs(want[keep]), 2.0 ** -20)).max())))
        assert ok[keep].all(), (k, float(err[keep].max()))
        assert not terms[~keep].any()
        assert sums[k] == int(np.rint(np.clip(terms[keep].astype(np.float64), 0, 4096) * tt.SCALE).astype(np.int64).sum()), k
    pieces = cal.NllSweep(dev)
    for i in range(n):          # one image: 1,600 tiles, one per workgroup
        pieces.add(torch.from_numpy(np.ascontiguousarray(z[:, i:i + 1]).reshape(p, c, hw, 1)).to(dev), torch.from_numpy(y[i:i + 1]).to(dev),
                   None if mask is None else torch.from_numpy(mask[i:i + 1]).to(dev), passes=p)
    assert pieces.sums() == sums and pieces.voxels == sweep.voxels


@pytest.mark.timeout(300)
def test_temperature_invalid_targets_in_later_trips_are_counted_and_refused(dev):
    import test_gpu_temperature as tt
    from rcu_amd import _lib
    from rcu_amd import calibration as cal
    n, hw = cl.TEMPERATURE_SHAPE
    per_round = cl.TN_MAX_GROUPS * cl.TN_TILE
    z, y = tt._case(2, 2, n=n, hw=hw, seed=4)
    flat = y.reshape(-1)
    flat[per_round + 5:per_round + 12] = 2                    # second trip
    flat[2 * per_round + 70] = 255                            # third trip
    flat[-3:] = 7                                             # the partial last tile
    bad = 7 + 1 + 3
    out = torch.zeros(3, dtype=torch.int64, device=dev)
    ws = torch.empty(_lib.load().rcu_temperature_nll_workspace_bytes(y.size, 1), dtype=torch.uint8, device=dev)
    zt, yt = torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev)
    _lib.check(_lib.load().rcu_temperature_nll(_lib.ptr(zt), 2, n, hw, 2, _lib.ptr(yt), None, (ctypes.c_float * 1)(1.0), 1, _lib.ptr(out),
                                               _lib.ptr(ws), _lib.current_stream()))
    got = out.cpu().tolist()
    assert got[1] == y.size - bad and got[2] == bad
    valid = y < 2
    want = tt.oracle_terms(z, np.where(valid, y, 0), 1.0)
    assert abs(got[0] / tt.SCALE - want[valid].sum()) <= 1e-5 * want[valid].sum()
    sweep = cal.NllSweep(dev)
    sweep.add(zt.reshape(2 * n, 2, hw, 1), yt, passes=2)
    with pytest.raises(ValueError, match='{} voxels'.format(bad)):
        sweep.sums()


# ------------------------------------------------------------------------------------------------------------------- quantile apply
@pytest.mark.timeout(300)
def test_quantile_apply_above_the_cap(dev):
    import test_gpu_quantiles as tq
    from conftest import load_golden
    from rcu_amd import evaluation as ev
    g33 = load_golden('g33_quantiles')
    q = 1000
    source = np.concatenate([g33['ties_maps'].reshape(-1), g33['lognormal_maps'].reshape(-1), g33['special_maps'].reshape(-1)]).astype(np.float32)
    finite = source[~np.isnan(source)]
    n_pop, ranks, keys = qr.table(qr.population_keys([finite]), q)
    table = ev.QuantileTable(q, n_pop, keys, ranks)
    special = np.array([np.nan, np.inf, -np.inf, -np.nan], dtype=np.float32)
    lib = ev._lib
    bounds = (ctypes.c_uint32 * (q - 1))(*[int(k) for k in keys])
    ws = torch.empty(max(lib.load().rcu_quantile_apply_workspace_bytes(q), 8), device=dev, dtype=torch.uint8)

    def planted(n, per_round):
        x = np.resize(source, n).copy()
        x[:3] = special[:3]                                       # the head
        x[2 * per_round + 5:2 * per_round + 9] = special          # the body of the third trip
        x[n - 3:] = special[1:]                                   # the tail
        level = np.where(np.isnan(x), 0, qr.levels(qr.key(x), keys))
        assert level.max() == q - 1 and level.min() == 0
        return x, level, qr.rescaled(level, q)

    def same(got, lv, level, want, tag):
        assert np.array_equal(lv.cpu().numpy().astype(np.int64), level), tag
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), tag

    # the 16-byte form: aligned (head 0, tail 3) ...
    x, level, want = planted(cl.QUANTILE_N16, cl.ROWS['quantile_apply_16'].walkers * 4)
    got, lv = ev.quantile_rescale(table, x, return_levels=True)
    same(got, lv, level, want, 'aligned')
    # ... and input, output and levels one element off their allocations (head 3); n and n + 3 (tail 0 and tail 3)
    for n in (cl.QUANTILE_N16, cl.QUANTILE_N16 + 3):
        x, level, want = planted(n, cl.ROWS['quantile_apply_16'].walkers * 4)
        src = tq.off_by_one(x, dev, torch.float32)
        out, lv = torch.zeros(n + 2, device=dev, dtype=torch.float32), torch.full((n + 2,), -1, device=dev, dtype=torch.int16)
        lib.check(lib.load().rcu_quantile_apply(lib.ptr(src), n, bounds, q, lib.ptr(out[1:]), lib.ptr(lv[1:]), lib.ptr(ws), lib.current_stream()))
        same(out[1:-1], lv[1:-1], level, want, ('head 3', n))
        assert float(out[0]) == 0 and float(out[-1]) == 0 and int(lv[0]) == -1 and int(lv[-1]) == -1      # nothing written around the map
    # the element-by-element form: the input alone is off its allocation
    x, level, want = planted(cl.QUANTILE_N4, cl.ROWS['quantile_apply_4'].walkers)
    got, lv = ev.quantile_rescale(table, tq.off_by_one(x, dev, torch.float32), return_levels=True)
    same(got, lv, level, want, 'scalar')


# ------------------------------------------------------------------------------------------------------------------- head stream
HEAD_MODELS = ((3, False, True), (8, False, True), (2, True, True), (2, False, False))      # (C, sigma twin, fused head allowed)
P_TOL, H_TOL = 1e-6, 2e-6      # test_gpu_step_seam.py: per pass, the bounds of the maps; one pass here
HEAD_FLAGS = (ref.MI, ref.EXACT | ref.MI | ref.VAR)


class _Run:
    pass


_HEAD_RUNS = {}


@pytest.fixture(scope='module', autouse=True)
def _release_head_runs():
    yield
    _HEAD_RUNS.clear()      # the plans and their workspaces go with the module


@pytest.fixture(scope='module', params=HEAD_MODELS, ids=lambda p: 'C{}-{}{}'.format(p[0], 'sigma' if p[1] else 'plain', '' if p[2] else '-unfused'))
def head(request, dev):
    return _head_run(request.param, dev)


@pytest.fixture(scope='module')
def sigma_head(dev):
    return _head_run(HEAD_MODELS[2], dev)


def _head_run(param, dev):
    """One model on the plan of five 508 x 516 slices: the whole batch, materialised, the masks of the batch and of its five one-slice calls, and
    the float64 oracle of the whole batch (once per model)."""
    if param in _HEAD_RUNS:
        return _HEAD_RUNS[param]
    from oracle import unet_oracle as uo
    from rcu_amd.model import UNet
    C, sigma, fused = param
    params = dict(nb_classes=C, dropout=0.2, sigma_out=sigma, **cl.HEAD_MODEL)
    state = uo.synthetic_state(1000 + 100 * C + 32, **params)
    m = UNet(**params)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    m = m.to(dev)
    n, h, w = cl.HEAD_SHAPE
    m.reserve(h, w, n)                                            # one plan for the batch and its slices
    rows = m.layer_table(h, w, n)
    if not fused:
        assert rows[-1]['head_fusable'], rows[-1]
        m.set_fuse_head(False)
    else:
        assert not rows[-1]['head_fusable'], rows[-1]             # the standalone head runs
    assert (rows[-1]['cout'] // (2 if sigma else 1) + 31) // 32 * 32 == 32      # 32 head channels: the streaming form
    r = _Run()
    r.C, r.sigma, r.m, r.n, r.h, r.w = C, sigma, m, n, h, w
    g = torch.Generator().manual_seed(C)
    r.x_cpu = torch.randn(n, 2, h, w, generator=g)
    r.x = r.x_cpu.to(dev)
    _, sites = uo.unet_plan(**params)
    r.masks = uo.sample_masks(sites, n, 0.2, g)
    r.slice_masks = [[ms[i:i + 1] for ms in r.masks] for i in range(n)]
    out = m(r.x, r.masks)
    r.logits, r.raw = (out if sigma else (out, None))
    want = uo.unet_forward(state, r.x_cpu, r.masks, dtype=torch.float64, **params)
    r.oracle_logits = (want[0] if sigma else want).numpy()
    r.oracle_raw = want[1].numpy() if sigma else None
    _HEAD_RUNS[param] = r
    return r


def _statistics(r, n, flags, dev):
    import test_gpu_step_seam as ts
    return ts._statistics(r.C, n, r.h, r.w, flags, dev)


@pytest.mark.timeout(600)
def test_head_stream_logits_above_the_cap(head, dev):
    import test_gpu_step_seam as ts
    r = head
    ts._within('logits', r.C, r.logits.cpu().numpy(), r.oracle_logits, ts.LOGIT_TOL, ('above the cap', r.sigma))
    if r.sigma:
        ts._within('raw sigma', r.C, r.raw.cpu().numpy(), r.oracle_raw, ts.LOGIT_TOL, ('above the cap',))
    for i in range(r.n):
        out = r.m(r.x[i:i + 1], r.slice_masks[i])
        lg, raw = out if r.sigma else (out, None)
        assert torch.equal(lg, r.logits[i:i + 1]), i
        assert raw is None or torch.equal(raw, r.raw[i:i + 1]), i


@pytest.mark.timeout(600)
def test_head_stream_statistics_above_the_cap(head, dev):
    import test_gpu_step_seam as ts
    r = head
    softmax = ref.softmax(r.oracle_logits)[None]
    for flags in HEAD_FLAGS:
        st = _statistics(r, r.n, flags, dev)
        r.m.forward_accumulate(r.x, st, r.masks)
        mat = _statistics(r, r.n, flags, dev)
        mat.accumulate(r.logits)
        assert torch.equal(st.blob, mat.blob), flags                  # the bits of the materialised logits
        planes, want = ts._planes(st), ref.statistics_planes(softmax, flags)
        assert planes.shape == want.shape
        ts._within('sum p', r.C, planes[:r.C], want[:r.C], P_TOL, ('above the cap', flags))
        if flags & ref.VAR:
            ts._within('sum p^2', r.C, planes[r.C:2 * r.C], want[r.C:2 * r.C], P_TOL, ('above the cap', flags))
        ts._within('sum H', r.C, planes[-1], want[-1], H_TOL, ('above the cap', flags))
        whole = st.blob.view(-1, r.n, r.h, r.w)
        for i in range(r.n):
            one = _statistics(r, 1, flags, dev)
            r.m.forward_accumulate(r.x[i:i + 1], one, r.slice_masks[i])
            assert torch.equal(one.blob.view(-1, r.h, r.w), whole[:, i]), (flags, i)


@pytest.mark.timeout(600)
@pytest.mark.parametrize('is_log_sigma', [False, True])
def test_head_stream_sigma_sum_above_the_cap(sigma_head, dev, is_log_sigma):
    import test_gpu_step_seam as ts
    r = sigma_head
    want = ref.sigma_of(r.oracle_raw, is_log_sigma)
    scale = max(1.0, float(want.max()))
    flags = ref.EXACT | ref.MI | ref.VAR
    st = _statistics(r, r.n, flags, dev)
    sigma_sum = torch.zeros(r.n, r.C, r.h, r.w, device=dev)
    r.m.forward_accumulate_sigma(r.x, st, sigma_sum, r.masks, is_log_sigma)
    mat = _statistics(r, r.n, flags, dev)
    mat.accumulate(r.logits)
    assert torch.equal(st.blob, mat.blob)
    ts._within('sigma sum / max(1, max sigma)', r.C, sigma_sum.cpu().numpy() / scale, want / scale, ts.SIGMA_TOL, ('above the cap', is_log_sigma))
    whole = st.blob.view(-1, r.n, r.h, r.w)
    for i in range(r.n):
        one = _statistics(r, 1, flags, dev)
        one_sum = torch.zeros(1, r.C, r.h, r.w, device=dev)
        r.m.forward_accumulate_sigma(r.x[i:i + 1], one, one_sum, r.slice_masks[i], is_log_sigma)
        assert torch.equal(one_sum, sigma_sum[i:i + 1]) and torch.equal(one.blob.view(-1, r.h, r.w), whole[:, i]), i


@pytest.mark.timeout(600)
def test_head_stream_sampling_above_the_cap(sigma_head, dev):
    """head_stream_sample_kernel: one pass, S = 3 -- the bits of rcu_logit_sampling on the materialised logits and sigma, and of the one-slice
    calls under the slices' global indices."""
    from rcu_amd import steps
    r = sigma_head
    S, first_sample, key = 3, 2 ** 32 + 5, steps.pass_seed(20, 1)
    flags = ref.EXACT | ref.MI
    for is_log_sigma in (False, True):
        fused = _statistics(r, r.n, flags, dev)
        fused_sigma = torch.zeros(r.n, r.C, r.h, r.w, device=dev)
        r.m.forward_sample_sigma(r.x, fused, fused_sigma, [key], first_sample, S, masks=r.masks, is_log_sigma=is_log_sigma)
        mat = _statistics(r, r.n, flags, dev)
        mat.accumulate(steps.sample_logits(r.logits, r.raw, S, key, first_sample, is_log_sigma), is_probabilities=True)
        assert torch.equal(fused.blob, mat.blob), is_log_sigma
        plain = _statistics(r, r.n, flags, dev)
        plain.accumulate(r.logits)
        assert not torch.equal(fused.blob, plain.blob)                # the sampling did change the statistics
        whole = fused.blob.view(-1, r.n, r.h, r.w)
        for i in range(r.n):
            one = _statistics(r, 1, flags, dev)
            one_sigma = torch.zeros(1, r.C, r.h, r.w, device=dev)
            r.m.forward_sample_sigma(r.x[i:i + 1], one, one_sigma, [key], first_sample + i, S, masks=r.slice_masks[i], is_log_sigma=is_log_sigma)
            assert torch.equal(one.blob.view(-1, r.h, r.w), whole[:, i]) and torch.equal(one_sigma, fused_sigma[i:i + 1]), (is_log_sigma, i)
