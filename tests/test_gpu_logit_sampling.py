"""Test-time logit sampling of sigma-head models on the GPU (include/rcu.h "Test-time logit sampling"): the noise against a numpy restatement
of its definition, the sampled predictive against a float64 oracle, batch independence, the fused head against the materialised path, the MC
step's pass groups and lanes, the entropy split, and the aleatoric script."""
import os

import numpy as np
import pytest
import torch

from oracle import mask_oracle as mo

pytestmark = pytest.mark.gpu
PARAMS = dict(nb_classes=2, in_channels=4, depth=3, start_filters=32, dropout=0.05, sigma_out=True)


@pytest.fixture(scope='module')
def lib():
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    return _lib


def _ptr(t):
    from rcu_amd import _lib
    return _lib.ptr(t)


def _stream():
    from rcu_amd import _lib
    return _lib.current_stream()


def normals_np(key, first_sample, n, hw, C, S):
    """z[i, p, s, c] of the definition (float64 transcendentals of the float32 uniforms)."""
    J = S * C
    Q = (J + 3) // 4
    g = np.uint64(first_sample) + np.arange(n, dtype=np.uint64)
    cnt = np.empty((n, hw, Q, 4), dtype=np.uint32)
    cnt[..., 0] = np.arange(hw, dtype=np.uint32)[None, :, None]
    cnt[..., 1] = (g & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None, None]
    cnt[..., 2] = (g >> np.uint64(32)).astype(np.uint32)[:, None, None]
    cnt[..., 3] = (np.uint32(0x80000000) | np.arange(Q, dtype=np.uint32))[None, None, :]
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    w = mo.philox4x32_10(cnt, (key & 0xFFFFFFFF, key >> 32))
    u = ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    u = u.astype(np.float64)
    z = np.empty(u.shape, dtype=np.float64)
    for k in range(2):
        r = np.sqrt(-2.0 * np.log(u[..., 2 * k]))
        z[..., 2 * k] = r * np.cos(2.0 * np.pi * u[..., 2 * k + 1])
        z[..., 2 * k + 1] = r * np.sin(2.0 * np.pi * u[..., 2 * k + 1])
    return z.reshape(n, hw, Q * 4)[..., :J].reshape(n, hw, S, C)


def sample_np(mu, raw, S, key, first_sample, is_log_sigma=False):
    """Float64 oracle of p_bar for [n][C][hw] logits and raw sigma -> [n][C][hw]."""
    mu = np.asarray(mu, dtype=np.float64)
    n, C, hw = mu.shape
    raw = np.asarray(raw, dtype=np.float64)
    sig = np.exp(raw) if is_log_sigma else np.abs(raw)
    z = normals_np(key, first_sample, n, hw, C, S)
    x = mu.transpose(0, 2, 1)[:, :, None, :] + sig.transpose(0, 2, 1)[:, :, None, :] * z
    x = x - x.max(-1, keepdims=True)
    e = np.exp(x)
    p = (e / e.sum(-1, keepdims=True)).mean(2)
    return p.transpose(0, 2, 1)


def _entropy(p, axis):
    return -np.sum(np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0), axis=axis)


def _normals(lib, key, first, n, hw, C, S):
    out = torch.empty(n * hw * S * C, device='cuda', dtype=torch.float32)
    lib.check(lib.load().rcu_logit_normals(key, first, n, hw, C, S, _ptr(out), _stream()))
    return out.view(n, hw, S, C).cpu().numpy()


def test_normals_follow_the_definition(lib):
    key = 0xF00DFACE12345678
    for n, hw, C, S, first in ((2, 70001, 2, 1, 2 ** 32 + 5), (3, 1000, 3, 7, 3), (1, 300, 2, 64, 2 ** 33 + 1), (2, 257, 3, 64, 7)):
        got = _normals(lib, key, first, n, hw, C, S)
        want = normals_np(key, first, n, hw, C, S)
        assert np.all(np.abs(got - want) <= 2e-6 * np.maximum(1.0, np.abs(want))), (n, hw, C, S)
    # a draw of 8 samples is the prefix of a draw of 32, bit for bit
    a = _normals(lib, key, 11, 2, 500, 3, 8)
    b = _normals(lib, key, 11, 2, 500, 3, 32)
    assert np.array_equal(a, b[:, :, :8])
    # the law: 2^22 draws, mean / variance / kurtosis within 5 standard errors of N(0, 1)
    z = _normals(lib, 12345, 0, 4, 1 << 16, 2, 8).astype(np.float64).reshape(-1)
    m = z.size
    assert m >= 1 << 22
    assert abs(z.mean()) < 5 * np.sqrt(1.0 / m)
    assert abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / m)
    assert abs(np.mean(z ** 4) - 3.0) < 5 * np.sqrt(96.0 / m)


def _sampling(lib, mu, raw, S, key, first, is_log_sigma=False, probs=True, stats=None):
    n, C, h, w = mu.shape
    out = torch.empty_like(mu) if probs else None
    lib.check(lib.load().rcu_logit_sampling(_ptr(mu), _ptr(raw), n, h * w, C, int(is_log_sigma), S, key, first, _ptr(out),
                                            None if stats is None else _ptr(stats.blob), 0 if stats is None else stats.flags, _stream()))
    if stats is not None:
        stats.count += 1
    return out


def test_sampled_predictive_against_the_float64_oracle(lib):
    from rcu_amd import steps
    g = torch.Generator().manual_seed(5)
    for C in range(1, 9):
        for S in (1, 10, 64):
            for is_log in (False, True):
                mu = (torch.rand(2, C, 9, 13, generator=g) * 12 - 6)
                raw = torch.rand(2, C, 9, 13, generator=g) * (np.log(8.0) + 3) - 3 if is_log else torch.rand(2, C, 9, 13, generator=g) * 16 - 8
                got = _sampling(lib, mu.cuda(), raw.cuda(), S, 77 + S, 2 ** 32 + 3, is_log).cpu().numpy()
                want = sample_np(mu.numpy().reshape(2, C, -1), raw.numpy().reshape(2, C, -1), S, 77 + S, 2 ** 32 + 3, is_log).reshape(got.shape)
                assert np.max(np.abs(got - want)) <= 2e-5, (C, S, is_log)
                assert np.max(np.abs(got.astype(np.float64).sum(1) - 1.0)) <= 1e-6
                # the steps' wrapper is the same call
                assert torch.equal(steps.sample_logits(mu.cuda(), raw.cuda(), S, 77 + S, 2 ** 32 + 3, is_log).cpu(), torch.from_numpy(got))
    # sigma = 0: softmax(mu)
    mu = torch.rand(3, 3, 8, 8, generator=g) * 12 - 6
    got = _sampling(lib, mu.cuda(), torch.zeros_like(mu).cuda(), 10, 1, 0).cpu()
    assert float((got - torch.softmax(mu.double(), 1)).abs().max()) <= 1e-6


def test_batch_independence(lib):
    from rcu_amd import steps
    g = torch.Generator().manual_seed(6)
    mu = (torch.rand(12, 2, 16, 16, generator=g) * 12 - 6).cuda()
    raw = (torch.rand(12, 2, 16, 16, generator=g) * 8).cuda()
    key, first = 2 ** 40 + 9, 1000

    def stats_of(n):
        return steps.McStatistics(n, 2, 16, 16, 'cuda', do_mi=True, exact=True)

    whole = stats_of(12)
    p_whole = _sampling(lib, mu, raw, 10, key, first, stats=whole)
    parts = [stats_of(5), stats_of(7)]
    p_a = _sampling(lib, mu[:5].contiguous(), raw[:5].contiguous(), 10, key, first, stats=parts[0])
    p_b = _sampling(lib, mu[5:].contiguous(), raw[5:].contiguous(), 10, key, first + 5, stats=parts[1])
    assert torch.equal(p_whole, torch.cat([p_a, p_b]))
    hw = 16 * 16
    blob = whole.blob.view(-1, 12 * hw)          # planes [sum p_c (2)] [sum H]
    assert torch.equal(blob[:, :5 * hw], parts[0].blob.view(-1, 5 * hw))
    assert torch.equal(blob[:, 5 * hw:], parts[1].blob.view(-1, 7 * hw))


def _model(state, dev='cuda'):
    from rcu_amd.model import UNet
    m = UNet(**PARAMS)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    return m.to(dev)


def _oracle_masks(sites, seed, n, first_sample):
    """The masks of the pass keyed ``seed`` (mask_oracle.pass_mask, every site at the model's p) as the oracle forward takes them."""
    flat = mo.pass_mask(seed, n, [c for _, c in sites], [1.0 - PARAMS['dropout']] * len(sites), first_sample=first_sample)
    return [torch.from_numpy(np.ascontiguousarray(m)).view(n, -1) for m in np.split(flat, np.cumsum([n * c for _, c in sites])[:-1])]


@pytest.mark.parametrize('is_log_sigma', [False, True])
def test_fused_head_equals_the_materialised_path(lib, is_log_sigma):
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    st = uo.synthetic_state(31, **PARAMS)
    m = _model(st)
    n, h, w, S = 2, 48, 40, 10
    x = torch.randn(n, 4, h, w, generator=torch.Generator().manual_seed(2)).cuda()
    m.reserve(h, w, 4 * n)
    first = 2 ** 32 + 17
    for passes in (1, 4):
        keys = [steps.pass_seed(20, t) for t in range(1, passes + 1)]
        steps.set_dropout_mode(m, True)
        sets = [m.seeded_masks(n, 'cuda', [k], first) for k in keys]
        steps.set_dropout_mode(m, False)
        group = sets[0] if passes == 1 else m.group_masks(sets, n, 'cuda')
        fused = steps.McStatistics(n, 2, h, w, 'cuda', do_mi=True, exact=True)
        fused_sigma = torch.zeros(n, 2, h, w, device='cuda')
        m.forward_sample_sigma(x, fused, fused_sigma, keys, first, S, masks=group, is_log_sigma=is_log_sigma)
        mat = steps.McStatistics(n, 2, h, w, 'cuda', do_mi=True, exact=True)
        for k, ms in zip(keys, sets):
            logits, raw = m(x, ms)
            _sampling(lib, logits, raw, S, k, first, is_log_sigma, probs=False, stats=mat)
        torch.cuda.synchronize()
        assert torch.equal(fused.blob, mat.blob), passes
        plain = steps.McStatistics(n, 2, h, w, 'cuda', do_mi=True, exact=True)
        plain_sigma = torch.zeros(n, 2, h, w, device='cuda')
        m.forward_accumulate_sigma(x, plain, plain_sigma, group, is_log_sigma, passes=passes)
        assert torch.equal(fused_sigma, plain_sigma), passes
        assert not torch.equal(fused.blob, plain.blob)        # the sampling did change the statistics


def test_mc_step_groups_lanes_oracle_and_entropy_split(lib, monkeypatch):
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    st = uo.synthetic_state(32, **PARAMS)
    m = _model(st)
    n, h, w, T, S = 2, 32, 32, 6, 10
    x = torch.randn(n, 4, h, w, generator=torch.Generator().manual_seed(3))
    ctx = steps.TorchTestContext('cuda', m)
    runs = []
    for group in range(1, T + 1):
        for lanes in (1, 2):
            monkeypatch.setattr(steps.McPredictStep, 'GROUP_PIXELS', group * n * h * w)
            bc = steps.BatchContext({'images': x.clone()}, 0)
            steps.AleatoricMcPredictStep(T, do_mi=True, lanes=lanes, logit_samples=S, seed=20)(bc, None, ctx)
            steps.MultiPredictionSummary(do_mi=True)(bc, None, ctx)
            runs.append({k: v.cpu() for k, v in bc.output.items()})
    for r in runs[1:]:
        for key in ('probabilities', 'entropy', 'mutual_info', 'ws_probabilities'):
            assert torch.equal(r[key], runs[0][key]), key
        assert float(((r['sigma'] - runs[0]['sigma']).abs() / runs[0]['sigma'].abs().clamp_min(1.0)).max()) <= 1e-6
    out = runs[0]
    steps.set_dropout_mode(m, False)
    logits, raw = m(x.cuda())
    ws = steps.sample_logits(logits, raw, S, steps.pass_seed(20, 0), 0)
    assert torch.equal(out['ws_probabilities'], ws.cpu())
    # the oracle: forward under the masks of mask_oracle, sampling in numpy
    pb = []
    for t in range(1, T + 1):
        lg, rw = uo.unet_forward(st, x, _oracle_masks(m.dropout_sites(), steps.pass_seed(20, t), n, 0), **PARAMS)
        pb.append(sample_np(lg.numpy().reshape(n, 2, -1), rw.numpy().reshape(n, 2, -1), S, steps.pass_seed(20, t), 0))
    pb = np.stack(pb)                      # [T, n, C, hw]
    mean = pb.mean(0)
    ent = _entropy(mean, 1)
    aleatoric = _entropy(pb, 2).mean(0)
    assert np.max(np.abs(out['probabilities'].numpy().reshape(n, 2, -1) - mean)) < 1e-4
    assert np.max(np.abs(out['entropy'].numpy().reshape(n, -1) - ent)) < 1e-4
    assert np.max(np.abs(out['mutual_info'].numpy().reshape(n, -1) - (ent - aleatoric))) < 1e-4
    assert np.max(np.abs((out['entropy'] - out['mutual_info']).numpy().reshape(n, -1) - aleatoric)) < 1e-4


def test_zero_samples_keep_the_bytes_of_both_steps(lib):
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    st = uo.synthetic_state(33, **PARAMS)
    m = _model(st)
    x = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(4))
    ctx = steps.TorchTestContext('cuda', m)
    a, b = steps.BatchContext({'images': x.clone()}, 0), steps.BatchContext({'images': x.clone()}, 0)
    steps.AleatoricPredictStep(True)(a, None, ctx)
    steps.AleatoricPredictStep(True, logit_samples=0, seed=9)(b, None, ctx)
    assert set(a.output) == set(b.output)
    for k in a.output:
        assert torch.equal(a.output[k], b.output[k]), k
    logits, raw = m(x.cuda())
    assert torch.equal(b.output['probabilities'], steps.softmax(logits))
    _, sites = uo.unet_plan(**PARAMS)
    g = torch.Generator().manual_seed(8)
    masks = [uo.sample_masks(sites, 2, 0.3, g) for _ in range(4)]
    outs = []
    for kw in ({}, dict(logit_samples=0, seed=3)):
        bc = steps.BatchContext({'images': x.clone()}, 0)
        steps.AleatoricMcPredictStep(4, do_mi=True, masks=masks, **kw)(bc, None, ctx)
        steps.MultiPredictionSummary(do_mi=True)(bc, None, ctx)
        outs.append(bc.output)
    assert set(outs[0]) == set(outs[1])
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_aleatoric_script_samples_logits(tmp_path):
    from test_gpu_scripts import _setup, _with_others, _files
    from oracle import unet_oracle as uo
    from rcu_amd import nifti, scripts, steps
    cfg, vols, states, params = _setup(tmp_path, sigma=True)
    with pytest.raises(ValueError, match='others.logit_samples'):
        scripts.test_default('brats', _with_others(cfg, 'default', logit_samples=10), None)
    from rcu_amd.model import UNet
    sites = UNet(**params).dropout_sites()
    for tag, mc in (('s', None), ('smc', 4)):
        one = scripts.test_aleatoric('brats', _with_others(cfg, tag + '1', logit_samples=10, mc=mc))
        two = scripts.test_aleatoric('brats', _with_others(cfg, tag + '2', logit_samples=10, mc=mc))
        assert _files(one) == _files(two) and len(_files(one)) == 3 * len(vols)
        offset = 0
        for name in sorted(vols):
            images = vols[name][0]
            k = images.shape[0]
            x = torch.from_numpy(images).permute(0, 3, 1, 2).contiguous()
            if mc is None:
                lg, rw = uo.unet_forward(states[0], x, None, **params)
                ref = sample_np(lg.numpy().reshape(k, 2, -1), rw.numpy().reshape(k, 2, -1), 10, steps.pass_seed(20, 0), offset)
            else:
                pb = []
                for t in range(1, mc + 1):
                    lg, rw = uo.unet_forward(states[0], x, _oracle_masks(sites, steps.pass_seed(20, t), k, offset), **params)
                    pb.append(sample_np(lg.numpy().reshape(k, 2, -1), rw.numpy().reshape(k, 2, -1), 10, steps.pass_seed(20, t), offset))
                ref = np.mean(pb, 0)
            got = nifti.read(os.path.join(one.test_dir, name + '_probabilities.nii.gz'))[0]
            assert np.max(np.abs(got.reshape(k, -1) - ref[:, 1])) < 1e-4, (tag, name)
            offset += k
    # others.is_log_sigma: true -- sigma = exp(raw) of the predicted class
    ctx = scripts.test_aleatoric('brats', _with_others(cfg, 'log', is_log_sigma=True))
    for name, (images, _, _) in vols.items():
        x = torch.from_numpy(images).permute(0, 3, 1, 2)
        logits, raw = uo.unet_forward(states[0], x, None, **params)
        ref_sigma = torch.gather(raw.exp(), 1, logits.argmax(1)[:, None])[:, 0].numpy()
        got = nifti.read(os.path.join(ctx.test_dir, name + '_sigma.nii.gz'))[0]
        assert (np.abs(got - ref_sigma) < 1e-4 * np.maximum(1.0, ref_sigma)).mean() > 0.999
