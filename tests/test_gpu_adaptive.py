"""Adaptive MC dropout on the device (csrc/rcu_adaptive.hip, steps.McPredictStep(adaptive=...), the ``others.mc_adaptive`` key): the four
kernels against the integer / float64 numpy restatement of tests/adaptive_reference.py and against the existing entry points, bit for bit; the
step against sums of existing-code pieces; the default BraTS script on the tiny synthetic dataset of tests/test_gpu_scripts.py.
Everything here is an equality of integers or of bits: there are no tolerances."""
import csv
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import adaptive_reference as ar

pytestmark = pytest.mark.gpu

N = 5
SHAPES = {'one_voxel': (9, 31), 'four_wide': (6, 52)}       # hw = 279 (odd: the one-value paths) and 312 = 4 * 78 (the 16-byte paths)
FLAG_SETS = (ar.EXACT, ar.EXACT | ar.MI, ar.EXACT | ar.MI | ar.VAR)
CLASSES = (2, 3, 8)
Q = 2.0 ** -40


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same_bits(a, b):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _off_by_one(t):
    """A copy of ``t`` one element behind the start of its allocation: contiguous, and not 16-byte aligned."""
    base = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = base[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0 and t.data_ptr() % 16 == 0
    return view


def _statistics(C, n, h, w, flags, dev, planes=None, misaligned=False):
    """McStatistics of the flag set, holding ``planes`` ([P, n, hw] float64) when given -- in a blob one element off its allocation if asked."""
    from rcu_amd import steps
    kw = dict(do_mi=bool(flags & ar.MI), do_var=bool(flags & ar.VAR), exact=bool(flags & ar.EXACT))
    if planes is None:
        return steps.McStatistics(n, C, h, w, dev, **kw)
    data = torch.from_numpy(np.ascontiguousarray(planes).reshape(-1)).to(dev)
    st = steps.McStatistics(n, C, h, w, dev, blob=_off_by_one(data) if misaligned else torch.empty_like(data), **kw)      # (rcu_mc_begin zeroes it)
    st.blob.copy_(data)
    return st


def _planes(st):
    return st.blob.cpu().numpy().reshape(-1, st.n, st.hw)


def _quantum_planes(seed, C, n, hw, flags, passes):
    """[P, n, hw] float64 multiples of 2^-40: the class sums of a voxel add up to ``passes``, the leading one (a random class) is 0.9 .. 1 of
    it -- about a tenth of the voxels is settled at tolerance 0.01 --, the other planes are arbitrary."""
    rng = np.random.RandomState(seed)
    total = passes << 40
    lead = np.rint(rng.uniform(0.9, 1.0, size=(n, hw)) * total).astype(np.int64)
    k = np.floor(rng.dirichlet(np.ones(C), size=(n, hw)) * (total - lead)[..., None]).astype(np.int64)      # [n, hw, C] quanta of the rest
    which = rng.randint(C, size=(n, hw))
    k[np.arange(n)[:, None], np.arange(hw)[None, :], which] = 0
    k[np.arange(n)[:, None], np.arange(hw)[None, :], which] = total - k.sum(axis=-1)
    assert np.all(k.sum(axis=-1) == total) and np.all(k >= 0)
    sums = [np.moveaxis(k, -1, 0).astype(np.float64) * Q]
    for _ in range(ar.plane_count(C, flags) - C):
        sums.append(rng.randint(0, passes << 20, size=(1, n, hw)).astype(np.float64) * Q)
    return np.concatenate(sums)


# ---------------------------------------------------------------------------------- rcu_mc_slice_scores
@pytest.mark.parametrize('flags', FLAG_SETS)
@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('C', CLASSES)
def test_slice_scores_are_the_integers_of_the_restatement(dev, C, shape, flags):
    from rcu_amd import steps
    h, w = SHAPES[shape]
    hw, t = h * w, 5
    thr = ar.thr_q(0.01, t)
    planes = _quantum_planes(11 * C + flags, C, N, hw, flags, t)
    # planted: a voxel exactly on thr_q (settled) and one 2^-40 below it (unsettled), at the first and the last voxel of the first and last slice
    for (s, v), q in {(0, 0): thr, (0, hw - 1): thr - 1, (N - 1, 0): thr - 1, (N - 1, hw - 1): thr}.items():
        planes[:C, s, v] = 0.0
        planes[C - 1, s, v] = q * Q
        planes[0, s, v] = (t * (1 << 40) - q) * Q
    want_unsettled, want_margin = ar.slice_scores(planes, C, thr)
    lead = ar.leading_q(planes, C)
    assert lead[0, 0] == thr and lead[0, hw - 1] == thr - 1 and lead[N - 1, 0] == thr - 1 and lead[N - 1, hw - 1] == thr
    assert 0 < want_unsettled.min() and want_unsettled.max() < hw            # the counts are informative
    for misaligned in (False, True):                                          # the 16-byte loads (hw even) and the one-value loads: the same integers
        st = _statistics(C, N, h, w, flags, dev, planes, misaligned)
        unsettled, margin = steps.split_scores(steps.slice_scores(st, thr))
        print('C={} {} flags={} misaligned={}: unsettled {} margin_q {}'.format(C, shape, flags, misaligned, unsettled, margin))
        assert unsettled == want_unsettled.tolist() and margin == want_margin.tolist()
        # one quantum up: the planted voxels on the threshold become unsettled too
        up, _ = steps.split_scores(steps.slice_scores(st, thr + 1))
        assert up == ar.slice_scores(planes, C, thr + 1)[0].tolist() and up[0] == want_unsettled[0] + 1 and up[-1] == want_unsettled[-1] + 1
    # everything settled: a count of zero and the margin of the restatement
    zero, margin = steps.split_scores(steps.slice_scores(st, 0))
    assert zero == [0] * N and margin == want_margin.tolist()
    with pytest.raises(ValueError, match='exact'):
        steps.slice_scores(_statistics(C, N, h, w, flags & ~ar.EXACT | ar.VAR, dev), thr)


# ---------------------------------------------------------------------------------- rcu_dropout_masks_indexed
def _draw(dev, seeds, n, channels, keeps, first_sample=None, index=None):
    from rcu_amd import _lib
    g, count = len(seeds), len(channels)
    out = torch.full((g * n * sum(channels),), -7.0, device=dev)
    args = ((ctypes.c_int32 * count)(*channels), (ctypes.c_float * count)(*keeps), count, _lib.ptr(out), _lib.current_stream())
    arr = (ctypes.c_uint64 * g)(*seeds)
    if index is None:
        _lib.check(_lib.load().rcu_dropout_masks(arr, g, n, first_sample, *args))
    else:
        _lib.check(_lib.load().rcu_dropout_masks_indexed(arr, g, n, _lib.ptr(index), *args))
    rows = torch.split(out, [g * n * c for c in channels])
    return [r.view(g, n, c).cpu().numpy() for r, c in zip(rows, channels)]      # per site [pass, sample, channel]


@pytest.mark.parametrize('keeps', [(0.8, 0.5, 0.9), (0.8, -1.0, -1.0), (-1.0, 0.5, -1.0), (-1.0, -1.0, 0.9)],
                         ids=['all-active', 'site0', 'site1', 'site2'])
def test_indexed_masks_are_the_rows_of_the_contiguous_draw(dev, keeps):
    channels, seeds = (8, 16, 5), (20, (1 << 63) + 12345, 7)
    high = (1 << 32) + 1
    index = [high + 4, 3, high, 9, 4]                        # out of order, with gaps, the first above 2^32
    got = _draw(dev, seeds, len(index), channels, keeps, index=torch.tensor(index, device=dev, dtype=torch.int64))
    low_rows = _draw(dev, seeds, 7, channels, keeps, first_sample=3)          # samples 3 .. 9
    high_rows = _draw(dev, seeds, 5, channels, keeps, first_sample=high)      # samples 2^32 + 1 .. 2^32 + 5
    for s, c in enumerate(channels):
        want = np.stack([high_rows[s][:, g - high] if g >= high else low_rows[s][:, g - 3] for g in index], axis=1)
        assert _same_bits(got[s], want), (s, keeps)
        if keeps[s] < 0:
            assert np.all(got[s] == 1.0)
        else:
            assert set(np.unique(got[s])) == {np.float32(0.0), np.float32(1.0) / np.float32(keeps[s])}
    assert not _same_bits(low_rows[0][:, 0], low_rows[0][:, 1]) or keeps[0] < 0      # neighbouring samples differ


def test_model_seeded_masks_take_a_sample_index(dev):
    from rcu_amd import steps
    from rcu_amd.model import UNet
    m = UNet(nb_classes=2, in_channels=2, depth=2, start_filters=32, dropout=0.2).to(dev)
    steps.set_dropout_mode(m, True)
    full = m.seeded_masks(6, dev, [5, 6], first_sample=7)
    index = torch.tensor([12, 8, 9], device=dev, dtype=torch.int64)
    part = m.seeded_masks(3, dev, [5, 6], sample_index=index)
    sites = m.dropout_sites()
    for f, p, (_, c) in zip(torch.split(full, [2 * 6 * c for _, c in sites]), torch.split(part, [2 * 3 * c for _, c in sites]), sites):
        assert _same_bits(p.view(2, 3, c), f.view(2, 6, c)[:, [5, 1, 2]])
    with pytest.raises(ValueError, match='sample_index'):
        m.seeded_masks(3, dev, [5], sample_index=index.to(torch.int32))


# ---------------------------------------------------------------------------------- rcu_mc_merge_slices
@pytest.mark.parametrize('flags', FLAG_SETS)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_merge_adds_the_compact_rows_and_leaves_the_rest(dev, shape, flags):
    from rcu_amd import steps
    h, w = SHAPES[shape]
    C = 3
    dst_planes = _quantum_planes(5 + flags, C, N, h * w, flags, 4)
    src_planes = _quantum_planes(6 + flags, C, 3, h * w, flags, 2)
    index = [4, -1, 1]
    want = ar.merge_slices(dst_planes.copy(), src_planes, index)
    for misaligned in (False, True):
        dst = _statistics(C, N, h, w, flags, dev, dst_planes, misaligned)
        src = _statistics(C, 3, h, w, flags, dev, src_planes, misaligned)
        steps.merge_slices(src, dst, torch.tensor(index, device=dev, dtype=torch.int32))
        got = _planes(dst)
        assert _same_bits(got, want), (shape, flags, misaligned)
        assert _same_bits(got[:, [0, 2, 3]], dst_planes[:, [0, 2, 3]])           # untouched slices keep every bit
        assert _same_bits(_planes(src), src_planes)
    with pytest.raises(ValueError):
        steps.merge_slices(src, dst, torch.tensor(index, device=dev, dtype=torch.int64))


# ---------------------------------------------------------------------------------- rcu_mc_finalize_counts
def _finalize(st, count, outs, counts=None):
    """rcu_mc_finalize (``count``) or rcu_mc_finalize_counts (``counts``) into the given tensors (None = NULL)."""
    from rcu_amd import _lib
    lib, ptrs = _lib.load(), [_lib.ptr(o) for o in outs]
    if counts is None:
        _lib.check(lib.rcu_mc_finalize(_lib.ptr(st.blob), st.n, st.hw, st.nb_classes, int(count), st.flags, *ptrs, _lib.current_stream()))
    else:
        _lib.check(lib.rcu_mc_finalize_counts(_lib.ptr(st.blob), st.n, st.hw, st.nb_classes, _lib.ptr(counts), st.flags, *ptrs, _lib.current_stream()))


def _maps(st, dev, wanted=(True, True, True, True)):
    shapes = [(st.n, st.nb_classes, st.height, st.width)] + 3 * [(st.n, 1, st.height, st.width)]
    have = (True, True, st.do_mi, st.do_var)
    return [torch.full(s, -3.0, device=dev) if (ok and w) else None for s, ok, w in zip(shapes, have, wanted)]


def _accumulated(C, n, h, w, flags, dev, passes=4):
    st = _statistics(C, n, h, w, flags, dev)
    g = torch.Generator().manual_seed(100 * C + flags)
    for _ in range(passes):
        st.accumulate((torch.randn(n, C, h, w, generator=g) * 3).to(dev))
    return st


@pytest.mark.parametrize('flags', FLAG_SETS)
@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('C', CLASSES)
def test_finalize_with_counts_writes_the_bits_of_finalize(dev, C, shape, flags):
    h, w = SHAPES[shape]
    st = _accumulated(C, N, h, w, flags, dev)
    # constant counts: all outputs and every subset of NULL outputs
    same = torch.full((N,), 4, device=dev, dtype=torch.int32)
    for wanted in itertools.product((True, False), repeat=4):
        a, b = _maps(st, dev, wanted), _maps(st, dev, wanted)
        _finalize(st, 4, a)
        _finalize(st, None, b, counts=same)
        for x, y in zip(a, b):
            assert (x is None) == (y is None) and (x is None or _same_bits(x, y)), (C, shape, flags, wanted)
    # mixed counts: slice i = rcu_mc_finalize on that slice's planes copied out as a one-slice blob
    counts = [2, 3, 4, 2, 5]
    got = _maps(st, dev)
    _finalize(st, None, got, counts=torch.tensor(counts, device=dev, dtype=torch.int32))
    planes = _planes(st)
    for i, t in enumerate(counts):
        one = _statistics(C, 1, h, w, flags, dev, planes[:, i:i + 1])
        want = _maps(one, dev)
        _finalize(one, t, want)
        for x, y in zip(got, want):
            assert x is None or _same_bits(x[i:i + 1], y), (C, shape, flags, i)
    # and the float64 restatement agrees to float32 rounding (a check of the test's own reading of the layout)
    ref = ar.finalise_counts(planes, C, counts, flags)
    assert np.max(np.abs(got[0].cpu().numpy().reshape(N, C, -1) - ref['probabilities'])) < 1e-6


# ---------------------------------------------------------------------------------- the step
T, CHECK_AT, FIRST_SAMPLE, SEED = 6, [2, 4], 7, 20
SLICES, H, W = 6, 12, 20
STEP_PARAMS = dict(nb_classes=2, in_channels=2, depth=2, start_filters=64, dropout=0.2)


class _StepRun:
    pass


def _run_step(r, dev, summary=None, **kw):
    """One McPredictStep (+ MultiPredictionSummary) over the run's images at first sample 7 -> (statistics, output dict)."""
    from rcu_amd import steps
    kw.setdefault('seed', SEED)
    step = steps.McPredictStep(kw.pop('mc_steps', T), **kw)
    bc = steps.BatchContext({'images': r.x}, 0, sample_offset=FIRST_SAMPLE)
    ctx = steps.TorchTestContext('cuda', model=r.m)
    step(bc, None, ctx)
    stats = bc.output['multi_probabilities']
    if summary is not None:
        summary(bc, None, ctx)
    torch.cuda.synchronize()
    return stats, bc.output


def _margins(stats, t):
    """min over the voxels of a slice of the leading class sum, as integers (the numpy restatement on existing-code statistics)."""
    return ar.slice_scores(_planes(stats), stats.nb_classes, 0)[1]


@pytest.fixture(scope='module')
def run(dev):
    """The small U-Net of the step-seam tests, six slices chosen so that ONE tolerance retires slices 0, 1 at checkpoint 2, slices 2, 3 at 4
    and none of 4, 5.  A synthetic_state net's probabilities sit near 0.5 and a slice's margin is a function of (image, global index) alone:
    candidate images of several contrasts are scored at every position by the plain steps McPredictStep(2) and McPredictStep(4) -- existing
    code -- and the numpy restatement; the tolerance lies between two sorted margins."""
    from oracle import unet_oracle as uo
    from rcu_amd.model import UNet
    r = _StepRun()
    state = uo.synthetic_state(13, **STEP_PARAMS)
    r.m = UNet(**STEP_PARAMS)
    r.m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    r.m = r.m.to(dev)
    for lane in (0, 1):
        r.m.reserve(H, W, SLICES * T, lane)              # one plan for every step below: bit-identity is a property of a plan
    g = torch.Generator().manual_seed(5)
    scales = [0.25 * 1.5 ** (k % 12) for k in range(18)]
    pool = [torch.randn(2, H, W, generator=g) * s for s in scales]
    K = len(pool)
    m2 = np.zeros((K, SLICES), dtype=np.int64)            # margin_q of candidate k at position i after 2 passes, after 4
    m4 = np.zeros((K, SLICES), dtype=np.int64)
    for shift in range(K):
        r.x = torch.stack([pool[(shift + i) % K] for i in range(SLICES)]).to(dev)
        for t, table in ((2, m2), (4, m4)):
            q = _margins(_run_step(r, dev, mc_steps=t, ws_pass=False)[0], t)
            for i in range(SLICES):
                table[(shift + i) % K, i] = q[i]
    # as mean probabilities: r2 = m2 / (2 * 2^40), r4 = m4 / (4 * 2^40); the bar X = 1 - tolerance must satisfy, for the chosen candidates,
    #   positions 0, 1: r2 >= X;   positions 2, 3: r2 < X <= r4;   positions 4, 5: r2 < X and r4 < X
    r2, r4 = m2 / (2.0 * 2 ** 40), m4 / (4.0 * 2 ** 40)
    choice = None
    for X in sorted(set(r4[:, 2]) | set(r4[:, 3])):
        picks = []
        for i in range(SLICES):
            if i < 2:
                ok = [k for k in range(K) if r2[k, i] >= X]
            elif i < 4:
                ok = [k for k in range(K) if r2[k, i] < X <= r4[k, i]]
            else:
                ok = [k for k in range(K) if r2[k, i] < X and r4[k, i] < X]
            if not ok:          # (a candidate may serve at two positions: its masks, and so its margins, differ with the global index)
                break
            picks.append(ok[0])
        if len(picks) == SLICES:
            choice = (X, picks)
            break
    print('margins after 2 passes (candidate x position):\n{}\nafter 4 passes:\n{}\nchoice {}'.format(r2, r4, choice))
    assert choice is not None, 'no six candidates give the pattern 2 2 4 4 6 6 under one tolerance'
    X, picks = choice
    r.x = torch.stack([pool[k] for k in picks]).to(dev)
    below = max([r2[k, i] for i, k in enumerate(picks) if i >= 2] + [r4[k, i] for i, k in enumerate(picks) if i >= 4])
    assert below < X
    r.tolerance = 1.0 - (below + X) / 2                    # between two sorted margins
    r.plain = {t: _run_step(r, dev, mc_steps=t) for t in (2, 4, 6)}
    # the restatement's decision on the existing-code statistics: the pattern the step must reproduce
    q2, q4 = _margins(r.plain[2][0], 2), _margins(r.plain[4][0], 4)
    gone2 = q2 >= ar.thr_q(r.tolerance, 2)
    gone4 = ~gone2 & (q4 >= ar.thr_q(r.tolerance, 4))
    assert gone2.tolist() == [True, True] + [False] * 4 and gone4.tolist() == [False, False, True, True, False, False], (q2, q4, r.tolerance)
    r.q2, r.q4 = q2, q4
    return r


def _adaptive(tolerance, **kw):
    return dict(check_at=CHECK_AT, tolerance=tolerance, **kw)


def test_nothing_retires_every_output_is_the_plain_steps(run, dev):
    from rcu_amd import steps
    assert max(run.q2) < 2 << 40 and max(run.q4) < 4 << 40      # no slice is saturated: tolerance 0 retires nothing
    stats, out = _run_step(run, dev, adaptive=_adaptive(0.0), do_mi=True, do_var=True, summary=steps.MultiPredictionSummary(True, True))
    _, want = _run_step(run, dev, do_mi=True, do_var=True, summary=steps.MultiPredictionSummary(True, True))
    assert isinstance(stats, steps.AdaptiveMcStatistics) and out['mc_passes'].view(-1).tolist() == [T] * SLICES
    assert stats.spans == [list(range(SLICES))] * 3 and stats.passes_run == SLICES * T and [c['retired'] for c in stats.checkpoints] == [[], []]
    for key in ('ws_probabilities', 'probabilities', 'entropy', 'mutual_info', 'variance'):
        assert _same_bits(out[key], want[key]), key
    with pytest.raises(ValueError, match='stack'):
        stats.as_tensor()


def test_everything_retires_at_the_first_checkpoint_and_nothing_more_is_launched(run, dev, monkeypatch):
    from rcu_amd import steps
    calls = []
    original = run.m.forward_accumulate
    monkeypatch.setattr(run.m, 'forward_accumulate', lambda *a, **k: (calls.append(k.get('passes', 1)), original(*a, **k))[1])
    stats, out = _run_step(run, dev, adaptive=_adaptive(0.6), summary=steps.MultiPredictionSummary())      # 1 - eps = 0.4 < 1 / C
    adaptive_calls = list(calls)
    del calls[:]
    plain_stats, want = _run_step(run, dev, mc_steps=2, summary=steps.MultiPredictionSummary())
    assert adaptive_calls == calls and sum(calls) == 2
    assert out['mc_passes'].view(-1).tolist() == [2] * SLICES and stats.spans == [list(range(SLICES))] and stats.passes_run == 2 * SLICES
    assert _same_bits(stats.blob, plain_stats.blob)
    for key in ('ws_probabilities', 'probabilities', 'entropy'):
        assert _same_bits(out[key], want[key]), key


def _pieces(run, dev):
    """The statistics of pattern (c) as a sum of existing-code pieces: the plain 2-pass statistics, plus forward_accumulate on the gathered
    images with the gathered rows of the contiguous mask draws of passes 3, 4 (slices 2..5) and 5, 6 (slices 4, 5)."""
    from rcu_amd import steps
    m, sites = run.m, run.m.dropout_sites()
    want = _planes(run.plain[2][0]).copy()
    for jobs, idx in (((3, 4), [2, 3, 4, 5]), ((5, 6), [4, 5])):
        x = run.x[idx].contiguous()
        compact = steps.McStatistics(len(idx), 2, H, W, dev, exact=True)
        for j in jobs:
            steps.set_dropout_mode(m, True)
            full = m.seeded_masks(SLICES, dev, [steps.pass_seed(SEED, j)], FIRST_SAMPLE)
            rows = [f.view(SLICES, c)[idx].cpu().numpy() for f, (_, c) in zip(torch.split(full, [SLICES * c for _, c in sites]), sites)]
            m.forward_accumulate(x, compact, rows)
            steps.set_dropout_mode(m, False)
        want[:, idx] += _planes(compact)
    return want


def test_two_retire_at_2_two_at_4_two_run_to_6(run, dev):
    from rcu_amd import steps
    stats, out = _run_step(run, dev, adaptive=_adaptive(run.tolerance), summary=steps.MultiPredictionSummary())
    assert out['mc_passes'].view(-1).tolist() == [2, 2, 4, 4, 6, 6] and out['mc_passes'].dtype == torch.int32
    assert stats.spans == [[0, 1, 2, 3, 4, 5], [2, 3, 4, 5], [4, 5]] and stats.passes_run == 12 + 8 + 4
    c2, c4 = stats.checkpoints
    assert (c2['t'], c2['retired'], c2['margin_q']) == (2, [0, 1], run.q2.tolist()) and c2['thr_q'] == ar.thr_q(run.tolerance, 2)
    assert (c4['t'], c4['active'], c4['retired'], c4['margin_q']) == (4, [2, 3, 4, 5], [2, 3], run.q4[2:].tolist())
    got = _planes(stats)
    # retired slices: the plain step of their count, statistics and maps
    for t, idx in ((2, [0, 1]), (4, [2, 3]), (6, [4, 5])):
        plain_stats, plain_out = run.plain[t]
        if t < 6:
            assert _same_bits(got[:, idx], _planes(plain_stats)[:, idx]), t
    assert _same_bits(out['ws_probabilities'], run.plain[6][1]['ws_probabilities'])
    # the slices that stayed active: the sum of existing-code pieces ...
    assert _same_bits(got, _pieces(run, dev))
    # ... and the plain 6-pass step on the same reserved plan: a slice's bits do not depend on its place in a launch
    assert _same_bits(got[:, [4, 5]], _planes(run.plain[6][0])[:, [4, 5]])
    for t, idx in ((2, [0, 1]), (4, [2, 3]), (6, [4, 5])):
        want = steps.MultiPredictionSummary()
        bc = steps.BatchContext({'images': run.x}, 0)
        bc.output['multi_probabilities'] = run.plain[t][0]
        want(bc, None, steps.TorchTestContext('cuda', model=run.m))
        for key in ('probabilities', 'entropy'):
            assert _same_bits(out[key][idx], bc.output[key][idx]), (key, t)


@pytest.mark.parametrize('lanes,group_pixels', [(1, None), (2, SLICES * H * W), (1, SLICES * H * W), (2, 1 << 40)],
                         ids=['one-lane', 'two-lanes-pass-per-launch', 'one-lane-pass-per-launch', 'two-lanes-one-launch'])
def test_lanes_and_groups_do_not_move_a_bit(run, dev, lanes, group_pixels):
    base, _ = _run_step(run, dev, adaptive=_adaptive(run.tolerance))
    stats, out = _run_step(run, dev, adaptive=_adaptive(run.tolerance), lanes=lanes, group_pixels=group_pixels)
    assert out['mc_passes'].view(-1).tolist() == [2, 2, 4, 4, 6, 6] and stats.spans == base.spans
    assert _same_bits(stats.blob, base.blob)
    assert [c['margin_q'] for c in stats.checkpoints] == [c['margin_q'] for c in base.checkpoints]


def test_the_recipe_replays_the_recorded_lists(run, dev):
    from rcu_amd import steps
    stats, out = _run_step(run, dev, adaptive=_adaptive(run.tolerance), summary=steps.MultiPredictionSummary(do_mi=True))      # the step tracked no MI
    assert not stats.do_mi and 'mutual_info' in out
    again = stats.recipe(True, False)
    assert again.do_mi and again.counts.tolist() == [2, 2, 4, 4, 6, 6] == stats.counts.tolist() and again.spans == stats.spans
    assert again.checkpoints == stats.checkpoints                              # recorded, not decided again
    assert _same_bits(again.finalize(do_mi=True)['mutual_info'], out['mutual_info'])
    assert _same_bits(again.finalize()['probabilities'], out['probabilities'])
    assert _same_bits(_planes(again)[:2], _planes(stats))                      # the class sums of the replay are those of the run
    with pytest.raises(ValueError, match='stack'):
        stats.recipe(False, False, materialize=True)


def test_max_unsettled_and_injected_masks(run, dev):
    """max_unsettled = hw retires every slice at the first checkpoint whatever the tolerance; injected masks (the draws of the seeded run,
    split into per-pass sets) give the bits of the seeded run."""
    from rcu_amd import steps
    stats, out = _run_step(run, dev, adaptive=_adaptive(0.0, max_unsettled=H * W))
    assert out['mc_passes'].view(-1).tolist() == [2] * SLICES and _same_bits(stats.blob, run.plain[2][0].blob)
    steps.set_dropout_mode(run.m, True)
    sets = [run.m.seeded_masks(SLICES, dev, [steps.pass_seed(SEED, j)], FIRST_SAMPLE) for j in range(1, T + 1)]
    steps.set_dropout_mode(run.m, False)
    seeded, _ = _run_step(run, dev, adaptive=_adaptive(run.tolerance))
    injected, out = _run_step(run, dev, adaptive=_adaptive(run.tolerance), seed=None, masks=sets)
    assert out['mc_passes'].view(-1).tolist() == [2, 2, 4, 4, 6, 6] and _same_bits(injected.blob, seeded.blob)


# ---------------------------------------------------------------------------------- the script
def _adaptive_rows(ctx):
    with open(os.path.join(ctx.test_dir, 'adaptive.csv')) as f:
        return list(csv.DictReader(f))


@pytest.mark.timeout(600)
def test_default_script_with_and_without_the_key(tmp_path, monkeypatch):
    from rcu_amd import scripts
    from test_gpu_scripts import _files, _setup, _with_others
    cfg, vols, _, _ = _setup(tmp_path, mc=6)
    captured, make_row = [], scripts.adaptive_csv_row           # the slice rows ([passes, margin_q at 2, at 4]) every subject's CSV row is made from
    monkeypatch.setattr(scripts, 'adaptive_csv_row', lambda rows, *a: (captured.append(np.array(rows)), make_row(rows, *a))[1])
    plain = scripts.test_default('brats', _with_others(cfg, 'plain'), None)
    # a tolerance below every margin: nothing retires, and the run writes the bytes of the run without the key
    none = scripts.test_default('brats', _with_others(cfg, 'none', mc_adaptive=dict(check_at=[2, 4], tolerance=0.0, max_unsettled=0)), None)
    rows = _adaptive_rows(none)
    assert [r['subject'] for r in rows] == sorted(vols)
    assert all(int(r['retired_at_2']) == 0 and int(r['retired_at_4']) == 0 and int(r['passes_run']) == int(r['passes_plain']) == 6 * int(r['slices'])
               for r in rows)
    assert [int(r['slices']) for r in rows] == [vols[name][0].shape[0] for name in sorted(vols)]
    assert _files(none) == _files(plain) and len(_files(plain)) == 2 * len(vols)
    with open(os.path.join(none.test_dir, 'metrics.csv'), 'rb') as a, open(os.path.join(plain.test_dir, 'metrics.csv'), 'rb') as b:
        assert a.read() == b.read()
    assert not os.path.exists(os.path.join(plain.test_dir, 'adaptive.csv'))
    # a bar between the two middle margins of the slices at checkpoint 2 (the slice rows of the first run): the upper half retires there, the
    # files exist, the table adds up
    r2 = sorted(float(q) / (2.0 * 2 ** 40) for block in captured for q in np.asarray(block).reshape(-1, 3)[:, 1])
    assert len(r2) == sum(int(r['slices']) for r in rows) and r2[5] < r2[6]
    bar = (r2[5] + r2[6]) / 2
    some = scripts.test_default('brats', _with_others(cfg, 'some', mc_adaptive=dict(check_at=[2, 4], tolerance=1.0 - bar)), None)
    rows = _adaptive_rows(some)
    print(rows)
    assert sum(int(r['retired_at_2']) for r in rows) == len(r2) - 6
    for r in rows:
        saved = int(r['retired_at_2']) * (6 - 2) + int(r['retired_at_4']) * (6 - 4)
        assert int(r['slices']) * 6 - saved == int(r['passes_run']) and int(r['passes_plain']) == int(r['slices']) * 6
        if int(r['retired_at_2']) + int(r['retired_at_4']):
            assert float(r['min_margin_retired']) >= bar
        if r['min_margin_active']:
            assert float(r['min_margin_active']) < bar
    assert set(_files(some)) == set(_files(plain))
