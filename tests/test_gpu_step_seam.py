"""The code between the last conv and the written maps -- the head kernels and the aggregation kernels of csrc/rcu_pointwise.hip with the
per-voxel arithmetic of csrc/rcu_head_common.h -- against the float64 reference of tests/step_seam_reference.py, at every class count 1..8
(standalone entry points) and at C in {1, 2, 3, 4, 8} x {32, 64} filters x {no sigma twin, sigma twin} inside the forward pass.
tests/test_step_seam_reference_cpu.py pins the reference and the planted inputs without a device.  Run on the GPU box:
``python -m pytest tests/test_gpu_step_seam.py -m gpu``; with -s every distance is printed before it is asserted, and a table of the worst
distance per quantity and class count at the end."""
import itertools

import numpy as np
import pytest
import torch

import step_seam_reference as ref

pytestmark = pytest.mark.gpu

# Every bound is one the project already uses:
#   P_TOL / H_TOL / MI_TOL / VAR_TOL   softmax, mean: 1e-6; entropy, mutual information: 2e-6; variance: 1e-7 -- the bounds of
#                                      test_gpu_parity.py::test_mc_summary_golden on fixture G6.  They stand unchanged: on the planted inputs at
#                                      C = 8 the float32 torch oracle is 7.7e-8 / 3.1e-7 / 4.1e-7 / 2.2e-8 from the reference, less than half of
#                                      each bound (5e-7 / 1e-6 / 1e-6 / 5e-8; asserted in test_step_seam_reference_cpu.py)
#   statistics planes                  T x (1e-6 for sum p and sum p^2, 2e-6 for sum H): T addends, each within the bound of its map
#   EXACT_H_TOL                        1e-5, test_exact_statistics_are_sums_of_quantised_addends_in_any_order's bound on the H plane
#   LOGIT_TOL                          2e-6, test_gpu_parity.py's bound on logits (and raw sigma) against the float64 oracle
#   sigma                              2e-6 x max(1, max sigma) per pass: float32 expf of a float32 raw value
# Measured on an MI355X, worst over shapes, sources and flag sets (-s prints them; "-" = not defined):
#   C                                    1        2        3        4        5        6        7        8      bound
#   softmax (also rcu_aleatoric's)      0  7.6e-08  1.2e-07  1.7e-07  2.0e-07  2.0e-07  2.3e-07  2.0e-07     1e-6
#   softmax row sum - 1                 0  7.6e-08  1.3e-07  1.7e-07  2.0e-07  2.0e-07  2.4e-07  2.2e-07     1e-6
#   mean of one pass                    0  7.6e-08  1.2e-07  1.6e-07  1.8e-07  1.8e-07  1.9e-07  2.0e-07     1e-6
#   sum p          (head included)      0  5.6e-07  4.2e-07  5.2e-07  4.5e-07  4.5e-07  4.2e-07  3.8e-07     5e-6
#   sum p^2        (head included)      0  4.8e-07  4.7e-07  5.4e-07  4.9e-07  4.3e-07  5.6e-07  5.3e-07     5e-6
#   sum H          (head included)      0  7.6e-07  1.0e-06  1.4e-06  7.5e-07  1.3e-06  1.5e-06  2.1e-06     1e-5
#   sum H (exact, probabilities)        0  1.7e-07  6.3e-07  3.8e-07  5.0e-07  1.2e-06  1.3e-06  1.2e-06     1e-5
#   probabilities                       0  1.3e-07  9.2e-08  1.2e-07  1.1e-07  8.2e-08  1.1e-07  7.8e-08     1e-6
#   entropy                             0  1.4e-07  2.1e-07  2.7e-07  3.5e-07  3.6e-07  4.3e-07  4.4e-07     2e-6
#   mutual_info                         0  1.6e-07  2.3e-07  2.8e-07  3.1e-07  3.8e-07  4.3e-07  4.2e-07     2e-6
#   variance                            0  3.7e-08  3.3e-08  2.9e-08  2.4e-08  1.8e-08  2.0e-08  1.9e-08     1e-7
#   sigma / max(1, sigma), exp    6.3e-08  7.9e-08  7.3e-08  7.4e-08  7.1e-08  7.4e-08  7.2e-08  7.4e-08     2e-6
#   head: logits                  1.2e-07  1.3e-07  1.2e-07  1.5e-07        -        -        -  1.9e-07     2e-6
#   head: raw sigma               9.5e-08  1.3e-07  1.3e-07  1.9e-07        -        -        -  1.8e-07     2e-6
#   head: sigma sum / max sigma   9.4e-07  1.1e-06  9.0e-07  9.1e-07        -        -        -  1.1e-06     1e-5
# Everything else in the file is an equality of bits or of integers.
P_TOL, H_TOL, MI_TOL, VAR_TOL = 1e-6, 2e-6, 2e-6, 1e-7
EXACT_H_TOL = 1e-5
LOGIT_TOL = 2e-6
SIGMA_TOL = 2e-6
MAP_TOL = {'probabilities': P_TOL, 'entropy': H_TOL, 'mutual_info': MI_TOL, 'variance': VAR_TOL}
T = ref.PASSES
CLASS_COUNTS = tuple(range(1, 9))
WORST = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    yield torch.device('cuda')
    if WORST:
        quantities = sorted({q for q, _ in WORST})
        print('\nworst distance per quantity (rows) and class count (columns 1..8):')
        for q in quantities:
            print('  {:<28}'.format(q) + ' '.join('{:>8}'.format('{:.1e}'.format(WORST[q, C]) if (q, C) in WORST else '-') for C in CLASS_COUNTS))


def _within(quantity, C, got, want, bound, context=()):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (quantity, got.shape, want.shape)
    d = float(np.max(np.abs(got - want))) if got.size else 0.0
    WORST[quantity, C] = max(WORST.get((quantity, C), 0.0), d)
    print('{} C={} {}: {:.3e} (bound {:.1e})'.format(quantity, C, context, d, bound))
    assert d <= bound, (quantity, C, context, d, bound)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same_bits(a, b):
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    if torch.is_tensor(b):
        b = b.cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _off_by_one(t):
    """A copy of ``t`` one element behind the start of its allocation: contiguous, and not 16-byte aligned."""
    base = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = base[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0 and t.data_ptr() % 16 == 0
    return view


# ---------------------------------------------------------------------------------- the shared inputs and their references
_CACHE = {}


def _inputs(C, shape):
    """The seeded inputs of (C, shape) and their float64 references, made once and never written to."""
    key = (C, shape)
    if key not in _CACHE:
        n, h, w = ref.SHAPES[shape]
        logits = ref.grid_logits(7 * C, C, n, h, w)
        probs = ref.grid_probabilities(logits)
        soft = np.stack([ref.softmax(v) for v in logits])
        _CACHE[key] = dict(n=n, h=h, w=w, logits=logits, probs=probs, softmax=soft, raw=ref.raw_sigma(3 * C, C, n, h, w))
    return _CACHE[key]


def _statistics(C, n, h, w, flags, dev, blob=None):
    from rcu_amd import steps
    return steps.McStatistics(n, C, h, w, dev, do_mi=bool(flags & ref.MI), do_var=bool(flags & ref.VAR), exact=bool(flags & ref.EXACT), blob=blob)


def _planes(st):
    return st.blob.cpu().numpy().astype(np.float64).reshape(-1, st.n, st.height, st.width)


def _finalize(st, count, outs):
    """rcu_mc_finalize into the given tensors (None = NULL), in the order mean, entropy, mutual information, variance."""
    from rcu_amd import _lib
    _lib.check(_lib.load().rcu_mc_finalize(_lib.ptr(st.blob), st.n, st.hw, st.nb_classes, int(count), st.flags, *[_lib.ptr(o) for o in outs],
                                           _lib.current_stream()))


def _map_tensors(st, dev, fill=None):
    shapes = [(st.n, st.nb_classes, st.height, st.width)] + 3 * [(st.n, 1, st.height, st.width)]
    wanted = (True, True, st.do_mi, st.do_var)
    return [(torch.empty(s, device=dev) if fill is None else torch.full(s, fill, device=dev)) if ok else None for s, ok in zip(shapes, wanted)]


def _check_planes(C, planes, want, flags, context):
    """Planes within T x the bounds of the maps; ``want`` from ref.statistics_planes with the same flags."""
    _within('sum p', C, planes[:C], want[:C], T * P_TOL, context)
    if flags & ref.VAR:
        _within('sum p^2', C, planes[C:2 * C], want[C:2 * C], T * P_TOL, context)
    if flags & ref.MI:
        _within('sum H', C, planes[-1], want[-1], T * H_TOL, context)


def _check_maps(C, out, want, context):
    for k in want:
        _within(k, C, out[k].cpu().numpy(), want[k], MAP_TOL[k], context)


# ---------------------------------------------------------------------------------- 2. the standalone entry points, C = 1..8
@pytest.mark.parametrize('C', CLASS_COUNTS)
def test_softmax_and_the_mean_of_one_pass(dev, C):
    from rcu_amd import steps
    for shape in ref.SHAPES:
        d = _inputs(C, shape)
        x = torch.from_numpy(d['logits'].reshape(-1, C, d['h'], d['w'])).to(dev)          # the T passes as one batch: every planted row
        got = steps.softmax(x).cpu().numpy()
        _within('softmax', C, got, d['softmax'].reshape(got.shape), P_TOL, shape)
        _within('softmax row sum', C, got.astype(np.float64).sum(1), np.ones((x.shape[0], d['h'], d['w'])), P_TOL, shape)
        for flags in (0, ref.EXACT | ref.MI | ref.VAR):
            st = _statistics(C, d['n'], d['h'], d['w'], flags, dev)
            st.accumulate(torch.from_numpy(d['logits'][0]).to(dev))
            mean = st.finalize()['probabilities'].cpu().numpy()
            _within('mean of one pass', C, mean, d['softmax'][0], P_TOL, (shape, flags))
            _within('softmax row sum', C, mean.astype(np.float64).sum(1), np.ones((d['n'], d['h'], d['w'])), P_TOL, (shape, flags))


@pytest.mark.parametrize('source', ['logits', 'probs'])
@pytest.mark.parametrize('shape', list(ref.SHAPES))
@pytest.mark.parametrize('C', CLASS_COUNTS)
def test_statistics_and_finalised_maps(dev, C, shape, source):
    d = _inputs(C, shape)
    n, h, w = d['n'], d['h'], d['w']
    is_probs = source == 'probs'
    volumes = [torch.from_numpy(v).to(dev) for v in (d['probs'] if is_probs else d['logits'])]
    # what the statistics add: the float32 probabilities as they are, or the softmax of the logits
    addends = d['probs'] if is_probs else d['softmax']
    orders = (list(range(T)), list(reversed(range(T))), [int(t) for t in np.random.RandomState(C).permutation(T)])
    for flags in ref.FLAG_SETS:
        want = ref.statistics_planes(addends, flags)
        st = _statistics(C, n, h, w, flags, dev)
        for v in volumes:
            st.accumulate(v, is_probabilities=is_probs)
        assert st.blob.dtype == (torch.float64 if flags & (ref.VAR | ref.EXACT) else torch.float32)
        planes = _planes(st)
        assert planes.shape == want.shape
        _check_planes(C, planes, want, flags, (shape, source, flags))
        if flags & ref.EXACT:
            scaled = planes * 2.0 ** 40
            assert np.array_equal(scaled, np.round(scaled)), 'every exact plane is a multiple of 2^-40'
            for order in orders[1:]:
                other = _statistics(C, n, h, w, flags, dev)
                for t in order:
                    other.accumulate(volumes[t], is_probabilities=is_probs)
                assert torch.equal(st.blob, other.blob), (flags, order)
            if is_probs:      # the sums of the quantised float32 addends, bit for bit; the H plane has the device's logf in it
                k = C * (2 if flags & ref.VAR else 1)
                assert np.array_equal(planes[:k], want[:k]), (flags, 'sum p / sum p^2')
                if flags & ref.MI:
                    _within('sum H (exact, probs)', C, planes[-1], want[-1], EXACT_H_TOL, (shape, flags))
        out = st.finalize(do_mi=bool(flags & ref.MI), do_var=bool(flags & ref.VAR))
        _check_maps(C, out, ref.finalise(want, C, T, flags), (shape, source, flags))
        if flags & ref.VAR:
            assert float(out['variance'].min()) >= 0.0


@pytest.mark.parametrize('C', CLASS_COUNTS)
def test_null_outputs_leave_the_other_outputs_alone(dev, C):
    from rcu_amd import _lib
    lib, stream = _lib.load(), _lib.current_stream()
    for shape in ref.SHAPES:
        d = _inputs(C, shape)
        n, h, w = d['n'], d['h'], d['w']
        for flags in (ref.MI, ref.MI | ref.VAR):          # float32 planes (no variance output) and float64 planes
            st = _statistics(C, n, h, w, flags, dev)
            for v in d['logits']:
                st.accumulate(torch.from_numpy(v).to(dev))
            full = _map_tensors(st, dev)
            _finalize(st, T, full)
            for keep in itertools.product((False, True), repeat=4):
                outs = [o if (k and o is not None) else None for o, k in zip(_map_tensors(st, dev, fill=-7.0), keep)]
                _finalize(st, T, outs)
                for o, f in zip(outs, full):
                    assert o is None or _same_bits(o, f), (shape, flags, keep)
        logits = torch.from_numpy(d['logits'][1]).to(dev)
        raw = torch.from_numpy(d['raw']).to(dev)

        def aleatoric(keep, is_log):
            outs = [torch.full_like(logits, -7.0), torch.full_like(logits, -7.0), torch.full((n, h, w), 255, device=dev, dtype=torch.uint8),
                    torch.full((n, h, w), -7.0, device=dev)]
            outs = [o if k else None for o, k in zip(outs, keep)]
            _lib.check(lib.rcu_aleatoric(_lib.ptr(logits), _lib.ptr(raw), n, h * w, C, int(is_log), *[_lib.ptr(o) for o in outs], stream))
            return outs
        for is_log in (False, True):
            full = aleatoric((True,) * 4, is_log)
            for keep in itertools.product((False, True), repeat=4):
                for o, f in zip(aleatoric(keep, is_log), full):
                    assert o is None or _same_bits(o, f), (shape, is_log, keep)
        probs = torch.from_numpy(d['probs'][1]).to(dev)

        def prediction(keep):
            outs = [torch.full((n, h, w), 255, device=dev, dtype=torch.uint8) if keep[0] else None, torch.full((n, h, w), -7.0, device=dev) if keep[1] else None]
            _lib.check(lib.rcu_prediction_and_foreground(_lib.ptr(probs), n, h * w, C, _lib.ptr(outs[0]), _lib.ptr(outs[1]), stream))
            return outs
        full = prediction((True, True))
        for keep in itertools.product((False, True), repeat=2):
            for o, f in zip(prediction(keep), full):
                assert o is None or _same_bits(o, f), (shape, keep)


@pytest.mark.parametrize('C', CLASS_COUNTS)
def test_first_maximum_foreground_and_the_predicted_class_sigma(dev, C):
    from rcu_amd import _lib, steps
    lib, stream = _lib.load(), _lib.current_stream()
    for shape in ref.SHAPES:
        d = _inputs(C, shape)
        n, h, w = T * d['n'], d['h'], d['w']                     # the T passes as one batch: every planted row
        logits64 = d['logits'].reshape(n, C, h, w)
        want_pred = ref.first_argmax(logits64)                    # the grid makes it well-defined: no voxel is excluded
        assert want_pred.max() == C - 1 and want_pred.min() == 0
        probs = torch.from_numpy(d['probs'].reshape(n, C, h, w)).to(dev)
        pred, fg = steps.prediction_and_foreground(probs)
        assert pred.dtype == torch.uint8 and np.array_equal(pred.cpu().numpy(), want_pred), shape
        assert _same_bits(fg, np.ascontiguousarray(d['probs'].reshape(n, C, h, w)[:, 1 if C > 1 else 0])), shape
        logits = torch.from_numpy(logits64).to(dev)
        raw = torch.from_numpy(np.tile(d['raw'], (T, 1, 1, 1))).to(dev)
        for is_log in (False, True):
            p, s = torch.empty_like(logits), torch.empty_like(logits)
            a_pred, a_sp = torch.empty((n, h, w), device=dev, dtype=torch.uint8), torch.empty((n, h, w), device=dev)
            _lib.check(lib.rcu_aleatoric(_lib.ptr(logits), _lib.ptr(raw), n, h * w, C, int(is_log), _lib.ptr(p), _lib.ptr(s), _lib.ptr(a_pred),
                                         _lib.ptr(a_sp), stream))
            assert np.array_equal(a_pred.cpu().numpy(), want_pred), (shape, is_log)
            _within('aleatoric softmax', C, p.cpu().numpy(), d['softmax'].reshape(n, C, h, w), P_TOL, (shape, is_log))
            sig = ref.sigma_of(raw.cpu().numpy(), is_log)
            if is_log:
                _within('sigma / max(1, sigma)', C, s.cpu().numpy() / np.maximum(1.0, sig), sig / np.maximum(1.0, sig), SIGMA_TOL, (shape, is_log))
            else:
                assert _same_bits(s, np.abs(raw.cpu().numpy())) and not np.signbit(s.cpu().numpy()).any()
            # the predicted class' sigma: the bits of sigma_out at that class
            assert _same_bits(a_sp, torch.gather(s, 1, torch.from_numpy(want_pred.astype(np.int64)).to(dev)[:, None])[:, 0]), (shape, is_log)
            w_pred, w_sp = steps.sigma_of_prediction(logits, raw, is_log)
            assert torch.equal(w_pred, a_pred) and _same_bits(w_sp, a_sp)


@pytest.mark.parametrize('C', CLASS_COUNTS)
def test_votes_of_logits_and_of_probabilities(dev, C):
    from rcu_amd import steps
    bits = (0, 31, 32)
    for shape in ref.SHAPES:
        d = _inputs(C, shape)
        want = ref.vote_plane([d['logits'][t] for t in range(len(bits))], bits, 2)
        assert not want.any() if C == 1 else want[0].any() and want[1].any()
        for source, is_probs in (('logits', False), ('probs', True)):
            votes = steps.SampleVotes(d['n'], d['h'], d['w'], 64, dev)
            assert votes.n_words == 2
            for t, b in enumerate(bits):
                votes.cast(torch.from_numpy(d[source][t]).to(dev), b + 1, is_probabilities=is_probs)
            assert np.array_equal(votes.plane.cpu().numpy().view(np.uint32), want), (shape, source)
            # a vote ORs into the plane: the same volume on its bit again changes nothing
            votes.cast(torch.from_numpy(d[source][1]).to(dev), 32, is_probabilities=is_probs)
            assert np.array_equal(votes.plane.cpu().numpy().view(np.uint32), want), (shape, source)


@pytest.mark.parametrize('flags', [ref.MI, ref.EXACT | ref.MI | ref.VAR])
@pytest.mark.parametrize('C', CLASS_COUNTS)
def test_misaligned_views_take_the_one_voxel_kernels_and_carry_the_same_bits(dev, C, flags):
    d = _inputs(C, 'four_wide')
    n, h, w = d['n'], d['h'], d['w']
    volumes = [torch.from_numpy(v).to(dev) for v in d['logits']]
    aligned = _statistics(C, n, h, w, flags, dev)
    assert aligned.blob.data_ptr() % 16 == 0
    for v in volumes:
        assert v.data_ptr() % 16 == 0
        aligned.accumulate(v)
    maps = _map_tensors(aligned, dev)
    _finalize(aligned, T, maps)
    _check_planes(C, _planes(aligned), ref.statistics_planes(d['softmax'], flags), flags, ('aligned', flags))
    # the input view one float off its allocation
    st = _statistics(C, n, h, w, flags, dev)
    for v in volumes:
        st.accumulate(_off_by_one(v))
    assert torch.equal(st.blob, aligned.blob)
    # the statistics one element off theirs (accumulate writes them, finalize reads them)
    st = _statistics(C, n, h, w, flags, dev, blob=_off_by_one(aligned.blob))
    assert st.blob.data_ptr() % 16 != 0
    for v in volumes:
        st.accumulate(v)
    assert torch.equal(st.blob, aligned.blob)
    outs = _map_tensors(st, dev)
    _finalize(st, T, outs)
    for o, m in zip(outs, maps):
        assert o is None or _same_bits(o, m)
    # every output map, one at a time, one float off its allocation
    for k in range(4):
        if maps[k] is None:
            continue
        outs = _map_tensors(aligned, dev)
        outs[k] = _off_by_one(torch.zeros_like(maps[k]))
        _finalize(aligned, T, outs)
        for o, m in zip(outs, maps):
            assert o is None or _same_bits(o, m), k


# ---------------------------------------------------------------------------------- 3. the head forms inside the forward pass
MODELS = [(C, filters, sigma) for C in (1, 3, 4, 8) for filters in (32, 64) for sigma in (False, True)] + [(2, 64, True), (2, 32, True), (2, 64, False)]
HEAD_SHAPES = ((3, 12, 20),      # V = 720 = 11 waves + 16 lanes: the v < V tail of head_load32 and head_reduce
               (2, 9, 14))       # centre pad; HW = 126: the one-voxel statistics kernels behind the head
HEAD_FLAGS = (ref.MI, ref.MI | ref.VAR, ref.EXACT | ref.MI | ref.VAR)
GROUPINGS = ((1, 1, 1, 1, 1), (2, 3), (5,))
# synthetic_state seeds of the models that vote (no sigma twin, C > 1).  The logits of a synthetic_state net span 0.2 .. 0.5 around the classifier's
# biases, and under most seeds every voxel of every pass has one arg-max -- a vote plane of zeros or of ones.  These are the first seeds (searched
# with the float32 oracle on the inputs below) under which 10 % .. 90 % of the voxels vote in every pass at both shapes, and the two largest
# logits of every voxel are more than 4e-6 apart.
VOTING_SEEDS = {(3, 32): 48, (3, 64): 2, (4, 32): 139, (4, 64): 13, (8, 32): 165, (8, 64): 25, (2, 64): 13}


def _model(params, state, dev):
    from rcu_amd.model import UNet
    m = UNet(**params)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    return m.to(dev)


class _HeadRun:
    """One model at one shape: the inputs, the injected masks, the T materialised forwards and the float64 oracle's forwards."""


@pytest.fixture(scope='module', params=MODELS, ids=lambda p: 'C{}-f{}-{}'.format(p[0], p[1], 'sigma' if p[2] else 'plain'))
def head(request, dev):
    from oracle import unet_oracle as uo
    C, filters, sigma = request.param
    params = dict(nb_classes=C, in_channels=2, depth=2, start_filters=filters, dropout=0.2, sigma_out=sigma)
    state = uo.synthetic_state(1000 + 100 * C + filters if sigma or C == 1 else VOTING_SEEDS[C, filters], **params)
    m = _model(params, state, dev)
    _, sites = uo.unet_plan(**params)
    runs = []
    for k, (n, h, w) in enumerate(HEAD_SHAPES):
        r = _HeadRun()
        r.C, r.filters, r.sigma, r.n, r.h, r.w, r.m = C, filters, sigma, n, h, w, m
        m.reserve(h, w, n * T)                                    # one plan for single passes and groups: bit-identity is a property of a plan
        rows = m.layer_table(h, w, n * T)
        cout = rows[-1]['cout'] // (2 if sigma else 1)            # (a unit with a sigma twin reports both halves)
        assert (cout + 31) // 32 * 32 == filters, rows[-1]        # what launch_head chooses its CPH form by: 32, or 0 = a multiple of 32
        if request.param == MODELS[-1]:
            m.set_fuse_head(False)
        else:
            assert not rows[-1]['head_fusable'], rows[-1]          # the standalone head runs
        g = torch.Generator().manual_seed(10 * k + C)
        r.x_cpu = torch.randn(n, 2, h, w, generator=g)
        r.x = r.x_cpu.to(dev)
        r.mask_sets = [uo.sample_masks(sites, n, 0.2, g) for _ in range(T)]
        r.logits, r.raw, r.oracle_logits, r.oracle_raw = [], [], [], []
        for ms in r.mask_sets:
            out = m(r.x, ms)
            want = uo.unet_forward(state, r.x_cpu, ms, dtype=torch.float64, **params)
            r.logits.append(out[0] if sigma else out)
            r.oracle_logits.append((want[0] if sigma else want).numpy())
            if sigma:
                r.raw.append(out[1])
                r.oracle_raw.append(want[1].numpy())
        r.oracle_softmax = np.stack([ref.softmax(v) for v in r.oracle_logits])
        runs.append(r)
    return runs


def _grouped(r, groups, launch):
    """``launch(mask sets of the group, first pass, passes)`` for every group of a grouping of the T passes, in pass order."""
    first = 0
    for count in groups:
        sets = r.mask_sets[first:first + count]
        launch(sets[0] if count == 1 else sets, first, count)
        first += count
    assert first == T


def test_head_logits_and_raw_sigma(head):
    """One forward per pass: head_stream_kernel at 32 filters, head_kernel<., ., 0> at 64."""
    for r in head:
        for t in range(T):
            _within('logits', r.C, r.logits[t].cpu().numpy(), r.oracle_logits[t], LOGIT_TOL, (r.filters, r.sigma, r.h, r.w))
            if r.sigma:
                _within('raw sigma', r.C, r.raw[t].cpu().numpy(), r.oracle_raw[t], LOGIT_TOL, (r.filters, r.sigma, r.h, r.w))


def test_head_statistics_in_every_grouping_carry_the_bits_of_the_materialised_logits(head, dev):
    for r in head:
        for flags in HEAD_FLAGS:
            mat = _statistics(r.C, r.n, r.h, r.w, flags, dev)
            for lg in r.logits:
                mat.accumulate(lg)
            for groups in GROUPINGS:
                st = _statistics(r.C, r.n, r.h, r.w, flags, dev)
                _grouped(r, groups, lambda sets, first, count: r.m.forward_accumulate(r.x, st, sets, passes=count))
                assert st.count == T
                assert torch.equal(st.blob, mat.blob), (flags, groups, r.h, r.w)
            _check_planes(r.C, _planes(mat), ref.statistics_planes(r.oracle_softmax, flags), flags, ('head', r.filters, r.sigma, r.h, flags))


@pytest.mark.parametrize('is_log_sigma', [False, True])
def test_head_sigma_sums_in_every_grouping(head, dev, is_log_sigma):
    for r in head:
        if not r.sigma:
            continue
        want = sum(ref.sigma_of(v, is_log_sigma) for v in r.oracle_raw)
        scale = max(1.0, max(float(ref.sigma_of(v, is_log_sigma).max()) for v in r.oracle_raw))
        for flags in (ref.MI, ref.EXACT | ref.MI | ref.VAR):
            mat = _statistics(r.C, r.n, r.h, r.w, flags, dev)
            for lg in r.logits:
                mat.accumulate(lg)
            sums = []
            for groups in GROUPINGS:
                st = _statistics(r.C, r.n, r.h, r.w, flags, dev)
                sigma_sum = torch.zeros(r.n, r.C, r.h, r.w, device=dev)
                _grouped(r, groups, lambda sets, first, count: r.m.forward_accumulate_sigma(r.x, st, sigma_sum, sets, is_log_sigma, passes=count))
                assert torch.equal(st.blob, mat.blob), (flags, groups, r.h, r.w)
                sums.append(sigma_sum)
            assert torch.equal(sums[0], sums[1]) and torch.equal(sums[0], sums[2]), (flags, r.h, r.w)
            _within('sigma sum / max(1, max sigma)', r.C, sums[0].cpu().numpy() / scale, want / scale, T * SIGMA_TOL, (r.filters, r.h, is_log_sigma))


@pytest.mark.parametrize('is_log_sigma', [False, True])
def test_head_sampling_carries_the_bits_of_sample_logits(head, dev, is_log_sigma):
    """S = 3 in one pass and in a group of three: head_stream_sample_kernel and head_sample_kernel<., 32> at 32 filters, head_sample_kernel<., 0> at 64."""
    from rcu_amd import steps
    S, first_sample = 3, 2 ** 32 + 5
    for r in head:
        if not r.sigma:
            continue
        keys = [steps.pass_seed(20, t + 1) for t in range(4)]
        flags = ref.EXACT | ref.MI
        fused = _statistics(r.C, r.n, r.h, r.w, flags, dev)
        fused_sigma = torch.zeros(r.n, r.C, r.h, r.w, device=dev)
        r.m.forward_sample_sigma(r.x, fused, fused_sigma, keys[:1], first_sample, S, masks=r.mask_sets[0], is_log_sigma=is_log_sigma)
        r.m.forward_sample_sigma(r.x, fused, fused_sigma, keys[1:], first_sample, S, masks=r.mask_sets[1:4], is_log_sigma=is_log_sigma)
        mat = _statistics(r.C, r.n, r.h, r.w, flags, dev)
        plain = _statistics(r.C, r.n, r.h, r.w, flags, dev)
        plain_sigma = torch.zeros_like(fused_sigma)
        for t in range(4):
            mat.accumulate(steps.sample_logits(r.logits[t], r.raw[t], S, keys[t], first_sample, is_log_sigma), is_probabilities=True)
            r.m.forward_accumulate_sigma(r.x, plain, plain_sigma, r.mask_sets[t], is_log_sigma)
        assert fused.count == mat.count == 4
        assert torch.equal(fused.blob, mat.blob), (r.h, r.w)
        assert torch.equal(fused_sigma, plain_sigma), (r.h, r.w)
        if r.C > 1:
            assert not torch.equal(fused.blob, plain.blob)        # the sampling did change the statistics


def test_head_votes(head, dev):
    """Bits {0, 1, 31, 32, 33} in one call: two words, so two launches of head_votes_kernel<., 32> or <., 0>."""
    from rcu_amd import steps
    bits = (0, 1, 31, 32, 33)
    for r in head:
        if r.sigma:
            continue
        if r.C > 1:      # the arg-max of the float32 softmax is the arg-max of the logits where the two largest logits are apart
            top = np.sort(np.stack([lg.cpu().numpy() for lg in r.logits]).astype(np.float64), axis=2)
            assert float((top[:, :, -1] - top[:, :, -2]).min()) > 1e-6
        want = ref.vote_plane([lg.cpu().numpy() for lg in r.logits], bits, 2)
        for b in bits:                                             # every pass votes both ways (VOTING_SEEDS); a single class never votes
            voted = (want[b // 32] >> np.uint32(b % 32)) & np.uint32(1)
            assert (0.05 < voted.mean() < 0.95) if r.C > 1 else not voted.any(), (b, float(voted.mean()))
        standalone = steps.SampleVotes(r.n, r.h, r.w, 64, dev)
        for lg, b in zip(r.logits, bits):
            standalone.cast(lg, b + 1, is_probabilities=False)
        for flags in (ref.MI, ref.EXACT | ref.MI | ref.VAR):
            quiet = _statistics(r.C, r.n, r.h, r.w, flags, dev)
            r.m.forward_accumulate(r.x, quiet, r.mask_sets, passes=T)
            st = _statistics(r.C, r.n, r.h, r.w, flags, dev)
            votes = steps.SampleVotes(r.n, r.h, r.w, 64, dev)
            r.m.forward_accumulate(r.x, st, r.mask_sets, passes=T, votes=votes, bits=list(bits))
            assert torch.equal(votes.plane, standalone.plane), (flags, r.h, r.w)
            assert np.array_equal(votes.plane.cpu().numpy().view(np.uint32), want), (flags, r.h, r.w)
            assert torch.equal(st.blob, quiet.blob), (flags, r.h, r.w)
