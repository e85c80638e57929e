"""The ordering contract of include/rcu.h -- "all device work is enqueued on `stream`" -- as a test protocol and a table of cases.

Protocol (``run_behind_delay``).  A row holds the arguments of one entry point (or of the short sequence its contract describes: begin, accumulate,
finalize).  Its inputs start as POISON (zeros for labels and masks, 0.25 for floats: valid values that give another result), its outputs as a sentinel
byte pattern.  After a device synchronisation the following is enqueued on a side stream created by torch (non-blocking: it does not order with the
null stream): a DELAY, the copy of the real inputs over the poison, a garbage fill of every workspace the call initialises itself, the sentinel fill of
every output again (so that a launch that ran early on another stream is overwritten and seen), the ``*_begin`` call or the zeroing of an accumulator
where the contract asks the caller for it, the entry point with the side stream's handle, and a clone of every output.  Directly after the entry point
returns the host arrays it was given are overwritten with garbage and ``side.query()`` is recorded; only then the stream is synchronised.  The clones
must equal, bit for bit, what the same call gives on the default stream of a synchronised device (``run_plain``): a launch, memset or copy on any other
stream reads poison or is overwritten, a host array read after the return reads garbage.  ``query()`` must have been False for every entry point that
does not wait for the stream itself: every launch was then issued while the delay still ran.

Delay.  ``torch.cuda._sleep`` (a chain of 4096^2 matmuls where it is missing), at least 20 x the host time of the slowest table call on a quiet
device and at most 250 ms; tests/test_gpu_stream_order.py measures and prints both.  On the MI355X the slowest call is a U-Net call on the
240 x 240 plan at 0.19 ms of host time (some 30 launches): 20 x that is 4 ms.  The floor is 100 ms, twice the 50 ms a quiet host would need at the
least: the window also has to cover the protocol's own host work (a dozen small torch launches) on a machine whose CPUs others share, and a window
that closes early fails the query() assertion for no fault of the library.  A row then takes its delay plus a few milliseconds.  A U-Net row creates
its handle inside the window (creation writes the padded levels' zeros); as creation is host work of tens of milliseconds the delay is enqueued once
more behind it.

Host-blocking entry points (``BLOCKS_THE_HOST``): they return with the stream drained, so the caller's host thread stalls for the stream's whole
backlog.  On the MI355X that is rcu_density_moments alone (its flag read-back, as include/rcu.h says).  Every other call returned with the stream
busy, the labelling, compaction, pair-table and distance-transform calls included, and so did the three calls that copy a pageable host table with
hipMemcpyAsync (rcu_unc_counts_from_p, rcu_key_hist, rcu_quantile_apply): the runtime stages such a source before it returns -- the tables arrive
intact although the protocol overwrites them the moment the call is back, with the stream still busy.  Of the Python wrappers, those that return
host arrays wait for their own result (tests/stream_order_wrappers.py).
"""
import ctypes
import time
from ctypes import c_double, c_float, c_int32, c_uint32, c_uint64, c_void_p

import numpy as np
import torch

SENTINEL = 0xA5      # outputs before the call
GARBAGE = 0xC3       # workspaces before the call
SCRIBBLE = 0x5A      # host arrays after the call returned (finite as float32 and float64, in-range nowhere)
FLOAT_POISON = 0.25
DELAY_FACTOR, DELAY_MIN_MS, DELAY_MAX_MS = 20.0, 100.0, 250.0

MI, VAR, INPUT_PROBS, EXACT = 1, 2, 4, 8

# entry point -> why its device work cannot be observed through its arguments
EXEMPT = {}

# entry point -> why it waits for the stream before it returns (no query() assertion; the bytes are still compared)
BLOCKS_THE_HOST = {
    'rcu_density_moments': 'reads the bad-label flag word back from the workspace (hipMemcpyAsync + hipStreamSynchronize) to refuse a label >= K',
}


def lib():
    from rcu_amd import _lib
    return _lib.load()


def chk(status):
    from rcu_amd import _lib
    return _lib.check(status)


def vp(t):
    return None if t is None else c_void_p(t.data_ptr())


def as_bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


class Row:
    """The arguments of one protocol run: live device tensors (poison / sentinel / garbage until the protocol fills them) and the host arrays."""

    def __init__(self, dev):
        self.dev = dev
        self.inputs = []      # (live, real)
        self.outputs = []     # live tensors, sentinel-filled, cloned after the call
        self.zeroed = []      # outputs the CALLER zeroes before the call (accumulators without a *_begin): zeroed in stream order
        self.workspaces = []
        self.hosts = {}       # parameter name -> ctypes array
        self.setup = None     # host work inside the window before anything else (U-Net: create the handle); run once
        self.call = None      # call(stream) -> None or extra tensors to clone (views into library-owned memory)
        self.canon = None     # list of CPU byte tensors -> the same in a canonical form (tables whose slot order is a race)
        self.keep = []
        self.warm = False     # run a second time on the same row (U-Net: the warm handle)
        self._setup_done = False
        self._pristine = {}   # the host arrays' bytes: every run scribbles over them after the call

    def inp(self, real, poison=None):
        real = torch.as_tensor(np.ascontiguousarray(real) if isinstance(real, np.ndarray) else real).contiguous().to(self.dev)
        live = torch.empty_like(real)
        if poison is None:
            poison = torch.full_like(real, FLOAT_POISON) if real.is_floating_point() else torch.zeros_like(real)
        else:
            poison = torch.as_tensor(poison, dtype=real.dtype).to(self.dev).expand_as(real).contiguous()
        self.inputs.append((live, real, poison))
        return live

    def inout(self, real, poison=None):
        live = self.inp(real, poison)
        self.outputs.append(live)
        return live

    def out(self, shape, dtype, zeroed=False):
        t = torch.empty(shape, dtype=dtype, device=self.dev)
        self.outputs.append(t)
        if zeroed:
            self.zeroed.append(t)
        return t

    def ws(self, nbytes):
        t = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.dev)
        self.workspaces.append(t)
        return t

    def host(self, name, array):
        self.hosts[name] = array
        self._pristine[name] = ctypes.string_at(array, ctypes.sizeof(array))
        return array

    # ---- the states the protocol puts the row into
    def reset(self):
        for name, array in self.hosts.items():
            ctypes.memmove(array, self._pristine[name], ctypes.sizeof(array))
        for live, _, poison in self.inputs:
            live.copy_(poison)
        for t in self.outputs:
            if not any(t is live for live, _, _ in self.inputs):
                as_bytes(t).fill_(SENTINEL)

    def fill(self):
        """In stream order: the real inputs, garbage workspaces, sentinel outputs, zeroed accumulators."""
        for live, real, _ in self.inputs:
            live.copy_(real)
        for t in self.workspaces:
            t.fill_(GARBAGE)
        for t in self.outputs:
            if not any(t is live for live, _, _ in self.inputs):
                as_bytes(t).fill_(SENTINEL)
        for t in self.zeroed:
            t.zero_()

    def scribble(self):
        for array in self.hosts.values():
            ctypes.memset(array, SCRIBBLE, ctypes.sizeof(array))

    def run_setup(self):
        if self.setup is not None and not self._setup_done:
            self.setup()
            self._setup_done = True
            return True
        return False


class Delay:
    """A fixed amount of device time on the current stream."""

    def __init__(self, dev):
        self.dev = dev
        self.ms = DELAY_MIN_MS
        self.how = 'torch.cuda._sleep'
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.cycles_per_ms = None
        try:
            torch.cuda._sleep(1000)
            torch.cuda.synchronize()
            probe = 20_000_000
            start.record()
            torch.cuda._sleep(probe)
            end.record()
            torch.cuda.synchronize()
            took = start.elapsed_time(end)
            if took > 0.5:
                self.cycles_per_ms = probe / took
        except (AttributeError, RuntimeError):
            pass
        if self.cycles_per_ms is None:
            self.how = 'a chain of 4096^2 float32 matmuls'
            self.a = torch.randn(4096, 4096, device=dev)
            self.b = torch.empty_like(self.a)
            torch.mm(self.a, self.a, out=self.b)
            torch.cuda.synchronize()
            start.record()
            for _ in range(8):
                torch.mm(self.a, self.a, out=self.b)
            end.record()
            torch.cuda.synchronize()
            self.ms_per_matmul = max(start.elapsed_time(end) / 8, 1e-3)

    def set_from_host_ms(self, slowest_host_ms):
        self.ms = min(max(DELAY_FACTOR * slowest_host_ms, DELAY_MIN_MS), DELAY_MAX_MS)
        return self.ms

    def enqueue(self):
        if self.cycles_per_ms is not None:
            torch.cuda._sleep(int(self.ms * self.cycles_per_ms))
        else:
            for _ in range(int(self.ms / self.ms_per_matmul) + 1):
                torch.mm(self.a, self.a, out=self.b)


def _collect(row, tensors):
    out = [as_bytes(t).cpu() for t in tensors]
    return row.canon(out) if row.canon is not None else out


def run_plain(row):
    """The expected value: the call on the default stream of a synchronised device with the real inputs.  -> (outputs, host ms of the call)"""
    row.reset()
    torch.cuda.synchronize()
    row.run_setup()
    row.fill()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    extra = row.call(c_void_p(0))
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    row.scribble()
    return _collect(row, list(row.outputs) + list(extra or ())), host_ms


def run_behind_delay(row, side, delay, entry_stream=None, consumer=None):
    """The protocol of the module docstring.  ``entry_stream``: the handle the entry point is given instead of ``side``'s (the null-stream control);
    ``consumer``: the stream the outputs are cloned on instead of ``side`` (the unordered-consumer control).  -> (outputs, side.query() after the return)"""
    row.reset()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        delay.enqueue()
        if row.run_setup():
            delay.enqueue()
        row.fill()
        extra = row.call(c_void_p(side.cuda_stream) if entry_stream is None else entry_stream)
        row.scribble()
        idle = side.query()
        tensors = list(row.outputs) + list(extra or ())
        if consumer is None:
            clones = [t.clone() for t in tensors]
    if consumer is not None:
        with torch.cuda.stream(consumer):
            clones = [t.clone() for t in tensors]
    side.synchronize()
    torch.cuda.synchronize()
    return _collect(row, clones), idle


def same_bytes(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------------ the case table
class Case:
    def __init__(self, build, variants, hosts):
        self.build, self.variants, self.hosts = build, tuple(variants), tuple(hosts)


CASES = {}


def case(names, variants=(None,), hosts=()):
    def register(build):
        for name in ([names] if isinstance(names, str) else names):
            assert name not in CASES, name
            CASES[name] = Case(build, variants, hosts)
        return build
    return register


def build_row(name, variant, dev):
    row = Row(dev)
    CASES[name].build(row, variant)
    assert set(row.hosts) == set(CASES[name].hosts), (name, sorted(row.hosts), CASES[name].hosts)
    return row


N = 3
PW = ((2, 1000), (2, 1001), (3, 1000), (3, 1001))      # (classes, hw): the 16-byte and the one-element kernels, two class counts
HW = (1000, 1001)
VOL = (11, 21, 45)                                     # the batch volumes of tests/test_gpu_components.py
NPV = VOL[0] * VOL[1] * VOL[2]


def rng(*key):
    """A seeded generator per (case, variant): the same data on every run and machine."""
    return np.random.RandomState(sum((i + 1) * ord(ch) for i, ch in enumerate(repr(key))) % (2 ** 31))


def f32(r, *shape):
    return r.standard_normal(shape).astype(np.float32)


def prob(r, *shape):
    return r.random_sample(shape).astype(np.float32)


def u8(r, shape, p=0.5, hi=1):
    return ((r.random_sample(shape) < p) * r.randint(1, hi + 1, size=shape)).astype(np.uint8)


def softmax_np(x, axis=1):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return (e / e.sum(axis=axis, keepdims=True)).astype(np.float32)


def stats_bytes(n, hw, C, flags):
    return int(lib().rcu_mc_stats_bytes(n, hw, C, flags))


# ---- step seam: pointwise
@case('rcu_softmax', PW)
def _softmax(row, v):
    C, hw = v
    x = row.inp(f32(rng('softmax', v), N, C, hw))
    y = row.out((N, C, hw), torch.float32)
    row.call = lambda s: chk(lib().rcu_softmax(vp(x), vp(y), N, hw, C, s))


@case('rcu_aleatoric', PW)
def _aleatoric(row, v):
    C, hw = v
    r = rng('aleatoric', v)
    x, sg = row.inp(f32(r, N, C, hw)), row.inp(f32(r, N, C, hw))
    p, so = row.out((N, C, hw), torch.float32), row.out((N, C, hw), torch.float32)
    pred, sp = row.out((N, hw), torch.uint8), row.out((N, hw), torch.float32)
    row.call = lambda s: chk(lib().rcu_aleatoric(vp(x), vp(sg), N, hw, C, int(C == 3), vp(p), vp(so), vp(pred), vp(sp), s))


@case('rcu_prediction_and_foreground', PW)
def _prediction(row, v):
    C, hw = v
    p = row.inp(softmax_np(f32(rng('pred', v), N, C, hw)))
    pred, fg = row.out((N, hw), torch.uint8), row.out((N, hw), torch.float32)
    row.call = lambda s: chk(lib().rcu_prediction_and_foreground(vp(p), N, hw, C, vp(pred), vp(fg), s))


@case(('rcu_mc_begin', 'rcu_mc_accumulate', 'rcu_mc_finalize'), PW)
def _mc_sequence(row, v):
    """begin, two accumulates, finalize: the sequence of the contract in one protocol run."""
    C, hw = v
    flags = (MI | VAR | EXACT) if C == 2 else MI
    r = rng('mc', v)
    a, b = row.inp(f32(r, N, C, hw)), row.inp(f32(r, N, C, hw))
    stats = row.out((stats_bytes(N, hw, C, flags),), torch.uint8)
    mean, ent, mi = row.out((N, C, hw), torch.float32), row.out((N, hw), torch.float32), row.out((N, hw), torch.float32)
    var = row.out((N, hw), torch.float32) if flags & VAR else None

    def call(s):
        L = lib()
        chk(L.rcu_mc_begin(vp(stats), N, hw, C, flags, s))
        chk(L.rcu_mc_accumulate(vp(a), vp(stats), N, hw, C, flags, s))
        chk(L.rcu_mc_accumulate(vp(b), vp(stats), N, hw, C, flags, s))
        chk(L.rcu_mc_finalize(vp(stats), N, hw, C, 2, flags, vp(mean), vp(ent), vp(mi), vp(var), s))
    row.call = call


SITES = ((32, 0.9), (32, 0.5), (64, -1.0), (16, 0.0))


def _site_arrays(row):
    ch = row.host('site_channels_host', (c_int32 * len(SITES))(*[c for c, _ in SITES]))
    keep = row.host('site_keep_host', (c_float * len(SITES))(*[k for _, k in SITES]))
    return ch, keep, sum(c for c, _ in SITES)


@case('rcu_dropout_masks', ((2, 3), (1, 5)), hosts=('seeds_host', 'site_channels_host', 'site_keep_host'))
def _dropout_masks(row, v):
    passes, n = v
    seeds = row.host('seeds_host', (c_uint64 * passes)(*[0x9E3779B97F4A7C15 * (t + 1) & (2 ** 64 - 1) for t in range(passes)]))
    ch, keep, floats = _site_arrays(row)
    out = row.out((passes * n * floats,), torch.float32)
    row.call = lambda s: chk(lib().rcu_dropout_masks(seeds, passes, n, 1234567, ch, keep, len(SITES), vp(out), s))


@case('rcu_dropout_masks_indexed', ((2, 3),), hosts=('seeds_host', 'site_channels_host', 'site_keep_host'))
def _dropout_masks_indexed(row, v):
    passes, n = v
    seeds = row.host('seeds_host', (c_uint64 * passes)(*[11 + t for t in range(passes)]))
    ch, keep, floats = _site_arrays(row)
    index = row.inp(np.array([77, 5, 40000], dtype=np.int64))
    out = row.out((passes * n * floats,), torch.float32)
    row.call = lambda s: chk(lib().rcu_dropout_masks_indexed(seeds, passes, n, vp(index), ch, keep, len(SITES), vp(out), s))


# ---- metric seam
def _volumes(r, npv, with_mask=True):
    p = prob(r, N, npv)
    target = u8(r, (N, npv), 0.4)
    pred = u8(r, (N, npv), 0.4)
    mask = u8(r, (N, npv), 0.8) if with_mask else None
    return p, pred, target, mask


@case('rcu_ece_hist', tuple((hw, m) for hw in HW for m in (True, False)), hosts=('thr_host',))
def _ece_hist(row, v):
    npv, with_mask = v
    p, _, target, mask = _volumes(rng('ece', v), npv, with_mask)
    from rcu_amd import _lib
    thr = row.host('thr_host', (c_float * 9)(*list(_lib.ece_thresholds(10))))
    p, target, mask = row.inp(p), row.inp(target), (row.inp(mask) if with_mask else None)
    res = row.out((N * ctypes.sizeof(_lib.EceResult),), torch.uint8)
    ws = row.ws(lib().rcu_ece_workspace_bytes(npv, N))
    row.call = lambda s: chk(lib().rcu_ece_hist(vp(p), vp(target), vp(mask), npv, N, thr, 10, vp(res), vp(ws), s))


@case('rcu_ece_bin_ids', HW, hosts=('thr_host',))
def _ece_bin_ids(row, v):
    from rcu_amd import _lib
    thr = row.host('thr_host', (c_float * 9)(*list(_lib.ece_thresholds(10))))
    p = row.inp(prob(rng('ids', v), v))
    ids = row.out((v,), torch.uint8)
    row.call = lambda s: chk(lib().rcu_ece_bin_ids(vp(p), v, thr, 10, vp(ids), s))


@case('rcu_unc_counts', tuple((hw, f64) for hw in HW for f64 in (1, 0)), hosts=('thr_host',))
def _unc_counts(row, v):
    npv, is_f64 = v
    p, pred, target, mask = _volumes(rng('unc', v), npv)
    unc = row.inp(p.astype(np.float64) if is_f64 else p)
    pred, target, mask = row.inp(pred), row.inp(target), row.inp(mask)
    thr = row.host('thr_host', (c_double * 11)(*[0.05] + [0.1 * k for k in range(1, 10)] + [0.95]))
    counts = row.out((N, 11, 8), torch.int64)
    ws = row.ws(lib().rcu_unc_workspace_bytes(npv, N))
    row.call = lambda s: chk(lib().rcu_unc_counts(vp(unc), is_f64, vp(pred), vp(target), vp(mask), npv, N, thr, 11, vp(counts), vp(ws), s))


@case('rcu_unc_counts_from_p', HW, hosts=('thr_host',))
def _unc_counts_from_p(row, v):
    L = lib()
    p, pred, target, mask = _volumes(rng('uncp', v), v)
    p, pred, target, mask = row.inp(p), row.inp(pred), row.inp(target), row.inp(mask)
    values = sorted(L.rcu_unc_from_p_threshold(i) for i in range(L.rcu_unc_from_p_num_thresholds()))
    thr = row.host('thr_host', (c_double * len(values))(*values))
    assert L.rcu_unc_from_p_supported(thr, len(values)) == 1
    counts = row.out((N, len(values), 8), torch.int64)
    ws = row.ws(L.rcu_unc_from_p_workspace_bytes(v, N))
    row.call = lambda s: chk(L.rcu_unc_counts_from_p(vp(p), vp(pred), vp(target), vp(mask), v, N, thr, len(values), vp(counts), vp(ws), s))


@case('rcu_normalised_entropy', HW)
def _normalised_entropy(row, v):
    p = row.inp(prob(rng('ent', v), N * v))
    o64, o32 = row.out((N * v,), torch.float64), row.out((N * v,), torch.float32)
    row.call = lambda s: chk(lib().rcu_normalised_entropy(vp(p), N * v, vp(o64), vp(o32), s))


LEVELS = 1000


@case('rcu_unc_hist', tuple((hw, f64) for hw in HW for f64 in (1, 0)))
def _unc_hist(row, v):
    npv, is_f64 = v
    p, pred, target, mask = _volumes(rng('uh', v), npv)
    unc = row.inp(p.astype(np.float64) if is_f64 else p)
    pred, target, mask = row.inp(pred), row.inp(target), row.inp(mask)
    hist = row.out((N, 4, LEVELS), torch.int64)
    ws = row.ws(lib().rcu_unc_hist_workspace_bytes(npv, N, LEVELS))
    row.call = lambda s: chk(lib().rcu_unc_hist(vp(unc), is_f64, vp(pred), vp(target), vp(mask), npv, N, LEVELS, vp(hist), vp(ws), s))


@case('rcu_unc_hist_from_p', HW)
def _unc_hist_from_p(row, v):
    p, pred, target, mask = _volumes(rng('uhp', v), v)
    p, pred, target, mask = row.inp(p), row.inp(pred), row.inp(target), row.inp(mask)
    hist = row.out((N, 4, LEVELS), torch.int64)
    ws = row.ws(lib().rcu_unc_hist_workspace_bytes(v, N, LEVELS))
    row.call = lambda s: chk(lib().rcu_unc_hist_from_p(vp(p), vp(pred), vp(target), vp(mask), v, N, LEVELS, vp(hist), vp(ws), s))


@case('rcu_calib_curve', HW)
def _calib_curve(row, v):
    p, _, target, mask = _volumes(rng('cc', v), v)
    p, target, mask = row.inp(p), row.inp(target), row.inp(mask)
    levels, totals = row.out((N, 3, LEVELS), torch.int64), row.out((N, 2, 4), torch.int64)
    ws = row.ws(lib().rcu_calib_curve_workspace_bytes(v, N, LEVELS))
    row.call = lambda s: chk(lib().rcu_calib_curve(vp(p), vp(target), vp(mask), v, N, LEVELS, vp(levels), vp(totals), vp(ws), s))


@case('rcu_calib_curve_terms', HW)
def _calib_curve_terms(row, v):
    p, _, target, _ = _volumes(rng('cct', v), v)
    p, target = row.inp(p), row.inp(target)
    level, nll = row.out((N * v,), torch.int32), row.out((N * v,), torch.float32)
    row.call = lambda s: chk(lib().rcu_calib_curve_terms(vp(p), vp(target), N * v, LEVELS, vp(level), vp(nll), s))


# ---- test-time augmentation
@case('rcu_tta_transform', ((25, 40, 3), (31, 31, 5)))
def _tta_transform(row, v):
    h, w, element = v
    x = row.inp(f32(rng('tta', v), N, 2, h, w))
    y = row.out((N, 2, h, w) if element < 4 else (N, 2, w, h), torch.float32)
    row.call = lambda s: chk(lib().rcu_tta_transform(vp(x), N, 2, h, w, element, vp(y), s))


@case('rcu_mc_fold_transformed', ((25, 40, 1, MI, 2), (31, 31, 6, MI | VAR | EXACT, 3)))
def _mc_fold(row, v):
    h, w, element, flags, C = v
    r = rng('fold', v)
    dtype = np.float64 if flags & (VAR | EXACT) else np.float32
    count = stats_bytes(N, h * w, C, flags) // np.dtype(dtype).itemsize
    src = row.inp(r.random_sample(count).astype(dtype))
    dst = row.inout(r.random_sample(count).astype(dtype))
    row.call = lambda s: chk(lib().rcu_mc_fold_transformed(vp(src), vp(dst), N, h, w, C, flags, element, s))


# ---- temperature scaling
def _temperature_inputs(row, v, tag):
    C, hw = v
    r = rng(tag, v)
    logits = row.inp(3 * f32(r, 2, N, C, hw))
    target = row.inp(r.randint(0, C + 1, size=(N, hw)).astype(np.uint8))      # some targets >= C: they are left out and counted
    mask = row.inp(u8(r, (N, hw), 0.8))
    return logits, target, mask


@case('rcu_temperature_nll', PW, hosts=('beta_host',))
def _temperature_nll(row, v):
    C, hw = v
    logits, target, mask = _temperature_inputs(row, v, 'tnll')
    beta = row.host('beta_host', (c_float * 4)(0.5, 1.0, 1.5, 2.25))
    out = row.out((6,), torch.int64, zeroed=True)
    ws = row.ws(lib().rcu_temperature_nll_workspace_bytes(N * hw, 4))
    row.call = lambda s: chk(lib().rcu_temperature_nll(vp(logits), 2, N, hw, C, vp(target), vp(mask), beta, 4, vp(out), vp(ws), s))


@case('rcu_temperature_nll_terms', PW)
def _temperature_nll_terms(row, v):
    C, hw = v
    logits, target, mask = _temperature_inputs(row, v, 'tterms')
    terms = row.out((N, hw), torch.float32)
    row.call = lambda s: chk(lib().rcu_temperature_nll_terms(vp(logits), 2, N, hw, C, vp(target), vp(mask), 1.5, vp(terms), s))


# ---- logit sampling
@case('rcu_logit_normals', PW)
def _logit_normals(row, v):
    C, hw = v
    out = row.out((N * hw * 3 * C,), torch.float32)
    row.call = lambda s: chk(lib().rcu_logit_normals(0xC0FFEE, 17, N, hw, C, 3, vp(out), s))


@case('rcu_logit_sampling', PW)
def _logit_sampling(row, v):
    C, hw = v
    r = rng('ls', v)
    flags = MI if C == 3 else (MI | EXACT)
    logits, sigma = row.inp(f32(r, N, C, hw)), row.inp(f32(r, N, C, hw))
    probs = row.out((N, C, hw), torch.float32)
    stats = row.out((stats_bytes(N, hw, C, flags),), torch.uint8)

    def call(s):
        chk(lib().rcu_mc_begin(vp(stats), N, hw, C, flags, s))
        chk(lib().rcu_logit_sampling(vp(logits), vp(sigma), N, hw, C, int(C == 3), 4, 0xFEED, 9, vp(probs), vp(stats), flags, s))
    row.call = call


# ---- connected components, distance transform, patches: the batch volumes of their GPU tests
def _plain(fn):
    """Host-side preparation of a row: a call on the default stream, finished before the protocol starts."""
    fn(c_void_p(0))
    torch.cuda.synchronize()


def _labels_of(mask_np, dev, conn=26):
    mask = torch.as_tensor(mask_np).to(dev)
    labels = torch.empty(mask.shape, dtype=torch.int32, device=dev)
    _plain(lambda s: chk(lib().rcu_cc_label(vp(mask), VOL[0], VOL[1], VOL[2], N, conn, vp(labels), s)))
    return labels.cpu().numpy()


@case('rcu_cc_label', (26, 6))
def _cc_label(row, v):
    mask = row.inp(u8(rng('ccl', v), (N,) + VOL, 0.25, hi=5))
    labels = row.out((N, NPV), torch.int32)
    row.call = lambda s: chk(lib().rcu_cc_label(vp(mask), VOL[0], VOL[1], VOL[2], N, v, vp(labels), s))


@case(('rcu_cc_compact', 'rcu_cc_relabel', 'rcu_cc_table'))
def _cc_tables(row, v):
    """compact, relabel, table on one workspace (the ranks compact leaves in it are what the other two read)."""
    r = rng('cct')
    labels_np = _labels_of(u8(r, (N,) + VOL, 0.12), row.dev)
    entries = int(sum((vol.reshape(-1) == np.arange(1, NPV + 1)).sum() for vol in labels_np))
    labels, other, unc = row.inp(labels_np), row.inp(u8(r, (N, NPV), 0.5)), row.inp(prob(r, N, NPV))
    counts, dense = row.out((N,), torch.int32), row.out((N, NPV), torch.int32)
    table = row.out((entries * 24,), torch.uint8)
    ws = row.ws(lib().rcu_cc_workspace_bytes(NPV, N))

    def call(s):
        L = lib()
        chk(L.rcu_cc_compact(vp(labels), NPV, N, vp(counts), vp(ws), s))
        chk(L.rcu_cc_relabel(vp(labels), NPV, N, vp(ws), vp(dense), s))
        chk(L.rcu_cc_table(vp(labels), vp(other), vp(unc), 1, NPV, N, vp(ws), vp(table), entries, s))
    row.call = call


def _sorted_slots(capacity):
    def canon(outs):
        table = outs[0]
        slots = table[:N * capacity * 16].view(torch.int32).reshape(N, capacity, 4).to(torch.int64) & 0xFFFFFFFF
        key = (slots[..., 0] << 32) | slots[..., 1]
        order = key.argsort(dim=1, stable=True)
        return [torch.gather(slots, 1, order[..., None].expand(-1, -1, 4)), table[N * capacity * 16:]] + outs[1:]
    return canon


@case('rcu_cc_pairs')
def _cc_pairs(row, v):
    r = rng('pairs')
    a = row.inp(_labels_of(u8(r, (N,) + VOL, 0.15), row.dev))
    b = row.inp(_labels_of(u8(r, (N,) + VOL, 0.15), row.dev, 6))
    inside = row.inp(u8(r, (N, NPV), 0.5))
    capacity = 32768            # a power of two >= 2 * n_per_volume: nothing is dropped
    table = row.out((lib().rcu_cc_pairs_bytes(capacity, N),), torch.uint8)
    row.canon = _sorted_slots(capacity)      # the ORDER of the slots is the race's (include/rcu.h); the sorted table is the function of the inputs
    row.call = lambda s: chk(lib().rcu_cc_pairs(vp(a), vp(b), vp(inside), NPV, N, capacity, vp(table), s))


@case('rcu_edt_sq', (1, 0))
def _edt_sq(row, v):
    mask = row.inp(u8(rng('edt', v), (N,) + VOL, 0.3))
    out = row.out((N, NPV), torch.int32)
    row.call = lambda s: chk(lib().rcu_edt_sq(vp(mask), VOL[0], VOL[1], VOL[2], N, v, vp(out), s))


def _distances(r):
    target = u8(r, (N, NPV), 0.3)
    d = r.randint(1, 30, size=(N, NPV)).astype(np.int32)
    return target, np.where(target != 0, d, 0).astype(np.int32), np.where(target != 0, 0, d).astype(np.int32)


@case('rcu_border_mask')
def _border_mask(row, v):
    _, d_in, d_out = _distances(rng('border'))
    d_in, d_out = row.inp(d_in), row.inp(d_out)
    mask, dist = row.out((N * NPV,), torch.uint8), row.out((N * NPV,), torch.float64)
    row.call = lambda s: chk(lib().rcu_border_mask(vp(d_in), vp(d_out), N * NPV, 2, 3, vp(mask), vp(dist), s))


@case('rcu_boundary_table')
def _boundary_table(row, v):
    r = rng('btable')
    target, d_in, d_out = _distances(r)
    pred, target, d_in, d_out = row.inp(u8(r, (N, NPV), 0.3)), row.inp(target), row.inp(d_in), row.inp(d_out)
    unc = row.inp(r.random_sample((N, NPV)))
    bands = 4
    table = row.out((N * 2 * (bands + 1) * 32,), torch.uint8)
    row.call = lambda s: chk(lib().rcu_boundary_table(vp(pred), vp(target), vp(d_in), vp(d_out), vp(unc), 2, NPV, N, bands, vp(table), s))


@case('rcu_surface_distance_hist')
def _surface_distance_hist(row, v):
    r = rng('surface')
    pred, target = row.inp(u8(r, (N,) + VOL, 0.4)), row.inp(u8(r, (N,) + VOL, 0.4))
    bins = int(lib().rcu_surface_distance_bins(*VOL))
    hist = row.out((N, 2, bins), torch.int32)
    ws = row.ws(lib().rcu_surface_distance_workspace_bytes(NPV, N))
    row.call = lambda s: chk(lib().rcu_surface_distance_hist(vp(pred), vp(target), VOL[0], VOL[1], VOL[2], N, vp(hist), vp(ws), s))


@case('rcu_patch_table', (3, 0))
def _patch_table(row, v):
    r = rng('patch', v)
    pred, target, mask = row.inp(u8(r, (N,) + VOL, 0.3)), row.inp(u8(r, (N,) + VOL, 0.3)), row.inp(u8(r, (N,) + VOL, 0.8))
    unc = row.inp(prob(r, N, NPV)) if v else None
    patches = int(lib().rcu_patch_count(VOL[0], VOL[1], VOL[2], 2, 4, 8))
    table = row.out((N, patches, 4), torch.int64)
    row.call = lambda s: chk(lib().rcu_patch_table(vp(pred), vp(target), vp(mask), vp(unc), v, VOL[0], VOL[1], VOL[2], N, 2, 4, 8, vp(table), s))


@case('rcu_patch_hist')
def _patch_hist(row, v):
    r = rng('phist')
    patches = 1001
    n = r.randint(0, 65, size=(N, patches))
    errors = (n * r.random_sample(n.shape)).astype(np.int64)
    fg = np.maximum(errors, (n * r.random_sample(n.shape)).astype(np.int64))
    sum_q = (n * r.random_sample(n.shape) * 2 ** 24).astype(np.int64)
    table = row.inp(np.stack([n, errors, fg, sum_q], -1).astype(np.int64))
    hist = row.out((N, 3, 100), torch.int64)
    row.call = lambda s: chk(lib().rcu_patch_hist(vp(table), patches, N, 100, 500, vp(hist), s))


# ---- sample agreement
@case('rcu_mc_votes', ((2, 1000, INPUT_PROBS, 2, 37), (3, 1001, 0, 1, 3)))
def _mc_votes(row, v):
    C, hw, flags, words, bit = v
    x = f32(rng('votes', v), N, C, hw)
    x = row.inp(softmax_np(x) if flags else x)
    votes = row.out((words, N * hw), torch.int32, zeroed=True)
    row.call = lambda s: chk(lib().rcu_mc_votes(vp(x), N, hw, C, flags, vp(votes), words, bit, s))


@case('rcu_agreement_tables', HW)
def _agreement_tables(row, v):
    passes = 40
    votes = row.inp(rng('agree', v).randint(-2 ** 31, 2 ** 31, size=(2, N * v)).astype(np.int32))
    hist, pairs = row.out((N, passes + 1), torch.int64), row.out((N, passes * (passes + 1) // 2), torch.int64)
    row.call = lambda s: chk(lib().rcu_agreement_tables(vp(votes), 2, v, N, passes, vp(hist), vp(pairs), s))


# ---- corruptions
def _blur_taps(amount):
    radius = int(4 * amount + 0.5)
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-k * k / (2 * amount * amount))
    return (w / w.sum()).astype(np.float32)


def _bias_aux(r, channels, h, w):
    coef = r.standard_normal((channels, 8))
    coef /= np.abs(coef).sum(1, keepdims=True)
    A = np.stack([np.cos(np.pi * u * (np.arange(h) + 0.5) / h) for u in range(3)])
    B = np.stack([np.cos(np.pi * u * (np.arange(w) + 0.5) / w) for u in range(3)])
    return np.concatenate([coef.reshape(-1), A.reshape(-1), B.reshape(-1)]).astype(np.float32)


@case('rcu_corrupt', ('gaussian_blur', 'bias_field', 'contrast', 'gaussian_noise'), hosts=('aux_host',))
def _corrupt(row, v):
    from rcu_amd import _lib
    kind = _lib.CORRUPTION_KINDS.index(v)
    h, w, channels = 25, 40, 2
    r = rng('corrupt', v)
    x = row.inp(f32(r, N, channels, h, w))
    aux_np = {'gaussian_blur': _blur_taps(1.0), 'bias_field': _bias_aux(r, channels, h, w)}.get(v, np.zeros(1, np.float32))
    n_aux = len(aux_np) if v in ('gaussian_blur', 'bias_field') else 0
    aux = row.host('aux_host', (c_float * len(aux_np))(*aux_np.tolist()))
    amount = {'gaussian_blur': 1.0, 'bias_field': 0.3, 'contrast': 0.45, 'gaussian_noise': 0.3}[v]
    out = row.out((N, channels, h, w), torch.float32)
    ws = row.ws(lib().rcu_corrupt_workspace_bytes(N, channels, h, w, kind))
    row.call = lambda s: chk(lib().rcu_corrupt(vp(x), N, channels, h, w, kind, amount, 0xABCDEF, 21, aux if n_aux else None, n_aux, vp(out), vp(ws), s))


# ---- adaptive MC
@case('rcu_mc_slice_scores', PW)
def _slice_scores(row, v):
    C, hw = v
    stats = row.inp(rng('scores', v).randint(0, 3 * 2 ** 20, size=(C, N * hw)).astype(np.float64) * 2.0 ** -20)
    unsettled, margin = row.out((N,), torch.int32), row.out((N,), torch.int64)
    row.call = lambda s: chk(lib().rcu_mc_slice_scores(vp(stats), N, hw, C, EXACT, int(2.5 * 2 ** 40), vp(unsettled), vp(margin), s))


@case('rcu_mc_merge_slices', PW)
def _merge_slices(row, v):
    C, hw = v
    r = rng('merge', v)
    src = row.inp(r.randint(0, 2 ** 20, size=(C + 1, 2 * hw)).astype(np.float64) * 2.0 ** -20)
    dst = row.inout(r.randint(0, 2 ** 20, size=(C + 1, N * hw)).astype(np.float64) * 2.0 ** -20)
    index = row.inp(np.array([2, 0], dtype=np.int32), poison=np.array([0, 1], dtype=np.int32))      # distinct entries, as the contract demands
    row.call = lambda s: chk(lib().rcu_mc_merge_slices(vp(src), 2, vp(dst), N, hw, C, EXACT | MI, vp(index), s))


@case('rcu_mc_finalize_counts', PW)
def _finalize_counts(row, v):
    C, hw = v
    flags = MI | VAR | EXACT
    r = rng('fcounts', v)
    counts_np = np.array([2, 3, 4], dtype=np.int32)
    p = softmax_np(f32(r, N, C, hw)).astype(np.float64) * counts_np[:, None, None]
    planes = np.concatenate([p.transpose(1, 0, 2), (p * p / 2).transpose(1, 0, 2), r.random_sample((1, N, hw))])      # [C | C | 1][n][hw]
    stats = row.inp(planes.reshape(2 * C + 1, N * hw))
    assert stats.numel() * 8 == stats_bytes(N, hw, C, flags)
    counts = row.inp(counts_np, poison=2)
    mean, ent = row.out((N, C, hw), torch.float32), row.out((N, hw), torch.float32)
    mi, var = row.out((N, hw), torch.float32), row.out((N, hw), torch.float32)
    row.call = lambda s: chk(lib().rcu_mc_finalize_counts(vp(stats), N, hw, C, vp(counts), flags, vp(mean), vp(ent), vp(mi), vp(var), s))


# ---- feature-space density, Laplace, PostNet: features [n * hw][pitch]
F, PITCH = 20, 24


def _features(row, r, hw, pitch=PITCH):
    return row.inp(f32(r, N * hw, pitch))


@case('rcu_density_moments', tuple((hw, K) for hw in HW for K in (2, 3)))
def _density_moments(row, v):
    hw, K = v
    r = rng('dm', v)
    feats = _features(row, r, hw)
    labels = row.inp(r.randint(0, K, size=(N, hw)).astype(np.uint8))
    n_out, S, G = row.out((N, K), torch.int64), row.out((N, K, F), torch.float64), row.out((N, K, F, F), torch.float64)
    ws = row.ws(lib().rcu_density_moments_workspace_bytes(N, hw, F, K))
    row.call = lambda s: chk(lib().rcu_density_moments(vp(feats), PITCH, F, vp(labels), N, hw, K, vp(n_out), vp(S), vp(G), vp(ws), s))


@case('rcu_density_energy', tuple((hw, K) for hw in HW for K in (2, 3)))
def _density_energy(row, v):
    hw, K = v
    r = rng('de', v)
    feats = _features(row, r, hw)
    A, b, k = row.inp(0.2 * f32(r, K, F, F)), row.inp(f32(r, K, F)), row.inp(f32(r, K))
    energy, d2 = row.out((N * hw,), torch.float32), row.out((N * hw, K), torch.float32)
    row.call = lambda s: chk(lib().rcu_density_energy(vp(feats), PITCH, F, N * hw, K, vp(A), vp(b), vp(k), vp(energy), vp(d2), s))


@case('rcu_laplace_moments', PW)
def _laplace_moments(row, v):
    C, hw = v
    r = rng('lm', v)
    P = C * (C + 1) // 2
    feats = _features(row, r, hw)
    probs = row.inp(softmax_np(f32(r, N, C, hw)))
    w, S, G = row.out((N, P), torch.float64), row.out((N, P, F), torch.float64), row.out((N, P, F, F), torch.float64)
    ws = row.ws(lib().rcu_laplace_moments_workspace_bytes(N, hw, F, C))
    row.call = lambda s: chk(lib().rcu_laplace_moments(vp(feats), PITCH, F, vp(probs), N, hw, C, vp(w), vp(S), vp(G), vp(ws), s))


@case('rcu_laplace_predict', PW)
def _laplace_predict(row, v):
    C, hw = v
    r = rng('lp', v)
    feats, logits = _features(row, r, hw), row.inp(f32(r, N, C, hw))
    A, b, kappa = row.inp(0.2 * f32(r, C, F, F)), row.inp(f32(r, C, F)), row.inp(prob(r, C))
    probs, std = row.out((N, C, hw), torch.float32), row.out((N, C, hw), torch.float32)
    std_pred, pred = row.out((N, hw), torch.float32), row.out((N, hw), torch.uint8)
    row.call = lambda s: chk(lib().rcu_laplace_predict(vp(feats), PITCH, F, vp(logits), N, hw, C, vp(A), vp(b), vp(kappa), vp(probs), vp(std), vp(std_pred),
                                                       vp(pred), s))


@case('rcu_postnet_forward', tuple((hw, m) for hw in HW for m in (False, True)))
def _postnet_forward(row, v):
    hw, with_masks = v
    from rcu_amd.model import PostNet
    r = rng('postnet', v)
    torch.manual_seed(7)
    net = PostNet(32, 2, 3)
    for m in net.modules():      # BatchNorm that is not the identity
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.5, 0.5)
            m.running_var.uniform_(0.5, 1.5)
    net.weights_changed()
    handle = net._handle()
    row.keep.append(net)
    feats = _features(row, r, hw, 32)
    masks = row.inp(((r.random_sample((3, N, 32)) < 0.7) / 0.7).astype(np.float32)) if with_masks else None
    logits = row.out((N, 2, hw), torch.float32)
    row.call = lambda s: chk(lib().rcu_postnet_forward(handle, vp(feats), 32, N, hw, vp(masks), vp(logits), s))


# ---- quantile rescale
def _keys(x):
    b = np.where(x == 0, np.float32(0), x).astype(np.float32).view(np.uint32)
    return np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


@case('rcu_key_hist', HW, hosts=('prefixes_host',))
def _key_hist(row, v):
    r = rng('keyhist', v)
    maps_np = f32(r, N, v)
    maps, mask = row.inp(maps_np), row.inp(u8(r, (N, v), 0.8))
    shift, bits = 16, 8
    listed = sorted(set((_keys(maps_np) >> (shift + bits)).reshape(-1).tolist()))[::2]      # every other prefix that occurs: some voxels are skipped
    prefixes = row.host('prefixes_host', (c_uint32 * len(listed))(*listed))
    hist, counts = row.out((len(listed), 1 << bits), torch.int64, zeroed=True), row.out((2,), torch.int64, zeroed=True)
    ws = row.ws(lib().rcu_key_hist_workspace_bytes(len(listed)))
    row.call = lambda s: chk(lib().rcu_key_hist(vp(maps), vp(mask), v, N, prefixes, len(listed), shift, bits, vp(hist), vp(counts), vp(ws), s))


@case('rcu_quantile_apply', HW, hosts=('bounds_host',))
def _quantile_apply(row, v):
    r = rng('qapply', v)
    x = f32(r, N * v)
    quantiles = 16
    bounds_np = np.sort(_keys(x))[[int(np.ceil(k * x.size / quantiles)) - 1 for k in range(1, quantiles)]]
    bounds = row.host('bounds_host', (c_uint32 * (quantiles - 1))(*bounds_np.tolist()))
    x = row.inp(x)
    out, levels = row.out((N * v,), torch.float32), row.out((N * v,), torch.int16)
    ws = row.ws(lib().rcu_quantile_apply_workspace_bytes(quantiles))
    row.call = lambda s: chk(lib().rcu_quantile_apply(vp(x), N * v, bounds, quantiles, vp(out), vp(levels), vp(ws), s))


# ---- the model seam: a handle created, and run for the first time, inside the window; then once more warm
UNET_PARAMS = dict(nb_classes=2, in_channels=4, depth=4, start_filters=32, dropout=0.05)
PLANS = {'default': (48, 32), 'padded': (240, 240)}      # (3, 4, 48, 32); case B of tests/parity_power.py: levels 60 / 30 / 15 allocated 64 / 32 / 16
_state_cache = {}


def _unet(row, plan, n_max, sigma_out=False, provide_features=False):
    """-> (get_handle, model, h, w): the model is made now, its handle by row.setup inside the window."""
    from oracle import unet_oracle as uo
    from rcu_amd.model import UNet
    params = dict(UNET_PARAMS, sigma_out=sigma_out)
    key = (sigma_out,)
    if key not in _state_cache:
        _state_cache[key] = uo.sensitive_state(22, **params)
    model = UNet(provide_features=provide_features, **params)
    model.load_state_dict(_state_cache[key])
    h, w = PLANS[plan]
    box = {}

    def setup():
        box['handle'] = model._handle(h, w, n_max)
    row.setup = setup
    row.warm = True
    row.keep.append(model)
    return (lambda: box['handle']), model, h, w


def _mask_rows(row, model, rows, tag):
    """Dropout2d factors [site][rows][C_site] at p = 0.3, concatenated."""
    r = rng('masks', tag)
    chunks = [((r.random_sample((rows, c)) < 0.7) / 0.7).astype(np.float32).reshape(-1) for _, c in model.dropout_sites()]
    return row.inp(np.concatenate(chunks))


UNET_VARIANTS = ('default', 'padded')


@case('rcu_unet_forward', ('default', 'padded', 'default eval features', 'padded eval features', 'default head_features', 'default sigma'))
def _unet_forward(row, v):
    plan = v.split()[0]
    sigma_out, features, head = 'sigma' in v, 'eval features' in v, 'head_features' in v
    handle, model, h, w = _unet(row, plan, N, sigma_out=sigma_out, provide_features=features)
    x = row.inp(f32(rng('unet', v), N, 4, h, w))
    masks = None if features else _mask_rows(row, model, N, v)
    logits = row.out((N, 2, h, w), torch.float32)
    sigma = row.out((N, 2, h, w), torch.float32) if sigma_out else None

    def call(s):
        L = lib()
        if head:
            chk(L.rcu_unet_set_fuse_head(handle(), 0))
        chk(L.rcu_unet_forward(handle(), vp(x), N, vp(masks), vp(logits), vp(sigma), s))
        if features or head:      # rcu_unet_features / rcu_unet_head_features: views of the handle's workspace, read in stream order behind the forward
            return [model._features_view(handle(), N, h, w, row.dev, L.rcu_unet_head_features if head else None)]
    row.call = call


def _stats_row(row, model, h, w, flags):
    return row.out((stats_bytes(N, h * w, 2, flags),), torch.uint8)


@case('rcu_unet_forward_accumulate', UNET_VARIANTS)
def _unet_accumulate(row, v):
    handle, model, h, w = _unet(row, v, N)
    flags = MI | EXACT
    x, masks = row.inp(f32(rng('unet-acc', v), N, 4, h, w)), _mask_rows(row, model, N, v)
    stats = _stats_row(row, model, h, w, flags)

    def call(s):
        chk(lib().rcu_mc_begin(vp(stats), N, h * w, 2, flags, s))
        chk(lib().rcu_unet_forward_accumulate(handle(), vp(x), N, vp(masks), vp(stats), flags, s))
    row.call = call


@case('rcu_unet_forward_accumulate_passes', UNET_VARIANTS)
def _unet_accumulate_passes(row, v):
    handle, model, h, w = _unet(row, v, 2 * N)
    flags = MI | VAR | EXACT
    x, masks = row.inp(f32(rng('unet-passes', v), N, 4, h, w)), _mask_rows(row, model, 2 * N, v)
    stats = _stats_row(row, model, h, w, flags)

    def call(s):
        chk(lib().rcu_mc_begin(vp(stats), N, h * w, 2, flags, s))
        chk(lib().rcu_unet_forward_accumulate_passes(handle(), vp(x), N, 2, vp(masks), vp(stats), flags, s))
    row.call = call


@case(('rcu_unet_forward_accumulate_sigma', 'rcu_unet_forward_accumulate_sigma_passes'), UNET_VARIANTS)
def _unet_accumulate_sigma(row, v):
    """One pass, then a group of two, into the same statistics and sigma sums."""
    handle, model, h, w = _unet(row, v, 2 * N, sigma_out=True)
    flags = MI | EXACT
    x = row.inp(f32(rng('unet-sigma', v), N, 4, h, w))
    one, two = _mask_rows(row, model, N, (v, 1)), _mask_rows(row, model, 2 * N, (v, 2))
    stats = _stats_row(row, model, h, w, flags)
    sigma_sum = row.out((N, 2, h, w), torch.float32, zeroed=True)

    def call(s):
        L = lib()
        chk(L.rcu_mc_begin(vp(stats), N, h * w, 2, flags, s))
        chk(L.rcu_unet_forward_accumulate_sigma(handle(), vp(x), N, vp(one), vp(stats), flags, vp(sigma_sum), 1, s))
        chk(L.rcu_unet_forward_accumulate_sigma_passes(handle(), vp(x), N, 2, vp(two), vp(stats), flags, vp(sigma_sum), 1, s))
    row.call = call


@case('rcu_unet_forward_sample_sigma_passes', UNET_VARIANTS, hosts=('keys_host',))
def _unet_sample_sigma(row, v):
    handle, model, h, w = _unet(row, v, 2 * N, sigma_out=True)
    flags = MI | EXACT
    x, masks = row.inp(f32(rng('unet-sample', v), N, 4, h, w)), _mask_rows(row, model, 2 * N, v)
    keys = row.host('keys_host', (c_uint64 * 2)(0x1234567, 0x89ABCDE))
    stats = _stats_row(row, model, h, w, flags)
    sigma_sum = row.out((N, 2, h, w), torch.float32, zeroed=True)

    def call(s):
        chk(lib().rcu_mc_begin(vp(stats), N, h * w, 2, flags, s))
        chk(lib().rcu_unet_forward_sample_sigma_passes(handle(), vp(x), N, 2, vp(masks), keys, 40, 3, vp(stats), flags, vp(sigma_sum), 0, s))
    row.call = call


@case('rcu_unet_forward_accumulate_votes', UNET_VARIANTS, hosts=('bits_host',))
def _unet_votes(row, v):
    handle, model, h, w = _unet(row, v, 2 * N)
    flags = MI | EXACT
    x, masks = row.inp(f32(rng('unet-votes', v), N, 4, h, w)), _mask_rows(row, model, 2 * N, v)
    bits = row.host('bits_host', (c_int32 * 2)(31, 32))      # the group straddles a word: one head launch per word
    stats = _stats_row(row, model, h, w, flags)
    votes = row.out((2, N * h * w), torch.int32, zeroed=True)

    def call(s):
        chk(lib().rcu_mc_begin(vp(stats), N, h * w, 2, flags, s))
        chk(lib().rcu_unet_forward_accumulate_votes(handle(), vp(x), N, 2, vp(masks), vp(stats), flags, vp(votes), 2, bits, s))
    row.call = call


@case('rcu_unet_run_layer', UNET_VARIANTS)
def _unet_run_layer(row, v):
    """An eval-mode forward, then the layer that writes the feature tensor once more UNDER MASKS: the features then carry the Dropout2d factors, which
    only a run_layer that ran behind the forward can have left there."""
    from rcu_amd import _lib
    handle, model, h, w = _unet(row, v, N, provide_features=True)
    x, masks = row.inp(f32(rng('unet-layer', v), N, 4, h, w)), _mask_rows(row, model, N, v)
    logits = row.out((N, 2, h, w), torch.float32)

    def call(s):
        L = lib()
        info, layer = _lib.LayerInfo(), None
        for i in range(L.rcu_unet_num_layers(handle())):
            chk(L.rcu_unet_layer_info(handle(), i, ctypes.byref(info)))
            if info.name.decode().startswith('up_convs.3.block.block.1'):
                layer = i
        assert layer is not None
        chk(L.rcu_unet_forward(handle(), vp(x), N, None, vp(logits), None, s))
        chk(L.rcu_unet_run_layer(handle(), layer, N, vp(masks), s))
        return [model._features_view(handle(), N, h, w, row.dev)]
    row.call = call
