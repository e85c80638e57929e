"""The case table of the stream-order protocol (tests/stream_order.py: a delay, poison, sentinel outputs and query()) for the entry points of the
fourth header, include/rcu_warp.h.  The rows live in a table of their own, as those of include/rcu_fit.h and include/rcu_knn.h do
(tests/stream_order_fit.py, tests/stream_order_knn.py): tests/stream_order.py's CASES cover include/rcu.h and its stale-row check would refuse a
row for a function that header does not declare."""
import numpy as np
import torch

import stream_order as so
import stream_order_fit as sof
import stream_order_knn as sok
import warp_reference as ref

CASES = {}


def case(name, variants, hosts=()):
    def register(build):
        assert name not in CASES and name not in so.CASES and name not in sof.CASES and name not in sok.CASES, name
        CASES[name] = so.Case(build, variants, hosts)
        return build
    return register


def build_row(name, variant, dev):
    row = so.Row(dev)
    CASES[name].build(row, variant)
    assert set(row.hosts) == set(CASES[name].hosts), (name, sorted(row.hosts), CASES[name].hosts)
    return row


def _mats(count):
    pool = [ref.matrix(10.0, 1.1, 1.5, -2.25), ref.matrix(-25.0, 0.85, flip=True), ref.IDENTITY, ref.D4[1]]
    return np.stack([pool[k % len(pool)] for k in range(count)])


# (n, channels, H, W, matrices): the image AND the matrices arrive on the stream (poison: 0.25 everywhere, another warp of another image)
@case('rcu_warp_affine', ((3, 4, 15, 17, 3), (2, 1, 32, 48, 1)))
def _warp_affine(row, v):
    n, c, h, w, count = v
    x = row.inp(so.f32(so.rng('warp', *v), n, c, h, w))
    mats = row.inp(_mats(count))
    out = row.out((count, n, c, h, w), torch.float32)
    row.call = lambda s: so.chk(so.lib().rcu_warp_affine(so.vp(x), n, c, h, w, so.vp(mats), count, so.vp(out), s))


# (n, C, H, W, groups, flags): the statistics are the caller's to zero, in stream order
@case('rcu_mc_accumulate_warped', ((3, 4, 15, 17, 3, so.EXACT | so.MI | so.VAR), (2, 2, 32, 48, 2, so.MI), (1, 3, 9, 5, 1, so.VAR | so.INPUT_PROBS)))
def _accumulate_warped(row, v):
    n, c, h, w, groups, flags = v
    r = so.rng('warped', *v)
    logits = so.f32(r, groups, n, c, h, w)
    x = row.inp(so.softmax_np(logits, axis=2).astype(np.float32) if flags & so.INPUT_PROBS else logits)
    mats = row.inp(_mats(groups))
    wide = bool(flags & (so.VAR | so.EXACT))
    stats = row.out((so.stats_bytes(n, h * w, c, flags & ~so.INPUT_PROBS) // (8 if wide else 4),), torch.float64 if wide else torch.float32, zeroed=True)
    row.call = lambda s: so.chk(so.lib().rcu_mc_accumulate_warped(so.vp(x), so.vp(stats), n, h, w, c, flags, so.vp(mats), groups, s))
