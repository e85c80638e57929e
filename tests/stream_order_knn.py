"""The case table of the stream-order protocol (tests/stream_order.py: a delay, poison, sentinel outputs and query()) for the entry points of the
third header, include/rcu_knn.h.  The rows live in a table of their own, as those of include/rcu_fit.h do (tests/stream_order_fit.py):
tests/stream_order.py's CASES cover include/rcu.h and its stale-row check would refuse a row for a function that header does not declare."""
import numpy as np
import torch

import knn_reference as ref
import stream_order as so
import stream_order_fit as sof

CASES = {}


def case(name, variants, hosts=()):
    def register(build):
        assert name not in CASES and name not in so.CASES and name not in sof.CASES, name
        CASES[name] = so.Case(build, variants, hosts)
        return build
    return register


def build_row(name, variant, dev):
    row = so.Row(dev)
    CASES[name].build(row, variant)
    assert set(row.hosts) == set(CASES[name].hosts), (name, sorted(row.hosts), CASES[name].hosts)
    return row


# (n, hw, first slice): the slice indices arrive on the stream (poison: slice 0 everywhere, which gives other keys)
@case('rcu_knn_sample_keys', ((3, 1061, 5), (2, 1, 2 ** 32 + 1)))
def _sample_keys(row, v):
    n, hw, first = v
    index = row.inp(torch.arange(first, first + n, dtype=torch.int64))
    keys = row.out((n, hw), torch.int64)
    row.call = lambda s: so.chk(so.lib().rcu_knn_sample_keys(n, hw, so.vp(index), ref.knn_seed(11), so.vp(keys), s))


# (F, pitch, M, k, normalize, with d2): 1061 voxels are three sets of workgroup work and a ragged last group; M = 300 is more than one staged piece
@case('rcu_knn_distances', ((32, 32, 300, 5, 1, True), (5, 8, 33, 8, 0, True), (32, 64, 40, 1, 1, False)))
def _distances(row, v):
    F, pitch, M, k, normalize, with_d2 = v
    r = so.rng('knn', F, M)
    nvox = 1061
    phi = np.maximum(r.normal(0.3, 1.0, (nvox, pitch)), 0.0).astype(np.float32)
    rows, sq = ref.bank_parameters(np.maximum(r.normal(0.3, 1.0, (M, F)), 0.0).astype(np.float32), bool(normalize))
    x, bank, bank_sq = row.inp(phi), row.inp(rows), row.inp(sq)
    score = row.out((nvox,), torch.float32)
    d2 = row.out((nvox, k), torch.float32) if with_d2 else None
    row.call = lambda s: so.chk(so.lib().rcu_knn_distances(so.vp(x), pitch, F, nvox, so.vp(bank), so.vp(bank_sq), M, k, normalize, so.vp(score),
                                                           so.vp(d2), s))
