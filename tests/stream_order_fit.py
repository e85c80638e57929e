"""The case table of the stream-order protocol (tests/stream_order.py: a delay, poison, sentinel outputs and query()) for the entry points of the
second header, include/rcu_fit.h.  The rows live in a table of their own: tests/stream_order.py's CASES cover include/rcu.h and its stale-row check
would refuse a row for a function that header does not declare."""
import torch

import auxfit_cases as cases
import auxfit_reference as ref
import stream_order as so

CASES = {}


def case(name, variants, hosts=()):
    def register(build):
        assert name not in CASES and name not in so.CASES, name
        CASES[name] = so.Case(build, variants, hosts)
        return build
    return register


def build_row(name, variant, dev):
    row = so.Row(dev)
    CASES[name].build(row, variant)
    assert set(row.hosts) == set(CASES[name].hosts), (name, sorted(row.hosts), CASES[name].hosts)
    return row


# (F, L, pitch): three slices of 1024 + 37 voxels, so that the call is its 2 L + 1 passes over more than one chunk per slice
@case('rcu_postnet_loss_grad', ((32, 3, 32), (8, 1, 64)))
def _postnet_loss_grad(row, v):
    F, L, pitch = v
    n, hw = 3, 1061
    phi, labels, params, _ = cases.make_inputs(11, n, hw, F, L)
    padded = torch.zeros((n * hw, pitch), dtype=torch.float32)
    padded[:, :F] = torch.from_numpy(phi)
    x, lab, par = row.inp(padded), row.inp(labels), row.inp(ref.pack(params, F, L))
    grads, loss = row.out((ref.param_count(F, L),), torch.float32), row.out((1,), torch.float64)
    mean, var = row.out((L, F), torch.float32), row.out((L, F), torch.float32)
    flags = row.out((1,), torch.int32, zeroed=True)      # the caller zeroes the flag word
    ws = row.ws(so.lib().rcu_postnet_fit_workspace_bytes(F, L, n, hw))
    row.call = lambda s: so.chk(so.lib().rcu_postnet_loss_grad(so.vp(x), pitch, F, n, hw, so.vp(lab), L, so.vp(par), so.vp(grads), so.vp(loss),
                                                               so.vp(mean), so.vp(var), so.vp(flags), so.vp(ws), s))
