"""The entry points of include/rcu_warp.h keep their work on the caller's stream: the protocol of tests/stream_order.py on the rows of
tests/stream_order_warp.py.  The side stream is proven not to order with the null stream by the rcu_softmax control of the first table."""
import pytest
import torch

import stream_order as so
import stream_order_warp as sow

pytestmark = pytest.mark.gpu
CONTROL = 'rcu_softmax'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def baseline(dev):
    """Every row (and the control) twice on the quiet default stream: the expected bytes, bit-repeatable, and the host time the delay comes from."""
    delay = so.Delay(dev)
    expected, slowest = {}, 0.0
    rows = [(sow.build_row, name, variant) for name in sorted(sow.CASES) for variant in sow.CASES[name].variants]
    rows.append((so.build_row, CONTROL, so.CASES[CONTROL].variants[0]))
    for build, name, variant in rows:
        row = build(name, variant, dev)
        first, _ = so.run_plain(row)
        second, host_ms = so.run_plain(row)
        assert so.same_bytes(first, second), '{}[{}]: not bit-repeatable on a quiet stream'.format(name, variant)
        expected[name, variant] = second
        slowest = max(slowest, host_ms)
        torch.cuda.synchronize()
    delay.set_from_host_ms(slowest)
    print('\nstream order (rcu_warp.h): slowest host call {:.3f} ms; delay {:.1f} ms by {}'.format(slowest, delay.ms, delay.how))
    return dict(expected=expected, delay=delay)


def null_stream_control(dev, baseline, side):
    variant = so.CASES[CONTROL].variants[0]
    got, _ = so.run_behind_delay(so.build_row(CONTROL, variant, dev), side, baseline['delay'], entry_stream=so.c_void_p(0))
    torch.cuda.synchronize()
    return not so.same_bytes(got, baseline['expected'][CONTROL, variant])


@pytest.fixture(scope='module')
def side(dev, baseline):
    tried = []
    for _ in range(4):
        stream = torch.cuda.Stream()
        tried.append(stream)      # (kept alive: a destroyed stream's queue would be handed out again)
        if null_stream_control(dev, baseline, stream):
            return stream
    pytest.fail('the protocol has no power here: a null-stream launch gave the right bytes behind the delay on each of {} side streams'.format(len(tried)))


@pytest.mark.parametrize('name', sorted(sow.CASES))
def test_entry_point_is_ordered_on_its_stream(dev, baseline, side, name):
    failures = []
    for variant in sow.CASES[name].variants:
        want = baseline['expected'][name, variant]
        got, idle = so.run_behind_delay(sow.build_row(name, variant, dev), side, baseline['delay'])
        print('{}[{}]: query() after the return = {}'.format(name, variant, idle))
        if not so.same_bytes(got, want):
            bad = [i for i, (a, b) in enumerate(zip(got, want)) if a.shape != b.shape or not torch.equal(a, b)]
            failures.append('{}: outputs {} differ from the quiet-stream call'.format(variant, bad))
        if idle:
            failures.append('{}: the stream was idle when the call returned (it waited for the stream, or the delay is too short)'.format(variant))
        torch.cuda.synchronize()
    assert not failures, '{}: {}'.format(name, '; '.join(failures))


def test_a_null_stream_launch_of_the_warped_accumulate_would_be_seen(dev, baseline, side):
    """The control on the new row itself: handed the null stream while its inputs arrive on the side stream, the call reads poison."""
    name = 'rcu_mc_accumulate_warped'
    variant = sow.CASES[name].variants[0]
    got, _ = so.run_behind_delay(sow.build_row(name, variant, dev), side, baseline['delay'], entry_stream=so.c_void_p(0))
    torch.cuda.synchronize()
    assert not so.same_bytes(got, baseline['expected'][name, variant])
