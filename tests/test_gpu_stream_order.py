"""Every entry point keeps its work on the caller's stream: the protocol and the case table of tests/stream_order.py on the MI355X, then the same
protocol one layer up, on the Python wrappers.  Run with -s to see the delay, the host time it was derived from and every case's query()."""
import pytest
import torch

import stream_order as so
import stream_order_wrappers as sw

pytestmark = pytest.mark.gpu

_hip_errors = []      # a HIP runtime error in one test: nothing more is started on the device


@pytest.fixture(autouse=True)
def stop_after_a_hip_error():
    if _hip_errors:
        pytest.exit('a HIP runtime error was raised earlier ({}): nothing more runs on the GPU'.format(_hip_errors[0]), returncode=3)
    yield


def _note_hip_error(e):
    text = str(e)
    if getattr(e, 'status', 0) == -2 or 'HIP error' in text or 'illegal memory access' in text or 'hipError' in text:
        _hip_errors.append(text[:200])


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def baseline(dev):
    """Every case once, plainly, on the quiet default stream: the expected bytes (kept on the host, shared by the tests and never changed), whether the
    call is bit-repeatable, and the host time the delay is derived from."""
    delay = so.Delay(dev)
    expected, errors, slowest = {}, {}, (0.0, None)
    for name, variant in [(name, variant) for name in sorted(so.CASES) for variant in so.CASES[name].variants]:
        try:
            row = so.build_row(name, variant, dev)
            first, _ = so.run_plain(row)          # (a U-Net row: the first forward of a fresh handle; everywhere: the kernels' code objects load)
            second, host_ms = so.run_plain(row)
            if not so.same_bytes(first, second):
                raise AssertionError('not bit-repeatable on a quiet stream')
            expected[name, variant] = second
            if host_ms > slowest[0]:
                slowest = (host_ms, '{}[{}]'.format(name, variant))
            del row
        except Exception as e:  # noqa: BLE001 - the case's own test reports it
            errors[name, variant] = e
            _note_hip_error(e)
            if _hip_errors:
                break
        torch.cuda.synchronize()
    delay.set_from_host_ms(slowest[0])
    print('\nstream order: slowest host call {:.3f} ms ({}); delay {:.1f} ms by {}'.format(slowest[0], slowest[1], delay.ms, delay.how))
    return dict(expected=expected, errors=errors, delay=delay)


def null_stream_control(dev, baseline, side):
    """rcu_softmax handed the null stream while its inputs arrive on ``side`` behind the delay -> True if the result differs from the expected bytes."""
    variant = so.CASES['rcu_softmax'].variants[0]
    row = so.build_row('rcu_softmax', variant, dev)
    got, _ = so.run_behind_delay(row, side, baseline['delay'], entry_stream=so.c_void_p(0))
    torch.cuda.synchronize()
    return not so.same_bytes(got, baseline['expected']['rcu_softmax', variant])


@pytest.fixture(scope='module')
def side(dev, baseline):
    """A side stream that does not order with the null stream: the machines run with few hardware queues, and two streams can share one."""
    assert ('rcu_softmax', so.CASES['rcu_softmax'].variants[0]) in baseline['expected'], baseline['errors']
    tried = []
    for _ in range(4):
        stream = torch.cuda.Stream()
        tried.append(stream)      # (kept alive: a destroyed stream's queue would be handed out again)
        if null_stream_control(dev, baseline, stream):
            print('stream order: side stream number {} does not order with the null stream'.format(len(tried)))
            return stream
    pytest.fail('the protocol has no power here: a null-stream launch gave the right bytes behind the delay on each of {} side streams'.format(len(tried)))


@pytest.mark.timeout(600)      # (the module's fixtures run here: every case once on the quiet stream)
def test_protocol_detects_a_null_stream_launch(dev, baseline, side):
    assert null_stream_control(dev, baseline, side)


@pytest.mark.timeout(120)
def test_protocol_detects_an_unordered_consumer(dev, baseline, side):
    """A correct rcu_softmax on ``side``, its output read on the default stream without a wait: the reader sees the sentinel."""
    variant = so.CASES['rcu_softmax'].variants[0]
    row = so.build_row('rcu_softmax', variant, dev)
    got, idle = so.run_behind_delay(row, side, baseline['delay'], consumer=torch.cuda.default_stream())
    torch.cuda.synchronize()
    assert not idle
    assert len(got) == 1 and bool((got[0] == so.SENTINEL).all()), 'an unordered reader saw something other than the sentinel'
    assert not so.same_bytes(got, baseline['expected']['rcu_softmax', variant])


@pytest.mark.timeout(120)
@pytest.mark.parametrize('name', sorted(so.CASES))
def test_entry_point_is_ordered_on_its_stream(dev, baseline, side, name):
    failures = []
    for variant in so.CASES[name].variants:
        if (name, variant) in baseline['errors']:
            raise baseline['errors'][name, variant]
        want = baseline['expected'][name, variant]
        row = so.build_row(name, variant, dev)
        for run in (('first', 'warm') if row.warm else ('only',)):
            try:
                got, idle = so.run_behind_delay(row, side, baseline['delay'])
            except Exception as e:
                _note_hip_error(e)
                raise
            print('{}[{}] {}: query() after the return = {}'.format(name, variant, run, idle))
            if not so.same_bytes(got, want):
                bad = [i for i, (a, b) in enumerate(zip(got, want)) if a.shape != b.shape or not torch.equal(a, b)]
                failures.append('{} {}: outputs {} differ from the quiet-stream call'.format(variant, run, bad))
            if idle and name not in so.BLOCKS_THE_HOST:
                failures.append('{} {}: the stream was idle when the call returned (it waited for the stream, or the delay is too short)'.format(variant, run))
        del row
        torch.cuda.synchronize()
    assert not failures, '{}: {}'.format(name, '; '.join(failures))


@pytest.mark.timeout(120)
@pytest.mark.parametrize('name', sorted(sw.WRAPPERS))
def test_python_wrappers_behind_a_busy_stream(dev, baseline, side, name):
    build = sw.WRAPPERS[name]
    try:
        want = sw.run_plain(build(dev))
        again = sw.run_plain(build(dev))
        assert so.same_bytes(want, again), '{}: not bit-repeatable on a quiet stream'.format(name)
        got, idle = sw.run_behind_delay(build(dev), side, baseline['delay'])
    except Exception as e:
        _note_hip_error(e)
        raise
    print('{}: query() after the return = {}'.format(name, idle))
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a.shape != b.shape or not torch.equal(a, b)]
    assert so.same_bytes(got, want), '{}: outputs {} differ from the quiet-stream call'.format(name, bad)
    assert idle is False or name in sw.BLOCKS_THE_HOST, '{}: the stream was idle when the wrapper returned'.format(name)
