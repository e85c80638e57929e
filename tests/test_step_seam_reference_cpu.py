"""Pins tests/step_seam_reference.py without a device: against the float32 torch oracle (oracle/summary_oracle.py) at every class count
1..8, against fixture G6, and the properties of the planted input sets that tests/test_gpu_step_seam.py relies on.

The distances to the torch oracle are float32 rounding of the ORACLE (the module under test works in float64); each bound below is the
bound the GPU tests put on the kernels for the same quantity, and the worst distance measured (C = 1..8, seeds 0..7) stands beside it."""
import numpy as np
import pytest
import torch

import step_seam_reference as ref
from oracle import summary_oracle as so

CLASS_COUNTS = tuple(range(1, 9))


def _maxdiff(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)))


def _random_stack(C, seed, T=ref.PASSES, n=2, h=7, w=11):
    """[T, n, C, h, w] float32 probabilities of random logits in [-6, 6] (the float32 softmax torch computes)."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.rand(T, n, C, h, w, generator=g) * 12 - 6
    return logits, torch.softmax(logits, 2)


@pytest.mark.parametrize('C', CLASS_COUNTS)
def test_summary_against_the_torch_oracle(C):
    worst = dict.fromkeys(('softmax', 'probabilities', 'entropy', 'mutual_info', 'variance', 'planes'), 0.0)
    for seed in range(8):
        logits, multi = _random_stack(C, seed)
        worst['softmax'] = max(worst['softmax'], _maxdiff(np.stack([ref.softmax(v) for v in logits.numpy()]), multi.numpy()))
        want = so.multi_prediction_summary(multi, do_mi=True, do_var=True)
        got = ref.summary(multi.numpy())
        for flags in ref.FLAG_SETS:        # the same maps through the statistics planes of every flag set
            planes = ref.statistics_planes(multi.numpy(), flags)
            assert planes.shape == (C * (2 if flags & ref.VAR else 1) + (1 if flags & ref.MI else 0), 2, 7, 11)
            fin = ref.finalise(planes, C, ref.PASSES, flags)
            assert set(fin) == {'probabilities', 'entropy'} | ({'mutual_info'} if flags & ref.MI else set()) | ({'variance'} if flags & ref.VAR else set())
            for k in fin:
                # float64 rounding without RCU_MC_EXACT (measured 1.1e-16); with it T addends each rounded by at most 2^-41 (measured 8.5e-13)
                worst['planes'] = max(worst['planes'], _maxdiff(fin[k], got[k]))
                assert _maxdiff(fin[k], got[k]) <= (2.0 ** -41 * ref.PASSES if flags & ref.EXACT else 1e-14), (flags, k)
            if flags & ref.EXACT:
                scaled = planes * 2.0 ** 40
                assert np.array_equal(scaled, np.round(scaled))
        for k in worst:
            if k in got:
                worst[k] = max(worst[k], _maxdiff(got[k], want[k].numpy()))
    print('C = {}: '.format(C) + ', '.join('{} {:.2e}'.format(k, v) for k, v in worst.items()))
    assert worst['softmax'] <= 1e-6            # measured 2.3e-7 at C = 8 (C = 1: 0)
    assert worst['probabilities'] <= 1e-6      # measured 1.1e-7 at C = 2
    assert worst['entropy'] <= 2e-6            # measured 2.8e-7 at C = 8
    assert worst['mutual_info'] <= 2e-6        # measured 3.3e-7 at C = 7
    assert worst['variance'] <= 1e-7           # measured 2.9e-8 at C = 2


@pytest.mark.parametrize('C', CLASS_COUNTS)
def test_aleatoric_outputs_against_the_torch_oracle(C):
    g = torch.Generator().manual_seed(100 + C)
    logits = torch.rand(2, C, 7, 11, generator=g) * 12 - 6
    raw = torch.randn(2, C, 7, 11, generator=g) * 2
    for is_log in (False, True):
        want = so.aleatoric_outputs(logits, raw, is_log)
        sig = ref.sigma_of(raw.numpy(), is_log)
        rel = float(np.max(np.abs(sig - want['sigma'].numpy()) / np.maximum(1.0, sig)))
        assert rel <= 1e-6, (is_log, rel)      # measured 0 (|raw|) and 5.8e-8 (exp: float32 rounding of the oracle)
        assert _maxdiff(ref.softmax(logits.numpy()), want['probabilities'].numpy()) <= 1e-6        # measured 1.9e-7
        pred, sp = ref.sigma_of_prediction(logits.numpy(), raw.numpy(), is_log)
        assert np.array_equal(pred, logits.argmax(1).numpy().astype(np.uint8))       # continuous logits: no ties
        assert np.array_equal(sp, torch.gather(torch.from_numpy(sig), 1, logits.argmax(1)[:, None])[:, 0].numpy())
        assert np.array_equal(ref.votes(logits.numpy()), (logits.argmax(1) != 0).numpy().astype(np.uint32))
    p = ref.softmax(logits.numpy())
    assert np.array_equal(ref.foreground(p), p[:, 1 if C > 1 else 0])
    assert np.max(np.abs(p.sum(1) - 1.0)) <= 1e-15


def test_fixture_g6(golden):
    """The three cases of g6_mc_summary within the bounds tests/test_gpu_parity.py::test_mc_summary_golden puts on the kernels."""
    g = golden('g6_mc_summary')
    for case in range(3):
        multi = g['multi_{}'.format(case)]
        got = ref.summary(multi)
        fin = ref.finalise(ref.statistics_planes(multi, ref.MI | ref.VAR), multi.shape[2], multi.shape[0], ref.MI | ref.VAR)
        for k, tol in (('probabilities', 1e-6), ('entropy', 2e-6), ('mutual_info', 2e-6), ('variance', 1e-7)):
            want = g['{}_{}'.format(k, case)]
            assert _maxdiff(got[k], want) < tol, (case, k)       # measured: 1.1e-7, 9.5e-8, 1.1e-7, 2.7e-8
            assert _maxdiff(fin[k], want) < tol, (case, k)
    assert _maxdiff(ref.entropy(g['kat_entropy_in'], axis=1), g['kat_entropy_out']) < 1e-6      # measured 9.1e-9


def test_first_maximum_and_vote_plane():
    x = np.array([[[1.0], [3.0], [3.0], [2.0]], [[4.0], [4.0], [1.0], [4.0]], [[0.0], [0.0], [0.0], [0.0]]])      # [3, 4, 1]
    assert ref.first_argmax(x).tolist() == [[1], [0], [0]]
    assert ref.votes(x).tolist() == [[1], [0], [0]]
    plane = ref.vote_plane([x, x, x[::-1].copy()], (0, 31, 32), 2)
    assert plane.dtype == np.uint32 and plane.shape == (2, 3, 1)
    assert plane[0, :, 0].tolist() == [0x80000001, 0, 0] and plane[1, :, 0].tolist() == [0, 0, 1]
    assert ref.votes(np.zeros((2, 1, 3))).sum() == 0          # a single class never votes
    assert np.array_equal(ref.quantise([2.0 ** -41, 1.5 * 2.0 ** -41, 3e-13, 1.0]), [0.0, 2.0 ** -40, 0.0, 1.0])


@pytest.mark.parametrize('C', CLASS_COUNTS)
def test_planted_inputs_have_the_properties_the_gpu_tests_assume(C):
    for name, (n, h, w) in ref.SHAPES.items():
        logits = ref.grid_logits(7 * C, C, n, h, w)
        assert logits.dtype == np.float32 and logits.shape == (ref.PASSES, n, C, h, w)
        assert np.array_equal(ref.grid_logits(7 * C, C, n, h, w), logits)           # seeded
        # no near-ties: two classes of a voxel are equal or at least a grid step apart (float32 values, the shifted rows included)
        assert ref.min_gap(logits) >= ref.GRID
        flat = logits.reshape(ref.PASSES, n, C, h * w).astype(np.float64)
        assert np.array_equal(flat * 8, np.round(flat * 8))
        probs = ref.grid_probabilities(logits)
        assert probs.dtype == np.float32
        pf = probs.reshape(ref.PASSES, n, C, h * w)
        p64 = np.stack([ref.softmax(v) for v in logits]).reshape(pf.shape)
        # the float32 cast keeps the order and the ties of the logits: arg-max of either is one answer, first maximum included
        assert np.array_equal(np.argmax(pf, axis=2), np.argmax(flat, axis=2))
        assert np.array_equal(np.argmax(pf[:, :, ::-1], axis=2), np.argmax(flat[:, :, ::-1], axis=2))
        rows = ref.planted_rows(n, h * w)
        assert set(rows) == set(ref.PLANTED)
        for t in range(ref.PASSES):
            for i, px in rows['equal']:
                assert np.all(flat[t, i, :, px] == flat[t, i, 0, px])
                assert abs(float(ref.entropy(p64[t, i, :, px], axis=0)) - np.log(C)) <= 1e-15       # uniform: H = log C
                assert abs(float(ref.entropy(pf[t, i, :, px], axis=0)) - np.log(C)) <= 2e-7         # and of the float32 cast
            for i, px in rows['tie_1_2']:
                if C >= 3:
                    r = flat[t, i, :, px]
                    assert r[1] == r[2] == r.max() and np.sum(r == r.max()) == 2
                    assert np.argmax(pf[t, i, :, px]) == 1 and pf[t, i, 1, px] == pf[t, i, 2, px]
            for i, px in rows['tie_0']:
                if C >= 2:
                    r = flat[t, i, :, px]
                    assert r[0] == r[C - 1] == r.max()
                    assert np.argmax(pf[t, i, :, px]) == 0 and pf[t, i, 0, px] == pf[t, i, C - 1, px]
            for i, px in rows['saturated']:
                k = t % C
                # float32 p is exactly 1 and 0: e^-120 is below the smallest float32 subnormal
                assert pf[t, i, k, px] == np.float32(1.0) and np.all(np.delete(pf[t, i, :, px], k) == 0.0)
                assert C == 1 or 0.0 < np.delete(p64[t, i, :, px], k).max() < 2.0 ** -149
                assert float(ref.entropy(pf[t, i, :, px], axis=0)) == 0.0            # the p > 0 guard
                with np.errstate(over='ignore', under='ignore'):
                    e32 = np.exp(logits.reshape(flat.shape)[t, i, :, px] - np.float32(60.0))
                assert e32.dtype == np.float32 and np.all(np.delete(e32, k) == 0.0)  # what a float32 kernel's exp gives
            for i, px in rows['shifted']:
                assert flat[t, i, :, px].min() >= 10000 - 6 and np.isfinite(p64[t, i, :, px]).all()
                assert abs(p64[t, i, :, px].sum() - 1.0) <= 1e-15
        raw = ref.raw_sigma(3 * C, C, n, h, w)
        assert raw.dtype == np.float32 and raw.shape == (n, C, h, w)
        rf = raw.reshape(n, C, -1)
        assert np.all(rf[0, :, 0] == 0) and np.all(np.signbit(rf[0, :, 1])) and np.all(rf[0, :, 2] < 0) and (rf < 0).mean() > 0.3
        assert np.all(ref.sigma_of(raw) >= 0) and np.all(ref.sigma_of(raw, True) > 0) and np.all(ref.sigma_of(rf[0, :, :2], True) == 1.0)
    assert ref.SHAPES['one_voxel'][1] * ref.SHAPES['one_voxel'][2] % 4 != 0 and ref.SHAPES['four_wide'][1] * ref.SHAPES['four_wide'][2] % 4 == 0


def test_the_torch_oracle_stays_inside_half_of_every_bound_on_the_planted_inputs():
    """The bounds of the finalised maps in tests/test_gpu_step_seam.py are fixture G6's.  They stay as they are because the float32 torch
    oracle itself, on the planted inputs at C = 8, uses less than half of each (else the bound would be four times the oracle's distance)."""
    C = 8
    worst = dict.fromkeys(('probabilities', 'entropy', 'mutual_info', 'variance'), 0.0)
    for n, h, w in ref.SHAPES.values():
        logits = ref.grid_logits(7 * C, C, n, h, w)
        for multi in (torch.softmax(torch.from_numpy(logits), 2), torch.from_numpy(ref.grid_probabilities(logits))):
            want = so.multi_prediction_summary(multi, do_mi=True, do_var=True)
            got = ref.summary(np.stack([ref.softmax(v) for v in logits]))
            for k in worst:
                worst[k] = max(worst[k], _maxdiff(got[k], want[k].numpy()))
    print(', '.join('{} {:.2e}'.format(k, v) for k, v in worst.items()))
    assert worst['probabilities'] <= 0.5 * 1e-6        # measured 7.7e-8
    assert worst['entropy'] <= 0.5 * 2e-6              # measured 3.1e-7
    assert worst['mutual_info'] <= 0.5 * 2e-6          # measured 4.1e-7
    assert worst['variance'] <= 0.5 * 1e-7             # measured 2.2e-8
