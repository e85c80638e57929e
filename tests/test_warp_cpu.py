"""The affine test-time augmentation without a GPU: the float64 restatement of include/rcu_warp.h (tests/warp_reference.py) against the torch
witness of tests/golden/g38_warp.npz; the fourth header's symbols, its argument validation and the untouched first three headers; the
stream-order table of the fourth header; the host side of rcu_amd.steps (matrices, inverse, the seeded draw, the mask keys, the step's
refusals); the ``others.tta_affine`` row of the scripts and every refusal by name."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import warp_reference as ref
from test_density_scripts_cpu import _context, _yaml_with
from test_stream_order_cpu import prototypes, stream_entry_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARP_NAMES = ('rcu_warp_affine', 'rcu_mc_accumulate_warped')


@pytest.fixture(scope='module')
def g38(golden):
    return golden('g38_warp')


# ------------------------------------------------------------------------------------------------------------------ the definition
def test_reference_with_float64_weights_is_within_1e_12_of_torch(g38):
    worst = 0.0
    for k in range(len(g38['shapes'])):
        x = g38['x_{}'.format(k)]
        for m, M in enumerate(g38['mats']):
            got = ref.warp(x, M, weights='float64')
            worst = max(worst, float(np.abs(got - g38['torch_{}_{}'.format(k, m)]).max() / np.abs(x).max()))
    print('float64 weights against grid_sample: {:.3g} of max|x|'.format(worst))
    assert worst <= 1e-12


def test_reference_with_the_definitions_weights_reproduces_the_fixture_exactly(g38):
    assert [tuple(s) for s in g38['shapes']] == [(15, 17), (32, 48), (1, 1), (33, 33), (24, 40)] and g38['mats'].shape == (4, 2, 3)
    for k in range(len(g38['shapes'])):
        x = g38['x_{}'.format(k)]
        assert x.dtype == np.float32
        for m, M in enumerate(g38['mats']):
            want = g38['ref_{}_{}'.format(k, m)]
            got = ref.warp(x, M)
            assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), (k, m)
            # the float32 weights move the value by no more than their rounding: 2 * 2^-24 of the taps' spread, far inside the device bound
            assert np.abs(want - g38['torch_{}_{}'.format(k, m)]).max() <= 4 * ref.U * np.abs(x).max()


def test_the_taps_are_the_definitions():
    t = ref.taps(ref.IDENTITY, 5, 7)
    assert np.array_equal(t['i0'], np.arange(5)[:, None] + np.zeros((1, 7), int)) and np.array_equal(t['j0'], np.arange(7)[None] + np.zeros((5, 1), int))
    assert not t['fy'].any() and not t['fx'].any() and t['fy'].dtype == np.float32
    assert t['i1'].max() == 4 and t['j1'].max() == 6      # the upper tap is clamped, its weight is zero
    # a half-pixel shift: weight one half away from the border, the border itself replicated
    t = ref.taps(ref.matrix(0.0, 1.0, 0.5, -0.5), 4, 4)
    assert np.array_equal(t['fy'][:-1], np.full((3, 4), 0.5, np.float32)) and not t['fy'][-1].any() and np.array_equal(t['i0'][-1], [3, 3, 3, 3])
    assert np.array_equal(t['j0'][0], [0, 0, 1, 2]) and np.array_equal(t['fx'][0], np.array([0, 0.5, 0.5, 0.5], np.float32))
    # 45 degrees / 1.3 on 15 x 17: the corners leave the plane and are clamped (a border pixel at weight zero), the centre is not
    t = ref.taps(ref.matrix(45.0, 1.3), 15, 17)
    clamped = ((t['i0'] == 0) & (t['fy'] == 0)) | (t['i0'] == 14) | ((t['j0'] == 0) & (t['fx'] == 0)) | (t['j0'] == 16)
    assert clamped[0, 0] and clamped[0, -1] and clamped[-1, 0] and clamped[-1, -1] and not clamped[4:11, 5:12].any() and clamped.mean() > 0.02


def test_integer_tap_matrices_are_the_d4_gathers():
    from rcu_amd import steps
    x = torch.randn(2, 3, 6, 6, generator=torch.Generator().manual_seed(3))
    for e in range(8):
        assert np.array_equal(np.array(steps.TTA_AFFINE[e], dtype=np.float64), ref.D4[e])
        assert ref.warp(x.numpy(), ref.D4[e]).astype(np.float32).tobytes() == steps.tta_torch(x, e).contiguous().numpy().tobytes(), e
        t = ref.taps(ref.D4[e], 6, 6)
        assert not t['fx'].any() and not t['fy'].any()
    y = torch.randn(2, 5, 8, generator=torch.Generator().manual_seed(4))
    for e in range(4):      # the flips on any plane
        assert np.array_equal(ref.warp(y.numpy(), ref.D4[e]), steps.tta_torch(y, e).numpy().astype(np.float64)), e


def test_the_float32_chain_stays_inside_the_bound():
    """The bound of include/rcu_warp.h, 12 u max|tap|, holds for a float32 emulation of the chain on the CPU (the GPU test holds the kernel to it)."""
    rng = np.random.default_rng(38)
    worst = 0.0
    for h, w in ((15, 17), (64, 64), (32, 48)):
        x = rng.standard_normal((4, h, w)).astype(np.float32)
        for M in (ref.matrix(10.0, 1.1, 1.5, -2.25), ref.matrix(-25.0, 0.85, flip=True), ref.matrix(45.0, 1.3)):
            want, tap = ref.warp(x, M, return_max_tap=True)
            worst = max(worst, float((np.abs(ref.warp_float32(x, M) - want) / (ref.U * np.maximum(tap, 1e-30))).max()))
    print('float32 emulation: {:.2f} of the {} u'.format(worst, ref.WARP_BOUND_ULPS))
    assert 0.5 < worst <= ref.WARP_BOUND_ULPS


# ------------------------------------------------------------------------------------------------------------------ C ABI
def _header(name):
    with open(os.path.join(ROOT, 'include', name)) as f:
        return f.read()


def test_the_fourth_header_declares_what_the_library_exports():
    from rcu_amd import _lib
    text = _header('rcu_warp.h')
    declared = dict(prototypes(text))
    assert set(declared) == set(WARP_NAMES) == set(_lib.WARP_SIGNATURES)
    lib = _lib.load()
    for name in WARP_NAMES:
        assert hasattr(lib, name), name
        assert name not in _lib.SIGNATURES and name not in _lib.FIT_SIGNATURES and name not in _lib.KNN_SIGNATURES, name
        assert len(declared[name]) == len(_lib.WARP_SIGNATURES[name][1]) and declared[name][-1] == 'void* stream', name
        assert getattr(lib, name).argtypes == _lib.WARP_SIGNATURES[name][1] and _lib.WARP_SIGNATURES[name][0] is ctypes.c_int
    assert [p.split()[-1] for p in declared['rcu_warp_affine']] == ['x_dev', 'n', 'channels', 'height', 'width', 'mats_dev', 'n_mats', 'out_dev', 'stream']
    assert [p.split()[-1] for p in declared['rcu_mc_accumulate_warped']] == ['in_dev', 'stats_dev', 'n', 'height', 'width', 'nb_classes', 'flags',
                                                                             'mats_dev', 'groups', 'stream']
    # pointer and size types, position by position
    kinds = {'size_t': ctypes.c_size_t, 'int': ctypes.c_int}
    for name in WARP_NAMES:
        for decl, argtype in zip(declared[name], _lib.WARP_SIGNATURES[name][1]):
            assert argtype is (ctypes.c_void_p if '*' in decl else kinds[decl.split()[0]]), (name, decl)
    assert '#include "rcu.h"' in text and 'Affine test-time augmentation' in text
    assert re.search(r'#define RCU_WARP_MAX_MATRICES 64\b', text) and _lib.RCU_WARP_MAX_MATRICES == 64
    for other in ('rcu.h', 'rcu_fit.h', 'rcu_knn.h'):      # the first three headers gained nothing
        assert 'rcu_warp' not in _header(other) and 'accumulate_warped' not in _header(other)
    assert set(n for n, _ in prototypes(_header('rcu.h'))) == set(_lib.SIGNATURES)
    assert set(n for n, _ in prototypes(_header('rcu_fit.h'))) == set(_lib.FIT_SIGNATURES)
    assert set(n for n, _ in prototypes(_header('rcu_knn.h'))) == set(_lib.KNN_SIGNATURES)
    makefile = open(os.path.join(ROOT, 'reliability-challenges-uncertainty_amd', 'csrc', 'Makefile')).read()
    assert 'rcu_warp.hip' in makefile and '../../include/rcu_warp.h' in makefile
    entry = open(os.path.join(ROOT, '__graft_entry__.py')).read()
    assert 'WARP_SIGNATURES' in entry


def test_every_stream_taking_prototype_of_the_fourth_header_has_a_row():
    import stream_order as so
    import stream_order_fit as sof
    import stream_order_knn as sok
    import stream_order_warp as sow
    found = stream_entry_points(_header('rcu_warp.h'))
    assert sorted(found) == sorted(WARP_NAMES) == sorted(sow.CASES) and all(hosts == [] for hosts in found.values())
    assert all(len(case.variants) >= 2 and callable(case.build) and case.hosts == () for case in sow.CASES.values())
    assert not set(sow.CASES) & (set(so.CASES) | set(so.EXEMPT) | set(sof.CASES) | set(sok.CASES)), 'the rows of the fourth header live in a table of their own'


def test_arguments_are_checked_without_a_device():
    from rcu_amd import _lib
    lib = _lib.load()
    p, q = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)      # never dereferenced: every call below is refused first

    def warp(x=p, n=2, channels=4, h=15, w=17, mats=p, n_mats=1, out=q):
        status = lib.rcu_warp_affine(x, n, channels, h, w, mats, n_mats, out, None)
        return status, lib.rcu_last_error().decode()

    for kw, word in ((dict(x=None), 'null argument'), (dict(mats=None), 'null argument'), (dict(out=None), 'null argument'),
                     (dict(n_mats=0), 'n_mats must be in 1..64, got 0'), (dict(n_mats=65), 'n_mats must be in 1..64, got 65'),
                     (dict(n=0), 'empty batch or plane'), (dict(h=0), 'empty batch or plane'), (dict(w=0), 'empty batch or plane'),
                     (dict(h=1 << 15, w=(1 << 15) + 1), 'plane larger than 2\\^30 pixels'), (dict(channels=0), 'channels must be >= 1'),
                     (dict(out=p), 'out must not overlap x'), (dict(out=ctypes.c_void_p((1 << 20) + 64)), 'out must not overlap x'),
                     (dict(x=ctypes.c_void_p((1 << 30) + 2 * 2 * 4 * 15 * 17 * 4 - 4), n_mats=2), 'out must not overlap x')):
        status, message = warp(**kw)
        assert status == _lib.RCU_ERR_INVALID and re.search(word, message) and message.startswith('rcu_warp_affine: '), (kw, message)

    def accumulate(inp=p, stats=q, n=2, h=15, w=17, c=4, flags=_lib.RCU_MC_EXACT, mats=p, groups=1):
        status = lib.rcu_mc_accumulate_warped(inp, stats, n, h, w, c, flags, mats, groups, None)
        return status, lib.rcu_last_error().decode()

    for kw, word in ((dict(inp=None), 'null argument'), (dict(stats=None), 'null argument'), (dict(mats=None), 'null argument'),
                     (dict(groups=0), 'groups must be in 1..64, got 0'), (dict(groups=65), 'groups must be in 1..64, got 65'),
                     (dict(n=0), 'empty batch or plane'), (dict(h=0), 'empty batch or plane'), (dict(w=-1), 'empty batch or plane'),
                     (dict(h=(1 << 15) + 1, w=1 << 15), 'plane larger than 2\\^30 pixels'), (dict(c=0), 'nb_classes must be in 1..8'),
                     (dict(c=9), 'nb_classes must be in 1..8'), (dict(flags=16), 'flags must be a combination .* got 16'), (dict(flags=-1), 'flags')):
        status, message = accumulate(**kw)
        assert status == _lib.RCU_ERR_INVALID and re.search(word, message) and message.startswith('rcu_mc_accumulate_warped: '), (kw, message)


# ------------------------------------------------------------------------------------------------------------------ the host side of the step
def test_affine_matrix_and_inverse():
    from rcu_amd import steps
    assert np.array_equal(steps.affine_matrix(), ref.IDENTITY) and np.array_equal(np.array(steps.AFFINE_IDENTITY), ref.IDENTITY)
    assert np.array_equal(steps.affine_matrix(flip=True), ref.D4[1])
    for args in ((10.0, 1.1, 1.5, -2.25, False), (-25.0, 0.85, 0.0, 0.0, True), (45.0, 1.3, 0.0, 0.0, False), (3.0, 0.9, -4.0, 7.5, True)):
        M = steps.affine_matrix(*args)
        assert M.dtype == np.float64 and M.shape == (2, 3) and M.tobytes() == ref.matrix(*args).tobytes()
        # R(rotation) / scale, the second column negated for flip, the shifts in the last column
        assert np.allclose(np.hypot(M[0, 0], M[1, 0]), 1.0 / args[1], rtol=1e-15) and np.sign(np.linalg.det(M[:, :2])) == (-1 if args[4] else 1)
        assert M[0, 2] == args[2] and M[1, 2] == args[3]
        inv = steps.affine_inverse(M)
        both = np.vstack([M, [0, 0, 1]]) @ np.vstack([inv, [0, 0, 1]])
        assert np.abs(both - np.eye(3)).max() < 1e-14 and np.abs(inv - ref.inverse(M)).max() < 1e-14
        assert np.abs(steps.affine_inverse(inv) - M).max() < 1e-14
    for e, back in enumerate(steps.TTA_INVERSE):      # integer taps invert exactly, to the inverse element
        assert np.array_equal(steps.affine_inverse(ref.D4[e]), ref.D4[back]), e
    for bad in ([[1, 2, 0], [2, 4, 0]], [[0, 0, 1], [0, 0, 1]], [[1e-200, 0, 0], [0, 1e-200, 0]]):
        with pytest.raises(ValueError, match='singular'):
            steps.affine_inverse(bad)
    for bad in ([[1, 0, float('nan')], [0, 1, 0]], [[float('inf'), 0, 0], [0, 1, 0]]):
        with pytest.raises(ValueError, match='finite'):
            steps.affine_inverse(bad)
    with pytest.raises(ValueError, match='scale'):
        steps.affine_matrix(scale=0.0)


def test_the_draw_is_a_function_of_seed_and_transform():
    from rcu_amd import steps
    opts = dict(rotation=10.0, scale=0.1, shift=2.0, flip=True)
    full = steps.affine_tta_draw(20, 64, **opts)
    assert full.shape == (64, 2, 3) and full.dtype == np.float64 and np.array_equal(full[0], ref.IDENTITY)
    for count in (1, 2, 7):      # transform v does not depend on how many are drawn
        assert steps.affine_tta_draw(20, count, **opts).tobytes() == full[:count].tobytes()
    assert steps.affine_tta_draw(20, 64, **opts).tobytes() == full.tobytes()
    other = steps.affine_tta_draw(21, 64, **opts)
    assert all(not np.array_equal(other[v], full[v]) for v in range(1, 64))
    assert len({full[v].tobytes() for v in range(64)}) == 64
    # the ranges
    lin = full[:, :, :2]
    det = np.linalg.det(lin)
    mag = 1.0 / np.sqrt(np.abs(det))                                   # the magnification: log2 uniform in +-log2(1.1)
    assert (mag <= 1.1 * (1 + 1e-12)).all() and (mag >= (1 / 1.1) * (1 - 1e-12)).all() and mag[1:].min() < 0.95 and mag[1:].max() > 1.05
    angle = np.degrees(np.arctan2(lin[:, 1, 0], lin[:, 0, 0]))          # first column: (cos, sin) / scale, whatever the flip
    assert (np.abs(angle) <= 10.0 + 1e-9).all() and angle.min() < -5 and angle.max() > 5
    assert (np.abs(full[:, :, 2]) <= 2.0).all() and np.abs(full[1:, :, 2]).max() > 1.5
    flips = det[1:] < 0
    assert 15 <= flips.sum() <= 48 and det[0] > 0                      # a fair coin over 63 draws
    assert (np.linalg.det(steps.affine_tta_draw(20, 64, rotation=10.0, scale=0.1, shift=2.0, flip=False)[:, :, :2]) > 0).all()
    # the uniforms: ((x >> 11) + 0.5) * 2^-53 of SplitMix64 -- never 0 or 1
    u = [steps._affine_uniform(20, v, e) for v in range(1, 64) for e in range(5)]
    assert 0.0 < min(u) < 0.02 and 0.98 < max(u) < 1.0 and abs(float(np.mean(u)) - 0.5) < 0.06
    # all amplitudes zero: every transform is the identity
    assert all(np.array_equal(m, ref.IDENTITY) for m in steps.affine_tta_draw(5, 4))
    for bad in (0, 65):
        with pytest.raises(ValueError, match='samples must be in 1..64'):
            steps.affine_tta_draw(20, bad, **opts)
    for name in ('rotation', 'scale', 'shift'):
        with pytest.raises(ValueError, match=name):
            steps.affine_tta_draw(20, 4, **dict(opts, **{name: -1.0}))


def test_the_mask_keys_are_disjoint_from_every_other_family():
    from rcu_amd import corruption, knn, steps
    for seed in (0, 20, 2 ** 31 - 2):
        passes = (1, 2, 3, 1023, 1024, 2047, 2048)
        assert all(steps.affine_pass_seed(seed, 0, t) == steps.pass_seed(seed, t) for t in passes)
        mine = {steps.affine_pass_seed(seed, v, t) for v in range(1, 64) for t in range(1, 2049)}
        assert len(mine) == 63 * 2048
        others = {steps.pass_seed(seed, t) for t in range(0, 2049)}
        others |= {steps.tta_pass_seed(seed, e, t) for e in range(8) for t in range(1, 2049)}
        others |= {corruption.corruption_seed(seed, s) for s in range(8)}
        others.add(knn.knn_seed(seed))
        assert not mine & others
        # the steps of 2^40: 65 .. 127 above the pass's own key
        assert steps.affine_pass_seed(seed, 1, 1) - steps.pass_seed(seed, 1) == 65 << 40
        assert steps.affine_pass_seed(seed, 63, 2048) - steps.pass_seed(seed, 2048) == 127 << 40
    for bad in (-1, 64):
        with pytest.raises(ValueError, match='transform index'):
            steps.affine_pass_seed(20, bad, 1)
    assert 'disjoint' in steps.affine_pass_seed.__doc__ or 'no key of one family equals a key of another' in steps.affine_pass_seed.__doc__


def test_the_step_refuses_what_it_cannot_run():
    from rcu_amd import steps
    from rcu_amd.model import UNet
    step = steps.AffineTtaMcPredictStep(4, mc_steps=5, seed=20, rotation=10.0, scale=0.1, shift=2.0, flip=True)
    assert step.transforms == 4 and step.samples == 20 and step.exact and np.array_equal(step.matrices[0], ref.IDENTITY)
    assert step.matrices.tobytes() == steps.affine_tta_draw(20, 4, 10.0, 0.1, 2.0, True).tobytes()
    assert all(np.abs(steps.affine_inverse(m) - i).max() == 0 for m, i in zip(step.matrices, step.inverses))
    assert steps.AffineTtaMcPredictStep(64, mc_steps=33, seed=1).exact is False and steps.AffineTtaMcPredictStep(64, mc_steps=32, seed=1).exact
    explicit = steps.AffineTtaMcPredictStep(matrices=[ref.IDENTITY, ref.D4[1]])
    assert explicit.transforms == 2 and explicit.samples == 2 and steps.AffineTtaMcPredictStep(2, matrices=[ref.IDENTITY, ref.D4[1]]).transforms == 2
    for bad in (0, 65, 2.5, True, None):
        with pytest.raises(ValueError, match='samples'):
            steps.AffineTtaMcPredictStep(bad, seed=1)
    with pytest.raises(ValueError, match='samples'):
        steps.AffineTtaMcPredictStep(3, matrices=[ref.IDENTITY])
    with pytest.raises(ValueError, match='matrices.*singular'):
        steps.AffineTtaMcPredictStep(matrices=[ref.IDENTITY, [[1, 2, 0], [2, 4, 0]]])
    with pytest.raises(ValueError, match='matrices.*finite'):
        steps.AffineTtaMcPredictStep(matrices=[[[1, 0, float('nan')], [0, 1, 0]]])
    with pytest.raises(ValueError, match='matrices'):
        steps.AffineTtaMcPredictStep(matrices=[ref.IDENTITY] * 65)
    with pytest.raises(ValueError, match='mc_steps'):
        steps.AffineTtaMcPredictStep(2, mc_steps=-1, seed=1)
    batch = steps.BatchContext({'images': torch.zeros(1, 4, 32, 32)}, 0, 0)
    with pytest.raises(ValueError, match='model.*UNet'):
        step(batch, None, steps.TorchTestContext('cpu', torch.nn.Conv2d(4, 2, 1)))
    with pytest.raises(ValueError, match='model.*sigma'):
        step(batch, None, steps.TorchTestContext('cpu', UNet(2, 4, depth=2, start_filters=8, sigma_out=True)))
    with pytest.raises(ValueError, match='finite'):
        steps.warp_affine(torch.zeros(1, 1, 4, 4), [[1, 0, float('inf')], [0, 1, 0]])


# ------------------------------------------------------------------------------------------------------------------ scripts
def _no_world(monkeypatch):
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)


KEY = dict(samples=4, rotation=10.0, scale=0.1, shift=2.0, flip=True)
KEY_YAML = '    tta_affine: {samples: 4, rotation: 10.0, scale: 0.1, shift: 2.0, flip: true}\n'


def test_the_key_is_a_row_of_the_one_table_and_its_absence_changes_nothing():
    from rcu_amd import distributed as rdist
    from rcu_amd import scripts, steps
    names = [row.name for row in scripts._OTHERS]
    assert names.count('tta_affine') == 1
    row = next(row for row in scripts._OTHERS if row.name == 'tta_affine')
    assert row.scripts == frozenset(('default',))
    owners = [other for owner, other, _ in scripts._RULES if owner == 'tta_affine']
    assert owners[:6] == ['tta', 'agreement', 'mc_adaptive', 'density', 'laplace', 'knn'] and owners[6] is scripts._sharded and len(owners) == 7
    assert not any(other == 'tta_affine' for _, other, _ in scripts._RULES)

    world = rdist.World()
    assert scripts._tta_affine(_context(dict()), world) is None and scripts._tta_affine(_context(dict(mc=20)), world) is None
    plain = scripts._default_steps(_context(dict()), world)
    assert [type(s) for s in plain] == [steps.SegmentationPredictStep] and plain[0].do_probs
    assert [type(s) for s in scripts._default_steps(_context(dict(mc=20)), world)] == [steps.McPredictStep, steps.MultiPredictionSummary]
    assert [type(s) for s in scripts._default_steps(_context(dict(tta=['identity', 'flip_h'])), world)] == [steps.TtaMcPredictStep,
                                                                                                           steps.MultiPredictionSummary]

    # alone: eval mode, no weight-scaling pass; with others.mc: V x T seeded passes and the weight-scaling pass
    for others, mc in ((dict(tta_affine=KEY), 0), (dict(tta_affine=KEY, mc=2), 2), (dict(tta_affine=KEY, mc=2, agreement=False), 2),
                       (dict(tta_affine=KEY, temperature=1.5, corruption=[dict(kind='gaussian_noise', severity=5)]), 0)):
        built, record = scripts._tta_affine(_context(others), world)
        assert [type(s) for s in built] == [steps.AffineTtaMcPredictStep, steps.MultiPredictionSummary]
        step = built[0]
        assert (step.transforms, step.mc_steps, step.seed, step.ws_pass, step.exact) == (4, mc, 20, mc > 0, True)
        assert step.matrices.tobytes() == steps.affine_tta_draw(20, 4, 10.0, 0.1, 2.0, True).tobytes()
        assert record == dict(seed=20, samples=4, mc=mc, rotation=10.0, scale=0.1, shift=2.0, flip=True, matrices=step.matrices.tolist())
        assert record['matrices'][0] == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
        plan = scripts._default_plan(_context(others), world, affine_steps=built)
        assert plan == (built, (), [])
    assert scripts._tta_affine(_context(dict(tta_affine=dict(samples=3)), seed=None), world)[1]['seed'] == 0
    assert scripts._tta_affine(_context(dict(tta_affine=dict(samples=2), group_pixels=1234, exact=False)), world)[0][0].group_pixels == 1234
    hook = scripts.TtaAffineRecordHook(dict(a=1))
    assert hook.file_name == 'tta_affine.json' and isinstance(hook, scripts.CorruptionRecordHook)


@pytest.mark.parametrize('key, value', [('tta', ['identity', 'flip_h']), ('agreement', True), ('mc_adaptive', dict(check_at=[5], tolerance=0.01)),
                                        ('density', 'density.npz'), ('laplace', 'laplace.npz'), ('knn', 'knn.npz')])
def test_the_key_does_not_compose_with_the_keys_of_its_rules(key, value):
    from rcu_amd import distributed as rdist
    from rcu_amd import scripts
    with pytest.raises(ValueError, match='others.tta_affine does not compose with others.{}'.format(key)):
        scripts._tta_affine(_context({'tta_affine': KEY, 'mc': 20, key: value}), rdist.World())


def test_a_multi_rank_launch_and_malformed_options_are_refused_by_key():
    from rcu_amd import distributed as rdist
    from rcu_amd import scripts
    with pytest.raises(ValueError, match='others.tta_affine is not sharded'):
        scripts._tta_affine(_context(dict(tta_affine=KEY, mc=2)), rdist.World(rank=0, world=2))
    world = rdist.World()
    for bad, word in ((4, 'must be a mapping'), (dict(rotation=10.0), 'must be a mapping with samples'), (dict(samples=4, angle=3), 'must be a mapping'),
                      (dict(samples=0), 'samples'), (dict(samples=65), 'samples'), (dict(samples=2.5), 'samples'), (dict(samples=4, flip=1), 'flip'),
                      (dict(samples=4, rotation=-1.0), 'rotation'), (dict(samples=4, scale='big'), 'could not convert'),
                      (dict(samples=4, shift=float('nan')), 'shift')):
        with pytest.raises(ValueError, match='others.tta_affine.*' + word):
            scripts._tta_affine(_context(dict(tta_affine=bad)), world)


@pytest.mark.parametrize('others, word', [(KEY_YAML + '    tta: [identity, flip_h]\n', 'others.tta_affine does not compose with others.tta'),
                                          (KEY_YAML + '    mc: 20\n    agreement: true\n', 'others.tta_affine does not compose with others.agreement'),
                                          (KEY_YAML + '    density: d.npz\n', 'others.tta_affine does not compose with others.density'),
                                          (KEY_YAML + '    knn: k.npz\n', 'others.tta_affine does not compose with others.knn'),
                                          (KEY_YAML + '    laplace: l.npz\n', 'others.tta_affine does not compose with others.laplace'),
                                          ('    tta_affine: {samples: 0}\n', 'others.tta_affine: samples')])
def test_default_script_refuses_before_it_touches_anything(tmp_path, monkeypatch, others, word):
    from rcu_amd import scripts
    _no_world(monkeypatch)
    with pytest.raises(ValueError, match=word):
        scripts.test_default('brats', _yaml_with(tmp_path, others), None, device='cpu')
    assert not (tmp_path / 'out').exists()


def test_default_script_refuses_a_two_rank_launch_by_key(monkeypatch):
    from rcu_amd import distributed as rdist
    from rcu_amd import scripts
    monkeypatch.setattr(scripts, '_context', lambda device, config_file: (_context(dict(tta_affine=KEY, mc=2)), rdist.World(rank=0, world=2)))
    with pytest.raises(ValueError, match='others.tta_affine is not sharded'):
        scripts.test_default('brats', 'unused.yaml', None, device='cpu')


@pytest.mark.parametrize('script', ['test_ensemble', 'test_aleatoric', 'test_auxiliary_feat', 'test_auxiliary_segm', 'fit_temperature', 'fit_density',
                                    'fit_laplace', 'fit_auxiliary_feat', 'fit_knn'])
def test_other_scripts_refuse_the_key(tmp_path, monkeypatch, script):
    from rcu_amd import scripts
    _no_world(monkeypatch)
    path = _yaml_with(tmp_path, '    model_dir: [{}]\n'.format(tmp_path / 'train' / 'model_x') + KEY_YAML)
    with pytest.raises(ValueError, match='others.tta_affine'):
        if script.startswith('fit_'):
            getattr(scripts, script)('brats', str(path), device='cpu')
        else:
            getattr(scripts, script)('brats', config_file=str(path), device='cpu')
    assert not (tmp_path / 'out').exists()
