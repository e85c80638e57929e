"""No device: the table of tests/capped_launches.py against the caps in the kernel sources, and the reference side of the PostNet tests -- the
float64 chain of tests/postnet_reference.py against the float64 torch oracle, and the float32 torch oracle within the derived bound on every
PostNet case the GPU tests run (a bound that the reference itself breaks is wrong)."""
import os
import re

import numpy as np
import pytest
import torch

import capped_launches as cl
import postnet_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'reliability-challenges-uncertainty_amd', 'csrc')


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(name, pattern):
    found = re.findall(pattern, _source(name))
    assert len(found) == 1, (name, pattern, found)
    return found[0]


def test_the_caps_of_the_table_are_the_caps_of_the_sources():
    assert int(_one('rcu_temperature.hip', r'constexpr unsigned TN_MAX_GROUPS = (\d+);')) == cl.TN_MAX_GROUPS
    assert int(_one('rcu_temperature.hip', r'constexpr int TN_TILE = (\d+);')) == cl.TN_TILE
    assert int(_one('rcu_temperature.hip', r'constexpr int TN_STAGE_MAX = (\d+);')) == cl.TN_STAGE_MAX
    a, b = _one('rcu_quantile.hip', r'constexpr unsigned QA_MAX_GROUPS = (\d+) \* (\d+);')
    assert int(a) * int(b) == cl.QA_MAX_GROUPS
    assert int(_one('rcu_quantile.hip', r'constexpr int QA_THREADS = (\d+);')) == cl.QA_THREADS
    assert int(_one('rcu_pointwise.hip', r'#define RCU_HEAD_WGS (\d+)')) == cl.HEAD_WGS_PER_CU
    assert int(_one('rcu_pointwise.hip', r'static constexpr int PW_THREADS = (\d+);')) == cl.HEAD_THREADS
    caps = re.findall(r'cap = (\d+)u \* RCU_HEAD_WGS;', _source('rcu_pointwise.hip'))
    assert caps == [str(cl.HEAD_CUS)] * 2, caps          # launch_head and launch_head_sampled
    for name in ('rcu_postnet.hip', 'rcu_density.hip'):
        a, b = _one(name, r'wgs < (\d+) \? wgs : (\d+)\)')
        assert int(a) == int(b) == cl.POSTNET_WGS, name
        assert len(re.findall(r'const size_t wgs = \(ngroups \+ 3\) / 4;', _source(name))) == 1, name          # 4 waves ...
        assert len(re.findall(r'const size_t ngroups = \(nvox \+ 31\) / 32;', _source(name))) == 2, name      # ... of 32 voxels (kernel, launcher)


@pytest.mark.parametrize('name', sorted(cl.ROWS))
def test_every_row_has_a_third_trip_a_partial_last_item_and_one_trip_pieces(name):
    r = cl.ROWS[name]
    assert r.work == r.n_images * r.hw and r.items == (r.work + r.item - 1) // r.item
    assert r.items > 2 * r.walkers and r.third_trips == r.items - 2 * r.walkers >= 1, r
    assert r.items <= 3 * r.walkers, 'the table says THIRD trip: no walker takes a fourth'
    assert r.last_item == r.work - (r.items - 1) * r.item, r
    if r.item > 1:
        assert 1 <= r.last_item < r.item, r
    else:                       # one element per thread: what is ragged is the last round
        assert r.work % r.walkers != 0, r
    if r.n_images > 1:
        assert r.hw % r.item != 0, 'items were meant to straddle image boundaries'
        assert r.one_image_items <= r.walkers, 'a single image was meant to be a one-trip call'
    if name in cl.STATED:
        s = cl.STATED[name]
        assert (r.hw, r.hw % r.item, r.work, r.items, r.walkers, r.third_trips, r.last_item) == \
            (s['hw'], s['hw_mod'], s['work'], s['items'], s['walkers'], s['third_trips'], s['last_item'])


def test_the_shapes_are_the_rows():
    n, h, w = cl.POSTNET_SHAPE
    assert (n, h * w) == (cl.ROWS['postnet'].n_images, cl.ROWS['postnet'].hw) == (cl.ROWS['density_energy'].n_images, cl.ROWS['density_energy'].hw)
    n, h, w = cl.HEAD_SHAPE
    assert (n, h * w) == (cl.ROWS['head_stream'].n_images, cl.ROWS['head_stream'].hw)
    assert cl.TEMPERATURE_SHAPE == (cl.ROWS['temperature'].n_images, cl.ROWS['temperature'].hw)
    assert cl.QUANTILE_N16 % 4 == 3 and cl.QUANTILE_N4 % 4 == 3          # a 3-element tail
    for p, c in cl.TEMPERATURE_CASES:
        assert p * (c - 1) <= cl.TN_STAGE_MAX                              # the staged form
    for p, c in cl.UNSTAGED_CASES + ((257, 2),):
        assert p * (c - 1) > cl.TN_STAGE_MAX
    assert 36 * 7 <= cl.TN_STAGE_MAX
    # the largest LDS image: 96 channels, 3 hidden convs
    layer = lambda cb: (cb * cb * 1024 + 2 * cb * 32) * 4      # noqa: E731  (pn_layer_floats, rcu_kernels.h)
    assert 4 * layer(3) == 4 * 37632 == 150528 <= 160 * 1024 < 5 * layer(3)
    assert 12 * layer(1) <= 160 * 1024


# ------------------------------------------------------------------------------------------ the reference side of the PostNet tests
def _oracle(state, x, nb_convs, masks, dtype):
    from oracle import unet_oracle as uo
    return uo.postnet_forward(state, torch.from_numpy(x), nb_convs, masks, dtype=dtype).numpy()


def _check_reference(state, x, nb_convs, masks, tag):
    logits, bound = pr.forward(state, x, nb_convs, masks)
    # two float64 routes (numpy matrix products here, torch's convolutions and batch_norm there) agree to float64 rounding
    o64 = _oracle(state, x, nb_convs, masks, torch.float64)
    assert o64.dtype == np.float64 and float(np.abs(o64 - logits).max()) < 1e-12, tag
    used = pr.fraction_used(_oracle(state, x, nb_convs, masks, torch.float32), logits, bound)
    print('float32 oracle {}: largest fraction of the bound used {:.4f}'.format(tag, used))
    assert used <= 1.0, (tag, used)
    return used


@pytest.mark.parametrize('channels', pr.SEAM_CHANNELS)
@pytest.mark.parametrize('shape', pr.SEAM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_float32_oracle_within_the_bound_small_cases(shape, channels):
    for classes in pr.SEAM_CLASSES:
        for nb_convs in pr.SEAM_CONVS:
            state, x, masks = pr.seam_case(shape, channels, classes, nb_convs)
            _check_reference(state, x, nb_convs, None, (shape, channels, classes, nb_convs, 'eval'))
            if masks is not None:
                _check_reference(state, x, nb_convs, masks, (shape, channels, classes, nb_convs, 'masked'))
                ones = [np.ones_like(m) for m in masks]
                a, b = pr.forward(state, x, nb_convs, None)[0], pr.forward(state, x, nb_convs, ones)[0]
                assert float(np.abs(a - b).max()) < 1e-12


@pytest.mark.parametrize('masked', [False, True], ids=['eval', 'masked'])
@pytest.mark.parametrize('case', cl.POSTNET_CASES, ids=lambda c: '-'.join(map(str, c)))
def test_float32_oracle_within_the_bound_above_the_cap(case, masked):
    channels, classes, nb_convs = case
    state, x, masks = cl.postnet_capped_case(channels, classes, nb_convs, masked)
    _check_reference(state, x, nb_convs, masks, (case, masked))


def test_the_chain_without_batchnorm_and_the_default_dtype():
    from oracle import unet_oracle as uo
    state, x, masks = pr.seam_case((3, 5, 7), 32, 2, 2)
    plain = {k: v for k, v in state.items() if '.bn.' not in k}
    for k in list(state):      # BatchNorm as the identity: what bn = 0 computes
        if k.endswith('.bn.weight'):
            state[k] = torch.full_like(state[k], float(np.sqrt(1.0 + pr.BN_EPS)))
        elif k.endswith('.bn.running_var'):
            state[k] = torch.ones_like(state[k])
        elif k.endswith('.bn.bias') or k.endswith('.bn.running_mean'):
            state[k] = torch.zeros_like(state[k])
    for m in (None, masks):
        without, bound = pr.forward(plain, x, 2, m, bn=False)
        assert float(np.abs(without - _oracle(state, x, 2, m, torch.float64)).max()) < 1e-6      # (sqrt(1 + eps) is rounded to float32)
        assert (bound > 0).all()
    # the default stays float32, the same bits as before the dtype argument
    a = uo.postnet_forward(state, torch.from_numpy(x), 2, masks)
    assert a.dtype == torch.float32 and torch.equal(a, uo.postnet_forward(state, torch.from_numpy(x), 2, masks, dtype=torch.float32))
