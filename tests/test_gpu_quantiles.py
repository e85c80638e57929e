"""The quantile rescale on the GPU (include/rcu.h "Quantile rescale"): rcu_key_hist against numpy integer for integer, quantile_table against
fixture G33 under three plans, rcu_quantile_apply against searchsorted and the definition's bits, and the `quantiles` action with
`--rescale quantile` end to end on a tiny synthetic density run."""
import csv
import ctypes
import glob
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import quantile_reference as qr
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
PLANS = ((16, 16), (12, 10, 10), (8, 8, 8, 8))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def g33():
    return load_golden('g33_quantiles')


def off_by_one(array, dev, dtype):
    """The array on the device, one element behind the start of its allocation (a float32 map: 4 bytes off, a uint8 mask: 1 byte off)."""
    flat = torch.from_numpy(np.ascontiguousarray(array).reshape(-1))
    room = torch.empty(flat.numel() + 1, device=dev, dtype=dtype)
    room[1:] = flat.to(dev)
    out = room[1:]
    assert out.data_ptr() % 16 != 0 if dtype == torch.float32 else out.data_ptr() % 4 != 0
    return out


def expected_hist(maps, mask, prefixes, shift, bits):
    """(hist, NaNs, population) of the definition, in numpy."""
    flat = maps.reshape(-1)
    inside = np.ones(flat.shape, bool) if mask is None else mask.reshape(-1) != 0
    nan = np.isnan(flat)
    keys = qr.key(flat[inside & ~nan])
    return qr.key_hist(keys, list(prefixes), shift, bits), int((inside & nan).sum()), int(inside.sum())


def prefix_tables(maps, shift, bits):
    """Prefix tables of 1, 3 and (where a row is small enough) 4095 entries for a pass: prefixes that occur in the data and one or two that do not."""
    width = 32 - shift - bits
    if width == 0:
        return [[], [0]]
    hi = np.unique(qr.key(maps.reshape(-1)[~np.isnan(maps.reshape(-1))]).astype(np.uint64) >> np.uint64(shift + bits)).astype(np.int64)
    absent = sorted(set(range(1 << width)) - set(hi.tolist()))[:2] if width <= 16 else [int(hi[0]) + 1 if int(hi[0]) + 1 not in hi else 1]
    tables = [[], [int(hi[len(hi) // 2])], sorted({int(hi[0]), int(hi[-1]), int(absent[0])})]
    if bits <= 8:
        many = set(hi[:4000].tolist())
        filler = (v for v in range(1 << width) if v not in many)
        while len(many) < 4095:
            many.add(next(filler))
        tables.append(sorted(many))
        assert len(tables[-1]) == 4095
    return tables


def volumes_for_shapes(g33):
    rng = np.random.RandomState(7)
    out = []
    for n in (1, 63, 65):
        out.append((np.exp(rng.normal(0, 2, (1, n))).astype(np.float32) * rng.choice([-1, 1], (1, n)).astype(np.float32), (rng.rand(1, n) < 0.6).astype(np.uint8)))
    two = g33['ties_maps'].copy()                     # 2 volumes of 5 x 48 x 52 = 12,480 voxels
    assert two.shape == (2, 12480)
    mask = (rng.rand(2, 12480) < 0.5).astype(np.uint8)
    mask[1] = 0                                       # one volume's mask is empty
    out.append((two, mask))
    return out


def test_key_hist_over_several_blocks_per_workgroup(dev):
    """Each way a count travels -- the packed u16 LDS histogram that is flushed after every block of 32,768 voxels (bits 16 and 14, no prefix),
    the u32 one (bits 12) and the global walk (three prefixes) -- with 1, 2 and 8 blocks per workgroup, on a volume of three blocks and a bit
    whose first 70,000 voxels hold ONE value: more than a u16 counter could take if the blocks were not flushed one by one."""
    from rcu_amd import _lib, evaluation as ev
    rng = np.random.RandomState(11)
    maps = np.exp(rng.normal(0, 2, (2, 3 * 32768 + 5))).astype(np.float32)
    maps[0, :70000] = 0.75
    maps[1, rng.rand(maps.shape[1]) < 0.85] = -3.0
    mask = (rng.rand(*maps.shape) < 0.9).astype(np.uint8)
    hi16 = sorted(set((qr.key(maps.reshape(-1)) >> 16).tolist()))
    cases = ((16, 16, []), (18, 14, []), (20, 12, [0]), (0, 16, [hi16[0], int(qr.key(np.float32([0.75]))[0] >> 16), hi16[-1]]))
    try:
        for shift, bits, prefixes in cases:
            prefixes = sorted(set(prefixes))
            for m in (None, mask):
                want = expected_hist(maps, m, prefixes, shift, bits)
                for blocks in (1, 2, 8, 0):
                    _lib.check(_lib.load().rcu_key_hist_set_blocks_per_workgroup(blocks))
                    for misaligned in (False, True):
                        a = off_by_one(maps, dev, torch.float32) if misaligned else maps
                        b = None if m is None else (off_by_one(m, dev, torch.uint8) if misaligned else m)
                        hist, nans, population = ev.key_histogram(a, b, prefixes, shift, bits, n_volumes=2)
                        assert np.array_equal(hist, want[0]) and (nans, population) == want[1:], (shift, bits, m is not None, blocks, misaligned)
    finally:
        _lib.check(_lib.load().rcu_key_hist_set_blocks_per_workgroup(0))


@pytest.mark.parametrize('shift,bits', ((16, 16), (0, 16), (20, 12), (0, 8), (18, 14), (3, 13)))
def test_key_hist_equals_numpy(dev, g33, shift, bits):
    from rcu_amd import evaluation as ev
    for maps, mask in volumes_for_shapes(g33):
        v = maps.shape[0]
        for prefixes in prefix_tables(maps, shift, bits):
            for m in (None, mask):
                want = expected_hist(maps, m, prefixes, shift, bits)
                for misaligned in (False, True):
                    a = off_by_one(maps, dev, torch.float32) if misaligned else maps
                    b = None if m is None else (off_by_one(m, dev, torch.uint8) if misaligned else m)
                    hist, nans, population = ev.key_histogram(a, b, prefixes, shift, bits, n_volumes=v)
                    where = (maps.shape, len(prefixes), m is not None, misaligned)
                    assert hist.dtype == np.int64 and hist.shape == want[0].shape, where
                    assert np.array_equal(hist, want[0]) and (nans, population) == want[1:], where


def test_key_hist_on_the_tie_heavy_and_special_fixtures(dev, g33):
    from rcu_amd import evaluation as ev
    for name in ('ties', 'special', 'equal', 'small', 'lognormal'):
        maps, mask = g33[name + '_maps'], g33.get(name + '_mask')
        pop = qr.population_keys(maps, mask)
        for plan in PLANS:
            _, passes = qr.select(pop, int(g33[name + '_Q']), plan)
            for prefixes, shift, bits, want in passes:      # every pass of the selection, with the prefixes the pass before it selected
                hist, nans, population = ev.key_histogram(maps, mask, prefixes, shift, bits, n_volumes=maps.shape[0])
                assert np.array_equal(hist, want) and nans == 0 and population == pop.size, (name, plan, shift)


def test_key_hist_counts_nans_and_adds_in_any_batching(dev, g33):
    from rcu_amd import evaluation as ev
    maps, mask = g33['lognormal_maps'].copy(), g33['lognormal_mask'].copy()
    maps[0, 5] = maps[0, 1000] = maps[2, 7] = np.nan      # (subject 2's mask is empty: its NaN is outside the population)
    mask[0, 5] = mask[0, 1000] = 1
    want = expected_hist(maps, mask, [], 16, 16)
    assert want[1] == 2
    got = ev.key_histogram(maps, mask, [], 16, 16, n_volumes=3)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    # one resident table: per-volume calls in reversed order add up to the bits of the one call
    for prefixes, shift, bits in (([], 16, 16), ([], 20, 12), (sorted(set((qr.key(maps[~np.isnan(maps)]) >> 16).tolist()))[:100], 0, 16)):
        one = ev.key_histogram(maps, mask, prefixes, shift, bits, n_volumes=3)
        out = (torch.zeros(one[0].shape, device=dev, dtype=torch.int64), torch.zeros(2, device=dev, dtype=torch.int64))
        for i in (2, 1, 0):
            assert ev.key_histogram(maps[i], mask[i], prefixes, shift, bits, out=out) is out
        assert np.array_equal(out[0].cpu().numpy(), one[0]) and tuple(int(c) for c in out[1].cpu()) == one[1:]


def subjects_of(g33, name):
    maps, mask = g33[name + '_maps'], g33.get(name + '_mask')
    return [('subject_{}'.format(i), maps[i], None if mask is None else mask[i]) for i in range(maps.shape[0])]


@pytest.mark.parametrize('name', ('normal', 'lognormal', 'ties', 'special', 'small', 'equal'))
def test_quantile_table_equals_the_fixture(dev, g33, name):
    from rcu_amd import evaluation as ev
    subjects, q = subjects_of(g33, name), int(g33[name + '_Q'])
    want = ev.QuantileTable(q, int(g33[name + '_N']), g33[name + '_keys'], g33[name + '_ranks'], 'all' if g33.get(name + '_mask') is None else 'mask')
    for plan in (None,) + PLANS:
        assert ev.quantile_table(subjects, q, plan=plan) == want, plan
    # the same subjects in another order, and handed over by a callable
    assert ev.quantile_table(lambda: iter(subjects[::-1]), q) == want


def test_quantile_table_narrows_its_plan_and_refuses_nan(dev, g33, monkeypatch):
    from rcu_amd import evaluation as ev
    subjects = subjects_of(g33, 'lognormal')
    want = ev.quantile_table(subjects, 1000)
    launches = []
    launch = ev._key_hist_launch
    monkeypatch.setattr(ev, '_key_hist_launch', lambda maps, mask, prefixes, shift, bits, hist, counts: (launches.append((shift, bits)),
                                                                                                       launch(maps, mask, prefixes, shift, bits, hist, counts)))
    monkeypatch.setattr(ev, 'QUANTILE_TABLE_BYTES', 1 << 20)      # (three prefixes of 2^16 digits already exceed it)
    assert ev.quantile_table(subjects, 1000) == want
    assert sorted(set(launches), reverse=True) == [(16, 16), (8, 8), (0, 8)]
    bad = [(s, m.copy(), k.copy()) for s, m, k in subjects]
    bad[1][1][3] = np.nan
    bad[1][2][3] = 1
    with pytest.raises(ValueError) as err:
        ev.quantile_table(bad, 1000)
    assert 'subject_1' in str(err.value) and 'NaN' in str(err.value)
    bad[1][2][3] = 0                                              # outside the population it is nobody's business
    assert ev.quantile_table(bad, 1000).N == want.N - int(subjects[1][2][3])
    with pytest.raises(ValueError):
        ev.quantile_table([(s, m, np.zeros_like(k)) for s, m, k in subjects], 1000)      # an empty population


@pytest.mark.parametrize('q', (2, 7, 1000, 4096))
def test_quantile_apply_equals_the_definition(dev, g33, q):
    from rcu_amd import evaluation as ev
    source = np.concatenate([g33['ties_maps'].reshape(-1), g33['lognormal_maps'].reshape(-1), g33['special_maps'].reshape(-1), [np.nan, -np.nan]]).astype(np.float32)
    n_pop, ranks, keys = qr.table(qr.population_keys([source[:-2]]), q)
    table = ev.QuantileTable(q, n_pop, keys, ranks)
    for n in (1, 3, 4, 63, 65, 1027, source.size):
        x = source[source.size - n:]                  # (the tail holds the special values and the NaNs)
        level = np.where(np.isnan(x), 0, qr.levels(qr.key(x), keys))
        want = qr.rescaled(level, q)
        for misaligned in (False, True):
            got, lv = ev.quantile_rescale(table, off_by_one(x, dev, torch.float32) if misaligned else x, return_levels=True)
            assert got.dtype == torch.float32 and lv.dtype == torch.int16 and tuple(got.shape) == x.shape
            assert np.array_equal(lv.cpu().numpy().astype(np.int64), level), (q, n, misaligned)
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (q, n, misaligned)
            assert np.array_equal(ev.quantile_rescale(table, x).cpu().numpy().view(np.uint32), want.view(np.uint32))
    # input, output and levels all one element off their allocations: the 16-byte path with a head and a tail
    lib = ev._lib
    bounds = (ctypes.c_uint32 * (q - 1))(*[int(k) for k in keys])
    ws = torch.empty(max(lib.load().rcu_quantile_apply_workspace_bytes(q), 8), device=dev, dtype=torch.uint8)
    for n in (2, 6, 66, 1030):
        x = source[source.size - n:]
        level = np.where(np.isnan(x), 0, qr.levels(qr.key(x), keys))
        src = off_by_one(x, dev, torch.float32)
        out, lv = torch.zeros(n + 2, device=dev, dtype=torch.float32), torch.full((n + 2,), -1, device=dev, dtype=torch.int16)
        lib.check(lib.load().rcu_quantile_apply(lib.ptr(src), n, bounds, q, lib.ptr(out[1:]), lib.ptr(lv[1:]), lib.ptr(ws), lib.current_stream()))
        out, lv = out.cpu().numpy(), lv.cpu().numpy()
        assert np.array_equal(out[1:-1].view(np.uint32), qr.rescaled(level, q).view(np.uint32)) and np.array_equal(lv[1:-1], level), (q, n)
        assert out[0] == 0 and out[-1] == 0 and lv[0] == -1 and lv[-1] == -1      # nothing written around the map
    # the level histogram at B = Q puts every voxel of the rescaled map into its level l
    x = source[:-2]
    level = qr.levels(qr.key(x), keys)
    rescaled = ev.quantile_rescale(table, x)
    zeros = np.zeros(x.shape, np.uint8)
    hist = ev.uncertainty_histogram(zeros, zeros, rescaled, q)[0]
    assert np.array_equal(hist[1].astype(np.int64), np.bincount(level, minlength=q)) and int(hist.sum()) == x.size


# ------------------------------------------------------------------------------------------- end to end
SUBJECTS = ('Brats18_Q_1', 'Brats18_R_1', 'Brats18_S_1')
SHAPE = (4, 24, 20)


def density_tree(root):
    """A tiny synthetic `density` run, written with nifti.py: 3 subjects of 4 x 24 x 20, distinct log-normal energies, one outlier voxel at 1e6; the
    T2 image is positive everywhere (the brain mask is the whole volume, so the levels file counts the population).  -> (gt dir, run dir, energies)"""
    from rcu_amd import nifti
    rng = np.random.RandomState(33)
    energy = np.exp(rng.normal(2.0, 1.5, (len(SUBJECTS),) + SHAPE)).astype(np.float32)
    flat = energy.reshape(-1)
    while True:                                       # distinct values: no ties
        _, first = np.unique(flat, return_index=True)
        repeated = np.setdiff1d(np.arange(flat.size), first)
        if repeated.size == 0:
            break
        flat[repeated] = np.nextafter(flat[repeated], np.float32(np.inf))
    energy[1, 2, 3, 4] = 1e6
    gt_root, run_dir = os.path.join(root, 'gt', 'HGG'), os.path.join(root, 'pred_density')
    os.makedirs(run_dir)
    for i, sub in enumerate(SUBJECTS):
        os.makedirs(os.path.join(gt_root, sub))
        t2 = (rng.rand(*SHAPE) + 0.5).astype(np.float32)
        seg = (rng.rand(*SHAPE) < 0.3).astype(np.uint8) * rng.randint(1, 5, SHAPE).astype(np.uint8)
        for mod, arr in (('flair', t2), ('t1', t2), ('t2', t2), ('t1ce', t2), ('seg', seg)):
            nifti.write(os.path.join(gt_root, sub, '{}_{}.nii.gz'.format(sub, mod)), arr)
        nifti.write(os.path.join(run_dir, '{}_density.nii.gz'.format(sub)), energy[i])
        nifti.write(os.path.join(run_dir, '{}_prediction.nii.gz'.format(sub)), (rng.rand(*SHAPE) > 0.5).astype(np.uint8))
    return os.path.join(root, 'gt'), run_dir, energy


def csv_digests(root):
    return {os.path.relpath(f, root): hashlib.sha256(open(f, 'rb').read()).hexdigest()
            for f in sorted(glob.glob(os.path.join(root, '**', '*.csv'), recursive=True))}


def level_counts(path):
    with open(path, newline='') as f:
        return np.array([sum(int(r[c]) for c in ('tp', 'tn', 'fp', 'fn')) for r in csv.DictReader(f)], dtype=np.int64)


def test_quantiles_action_end_to_end(dev, tmp_path):
    from rcu_amd import evalrun, evaluation as ev, scripts
    gt_dir, run_dir, energy = density_tree(str(tmp_path))
    runs = {'density': run_dir}
    n = energy.size

    def run(out, actions, **kw):
        scripts.eval_uncertainty('brats', runs, gt_dir, str(tmp_path / out), actions=actions, expected_subjects=list(SUBJECTS), **kw)
        return csv_digests(str(tmp_path / out))

    one = run('one', ('quantiles', 'ue_curves'), rescale='quantile')
    run('two', ('quantiles',))
    two = run('two', ('ue_curves',), rescale='quantile')
    assert one == two and sorted(one) == [os.path.join('quantiles', 'eval_quantiles_density.csv')] + [
        os.path.join('uncertainty', name.format('density_quantilerescale')) for name in
        ('eval_ue_curves_{}.csv', 'eval_ue_curves_pooled_{}.csv', 'eval_ue_levels_{}.csv')]
    # the table is the definition's, over the brain mask (here: every voxel)
    table = ev.load_quantiles(str(tmp_path / 'one' / 'quantiles' / 'eval_quantiles_density.csv'))
    n_ref, ranks, keys = qr.table(qr.population_keys(energy.reshape(len(SUBJECTS), -1)), 1000)
    assert table == ev.QuantileTable(1000, n_ref, keys, ranks, 'mask') and n_ref == n
    # no ties: every level of the pooled levels file holds r_{l+1} - r_l voxels
    counts = level_counts(str(tmp_path / 'one' / 'uncertainty' / 'eval_ue_levels_density_quantilerescale.csv'))
    assert np.array_equal(counts, np.diff(np.concatenate([[0], ranks, [n]]))) and counts.min() >= 5
    # the defect this fixes, on the reference rule alone: under the global min-max more than 99 % of the voxels land in level 0
    squeezed = ev.rescale_uncertainties(energy, energy.min(), energy.max())
    assert (qr.grid_level(squeezed, 1000) == 0).mean() > 0.99
    minmax = run('minmax', ('minmax', 'ue_curves'))
    assert level_counts(str(tmp_path / 'minmax' / 'uncertainty' / 'eval_ue_levels_density_globalrescale.csv'))[0] > 0.99 * n
    # ... and `--act minmax ue_curves` still writes the bytes the commit before this extension wrote (tests/golden/g33_minmax_digests.json)
    with open(os.path.join(GOLDEN, 'g33_minmax_digests.json')) as f:
        assert minmax == json.load(f)
    assert run('minmax_default', ('minmax', 'ue_curves'), rescale='minmax', quantiles=64) == minmax
    # a call without `quantiles` and without an earlier table, or with another Q, is refused by name
    with pytest.raises(ValueError) as err:
        run('none', ('ue_curves',), rescale='quantile')
    assert 'eval_quantiles_density.csv' in str(err.value) and '--rescale quantile' in str(err.value)
    with pytest.raises(ValueError) as err:
        run('two', ('ue_curves',), rescale='quantile', quantiles=500)
    assert '--quantiles' in str(err.value)
    # the other actions on the prepared uncertainty take the rescale too
    more = run('more', ('quantiles', 'bnf_ue', 'patches', 'components', 'lesions', 'boundary'), rescale='quantile', quantiles=64, levels=64)
    assert all('density_quantilerescale' in name or name.startswith('quantiles') for name in more) and len(more) > 11
