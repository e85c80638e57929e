"""The patch table and the patch level histogram on the GPU: rcu_patch_table / rcu_patch_hist against fixture G28 and the numpy restatement
(every patch size, the three uncertainty forms, masks, batches, the 16-byte path and its unaligned twin, one native volume), against the
host histogram and the voxel level histogram of rcu_unc_hist; SubjectBatch.metrics with 'patches'; the 'patches' action end to end."""
import os

import numpy as np
import pytest
import torch

from test_gpu_ue_curves import _all_csv, _rows, _tree
from test_patches_cpu import G28, ONE, fixture_histograms, fixture_table, numpy_patch_table

pytestmark = pytest.mark.gpu
LEVELS = (2, 10, 1000, 4096)
# set of G28 -> (case, dtype the map goes up as, with the mask)
SETS = {'v0': (0, np.float64, False), 'v0_mask': (0, np.float64, True), 'v0_f32': (0, np.float32, False), 'v1': (1, np.float32, False),
        'v2': (2, np.float32, False), 'img': (3, np.float32, False)}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def g28():
    with np.load(G28) as f:
        return {k: f[k] for k in f.files}


def inputs_of(g, name):
    c, dtype, masked = SETS[name]
    with np.errstate(over='ignore', invalid='ignore'):
        unc = g['uncertainty_{}'.format(c)].astype(dtype)
    return g['prediction_{}'.format(c)], g['target_{}'.format(c)], unc, (g['mask_0'] if masked else None)


def probability_like(rng, shape):
    """A float32 foreground probability with the ends of [0, 1] and their neighbourhood in it."""
    p = rng.rand(*shape).astype(np.float32)
    flat = p.reshape(-1)
    flat[:8] = [0.0, 1.0, 0.5, 1e-7, 0.999999, 1e-45, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))]
    flat[8::5] = np.where(rng.rand(flat[8::5].size) < 0.5, 1e-6, 1 - 1e-6)
    return p


@pytest.mark.parametrize('patch_index', range(9))
def test_table_equals_the_fixture(dev, g28, patch_index):
    from rcu_amd import evaluation as ev
    patch = tuple(int(v) for v in g28['patches'][patch_index])
    for name in SETS:
        pr, tg, unc, mask = inputs_of(g28, name)
        (got,) = ev.patch_table(pr, tg, unc, patch=patch, mask=mask)
        want = fixture_table(g28, name, patch_index)
        assert got.dtype == ev.PATCH_DTYPE and got.shape == want.shape
        assert np.array_equal(got, want), (name, patch)
        if unc.dtype == np.float32:                       # a map that a float32 holds gives one table in both forms
            assert np.array_equal(ev.patch_table(pr, tg, unc.astype(np.float64), patch=patch, mask=mask)[0], want), (name, patch)
        # no uncertainty (RCU_CC_UNC_NONE): the same counts, sum_q = 0
        none = want.copy()
        none['sum_q'] = 0
        assert np.array_equal(ev.patch_table(pr, tg, patch=patch, mask=mask)[0], none), (name, patch)
    # the mask on the other volumes, against the restatement (the fixture holds the masked table of volume 0 only)
    for name in ('v1', 'v2'):
        pr, tg, unc, _ = inputs_of(g28, name)
        for u in (unc, unc.astype(np.float64), None):
            assert np.array_equal(ev.patch_table(pr, tg, u, patch=patch, mask=g28['mask_0'])[0], numpy_patch_table(pr, tg, u, g28['mask_0'], patch))
    # the probability form equals the table of normalised_entropy(p) as a float64 map, integer for integer
    rng = np.random.RandomState(28 + patch_index)
    for shape in ((5, 13, 71), (1, 24, 40)):
        p = probability_like(rng, shape)
        pr, tg = (p > 0.5).astype(np.uint8), (rng.rand(*shape) < 0.3).astype(np.uint8)
        entropy = ev.normalised_entropy(p)
        assert entropy.dtype == torch.float64
        for mask in (None, (rng.rand(*shape) < 0.7).astype(np.uint8)):
            from_p = ev.patch_table(pr, tg, foreground_probability=p, patch=patch, mask=mask)[0]
            assert np.array_equal(from_p, ev.patch_table(pr, tg, entropy.reshape(shape), patch=patch, mask=mask)[0])
            assert np.array_equal(from_p, ev.patch_table(pr, tg, ev.EntropyOfProbability(p), patch=patch, mask=mask)[0])
            assert np.array_equal(from_p, numpy_patch_table(pr, tg, entropy.cpu().numpy().reshape(shape), mask, patch))
            assert int(from_p['sum_q'].max()) > 0


def test_batching_and_device_inputs(dev, g28):
    """Three volumes of an odd voxel count in one call: volumes 1 and 2 start off every alignment.  The rows are those of the single calls."""
    from rcu_amd import evaluation as ev
    names = ('v0', 'v1', 'v2')
    volumes = [inputs_of(g28, name) for name in names]
    rng = np.random.RandomState(4)
    ps = [probability_like(rng, (5, 13, 71)) for _ in names]
    for patch_index in (1, 2, 3, 5, 6):
        patch = tuple(int(v) for v in g28['patches'][patch_index])
        single_p = [ev.patch_table(v[0], v[1], foreground_probability=p, patch=patch)[0] for v, p in zip(volumes, ps)]
        for order in ((0, 1, 2), (2, 0, 2), (1, 1, 0)):
            pr, tg = np.stack([volumes[k][0] for k in order]), np.stack([volumes[k][1] for k in order])
            unc = np.stack([volumes[k][2].astype(np.float64) for k in order])
            mask = np.stack([g28['mask_0']] * 3)
            got = ev.patch_table(pr, tg, unc, patch=patch, n_volumes=3)
            assert len(got) == 3
            for k, table in zip(order, got):
                assert np.array_equal(table, fixture_table(g28, names[k], patch_index)), (patch, order, k)
            on_device = ev.patch_table(torch.from_numpy(pr).to(dev), torch.from_numpy(tg).to(dev), torch.from_numpy(unc).to(dev), patch=patch,
                                       n_volumes=3)
            assert all(np.array_equal(a, b) for a, b in zip(got, on_device))
            masked = ev.patch_table(pr, tg, unc, patch=patch, mask=mask, n_volumes=3)
            for k, table in zip(order, masked):
                assert np.array_equal(table, numpy_patch_table(volumes[k][0], volumes[k][1], volumes[k][2], g28['mask_0'], patch))
            from_p = ev.patch_table(pr, tg, foreground_probability=np.stack([ps[k] for k in order]), patch=patch, n_volumes=3)
            for k, table in zip(order, from_p):
                assert np.array_equal(table, single_p[k]), (patch, order, k)
            # float32 maps in a batch
            unc32 = np.stack([inputs_of(g28, 'v0_f32' if k == 0 else names[k])[2] for k in order])
            for k, table in zip(order, ev.patch_table(pr, tg, unc32, patch=patch, n_volumes=3)):
                assert np.array_equal(table, fixture_table(g28, 'v0_f32' if k == 0 else names[k], patch_index))
    with pytest.raises(ValueError):
        ev.patch_table(volumes[0][0], volumes[0][1][:, :, :70], volumes[0][2])
    with pytest.raises(ValueError):
        ev.patch_table(volumes[0][0], volumes[0][1], volumes[0][2], foreground_probability=ps[0])
    with pytest.raises(ValueError):
        ev.patch_table(volumes[0][0], volumes[0][1], volumes[0][2], patch=(1, 4, 17))


def _offset_view(a, dev):
    """The array on the device, one element behind the start of its allocation: a contiguous view no 16-byte (4-byte) load may touch."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    buf[1:].copy_(t.reshape(-1))
    view = buf[1:].reshape(a.shape)
    assert view.data_ptr() % max(4, 4 * t.element_size()) != 0 and view.is_contiguous()
    return view


@pytest.mark.parametrize('shape', [(3, 8, 128), (2, 12, 64)])
def test_the_16_byte_path_and_its_unaligned_twin(dev, shape):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(sum(shape))
    v = 2
    full = (v,) + shape
    pr = (rng.rand(*full) < 0.4).astype(np.uint8) * rng.choice([1, 2, 255], size=full).astype(np.uint8)
    tg = (rng.rand(*full) < 0.4).astype(np.uint8)
    mask = (rng.rand(*full) < 0.8).astype(np.uint8) * rng.choice([1, 128], size=full).astype(np.uint8)
    unc = rng.rand(*full) * 1.2 - 0.1
    unc[0, 0, 0, :6] = [np.nan, np.inf, -1.0, (5 + 0.5) / ONE, (6 + 0.5) / ONE, 1.0]
    p = np.stack([probability_like(rng, shape) for _ in range(v)])
    entropy = ev.normalised_entropy(p).cpu().numpy().reshape(full)
    for patch in ((1, 4, 4), (1, 8, 8), (2, 4, 16)):
        for m in (None, mask):
            want = {}
            for key, u in (('f32', unc.astype(np.float32)), ('f64', unc), ('p', entropy), ('none', None)):
                want[key] = [numpy_patch_table(pr[k], tg[k], None if u is None else u[k], None if m is None else m[k], patch) for k in range(v)]
            sources = {'f32': dict(uncertainty=unc.astype(np.float32)), 'f64': dict(uncertainty=unc), 'p': dict(foreground_probability=p), 'none': {}}
            for key, source in sources.items():
                got = ev.patch_table(pr, tg, patch=patch, mask=m, n_volumes=v, **source)
                assert all(np.array_equal(a, b) for a, b in zip(got, want[key])), (patch, key, m is not None)
                # the same arrays one element off their allocation: every array misaligned, the element path throughout
                shifted = {k: _offset_view(a, dev) for k, a in source.items()}
                got = ev.patch_table(_offset_view(pr, dev), _offset_view(tg, dev), patch=patch, mask=None if m is None else _offset_view(m, dev),
                                     n_volumes=v, **shifted)
                assert all(np.array_equal(a, b) for a, b in zip(got, want[key])), (patch, key, m is not None, 'offset')
            # only the map misaligned, only a label array misaligned
            got = ev.patch_table(pr, tg, _offset_view(unc.astype(np.float32), dev), patch=patch, mask=m, n_volumes=v)
            assert all(np.array_equal(a, b) for a, b in zip(got, want['f32']))
            got = ev.patch_table(pr, _offset_view(tg, dev), unc, patch=patch, mask=m, n_volumes=v)
            assert all(np.array_equal(a, b) for a, b in zip(got, want['f64']))


def test_histogram_equals_the_host_rule_and_the_fixture(dev, g28):
    from rcu_amd import evaluation as ev
    checked = 0
    for levels in LEVELS:
        for name, patch_index, per_mille, want in fixture_histograms(g28, levels):
            pr, tg, unc, mask = inputs_of(g28, name)
            patch = tuple(int(v) for v in g28['patches'][patch_index])
            got = ev.patch_histogram(pr, tg, unc, patch=patch, mask=mask, levels=levels, accuracy_per_mille=per_mille)
            assert got.dtype == np.uint64 and got.shape == (1, 3, levels)
            assert np.array_equal(got[0], want), (name, patch, levels, per_mille)
            checked += 1
        # the device histogram is the host rule on the device's table, batch of three, every patch size
        volumes = [inputs_of(g28, name) for name in ('v0', 'v1', 'v2')]
        pr, tg = np.stack([v[0] for v in volumes]), np.stack([v[1] for v in volumes])
        unc, mask = np.stack([v[2].astype(np.float64) for v in volumes]), np.stack([g28['mask_0']] * 3)
        for patch in g28['patches']:
            patch = tuple(int(v) for v in patch)
            for m in (None, mask):
                got = ev.patch_histogram(pr, tg, unc, patch=patch, mask=m, n_volumes=3, levels=levels, accuracy_per_mille=500)
                assert np.array_equal(got, ev.patch_histogram_of_table(ev.patch_table(pr, tg, unc, patch=patch, mask=m, n_volumes=3), levels, 500))
    assert checked == 4 * 134
    for bad in (dict(levels=1), dict(levels=4097), dict(accuracy_per_mille=1000), dict(accuracy_per_mille=-1), dict(patch=(0, 4, 4))):
        with pytest.raises(ValueError):
            ev.patch_histogram(*inputs_of(g28, 'v1')[:3], **bad)


def test_histogram_of_peaked_and_of_scattered_rows(dev):
    from rcu_amd import evaluation as ev
    shape = (3, 64, 256)
    n_patches = 3 * 16 * 64
    zeros = torch.zeros(shape, dtype=torch.uint8, device=dev)
    ones = torch.ones(shape, dtype=torch.uint8, device=dev)
    for levels in LEVELS:
        # every patch certain pure background: ONE key for every lane of every wave
        h = ev.patch_histogram(zeros, zeros, torch.zeros(shape, dtype=torch.float32, device=dev), levels=levels)[0]
        assert int(h[2, 0]) == n_patches and int(h.sum()) == n_patches
        # every patch inaccurate and as uncertain as can be
        h = ev.patch_histogram(ones, zeros, torch.full(shape, 2.0, dtype=torch.float64, device=dev), levels=levels)[0]
        assert int(h[1, levels - 1]) == n_patches and int(h.sum()) == n_patches
        # accurate with foreground, mean exactly 1/2: ON the boundary levels / 2 for an even number of levels
        h = ev.patch_histogram(ones, ones, torch.full(shape, 0.5, dtype=torch.float32, device=dev), levels=levels)[0]
        assert int(h[0, levels // 2 - 1]) == n_patches and int(h.sum()) == n_patches
    # 200,000 random rows through rcu_patch_hist alone: 49 workgroups flush into one output; as two volumes of 100,000 as well
    rng = np.random.RandomState(9)
    rows = 200000
    table = np.zeros(rows, dtype=ev.PATCH_DTYPE)
    table['n'] = rng.randint(0, 4097, rows) * (rng.rand(rows) < 0.9)
    table['errors'] = (rng.rand(rows) * (table['n'] + 1)).astype(np.uint64)
    table['foreground'] = np.maximum(table['errors'], (rng.rand(rows) < 0.5) * table['n'])
    table['sum_q'] = (rng.rand(rows) * table['n'] * ONE).astype(np.uint64)
    table['sum_q'][::7] = table['n'][::7] * np.uint64(ONE // 8)              # means exactly ON 125 / 1000, 512 / 4096
    table['sum_q'][1::7] = table['n'][1::7] * np.uint64(ONE)
    on_device = torch.from_numpy(table.view(np.uint64).reshape(1, rows, 4).view(np.int64)).to(dev)
    for levels in LEVELS:
        for per_mille in (0, 500, 999):
            got = ev._patch_hist_on_device(on_device, levels, per_mille).cpu().numpy().view(np.uint64)
            assert np.array_equal(got[0], ev.patch_histogram_of_table(table, levels, per_mille)), (levels, per_mille)
        got = ev._patch_hist_on_device(on_device.reshape(2, rows // 2, 4), levels, 500).cpu().numpy().view(np.uint64)
        assert np.array_equal(got, ev.patch_histogram_of_table([table[:rows // 2], table[rows // 2:]], levels, 500))
    # a table that does not start on a 16-byte boundary
    odd = torch.zeros(rows * 4 + 1, dtype=torch.int64, device=dev)
    odd[1:].copy_(on_device.reshape(-1))
    view = odd[1:].reshape(1, rows, 4)
    assert view.data_ptr() % 16 == 8
    assert np.array_equal(ev._patch_hist_on_device(view, 1000, 500).cpu().numpy().view(np.uint64)[0], ev.patch_histogram_of_table(table, 1000, 500))


@pytest.mark.parametrize('levels', (3, 10, 1000, 4096))
def test_unit_patches_equal_the_voxel_level_histogram(dev, levels):
    """Unit patches of a map of 24-bit dyadics: q(u) / 2^24 == u exactly and no such value lies between k / B and its float64 rounding, so
    the integer level rule and rcu_unc_hist's float64 rule agree on every voxel."""
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(levels)
    shape = (3, 37, 53)
    m = rng.randint(0, ONE + 1, shape)
    m.reshape(-1)[:4] = [0, ONE, ONE // 2, 1]
    k = rng.randint(0, levels + 1, 400)
    m.reshape(-1)[4:404] = (k * ONE) // levels            # the dyadics next to every kind of boundary
    m.reshape(-1)[404:804] = np.minimum((k * ONE) // levels + 1, ONE)
    u = (m / ONE).astype(np.float32)
    assert np.array_equal(u.astype(np.float64) * ONE, m)
    pr, tg = (rng.rand(*shape) < 0.5).astype(np.uint8), (rng.rand(*shape) < 0.4).astype(np.uint8)
    voxels = ev.uncertainty_histogram(pr, tg, u, levels)[0]           # tp, tn, fp, fn
    patches = ev.patch_histogram(pr, tg, u, patch=(1, 1, 1), levels=levels)[0]
    assert np.array_equal(patches[1], voxels[2] + voxels[3])
    assert np.array_equal(patches[0] + patches[2], voxels[0] + voxels[1])
    assert np.array_equal(patches[0], voxels[0]) and np.array_equal(patches[2], voxels[1])      # a correct voxel holds foreground iff it is a tp


def test_one_native_volume(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(12)
    shape = (155, 240, 240)
    unc = rng.rand(*shape).astype(np.float32)
    tg = np.zeros(shape, dtype=np.uint8)
    tg[40:100, 60:180, 70:170] = 1
    pr = np.roll(tg, (2, 3, -5), axis=(0, 1, 2))
    pr[rng.rand(*shape) < 0.001] = 1
    unc[(pr == 0) & (tg == 0)] *= np.float32(0.01)
    (got,) = ev.patch_table(pr, tg, unc, patch=(1, 4, 4))
    want = numpy_patch_table(pr, tg, unc, None, (1, 4, 4))
    assert got.shape == (155 * 60 * 60,) and np.array_equal(got, want)
    assert int(got['n'].sum()) == pr.size and int(got['errors'].sum()) == int((pr != tg).sum())
    h = ev.patch_histogram(pr, tg, unc, patch=(1, 4, 4))[0]
    assert np.array_equal(h, ev.patch_histogram_of_table(want))
    assert int(h[2, :10].sum()) > 0.5 * got.size                         # mostly certain background patches
    # cubes larger than a wave can fill the chip with: 10 x 15 x 15 lanes
    (cubes,) = ev.patch_table(pr, tg, unc, patch=(16, 16, 16))
    assert np.array_equal(cubes, numpy_patch_table(pr, tg, unc, None, (16, 16, 16)))


def test_subject_batch_metrics_with_patches(dev):
    from rcu_amd import evaluation as ev
    rng = np.random.RandomState(3)
    shapes = [(6, 16, 16), (6, 8, 32), (6, 16, 16), (1, 48, 32)]         # equal voxel counts, three shapes
    n = 6 * 16 * 16
    batch = ev.SubjectBatch(len(shapes), n, with_mask=True)
    subjects = []
    for slot, shape in enumerate(shapes):
        p = probability_like(rng, shape)
        pr, tg, m = (p > 0.5).astype(np.uint8), (rng.rand(*shape) < 0.3).astype(np.uint8), (rng.rand(*shape) < 0.6).astype(np.uint8)
        batch.put(slot, p, pr, tg, m)
        subjects.append((p, pr, tg))
    batch.upload()
    plain = batch.metrics(want=('minmax', 'ece', 'ue', 'ue_hist'))
    more = batch.metrics(want=('minmax', 'ece', 'ue', 'ue_hist', 'patches'))
    assert set(more) == set(plain) | {'patch_hist'}
    for key in ('min', 'max', 'counts', 'ue_hist'):
        assert plain[key].dtype == more[key].dtype and plain[key].tobytes() == more[key].tobytes(), key
    assert more['patch_hist'].dtype == np.uint64 and more['patch_hist'].shape == (len(shapes), 3, 1000)
    for slot, (p, pr, tg) in enumerate(subjects):         # no mask, like 'ue_hist'
        assert np.array_equal(more['patch_hist'][slot], ev.patch_histogram(pr, tg, foreground_probability=p)[0]), slot
    other = batch.metrics(want=('patches',), levels=64, patch=(2, 4, 8), accuracy_per_mille=900)['patch_hist']
    assert other.shape == (len(shapes), 3, 64)
    for slot, (p, pr, tg) in enumerate(subjects):
        assert np.array_equal(other[slot], ev.patch_histogram(pr, tg, foreground_probability=p, patch=(2, 4, 8), levels=64, accuracy_per_mille=900)[0])
    # one shape only: the whole batch in one call
    batch.used = 1
    assert np.array_equal(batch.metrics(want=('patches',))['patch_hist'][0], more['patch_hist'][0])
    with pytest.raises(ValueError):
        batch.metrics(want=('patches',), patch=(1, 4, 32))


# ----------------------------------------------------------------------------------------------------------- end to end
def test_patches_action_end_to_end(dev, tmp_path):
    from rcu_amd import evalrun, evaluation as ev
    rng = np.random.RandomState(5)
    subjects = ['Brats18_{}_1'.format(c) for c in 'ABCDEFGHI']
    gt_dir, run_dir, truth = _tree(tmp_path, subjects, 'probabilities', rng)
    gts = evalrun.collect_brats_ground_truth(gt_dir)
    entry = evalrun.get_eval_data('baseline_mc', run_dir, gts, expected_subjects=subjects)
    old = ['minmax', 'ece_dice', 'calib', 'bnf_ue', 'ue_curves']
    new = old + ['patches']
    base = str(tmp_path / 'eval')
    evalrun.evaluate_runs([entry], new, base, 'foreground')
    fused = _all_csv(base)
    patch_files = {k: v for k, v in fused.items() if os.path.basename(k).startswith('eval_patch')}
    assert sorted(os.path.basename(k) for k in patch_files) == ['eval_patch_levels_baseline_mc.csv', 'eval_patches_baseline_mc.csv',
                                                                'eval_patches_pooled_baseline_mc.csv']
    assert all(os.path.dirname(k) == evalrun.UNCERTAINTY_NAME for k in patch_files)
    # the plain loop and every batch size write the same bytes
    for tag, kwargs in (('plain', dict(fused=False)), ('b1', dict(batch_subjects=1)), ('b3', dict(batch_subjects=3)), ('b8', dict(batch_subjects=8))):
        other = str(tmp_path / ('eval_' + tag))
        evalrun.evaluate_runs([entry], new, other, 'foreground', **kwargs)
        assert _all_csv(other) == fused, tag
    # every other action's files do not feel the new one
    without = str(tmp_path / 'eval_old')
    evalrun.evaluate_runs([entry], old, without, 'foreground')
    assert _all_csv(without) == {k: v for k, v in fused.items() if k not in patch_files}
    alone = str(tmp_path / 'eval_alone')
    evalrun.evaluate_runs([entry], ['patches'], alone, 'foreground')
    assert _all_csv(alone) == patch_files
    # contents: per-subject rows, the pooled row, the levels file
    rows = _rows(os.path.join(base, 'uncertainty', 'eval_patches_baseline_mc.csv'))
    assert [r['subject_name'] for r in rows] == sorted(subjects)
    assert list(rows[0]) == ['test_id', 'subject_name'] + list(ev.PAVPU_KEYS)
    pooled = np.zeros((3, 1000), dtype=np.uint64)
    for r in rows:
        conf, pred, tgt = truth[r['subject_name']]
        h = ev.patch_histogram(pred, tgt, foreground_probability=conf)[0]
        pooled += h
        assert {k: r[k] for k in ev.PAVPU_KEYS} == {k: str(v) for k, v in ev.pavpu_metrics(h).items()}
        assert int(r['n_patches']) == 6 * 4 * 4
    (row,) = _rows(os.path.join(base, 'uncertainty', 'eval_patches_pooled_baseline_mc.csv'))
    assert {k: row[k] for k in ev.PAVPU_KEYS} == {k: str(v) for k, v in ev.pavpu_metrics(pooled).items()} and row['test_id'] == 'baseline_mc'
    levels = _rows(os.path.join(base, 'uncertainty', 'eval_patch_levels_baseline_mc.csv'))
    assert list(levels[0]) == ['level', 'threshold', 'accurate_fg', 'inaccurate', 'accurate_bg', 'pavpu', 'p_ac', 'p_ui'] and len(levels) == 1000
    assert np.array_equal(np.array([[int(r[c]) for r in levels] for c in ('accurate_fg', 'inaccurate', 'accurate_bg')], dtype=np.uint64), pooled)
    curve = ev.pavpu_curve(pooled)
    assert [r['pavpu'] for r in levels[1:]] == [str(c[0]) for c in curve[1:]] and levels[0]['pavpu'] == ''
    # the pooled files do not depend on the subject order either; other windows, levels and accuracy cut
    entry_rev = evalrun.get_eval_data('baseline_mc', run_dir, gts, expected_subjects=subjects)
    entry_rev.subject_files = entry_rev.subject_files[::-1]
    rev = str(tmp_path / 'eval_rev')
    evalrun.evaluate_runs([entry_rev], ['patches'], rev, 'foreground', batch_subjects=4)
    for name in ('eval_patches_pooled_baseline_mc.csv', 'eval_patch_levels_baseline_mc.csv'):
        assert _all_csv(rev)[os.path.join('uncertainty', name)] == fused[os.path.join('uncertainty', name)]
    cubes, cubes_plain = str(tmp_path / 'eval_cubes'), str(tmp_path / 'eval_cubes_plain')
    evalrun.evaluate_runs([entry], ['patches'], cubes, 'foreground', levels=64, patch=(4, 4, 4), patch_accuracy=900)
    evalrun.evaluate_runs([entry], ['patches'], cubes_plain, 'foreground', levels=64, patch=(4, 4, 4), patch_accuracy=900, fused=False)
    assert _all_csv(cubes) == _all_csv(cubes_plain)
    rows = _rows(os.path.join(cubes, 'uncertainty', 'eval_patches_baseline_mc.csv'))
    conf, pred, tgt = truth[rows[0]['subject_name']]
    expect = ev.pavpu_metrics(ev.patch_histogram(pred, tgt, foreground_probability=conf, patch=(4, 4, 4), levels=64, accuracy_per_mille=900)[0])
    assert {k: rows[0][k] for k in ev.PAVPU_KEYS} == {k: str(v) for k, v in expect.items()} and int(rows[0]['n_patches']) == 2 * 4 * 4
    assert len(_rows(os.path.join(cubes, 'uncertainty', 'eval_patch_levels_baseline_mc.csv'))) == 64
