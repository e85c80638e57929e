"""The nearest-neighbour feature uncertainty without a GPU (include/rcu_knn.h): the float64 restatement tests/knn_reference.py against fixture G37
(sklearn's brute-force neighbours, the Philox key table, a bank selection made by sorting triples); ``merge_candidates`` over every partition and
order of the slices; the bank's float32 parameters and its file; the third header's symbols, its argument validation and the untouched first two
headers; the stream-order table of the third header; the script rows and every refusal by name; the ``knn`` run type of the evaluation."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import knn_reference as ref
from test_density_scripts_cpu import _context, _yaml_with
from test_stream_order_cpu import prototypes, stream_entry_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNN_NAMES = ('rcu_knn_sample_keys', 'rcu_knn_distances')


@pytest.fixture(scope='module')
def g37(golden):
    return golden('g37_knn')


# ------------------------------------------------------------------------------------------------------------------ reference and fixture
@pytest.mark.parametrize('normalize', [0, 1])
@pytest.mark.parametrize('F', [1, 5, 32])
def test_reference_reproduces_the_witness_distances_to_1e_12(g37, F, normalize):
    phi, bank = g37['phi_{}'.format(F)], g37['bank_{}'.format(F)]
    assert phi.dtype == np.float32 and phi.shape == (257, F) and bank.shape == (100, F) and (phi >= 0).all()
    assert not phi[:2].any() and not bank[0].any() and np.array_equal(bank[1:6], phi[2:7]) and np.array_equal(bank[6], bank[8]) \
        and np.array_equal(bank[7], bank[8])
    rows, sq = ref.bank_parameters(bank, normalize)
    assert rows.tobytes() == g37['rows_{}_{}'.format(F, normalize)].tobytes() and sq.tobytes() == g37['sq_{}_{}'.format(F, normalize)].tobytes()
    got, want = ref.neighbours(phi, rows, 8, normalize), g37['d2_{}_{}'.format(F, normalize)]
    assert got.shape == want.shape == (257, 8) and (np.diff(got, axis=1) >= 0).all()
    assert (np.abs(got - want) <= 1e-12 * np.maximum(1.0, want)).all()
    # the definition's own form, max(0, |x|^2 + |b|^2 - 2 x.b), is the same number up to float64 cancellation
    x, b = ref.queries(phi, normalize), rows.astype(np.float64)
    form = np.maximum(0.0, (x * x).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * x @ b.T)
    assert (np.abs(np.sort(form, axis=1)[:, :8] - got) <= 1e-12 * np.maximum(1.0, got)).all()
    assert np.array_equal(ref.score(phi, rows, 3, normalize), np.sqrt(got[:, 2]))
    if normalize:
        norms = np.linalg.norm(rows.astype(np.float64), axis=1)
        assert norms[0] == 0.0 and ((norms == 0.0) | (np.abs(norms - 1.0) < 1e-6)).all() and np.array_equal(norms == 0.0, ~bank.any(axis=1))
        assert not ref.queries(phi, 1)[:2].any()      # a zero vector stays zero
    bound = ref.error_bound(phi, rows, normalize)
    assert bound.shape == (257,) and (bound > 0).all()


def test_keys_and_selection_reproduce_the_fixture_integer_for_integer(g37):
    from rcu_amd import knn
    got = [int(ref.key63(ref.knn_seed(int(s)), int(g), int(v))) for s, g, v in zip(g37['key_seed'], g37['key_g'], g37['key_v'])]
    assert got == g37['key63'].tolist() and all(0 <= k < 2 ** 63 for k in got) and len(set(got)) == len(got)
    assert int(g37['key_g'].max()) >= 2 ** 32
    for seed in (0, 7, 12345, 2 ** 31 - 1):
        assert knn.knn_seed(seed) == ref.knn_seed(seed)
    from rcu_amd import corruption, steps
    assert knn.knn_seed(7) - steps.pass_seed(7, 0) == 32 << 40 > corruption.corruption_seed(7, 7) - steps.pass_seed(7, 0) == 23 << 40
    keys = ref.slice_keys(int(g37['sel_seed']), range(3), 40)
    assert keys.shape == (3, 40) and keys[2, 5] == ref.key63(ref.knn_seed(7), 2, 5)
    chosen = ref.select_bank(g37['sel_labels'], keys, tuple(g37['sel_per_class']))
    for a, name in zip(chosen, ('sel_label', 'sel_key63', 'sel_g', 'sel_v')):
        assert np.array_equal(a, g37[name]), name
    assert chosen[0].tolist() == [0] * 5 + [1] * 4


# ------------------------------------------------------------------------------------------------------------------ merge_candidates
def _slices(g37, rng, slices=5, hw=40, F=3):
    labels = (rng.random((slices, hw)) < 0.3).astype(np.uint8)
    keys = ref.slice_keys(7, range(slices), hw)
    keys[1, 3] = keys[0, 9]      # a tie of two keys across slices, and one within a slice: the triple decides
    keys[2, 8] = keys[2, 4]
    labels[1, 3] = labels[0, 9] = labels[2, 8] = labels[2, 4] = 1
    features = rng.standard_normal((slices, hw, F)).astype(np.float32)
    return labels, keys, features


def _candidates(labels, keys, features, which):
    g, v = np.meshgrid(np.asarray(which), np.arange(labels.shape[1]), indexing='ij')
    g, v = g.reshape(-1), v.reshape(-1)
    return dict(features=features[g, v], labels=labels[g, v], key63=keys[g, v], g=g.astype(np.int64), v=v.astype(np.int64))


def test_merge_candidates_gives_one_bank_for_any_partition_and_order(g37):
    from rcu_amd import knn
    rng = np.random.default_rng(37)
    labels, keys, features = _slices(g37, rng)
    keys[0, 9] = keys[1, 3] = np.sort(keys[labels == 1])[2]      # (the tie sits inside the kept rows of class 1)
    per_class = (7, 6)
    want = ref.select_bank(labels, keys, per_class)
    banks = []
    partitions = [[[0, 1, 2, 3, 4]], [[0], [1], [2], [3], [4]], [[0, 1, 2], [3, 4]], [[4, 0], [2], [3, 1]]]
    for parts in partitions:
        for order in itertools.islice(itertools.permutations(parts), 6):
            kept = None
            for which in order:
                kept = knn.merge_candidates(kept, _candidates(labels, keys, features, which), per_class)
                assert all(len(kept[name]) <= sum(per_class) for name in kept)
            banks.append(kept)
    for kept in banks:
        for a, name in zip(want, ('labels', 'key63', 'g', 'v')):
            assert np.array_equal(kept[name].astype(np.int64), a), name
        assert kept['features'].tobytes() == features[kept['g'], kept['v']].tobytes()
        assert kept['features'].dtype == np.float32 and kept['labels'].dtype == np.uint8 and kept['key63'].dtype == np.int64
    # a class with fewer voxels than asked for keeps all of them
    all_of_it = knn.merge_candidates(None, _candidates(labels, keys, features, range(5)), (7, 1000))
    assert int((all_of_it['labels'] == 1).sum()) == int((labels == 1).sum())
    bank = knn.KnnBank(normalize=True, per_class=per_class, seed=7, **banks[0])
    assert bank.counts() == [7, 6] and bank.as_dict() == dict(F=3, M=13, counts=[7, 6], per_class=[7, 6], normalize=True, seed=7)


# ------------------------------------------------------------------------------------------------------------------ the bank and its file
def _bank(g37, F=32, normalize=True, m=40):
    from rcu_amd import knn
    rng = np.random.default_rng(F)
    labels = np.sort(rng.integers(0, 2, m)).astype(np.uint8)
    key63 = np.concatenate([np.sort(rng.integers(0, 2 ** 62, int((labels == c).sum()))) for c in (0, 1)]).astype(np.int64)
    return knn.KnnBank(g37['bank_{}'.format(F)][:m], labels, key63, np.arange(m, dtype=np.int64) % 3, np.arange(m, dtype=np.int64), normalize=normalize,
                       per_class=(30, 30), seed=5)


def test_bank_parameters_are_the_references_and_the_file_round_trips(g37, tmp_path):
    from rcu_amd import knn
    for F in (1, 5, 32):
        for normalize in (False, True):
            bank = _bank(g37, F, normalize)
            rows, sq = bank.float32_parameters()
            want = ref.bank_parameters(bank.features, normalize)
            assert rows.dtype == sq.dtype == np.float32 and rows.tobytes() == want[0].tobytes() and sq.tobytes() == want[1].tobytes()
            assert rows.tobytes() == g37['rows_{}_{}'.format(F, int(normalize))][:40].tobytes()
            path = tmp_path / 'knn_{}_{}.npz'.format(F, int(normalize))
            knn.save_knn(bank, path)
            back = knn.load_knn(str(path))
            for name in ('features', 'labels', 'key63', 'g', 'v'):
                assert getattr(back, name).tobytes() == getattr(bank, name).tobytes() and getattr(back, name).dtype == getattr(bank, name).dtype
            assert back.as_dict() == bank.as_dict() and (back.F, back.M, back.normalize, back.per_class, back.seed) == (F, 40, normalize, (30, 30), 5)
            with np.load(str(path), allow_pickle=False) as doc:
                assert sorted(doc.files) == sorted(('features', 'labels', 'key63', 'g', 'v', 'normalize', 'per_class', 'seed'))


def test_a_malformed_bank_file_is_refused_by_name(g37, tmp_path):
    from rcu_amd import knn
    bank = _bank(g37)
    arrays = dict(features=bank.features, labels=bank.labels, key63=bank.key63, g=bank.g, v=bank.v, normalize=np.bool_(True),
                  per_class=np.array((30, 30), dtype=np.int64), seed=np.int64(5))

    def written(name, **change):
        doc = dict(arrays, **change)
        path = str(tmp_path / name)
        with open(path, 'wb') as f:
            np.savez(f, **{k: v for k, v in doc.items() if v is not None})
        return path

    assert knn.load_knn(written('good.npz')).M == 40
    cases = [('missing.npz', dict(key63=None), 'no key63 array'), ('dtype.npz', dict(features=bank.features.astype(np.float64)), 'features must be float32'),
             ('labels.npz', dict(labels=bank.labels.astype(np.int64)), 'labels must be uint8'), ('short.npz', dict(g=bank.g[:-1]), 'M = 40 entries'),
             ('wide.npz', dict(features=np.zeros((40, 33), np.float32)), 'F must be in 1..32'), ('nan.npz', dict(features=bank.features * np.float32('nan')), 'not finite'),
             ('order.npz', dict(key63=bank.key63[::-1].copy()), 'not in the order class'), ('flat.npz', dict(features=bank.features.reshape(-1)), r'\[M, F\]'),
             ('scalar.npz', dict(per_class=np.int64(3)), 'per_class a vector')]
    for name, change, word in cases:
        path = written(name, **change)
        with pytest.raises(ValueError, match=word) as e:
            knn.load_knn(path)
        assert path in str(e.value) and 'cannot be read' in str(e.value), name
    with pytest.raises(ValueError, match='nothing.npz.*cannot be read'):
        knn.load_knn(tmp_path / 'nothing.npz')
    (tmp_path / 'text.npz').write_text('not an archive')
    with pytest.raises(ValueError, match='text.npz.*cannot be read'):
        knn.load_knn(tmp_path / 'text.npz')
    with open(str(tmp_path / 'pickled.npz'), 'wb') as f:
        np.savez(f, **dict(arrays, features=np.array([{'a': 1}], dtype=object)))
    with pytest.raises(ValueError, match='pickled.npz.*cannot be read'):
        knn.load_knn(tmp_path / 'pickled.npz')


def test_the_module_refuses_what_the_kernels_do_not_take(g37):
    from rcu_amd import knn
    from rcu_amd.model import UNet
    bank = _bank(g37)
    for bad in (0, 9, True, 2.0, '5'):
        with pytest.raises(ValueError, match='k must be an integer in 1..8'):
            knn.check_k(bank, bad)
    small = knn.KnnBank(bank.features[:3], bank.labels[:3], bank.key63[:3], bank.g[:3], bank.v[:3])
    with pytest.raises(ValueError, match="k = 4 exceeds the bank's M = 3 rows"):
        knn.check_k(small, 4)
    assert knn.check_k(small, 3) == 3
    with pytest.raises(ValueError, match='UNet'):
        knn.check_model(torch.nn.Conv2d(4, 2, 1))
    with pytest.raises(ValueError, match='up to 32 feature channels .start_filters., got 64'):
        knn.check_model(UNet(2, 4, depth=2, start_filters=64))
    assert knn.check_model(UNet(2, 4, depth=2, start_filters=8)) == 8
    with pytest.raises(ValueError, match='per_class must be an integer >= 1'):
        knn.fit_knn(UNet(2, 4, depth=2, start_filters=8), [], 0, 0)
    with pytest.raises(ValueError, match='up to 65536 rows'):
        knn.fit_knn(UNet(2, 4, depth=2, start_filters=8), [], 40000, 0)
    with pytest.raises(ValueError, match='no batches'):
        knn.fit_knn(UNet(2, 4, depth=2, start_filters=8), [], 10, 0)
    with pytest.raises(RuntimeError, match='only runs on the GPU'):
        knn.distances(bank, torch.zeros(1, 32, 4, 4), 5)
    with pytest.raises(ValueError, match='1..32 feature channels, got 64'):
        knn.distances(bank, torch.zeros(1, 64, 4, 4), 5)
    with pytest.raises(RuntimeError, match='only runs on the GPU'):
        knn.sample_keys(1, 4, [0], 0, device='cpu')


# ------------------------------------------------------------------------------------------------------------------ C ABI
def _header(name):
    with open(os.path.join(ROOT, 'include', name)) as f:
        return f.read()


def test_the_third_header_declares_what_the_library_exports():
    from rcu_amd import _lib
    text = _header('rcu_knn.h')
    declared = dict(prototypes(text))
    assert set(declared) == set(KNN_NAMES) == set(_lib.KNN_SIGNATURES)
    lib = _lib.load()
    for name in KNN_NAMES:
        assert hasattr(lib, name) and name not in _lib.SIGNATURES and name not in _lib.FIT_SIGNATURES, name
        assert len(declared[name]) == len(_lib.KNN_SIGNATURES[name][1]) and declared[name][-1] == 'void* stream', name
        assert getattr(lib, name).argtypes == _lib.KNN_SIGNATURES[name][1]
    assert [p.split()[-1] for p in declared['rcu_knn_distances']] == ['features_dev', 'channel_pitch', 'F', 'n_voxels', 'bank_dev', 'bank_sq_dev', 'M',
                                                                     'k', 'normalize', 'score_dev', 'd2_dev', 'stream']
    assert [p.split()[-1] for p in declared['rcu_knn_sample_keys']] == ['n', 'hw', 'slice_index_dev', 'key', 'keys_dev', 'stream']
    assert '#include "rcu.h"' in text and 'Nearest-neighbour feature uncertainty' in text
    for macro, value in (('RCU_KNN_MAX_FEATURES', 32), ('RCU_KNN_MAX_BANK', 65536), ('RCU_KNN_MAX_K', 8)):
        assert re.search(r'#define {} {}\b'.format(macro, value), text) and getattr(_lib, macro) == value
    # the first two headers gained nothing
    for other in ('rcu.h', 'rcu_fit.h'):
        assert 'rcu_knn' not in _header(other)
    assert set(n for n, _ in prototypes(_header('rcu.h'))) == set(_lib.SIGNATURES)
    assert set(n for n, _ in prototypes(_header('rcu_fit.h'))) == set(_lib.FIT_SIGNATURES)
    makefile = open(os.path.join(ROOT, 'reliability-challenges-uncertainty_amd', 'csrc', 'Makefile')).read()
    assert 'rcu_knn.hip' in makefile and '../../include/rcu_knn.h' in makefile


def test_every_stream_taking_prototype_of_the_third_header_has_a_row():
    import stream_order as so
    import stream_order_fit as sof
    import stream_order_knn as sok
    found = stream_entry_points(_header('rcu_knn.h'))
    assert sorted(found) == sorted(KNN_NAMES) == sorted(sok.CASES) and all(hosts == [] for hosts in found.values())
    assert all(len(case.variants) >= 2 and callable(case.build) and case.hosts == () for case in sok.CASES.values())
    assert not set(sok.CASES) & (set(so.CASES) | set(so.EXEMPT) | set(sof.CASES)), 'the rows of the third header live in a table of their own'


def test_arguments_are_checked_without_a_device():
    from rcu_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(1 << 20)      # never dereferenced: every call below is refused first

    def distances(features=p, pitch=32, F=32, nvox=100, bank=p, bank_sq=p, M=100, k=5, normalize=1, score=p, d2=p):
        status = lib.rcu_knn_distances(features, pitch, F, nvox, bank, bank_sq, M, k, normalize, score, d2, None)
        return status, lib.rcu_last_error().decode()

    for kw, word in ((dict(features=None), 'null argument'), (dict(bank=None), 'null argument'), (dict(bank_sq=None), 'null argument'),
                     (dict(score=None), 'null argument'), (dict(F=0), 'F must be in 1..32, got 0'), (dict(F=33, pitch=36), 'F must be in 1..32, got 33'),
                     (dict(M=0), 'M must be in 1..65536, got 0'), (dict(M=65537), 'M must be in 1..65536'), (dict(k=0), 'k must be in 1..8, got 0'),
                     (dict(k=9), 'k must be in 1..8, got 9'), (dict(M=3, k=4), 'k = 4 exceeds the bank\'s M = 3 rows'),
                     (dict(pitch=28), 'channel_pitch must be >= F and a multiple of 4, got 28'), (dict(F=5, pitch=6), 'channel_pitch'),
                     (dict(features=ctypes.c_void_p((1 << 20) + 4)), 'features_dev must be 16-byte aligned'), (dict(normalize=2), 'normalize must be 0 or 1'),
                     (dict(nvox=0), 'n_voxels must be in 1..2\\^40'), (dict(nvox=(1 << 40) + 1), 'n_voxels'),
                     (dict(d2=ctypes.c_void_p((1 << 20) + 2)), '4-byte aligned')):
        status, message = distances(**kw)
        assert status == _lib.RCU_ERR_INVALID and re.search(word, message) and message.startswith('rcu_knn_distances: '), (kw, message)

    def keys(n=2, hw=100, index=p, out=p):
        status = lib.rcu_knn_sample_keys(n, hw, index, 7, out, None)
        return status, lib.rcu_last_error().decode()

    for kw, word in ((dict(index=None), 'null argument'), (dict(out=None), 'null argument'), (dict(n=0), 'n and hw'), (dict(hw=0), 'n and hw'),
                     (dict(n=1 << 16, hw=1 << 16), 'n \\* hw <= 2\\^31'), (dict(hw=(1 << 31) + 1, n=1), '2\\^31'),
                     (dict(out=ctypes.c_void_p((1 << 20) + 4)), '8-byte aligned')):
        status, message = keys(**kw)
        assert status == _lib.RCU_ERR_INVALID and re.search(word, message) and message.startswith('rcu_knn_sample_keys: '), (kw, message)


# ------------------------------------------------------------------------------------------------------------------ scripts
@pytest.fixture()
def bank_file(tmp_path, g37):
    from rcu_amd import knn
    bank = _bank(g37)
    path = str(tmp_path / 'knn.npz')
    knn.save_knn(bank, path)
    return path, bank


def _no_world(monkeypatch):
    for key in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(key, raising=False)


def test_the_keys_are_rows_of_the_one_table(bank_file):
    from rcu_amd import distributed as rdist
    from rcu_amd import scripts, steps
    names = [row.name for row in scripts._OTHERS]
    assert names.count('knn') == names.count('knn_bank') == 1
    assert names[:10] == ['tta', 'mc', 'temperature', 'agreement', 'mc_adaptive', 'logit_samples', 'corruption', 'density', 'auxiliary_fit', 'knn']
    knn_row, bank_row = (next(row for row in scripts._OTHERS if row.name == name) for name in ('knn', 'knn_bank'))
    assert knn_row.scripts == frozenset(('default',)) and bank_row.scripts == frozenset(('fit_knn',))
    assert not any('fit_knn' in row.scripts for row in scripts._OTHERS if row.name != 'knn_bank')
    owners = [(owner, other) for owner, other, _ in scripts._RULES if owner == 'knn']
    assert owners == [('knn', key) for key in ('mc', 'tta', 'agreement', 'mc_adaptive', 'logit_samples', 'density', 'laplace')]
    assert [owner for owner, _, _ in scripts._RULES][-7:] == ['knn'] * 7      # after the rules that were there

    path, bank = bank_file
    assert scripts._knn(_context(dict())) is None and scripts._knn(_context(dict(mc=20, knn_k=3))) is None
    plain = scripts._default_steps(_context(dict()), rdist.World())
    assert [type(s) for s in plain] == [steps.SegmentationPredictStep] and plain[0].do_probs
    for others, k in ((dict(knn=path), 5), (dict(knn=path, knn_k=1), 1), (dict(knn=path, knn_k=8, temperature=1.5), 8),
                      (dict(knn=path, corruption=[dict(kind='gaussian_noise', severity=5)]), 5), (dict(knn=path, agreement=False), 5),
                      (dict(knn=path, device_metrics=['ece_dice']), 5)):
        step, record = scripts._knn(_context(others))
        assert isinstance(step, steps.KnnPredictStep) and step.k == k and step.bank.features.tobytes() == bank.features.tobytes()
        assert record == dict(bank.as_dict(), file=path, k=k)
    got_steps, entries, hooks = scripts._default_plan(_context(dict(knn=path)), rdist.World(), None, None, step)
    assert got_steps == [step] and entries == ('knn',) and [type(h) for h in hooks] == [scripts.KnnWriteHook]
    assert (scripts.KnnWriteHook.KEY, scripts.KnnWriteHook.ENTRY) == ('knn', 'knn') and scripts.DensityWriteHook.ENTRY == 'density'
    assert scripts.KnnRecordHook(record).file_name == 'knn.json'


@pytest.mark.parametrize('key, value', [('mc', 20), ('tta', ['identity', 'flip_h']), ('agreement', True), ('mc_adaptive', dict(check_at=[5], tolerance=0.01)),
                                        ('logit_samples', 8), ('density', 'density.npz'), ('laplace', 'laplace.npz')])
def test_the_key_does_not_compose_with_the_sampling_keys_density_or_laplace(bank_file, key, value):
    from rcu_amd import scripts
    with pytest.raises(ValueError, match='others.knn does not compose with others.{}'.format(key)):
        scripts._knn(_context({'knn': bank_file[0], key: value}))


def test_a_bank_or_k_that_cannot_be_used_is_refused_by_key(tmp_path, bank_file):
    from rcu_amd import scripts, steps
    from rcu_amd.model import UNet
    with pytest.raises(ValueError, match='others.knn.*nothing.npz.*cannot be read'):
        scripts._knn(_context(dict(knn=str(tmp_path / 'nothing.npz'))))
    with pytest.raises(ValueError, match='others.knn must be the path'):
        scripts._knn(_context(dict(knn=1.5)))
    for bad in (0, 9, 2.5, 'five', True):
        with pytest.raises(ValueError, match='others.knn_k: k must be an integer in 1..8'):
            scripts._knn(_context(dict(knn=bank_file[0], knn_k=bad)))
    # a bank whose F is not the model's, and a model that is no U-Net, are refused before anything runs
    step = steps.KnnPredictStep(bank_file[1], 5)
    batch = steps.BatchContext({'images': torch.zeros(1, 4, 32, 32)}, 0, 0)
    with pytest.raises(ValueError, match='the k-NN bank has F = 32 feature channels, the model has 8'):
        step(batch, None, steps.TorchTestContext('cpu', UNet(2, 4, depth=2, start_filters=8)))
    with pytest.raises(ValueError, match='UNet'):
        step(batch, None, steps.TorchTestContext('cpu', torch.nn.Conv2d(4, 2, 1)))
    with pytest.raises(ValueError, match='needs a knn.KnnBank'):
        steps.KnnPredictStep(object(), 5)


def test_default_script_refuses_before_it_touches_anything(tmp_path, monkeypatch, bank_file):
    from rcu_amd import scripts
    _no_world(monkeypatch)
    path = _yaml_with(tmp_path, '    mc: 20\n    knn: {}\n'.format(bank_file[0]))
    with pytest.raises(ValueError, match='others.knn does not compose with others.mc'):
        scripts.test_default('brats', path, None, device='cpu')
    assert not (tmp_path / 'out').exists()


@pytest.mark.parametrize('script', ['test_ensemble', 'test_aleatoric', 'test_auxiliary_feat', 'test_auxiliary_segm', 'fit_temperature', 'fit_density',
                                    'fit_laplace', 'fit_auxiliary_feat', 'fit_knn'])
@pytest.mark.parametrize('key, value, description', [('knn', 'knn.npz', 'nearest-neighbour feature uncertainty')])
def test_other_scripts_refuse_the_key(tmp_path, monkeypatch, script, key, value, description):
    from rcu_amd import scripts
    _no_world(monkeypatch)
    path = _yaml_with(tmp_path, '    model_dir: [{}]\n    {}: {}\n'.format(tmp_path / 'train' / 'model_x', key, value))
    with pytest.raises(ValueError, match='others.{} .{}. applies to the default test scripts only; the {} script does not take it'.format(
            key, description, script.replace('test_', ''))):
        if script.startswith('fit_'):
            getattr(scripts, script)('brats', str(path), device='cpu')
        else:
            getattr(scripts, script)('brats', config_file=str(path), device='cpu')
    assert not (tmp_path / 'out').exists()


@pytest.mark.parametrize('script', ['test_default', 'test_ensemble', 'test_aleatoric', 'test_auxiliary_feat', 'test_auxiliary_segm', 'fit_temperature',
                                    'fit_density', 'fit_laplace', 'fit_auxiliary_feat'])
def test_only_the_fit_script_takes_the_bank_options(tmp_path, monkeypatch, script):
    from rcu_amd import scripts
    _no_world(monkeypatch)
    path = _yaml_with(tmp_path, '    model_dir: [{}]\n    knn_bank: {{per_class: 16}}\n'.format(tmp_path / 'train' / 'model_x'))
    with pytest.raises(ValueError, match='others.knn_bank .the options of the k-NN bank. applies to the k-NN fit scripts only; the {} script does not take '
                                         'it'.format(script.replace('test_', ''))):
        if script.startswith('fit_'):
            getattr(scripts, script)('brats', str(path), device='cpu')
        elif script == 'test_default':
            scripts.test_default('brats', str(path), None, device='cpu')
        else:
            getattr(scripts, script)('brats', config_file=str(path), device='cpu')
    assert not (tmp_path / 'out').exists()


@pytest.mark.parametrize('others, word', [('    mc: 20\n', 'others.mc'), ('    tta: [identity]\n', 'others.tta'), ('    temperature: 1.5\n', 'others.temperature'),
                                          ('    corruption: gaussian_noise\n', 'others.corruption'), ('    agreement: true\n', 'others.agreement'),
                                          ('    logit_samples: 4\n', 'others.logit_samples'), ('    density: d.npz\n', 'others.density'),
                                          ('    laplace: l.npz\n', 'others.laplace'), ('    auxiliary_fit: {epochs: 1}\n', 'others.auxiliary_fit'),
                                          ('    mc_adaptive: {check_at: [5], tolerance: 0.01}\n', 'others.mc_adaptive')])
def test_fit_script_refuses_every_other_row_by_name(tmp_path, monkeypatch, others, word):
    from rcu_amd import scripts
    _no_world(monkeypatch)
    with pytest.raises(ValueError, match=word + '.*the fit_knn script does not take it'):
        scripts.fit_knn('brats', _yaml_with(tmp_path, others), device='cpu')
    assert not (tmp_path / 'out').exists()
    with pytest.raises(ValueError, match='brats'):
        scripts.fit_knn('other', 'x.yaml')


def test_fit_script_runs_in_one_process_and_checks_its_options(monkeypatch):
    from rcu_amd import distributed as rdist
    from rcu_amd import scripts
    monkeypatch.setattr(scripts, '_context', lambda device, config_file: (_context(dict()), rdist.World(rank=0, world=2)))
    with pytest.raises(ValueError, match='the knn fit runs in one process'):
        scripts.fit_knn('brats', 'unused.yaml', device='cpu')
    assert scripts.fit_knn.__test__ is False
    assert scripts._knn_bank_options(_context(dict())) == (1024, True)
    assert scripts._knn_bank_options(_context(dict(knn_bank=dict(per_class=16, normalize=False)))) == (16, False)
    for bad, word in ((dict(per_class=0), 'per_class must be an integer in 1..32768'), (dict(per_class=32769), 'per_class'), (dict(per_class=2.5), 'per_class'),
                      (dict(per_class=True), 'per_class'), (dict(normalize=1), 'normalize must be true or false'),
                      (dict(k=5), 'others.knn_bank takes normalize, per_class; got k')):
        with pytest.raises(ValueError, match=word):
            scripts._knn_bank_options(_context(dict(knn_bank=bad)))


@pytest.mark.parametrize('dataset', ['brats', 'isic'])
def test_entry_points_wrap_the_fit(dataset):
    text = open(os.path.join(ROOT, 'bin-dl', '{}_fit_knn.py'.format(dataset))).read()
    assert "scripts.fit_knn('{}', args.config_file)".format(dataset) in text and "add_argument('-config_file'" in text
    like = open(os.path.join(ROOT, 'bin-dl', '{}_fit_density.py'.format(dataset))).read()
    assert text.count('\n') == like.count('\n')


# ------------------------------------------------------------------------------------------------------------------ evaluation
def test_knn_is_a_run_type_beside_the_references():
    import importlib.util
    from rcu_amd import directories as dirs
    from rcu_amd import evalrun
    from rcu_amd import evaluation as ev
    assert evalrun.CONFIDENCE_ENTRY['knn'] == 'knn' and evalrun.CONFIDENCE_ENTRY['aleatoric'] == 'sigma'
    assert dirs.KNN_RUN_IDS == ('knn',) and 'knn' not in dirs.RUN_IDS and len(dirs.RUN_IDS) == 8
    assert dirs.prediction_dir('brats', 'knn').endswith(os.path.join('predictions', 'brats', 'knn'))
    with pytest.raises(ValueError, match="unknown run id 'knn_d2': the run types are baseline, .*density, laplace, laplace_std, knn"):
        dirs.prediction_dir('brats', 'knn_d2')
    assert evalrun.SaveQuantilesAction.ENTRIES[-1] == 'knn' and evalrun.SaveQuantilesAction.ENTRIES[:3] == ('sigma', 'density', 'laplace_std')
    # it takes sigma's path: the same rescale (global min-max, or the quantile table), then an uncertainty
    rng = np.random.default_rng(0)
    dist = np.abs(rng.standard_normal((3, 5, 7))).astype(np.float32)
    mm = (float(dist.min()), float(dist.max()))
    as_knn, id_knn = ev.get_uncertainty_preparation('knn', 'knn', rescale_sigma='global', min_max=mm)
    as_sigma, id_sigma = ev.get_uncertainty_preparation('sigma', 'aleatoric', rescale_sigma='global', min_max=mm)
    assert (id_knn, id_sigma) == ('knn_globalrescale', 'aleatoric_globalrescale')
    a, b = as_knn({'knn': dist.copy()})['uncertainty'], as_sigma({'sigma': dist.copy()})['uncertainty']
    assert np.array_equal(a, b) and 0.0 <= float(a.min()) < 1e-3 and 1.0 - 1e-3 < float(a.max()) <= 1.0
    spec = importlib.util.spec_from_file_location('eval_uncertainty_cli', os.path.join(ROOT, 'bin-eval', 'eval_uncertainty.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert 'others.knn' in cli.make_parser().format_help()
