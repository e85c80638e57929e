"""Input corruptions on the GPU (include/rcu.h "Input corruptions"): every kind against the float64 restatement of tests/corruption_reference.py,
batch independence, composition of stages, the batch step in front of the predict steps and the script surface."""
import csv
import glob
import json
import os

import numpy as np
import pytest
import torch

import corruption_reference as cr
from test_script_surface_cpu import BRATS_MC_YAML

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIRST = cr.FIRST_SAMPLE          # 2^32 + 5 wherever g enters
UNET = dict(nb_classes=2, in_channels=4, depth=3, start_filters=32, dropout=0.05, sigma_out=False)     # PARAMS of the logit-sampling test


@pytest.fixture(scope='module')
def lib():
    import rcu_amd.build as b
    b.build()
    from rcu_amd import _lib
    return _lib


def _stage(kind, amount):
    from rcu_amd import corruption as co
    return co.Stage(kind, co.KINDS.index(kind), float(amount), None, None)


def _run(x, kind, amount, key=cr.KEY, first=FIRST):
    """rcu_corrupt of a host array or device tensor -> device tensor."""
    from rcu_amd import corruption as co
    xt = torch.from_numpy(x).to(DEV) if isinstance(x, np.ndarray) else x
    return co.corrupt_stage(xt, _stage(kind, amount), key, first, torch.empty_like(xt))


def _cases(channels):
    for kind, amount in cr.CASES:
        amount = cr.case_amount(kind, amount, channels)
        if amount is not None:                       # (channel_drop needs a channel to drop and one to keep: C >= 2)
            yield kind, amount


@pytest.mark.parametrize('shape', cr.SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_every_kind_against_the_float64_restatement(lib, golden, shape):
    g = golden('g29_corruptions')
    x = g['x_{}x{}x{}'.format(*shape)]
    assert x.shape == (3,) + shape
    xt = torch.from_numpy(x).to(DEV)
    failures = []
    for kind, amount in _cases(shape[0]):
        got_t = _run(xt, kind, amount)
        got = got_t.cpu().numpy()
        want = cr.reference(kind, x, amount, cr.KEY, FIRST)
        if shape == cr.SHAPES[0]:                    # the frozen outputs of the smallest shape
            frozen = g['y_' + cr.case_name(kind, None if kind == 'channel_drop' else amount)]
            assert np.abs(frozen.astype(np.float64) - want.astype(np.float64)).max() <= 1e-12 * max(1.0, float(np.abs(frozen).max()))
        if kind in ('intensity_shift', 'channel_drop'):
            ok = want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
            print('{} {} {}: bit-equal {}'.format(shape, kind, amount, ok))
        else:
            z = cr.normals(cr.KEY, FIRST, 3, shape[1] * shape[2], shape[0]).transpose(0, 2, 1).reshape(x.shape) if kind == 'gaussian_noise' else None
            tol = cr.tolerance(kind, x, want, amount, z)
            err = np.abs(got.astype(np.float64) - want)
            worst = float((err / np.maximum(tol, 1e-300)).max())
            print('{} {} {}: max error {:.3e}, worst error / bound {:.3f}'.format(shape, kind, amount, float(err.max()), worst))
            ok = bool(np.all(err <= tol))
        if kind == 'gaussian_noise' and amount == 0.0:
            ok = ok and torch.equal(got_t, xt)       # a = 0 returns x bit for bit
        if not ok:
            failures.append((kind, amount))
        assert torch.equal(xt.cpu(), torch.from_numpy(x))       # the input is never written
    assert not failures, failures


def test_blur_at_the_largest_radius(lib):
    """sigma 8: r = 32, the largest halo (the kernel's LDS images take more than 64 KB), on planes barely taller than the radius."""
    x = cr.make_input((2, 40, 70), n=2, seed=8)
    want = cr.reference('gaussian_blur', x, 8.0)
    err = np.abs(_run(x, 'gaussian_blur', 8.0).cpu().numpy().astype(np.float64) - want)
    tol = cr.tolerance('gaussian_blur', x, want, 8.0)
    print('sigma 8: max error {:.3e}, bound {:.3e}'.format(float(err.max()), tol))
    assert cr.radius(8.0) == 32 and float(err.max()) <= tol


def test_noise_is_the_normal_of_the_logit_sampling(lib):
    """Channel c of a 4-channel draw is rcu_logit_normals(key, g, n, hw, 4, 1)[..., 0, c], scaled: one definition, two users."""
    n, c, h, w = 3, 4, 15, 16
    a = 0.3
    so = lib.load()
    z = torch.empty(n * h * w, 1, c, device=DEV)
    lib.check(so.rcu_logit_normals(cr.KEY, FIRST, n, h * w, c, 1, lib.ptr(z), lib.current_stream()))
    x = torch.from_numpy(cr.make_input((c, h, w))).to(DEV)
    zz = z.view(n, h * w, c).permute(0, 2, 1).reshape(n, c, h, w).contiguous()
    got = _run(x, 'gaussian_noise', a)
    # fmaf(a, z, x) in float64 and rounded once is what the kernel computes from the same float32 z
    want = (x.double() + float(np.float32(a)) * zz.double()).float()
    assert torch.equal(got, want)
    assert torch.equal(_run(torch.zeros_like(x), 'gaussian_noise', 1.0), zz)
    # another key, another slice index: other noise
    assert not torch.equal(_run(x, 'gaussian_noise', a, key=cr.KEY + 1), got)
    assert not torch.equal(_run(x, 'gaussian_noise', a, first=FIRST + 1), got)


@pytest.mark.parametrize('shape', [(4, 15, 16), (3, 30, 30), (8, 13, 20)], ids=lambda s: 'x'.join(str(v) for v in s))
def test_batch_independence_on_the_main_and_a_side_stream(lib, shape):
    """Every kind on n = 5 equals the concatenation of calls on 2 + 3 slices with the matching first_sample -- also on a side stream, and from
    pointers that are not 16-byte aligned (the scalar form of the kernels)."""
    x = torch.from_numpy(cr.make_input(shape, n=5, seed=31)).to(DEV)
    a_part, b_part = x[:2].contiguous(), x[2:].contiguous()
    flat = torch.empty(x.numel() + 1, device=DEV)
    shifted = flat[1:].view(x.shape)
    shifted.copy_(x)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 != 0
    side = torch.cuda.Stream(device=DEV)
    for kind, amount in _cases(shape[0]):
        whole = _run(x, kind, amount)
        parts = torch.cat([_run(a_part, kind, amount, first=FIRST), _run(b_part, kind, amount, first=FIRST + 2)])
        assert torch.equal(whole, parts), (kind, amount)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            on_side = torch.cat([_run(a_part, kind, amount, first=FIRST), _run(b_part, kind, amount, first=FIRST + 2)])
        side.synchronize()
        assert torch.equal(whole, on_side), (kind, amount)
        flat_out = torch.empty(x.numel() + 1, device=DEV)
        from rcu_amd import corruption as co
        unaligned = co.corrupt_stage(shifted, _stage(kind, amount), cr.KEY, FIRST, flat_out[1:].view(x.shape))
        assert torch.equal(whole, unaligned), (kind, amount)
        # a slice's result does not depend on its position: slice 3 alone
        alone = _run(x[3:4].contiguous(), kind, amount, first=FIRST + 3)
        assert torch.equal(whole[3:4], alone), (kind, amount)


def test_many_planes_walk_the_grid_stride(lib):
    """More planes than the grid's extent over planes (4096 planes, or images for the noise): the strided walk gives what the small batches give."""
    x = torch.from_numpy(cr.make_input((4, 6, 8), n=4200, seed=5)).to(DEV)
    for kind, amount in (('gaussian_noise', 0.3), ('gaussian_blur', 0.5), ('downsample', 3), ('contrast', 0.45), ('bias_field', 0.6), ('ghosting', 0.25),
                         ('channel_drop', 10.0)):
        whole = _run(x, kind, amount)
        tail = _run(x[4190:].contiguous(), kind, amount, first=FIRST + 4190)
        assert torch.equal(whole[4190:], tail), kind


def test_stages_compose_in_order_under_their_own_keys(lib):
    from rcu_amd import corruption as co
    seed = 20
    x = torch.from_numpy(cr.make_input((4, 70, 67))).to(DEV)
    keep = x.clone()
    stages = co.parse([{'kind': 'gaussian_blur', 'severity': 3}, {'kind': 'gaussian_noise', 'severity': 3}])
    got = co.corrupt(x, stages, seed, FIRST)
    blurred = co.corrupt_stage(x, stages[0], co.corruption_seed(seed, 0), FIRST, torch.empty_like(x))
    want = co.corrupt_stage(blurred, stages[1], co.corruption_seed(seed, 1), FIRST, torch.empty_like(x))
    assert torch.equal(got, want) and torch.equal(x, keep)
    assert got.data_ptr() != x.data_ptr()
    # the noise stage is keyed by its position: alone (stage 0) it draws other normals
    assert not torch.equal(co.corrupt(blurred, stages[1:], seed, FIRST), want)
    # out=, one to three stages: the result lands in out, the input stays
    for count in (1, 2, 3):
        many = co.parse([{'kind': 'ghosting', 'severity': 2}, {'kind': 'contrast', 'severity': 4}, {'kind': 'bias_field', 'severity': 5}][:count])
        out = torch.empty_like(x)
        res = co.corrupt(x, many, seed, FIRST, out=out)
        assert res.data_ptr() == out.data_ptr() and torch.equal(x, keep)
        step_by_step = x
        for s, stage in enumerate(many):
            step_by_step = co.corrupt_stage(step_by_step, stage, co.corruption_seed(seed, s), FIRST, torch.empty_like(x))
        assert torch.equal(res, step_by_step)
    with pytest.raises(ValueError):
        co.corrupt(x.cpu(), stages, seed, FIRST)
    with pytest.raises(ValueError):
        co.corrupt(x, stages, seed, FIRST, out=x)
    with pytest.raises(lib.RcuError, match='channel_drop'):
        co.corrupt(x, co.parse({'kind': 'channel_drop', 'channels': [5]}), seed, FIRST)       # channel 5 of 4: refused, never skipped


def _model():
    from oracle import unet_oracle as uo
    from rcu_amd.model import UNet
    model = UNet(**UNET)
    model.load_state_dict(uo.synthetic_state(20, **UNET))
    return model.to(DEV)


def _run_steps(model, images, offset, step_list):
    from rcu_amd import steps
    bc = steps.BatchContext({'images': images}, 0, sample_offset=offset)
    ctx = steps.TorchTestContext(DEV, model)
    for step in step_list:
        step(bc, None, ctx)
    torch.cuda.synchronize()
    return bc


@pytest.mark.parametrize('predict', ['mc', 'segmentation'])
def test_the_step_feeds_the_predict_steps_the_corrupted_batch(lib, predict):
    from rcu_amd import corruption as co
    from rcu_amd import steps
    model = _model()
    seed, offset = 20, 7
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2, 4, 32, 32, generator=gen)
    stages = co.parse([{'kind': 'gaussian_blur', 'severity': 2}, {'kind': 'gaussian_noise', 'severity': 3}])

    def predict_steps():
        if predict == 'mc':
            return [steps.McPredictStep(3, seed=seed), steps.MultiPredictionSummary()]
        return [steps.SegmentationPredictStep(do_probs=True)]

    through_step = _run_steps(model, x.clone(), offset, [steps.CorruptInputStep(stages, seed)] + predict_steps())
    corrupted = co.corrupt(x.to(DEV), stages, seed, offset)
    direct = _run_steps(model, corrupted.clone(), offset, predict_steps())
    clean = _run_steps(model, x.clone(), offset, predict_steps())
    assert torch.equal(through_step.input['images'], corrupted) and through_step.input['images'].is_cuda
    keys = [k for k, v in direct.output.items() if torch.is_tensor(v)]
    assert 'probabilities' in keys
    for k in keys:
        assert torch.equal(through_step.output[k], direct.output[k]), k
    assert not torch.equal(through_step.output['probabilities'], clean.output['probabilities'])
    # the host batch of the caller is not written
    host = x.clone()
    _run_steps(model, host, offset, [steps.CorruptInputStep(stages, seed)])
    assert torch.equal(host, x)


def _dataset(tmp_path):
    """The tiny synthetic BraTS dataset of tests/test_gpu_scripts.py: two volumes of 6 and 7 slices of 32 x 32, one model."""
    from oracle import unet_oracle as uo
    from rcu_amd import data as data_mod
    from rcu_amd import management as mgt
    from rcu_amd import nifti
    params = dict(nb_classes=2, in_channels=4, depth=4, start_filters=32, dropout=0.05)
    rng = np.random.RandomState(3)
    vols = {}
    for i in range(2):
        name = 'Brats18_T{}_1'.format(i)
        images = rng.randn(6 + i, 32, 32, 4).astype(np.float32)
        labels = (rng.rand(6 + i, 32, 32) < 0.3).astype(np.uint8)
        data_mod.write_volume(str(tmp_path / 'ds'), name, images, labels, nifti.ImageProperties((32, 32, 6 + i), (1.0, -2.0, 3.0), (1.0, 1.0, 2.5)))
        vols[name] = images
    mf = mgt.ModelFiles(str(tmp_path / 'train'), 'm')
    mgt.save_model(mf, 'unet', params, uo.synthetic_state(20, **params), epoch=2)
    split = str(tmp_path / 'split.json')
    with open(split, 'w') as f:
        json.dump({'train': [], 'valid': [], 'test': list(vols)}, f)
    return BRATS_MC_YAML.format(test_dir='{test_dir}', model_dir=mf.model_dir, split=split, dataset=str(tmp_path / 'ds')).replace('mc: 20', 'mc: 2'), vols


def _script_run(tmp_path, base, tag, batch_size, corruption):
    import yaml
    from rcu_amd import scripts
    doc = yaml.safe_load(base.replace('{test_dir}', str(tmp_path / 'out_{}'.format(tag))).replace('batch_size: 32', 'batch_size: {}'.format(batch_size)))
    if corruption is not None:
        doc['config']['others']['corruption'] = corruption
    path = str(tmp_path / 'cfg_{}.yaml'.format(tag))
    with open(path, 'w') as f:
        yaml.safe_dump(doc, f)
    ctx = scripts.test_default('brats', path, None)
    files = {os.path.basename(f): open(f, 'rb').read() for f in sorted(glob.glob(os.path.join(ctx.test_dir, '*.nii.gz')))}
    return ctx, files, open(os.path.join(ctx.test_dir, 'metrics.csv'), 'rb').read()


def test_scripts_corrupt_identically_for_any_batch_size_and_leave_clean_runs_alone(lib, tmp_path):
    from rcu_amd import corruption as co
    from rcu_amd import nifti
    base, vols = _dataset(tmp_path)
    spec = [{'kind': 'gaussian_blur', 'severity': 2}, {'kind': 'gaussian_noise', 'severity': 3}]
    ctx4, files4, csv4 = _script_run(tmp_path, base, 'c4', 4, spec)
    ctx3, files3, csv3 = _script_run(tmp_path, base, 'c3', 3, spec)
    assert len(files4) == 4 and sorted(files4) == sorted(files3)
    assert all(files4[k] == files3[k] for k in files4) and csv4 == csv3
    for ctx in (ctx4, ctx3):
        record = json.load(open(os.path.join(ctx.test_dir, 'corruption.json')))
        assert record == co.describe(co.parse(spec), 20)
    assert [r['subject'] for r in csv.DictReader(open(os.path.join(ctx4.test_dir, 'metrics.csv')))] == sorted(vols)
    # without the key: the files of a run through the same script whose YAML never had the key, no corruption.json, other maps than the corrupted run
    clean4, cfiles4, ccsv4 = _script_run(tmp_path, base, 'p4', 4, None)
    clean3, cfiles3, ccsv3 = _script_run(tmp_path, base, 'p3', 3, None)
    assert all(cfiles4[k] == cfiles3[k] for k in cfiles4) and ccsv4 == ccsv3 and sorted(cfiles4) == sorted(files4)
    assert not os.path.exists(os.path.join(clean4.test_dir, 'corruption.json'))
    assert sorted(os.listdir(clean4.test_dir)) == sorted(f for f in os.listdir(ctx4.test_dir) if f != 'corruption.json')
    assert any(cfiles4[k] != files4[k] for k in files4)
    # the clean run is the plain MC step on the clean slices, the corrupted run the same step on corrupt(slices): slice g of the run's stream of
    # slices is corrupted and masked under its global index (the loop coalesces the 13 slices into one step)
    from rcu_amd import steps
    model = ctx4.model
    images = torch.from_numpy(np.concatenate([vols[name] for name in sorted(vols)])).permute(0, 3, 1, 2).contiguous()
    for ctx, feed in ((clean4, images.to(DEV)), (ctx4, co.corrupt(images.to(DEV), co.parse(spec), 20, 0))):
        bc = _run_steps(model, feed, 0, [steps.McPredictStep(2, seed=20), steps.MultiPredictionSummary()])
        want = bc.output['probabilities'][:, 1].cpu().numpy()
        got = np.concatenate([nifti.read(os.path.join(ctx.test_dir, name + '_probabilities.nii.gz'))[0] for name in sorted(vols)])
        err = float(np.abs(got - want).max())
        print('script against the steps: max difference {:.3e}'.format(err))
        assert err < 2e-6       # (float32 summation order: the plan of a 13-slice batch made by another handle may pick another kernel)

