"""Affine test-time augmentation on the GPU (include/rcu_warp.h): rcu_warp_affine and rcu_mc_accumulate_warped against the float64 restatement
of tests/warp_reference.py and against the D4 kernels bit for bit, AffineTtaMcPredictStep against McPredictStep, TtaMcPredictStep and the
oracle forward, and ``others.tta_affine`` through the drop-in scripts.  With -s every distance is printed before it is asserted."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import warp_reference as ref
from test_gpu_step_seam import H_TOL, _off_by_one
from test_gpu_tta import OUTPUTS, PARAMS, _launch_ranks, _model, _oracle_summary, _run, _written

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# (n, C, H, W, input one element off its allocation): odd sizes no multiple of the 16 x 16 tile; several tiles; one pixel; the misaligned input
SHAPES = {'odd': (3, 4, 15, 17, False), 'rect': (2, 2, 32, 48, False), 'one': (1, 1, 1, 1, False), 'square-off': (2, 4, 64, 64, True)}
CONTINUOUS = {'10deg': ref.matrix(10.0, 1.1, 1.5, -2.25), '-25deg-flip': ref.matrix(-25.0, 0.85, flip=True), '45deg': ref.matrix(45.0, 1.3)}
EXACT, MI, VAR = 8, 1, 2


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _elements(h, w):
    return tuple(range(8 if h == w else 4))


def _matrices(h, w):
    """name -> matrix: the identity, the flips, rot90 on a square plane, and the three continuous transforms."""
    out = {'identity': ref.D4[0], 'flip_h': ref.D4[1], 'flip_v': ref.D4[2], 'rot180': ref.D4[3]}
    if h == w:
        out['rot90'] = ref.D4[5]
    out.update(CONTINUOUS)
    return out


_CACHE = {}


def _images(shape):
    """The seeded input of a shape, made once and never written to."""
    if shape not in _CACHE:
        n, c, h, w, _ = SHAPES[shape]
        _CACHE[shape] = np.random.default_rng(380 + n * c * h * w).standard_normal((n, c, h, w)).astype(np.float32)
    return _CACHE[shape]


def _upload(a, dev, off):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return _off_by_one(t) if off else t


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


# ------------------------------------------------------------------------------------------------------------------ the warp
@pytest.mark.parametrize('shape', list(SHAPES))
def test_warp_is_within_12_ulps_of_the_largest_tap(dev, shape):
    """|out_dev - out| <= 12 * 2^-24 * max|tap| per element, against the float64 reference evaluated with the definition's taps and float32
    weights: three lerps, each a rounded difference and a rounded fmaf.  A float32 emulation of the chain on the CPU uses 2.7 of the 12."""
    from rcu_amd import steps
    n, c, h, w, off = SHAPES[shape]
    x = _images(shape)
    mats = _matrices(h, w)
    got = steps.warp_affine(_upload(x, dev, off), np.stack(list(mats.values())))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (len(mats), n, c, h, w)
    got = got.cpu().numpy().astype(np.float64)
    worst = 0.0
    for k, (name, M) in enumerate(mats.items()):
        want, tap = ref.warp(x, M, return_max_tap=True)
        frac = float((np.abs(got[k] - want) / (ref.U * np.maximum(tap, 1e-300))).max()) if np.abs(got[k] - want).max() > 0 else 0.0
        print('{} {}: {:.2f} of {} u max|tap|'.format(shape, name, frac, ref.WARP_BOUND_ULPS))
        assert (np.abs(got[k] - want) <= ref.WARP_BOUND_ULPS * ref.U * tap).all(), (shape, name, frac)
        if name not in CONTINUOUS:
            assert frac == 0.0, (shape, name)
        worst = max(worst, frac)
    print('{}: largest fraction of the bound used {:.3f}'.format(shape, worst / ref.WARP_BOUND_ULPS))


@pytest.mark.parametrize('shape', list(SHAPES))
def test_integer_tap_matrices_are_the_d4_kernel_bit_for_bit(dev, shape):
    from rcu_amd import steps
    n, c, h, w, off = SHAPES[shape]
    x = _upload(_images(shape), dev, off)
    elements = _elements(h, w)
    got = steps.warp_affine(x, ref.D4[list(elements)])
    for k, e in enumerate(elements):
        assert _bytes(got[k]) == _bytes(steps.tta_transform(x, e)), (shape, steps.TTA_ELEMENTS[e])
        assert np.array_equal(np.array(steps.TTA_AFFINE[e], dtype=np.float64), ref.D4[e])


def test_the_bytes_of_a_slice_do_not_depend_on_the_batch_its_place_the_alignment_or_the_stream(dev):
    from rcu_amd import steps
    n, c, h, w, _ = SHAPES['odd']
    x = torch.from_numpy(_images('odd'))
    mats = np.stack(list(CONTINUOUS.values()))
    probs = torch.softmax(torch.from_numpy(np.random.default_rng(5).standard_normal((len(mats), n, c, h, w)).astype(np.float32)), 2)
    flags = EXACT | MI | VAR

    def run(index, off, stream):
        """-> (warped images, statistics planes) of the batch made of the slices ``index``"""
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            xs, ps = _upload(x[index].numpy(), dev, off), _upload(probs[:, index].numpy(), dev, off)
            out = steps.warp_affine(xs, mats)
            stats = _statistics(len(index), c, h, w, flags, dev)
            steps.accumulate_warped(ps, stats, mats, from_probs=True)
        torch.cuda.synchronize()
        return out, stats.blob.view(-1, len(index), h, w)

    whole, planes = run(list(range(n)), False, None)
    side = torch.cuda.Stream()
    for i in range(n):
        for index, at, off, stream in (([i], 0, False, None), ([0, i], 1, True, None), ([i, 0, 0, i, 1], 3, True, side)):
            out, st = run(index, off, stream)
            assert _bytes(out[:, at]) == _bytes(whole[:, i]), (i, index)
            assert _bytes(st[:, at]) == _bytes(planes[:, i]), (i, index)


# ------------------------------------------------------------------------------------------------------------------ the warped statistics
def _statistics(n, c, h, w, flags, dev):
    from rcu_amd import steps
    return steps.McStatistics(n, c, h, w, dev, do_mi=bool(flags & MI), do_var=bool(flags & VAR), exact=bool(flags & EXACT))


def _samples(shape, groups, dev):
    n, c, h, w, off = SHAPES[shape]
    logits = np.random.default_rng(77 + groups * h * w).standard_normal((groups, n, c, h, w)).astype(np.float32)
    t = torch.from_numpy(logits).to(dev)
    from rcu_amd import steps
    probs = torch.stack([steps.softmax(t[g]) for g in range(groups)])
    return (_off_by_one(t) if off else t), (_off_by_one(probs) if off else probs)


@pytest.mark.parametrize('shape', list(SHAPES))
def test_accumulate_from_probabilities_against_the_reference(dev, shape):
    """EXACT|MI|VAR: the class sums and the p^2 sums within groups * (12 u max|tap| + 2^-41) of the reference's (the tap bound per group,
    summed), the entropy sums within groups * 2e-6, the bound tests/test_gpu_step_seam.py puts on an addend of the entropy plane (H_TOL)."""
    from rcu_amd import steps
    n, c, h, w, _ = SHAPES[shape]
    mats = np.stack(list(_matrices(h, w).values()))
    groups = len(mats)
    _, probs = _samples(shape, groups, dev)
    stats = _statistics(n, c, h, w, EXACT | MI | VAR, dev)
    steps.accumulate_warped(probs, stats, mats, from_probs=True)
    torch.cuda.synchronize()
    assert stats.count == groups
    planes = stats.blob.cpu().numpy().reshape(2 * c + 1, n, h, w)
    host = probs.cpu().numpy()
    s1, s2, sh = ref.accumulate_warped(host, mats)
    bound = np.zeros_like(s1)
    for g in range(groups):
        bound += ref.WARP_BOUND_ULPS * ref.U * ref.warp(host[g], mats[g], return_max_tap=True)[1] + 2.0 ** -41
    d1, d2 = np.abs(planes[:c].swapaxes(0, 1) - s1), np.abs(planes[c:2 * c].swapaxes(0, 1) - s2)
    dh = np.abs(planes[2 * c] - sh)
    print('{}: sum p {:.3e}, sum p^2 {:.3e} (of the bound: {:.3f}, {:.3f}); sum H {:.3e} (bound {:.1e})'.format(
        shape, d1.max(), d2.max(), (d1 / bound).max(), (d2 / bound).max(), dh.max(), groups * H_TOL))
    assert (d1 <= bound).all() and (d2 <= bound).all()
    assert dh.max() <= groups * H_TOL
    # every addend is a multiple of 2^-40
    assert np.array_equal(planes * 2.0 ** 40, np.round(planes * 2.0 ** 40))


@pytest.mark.parametrize('flags', [EXACT | MI | VAR, EXACT, MI | VAR, MI, 0], ids=['EXACT|MI|VAR', 'EXACT', 'MI|VAR', 'float32-MI', 'float32'])
@pytest.mark.parametrize('shape', ['odd', 'square-off'])
def test_from_logits_is_softmax_then_the_probability_form_and_groups_add_in_ascending_order(dev, shape, flags):
    from rcu_amd import steps
    n, c, h, w, _ = SHAPES[shape]
    mats = np.stack(list(_matrices(h, w).values()))
    groups = len(mats)
    logits, probs = _samples(shape, groups, dev)
    a, b, one_by_one = (_statistics(n, c, h, w, flags, dev) for _ in range(3))
    steps.accumulate_warped(logits, a, mats)
    steps.accumulate_warped(probs, b, mats, from_probs=True)
    for g in range(groups):      # the float32 and the plain float64 forms: the g-ascending order, one rounded addition per group
        steps.accumulate_warped(probs[g:g + 1], one_by_one, mats[g:g + 1], from_probs=True)
    torch.cuda.synchronize()
    assert a.count == b.count == one_by_one.count == groups
    assert _bytes(a.blob) == _bytes(b.blob) == _bytes(one_by_one.blob)
    if flags & EXACT:      # any split over calls, any order
        order = np.random.default_rng(3).permutation(groups)
        c1 = _statistics(n, c, h, w, flags, dev)
        for part in (order[:1], order[1:4], order[4:]):
            part = [int(g) for g in part]
            steps.accumulate_warped(logits[part], c1, mats[part])
        torch.cuda.synchronize()
        assert c1.count == groups and _bytes(c1.blob) == _bytes(a.blob)


@pytest.mark.parametrize('flags', [EXACT | MI | VAR, MI | VAR, MI], ids=['EXACT|MI|VAR', 'MI|VAR', 'float32-MI'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_integer_tap_matrices_give_accumulate_then_fold(dev, shape, flags):
    """Samples of images transformed by g, read back through the matrix of g^-1: rcu_mc_accumulate into a scratch blob followed by
    rcu_mc_fold_transformed -- all elements into one blob under EXACT; one element into a fresh blob in the rounded forms (0 + x is x)."""
    from rcu_amd import steps
    n, c, h, w, _ = SHAPES[shape]
    elements = _elements(h, w)
    _, probs = _samples(shape, len(elements), dev)
    inverse = ref.D4[[steps.TTA_INVERSE[e] for e in elements]]
    runs = [list(range(len(elements)))] if flags & EXACT else [[k] for k in range(len(elements))]
    for run in runs:
        got, want = _statistics(n, c, h, w, flags, dev), _statistics(n, c, h, w, flags, dev)
        steps.accumulate_warped(probs[run], got, inverse[run], from_probs=True)
        for k in run:
            scratch = _statistics(n, c, h, w, flags, dev)
            scratch.accumulate(probs[k], is_probabilities=True)
            steps.fold_transformed(scratch, want, elements[k])
        torch.cuda.synchronize()
        assert got.count == want.count == len(run) and _bytes(got.blob) == _bytes(want.blob), (shape, run)


# ------------------------------------------------------------------------------------------------------------------ the step
STEP_CASES = {'eval-64': (2, 64, 64, 0), 'mc-64': (2, 64, 64, 2), 'mc-32x48': (2, 32, 48, 2)}
STEP_MATS = np.stack([ref.IDENTITY] + list(CONTINUOUS.values()))


def _step_setup(case, dev):
    from oracle import unet_oracle as uo
    n, h, w, T = STEP_CASES[case]
    state = uo.synthetic_state(33, **PARAMS)
    x = torch.randn(n, 4, h, w, generator=torch.Generator().manual_seed(5))
    return _model(PARAMS, state, dev), state, x, T


@pytest.mark.timeout(300)
@pytest.mark.parametrize('case', list(STEP_CASES))
def test_step_with_the_identity_and_with_the_flips_is_the_existing_steps_bit_for_bit(dev, case):
    from rcu_amd import steps
    m, _, x, T = _step_setup(case, dev)
    keys = set(OUTPUTS) | {'ws_probabilities'}
    mine = _run(steps.AffineTtaMcPredictStep(matrices=[ref.IDENTITY], mc_steps=T, seed=11, do_mi=True, do_var=True), m, x, first=3)
    if T:      # the identity's keys are McPredictStep's
        theirs = _run(steps.McPredictStep(T, do_mi=True, do_var=True, seed=11), m, x, first=3)
    else:
        theirs = _run(steps.TtaMcPredictStep(['identity'], do_mi=True, do_var=True), m, x, first=3)
    assert set(mine) == set(theirs)
    for key in keys:
        assert _bytes(mine[key]) == _bytes(theirs[key]), (case, key)
    # The four flips against TtaMcPredictStep: in eval mode, where the two steps run the same samples.  (Under MC dropout the masks of
    # transform v >= 1 are keyed by affine_pass_seed, 65.. steps of 2^40, and those of a D4 element by tta_pass_seed, 1..7 steps: the two steps
    # draw other masks by definition, so there is nothing to compare bit for bit.)
    flips = _run(steps.AffineTtaMcPredictStep(matrices=ref.D4[:4], do_mi=True, do_var=True), m, x, first=3)
    tta = _run(steps.TtaMcPredictStep(['identity', 'flip_h', 'flip_v', 'rot180'], do_mi=True, do_var=True), m, x, first=3)
    assert set(flips) == set(tta)
    for key in keys:
        assert _bytes(flips[key]) == _bytes(tta[key]), (case, key)


@pytest.mark.timeout(300)
@pytest.mark.parametrize('case', list(STEP_CASES))
def test_group_sizes_one_and_the_maximum_and_the_lanes_give_the_same_bytes(dev, case):
    from rcu_amd import steps
    m, _, x, T = _step_setup(case, dev)
    n, h, w, _ = STEP_CASES[case]

    def run(group_pixels, lanes=None):
        return _run(steps.AffineTtaMcPredictStep(matrices=STEP_MATS, mc_steps=T, seed=11, group_pixels=group_pixels, do_mi=True, do_var=True,
                                                 lanes=lanes), m, x, first=3)

    pairs = len(STEP_MATS) * max(T, 1)
    one, most, uneven = run(n * h * w), run(pairs * n * h * w), run(3 * n * h * w)
    assert steps.pass_group_size(m, n, h, w, n * h * w) == 1 and steps.pass_group_size(m, n, h, w, pairs * n * h * w) == pairs
    one_lane, three_lanes = run(n * h * w, lanes=1), run(n * h * w, lanes=3)
    for key in set(OUTPUTS) | {'ws_probabilities'}:
        assert _bytes(one[key]) == _bytes(most[key]) == _bytes(uneven[key]) == _bytes(one_lane[key]) == _bytes(three_lanes[key]), (case, key)


@pytest.mark.timeout(600)
@pytest.mark.parametrize('case', list(STEP_CASES))
def test_step_against_the_oracle_forward_on_the_device_warped_inputs(dev, case):
    """The oracle forward runs on the DEVICE-warped inputs, downloaded, with the step's masks; its softmax is warped back by warp_reference and
    summarised as tests/test_gpu_tta.py summarises its samples; the tolerances are that test's for the same net (1e-6): the warp-back is a
    convex combination and does not amplify them."""
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    m, state, x, T = _step_setup(case, dev)
    n, h, w, _ = STEP_CASES[case]
    first = 3
    got = _run(steps.AffineTtaMcPredictStep(matrices=STEP_MATS, mc_steps=T, seed=11, do_mi=True, do_var=True), m, x, first=first)
    warped = steps.warp_affine(x.to(dev), STEP_MATS).cpu()
    sites = m.dropout_sites()
    probs = []
    for v, M in enumerate(STEP_MATS):
        back = steps.affine_inverse(M)
        for t in range(1, max(T, 1) + 1):
            mk = None
            if T:
                steps.set_dropout_mode(m, True)
                flat = m.seeded_masks(n, dev, [steps.affine_pass_seed(11, v, t)], first)
                steps.set_dropout_mode(m, False)
                mk = [f.view(n, -1).cpu() for f in torch.split(flat, [n * c for _, c in sites])]
            logits = uo.unet_forward(state, warped[v], mk, **PARAMS)
            probs.append(torch.from_numpy(ref.warp(torch.softmax(logits.double(), 1).numpy(), back)))
    want = _oracle_summary(probs)
    tol = 1e-6
    for key in OUTPUTS:
        d = float((got[key].double() - want[key]).abs().max())
        print('{} {}: {:.3e} (bound {:.0e})'.format(case, key, d, tol))
        assert d < tol, (case, key, d)
    lg0 = uo.unet_forward(state, x, None, **PARAMS)
    assert float((got['ws_probabilities'].double() - torch.softmax(lg0.double(), 1)).abs().max()) < tol
    # the replayed recipe: V x T volumes on the canonical grid, transform-major
    bc = steps.BatchContext({'images': x.clone()}, 0, first)
    steps.AffineTtaMcPredictStep(matrices=STEP_MATS, mc_steps=T, seed=11)(bc, None, steps.TorchTestContext('cuda', m))
    multi = bc.output['multi_probabilities'].as_tensor()
    assert tuple(multi.shape) == (len(STEP_MATS) * max(T, 1), n, 2, h, w)
    for i, p in enumerate(probs):
        assert float((multi[i].cpu().double() - p).abs().max()) < tol, i


# ------------------------------------------------------------------------------------------------------------------ the drop-in scripts
KEY_YAML = '    tta_affine: {samples: 3, rotation: 10.0, scale: 0.1, shift: 2.0, flip: true}\n'


def _record(out_root):
    dirs = glob.glob(os.path.join(out_root, '*'))
    assert len(dirs) == 1, dirs
    with open(os.path.join(dirs[0], 'tta_affine.json')) as f:
        return json.load(f)


@pytest.mark.timeout(900)
def test_brats_script_with_the_key_and_mc_batch_sizes_and_two_ranks(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_gpu_scripts as tgs
    from rcu_amd import steps
    cfg, vols, _, _ = tgs._setup(tmp_path, mc=2)
    text = open(cfg).read()
    assert '    mc: 2\n' in text and 'batch_size: 4' in text
    text = text.replace('    mc: 2\n', '    mc: 2\n' + KEY_YAML)
    cfgs = {}
    for tag, batch in (('b8', 8), ('b32', 32), ('two', 8)):
        cfgs[tag] = str(tmp_path / 'cfg_{}.yaml'.format(tag))
        with open(cfgs[tag], 'w') as f:
            f.write(text.replace(str(tmp_path / 'out'), str(tmp_path / 'out_{}'.format(tag))).replace('batch_size: 4', 'batch_size: {}'.format(batch)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('WORLD_SIZE', None)
    path = os.path.join(ROOT, 'bin-dl', 'brats_test_default.py')
    for tag in ('b8', 'b32'):
        r = subprocess.run([sys.executable, path, '-config_file', cfgs[tag]], capture_output=True, text=True, timeout=400, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    b8, b32 = _written(str(tmp_path / 'out_b8')), _written(str(tmp_path / 'out_b32'))
    assert len(b8) == 2 * len(vols) + 1 and sorted(b8) == sorted(b32)
    for name in b8:
        assert b8[name] == b32[name], name
    record = _record(str(tmp_path / 'out_b8'))
    assert record == _record(str(tmp_path / 'out_b32'))
    assert record['samples'] == 3 and record['mc'] == 2 and record['seed'] == 20 and record['flip'] is True and record['rotation'] == 10.0
    assert len(record['matrices']) == 3 and record['matrices'][0] == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    assert np.array(record['matrices']).tobytes() == steps.affine_tta_draw(20, 3, 10.0, 0.1, 2.0, True).tobytes()
    # two ranks: refused with the key's name, nothing written
    r = _launch_ranks(path, cfgs['two'], env)
    assert r.returncode != 0 and 'others.tta_affine is not sharded' in r.stdout + r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert not glob.glob(str(tmp_path / 'out_two' / '*' / '*.nii.gz'))


@pytest.mark.timeout(600)
def test_isic_script_with_the_key_alone_writes_its_files(tmp_path):
    from PIL import Image
    from oracle import unet_oracle as uo
    from rcu_amd import management as mgt
    from rcu_amd import nifti
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_gpu_scripts as tgs
    params = dict(nb_classes=2, in_channels=3, depth=4, start_filters=8, dropout=0.2)
    prefix = tmp_path / 'isic' / 'ISIC-2017_Test_v2'
    img_dir, lab_dir = str(prefix) + '_Data', str(prefix) + '_Part1_GroundTruth'
    os.makedirs(img_dir)
    os.makedirs(lab_dir)
    rng = np.random.RandomState(7)
    ids = ['ISIC_0000020', 'ISIC_0000021']
    for id_ in ids:
        Image.fromarray(rng.randint(0, 255, (192, 256, 3)).astype(np.uint8)).save(os.path.join(img_dir, id_ + '.jpg'))
        Image.fromarray(((rng.rand(192, 256) > 0.6) * 255).astype(np.uint8)).save(os.path.join(lab_dir, id_ + '_segmentation.png'))
    mf = mgt.ModelFiles(str(tmp_path / 'train'), 'isic')
    mgt.save_model(mf, 'unet', params, uo.synthetic_state(21, **params))
    text = tgs.ISIC_MC_YAML.format(test_dir=str(tmp_path / 'out'), model_dir=mf.model_dir, dataset=str(prefix))
    assert '    mc: 2\n' in text
    cfg = str(tmp_path / 'test_isic_tta_affine.yaml')
    with open(cfg, 'w') as f:
        f.write(text.replace('    mc: 2\n', KEY_YAML))
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bin-dl', 'isic_test_default.py'), '-config_file', cfg], capture_output=True, text=True,
                       timeout=400, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    files = _written(str(tmp_path / 'out'))
    for id_ in ids:
        p = nifti.read(os.path.join(glob.glob(str(tmp_path / 'out' / '*'))[0], id_ + '_probabilities.nii.gz'))[0]
        assert p.shape == (192, 256) and p.dtype == np.float32 and np.all((p >= 0) & (p <= 1))
        assert id_ + '_prediction.nii.gz' in files
    record = _record(str(tmp_path / 'out'))
    assert record['samples'] == 3 and record['mc'] == 0 and record['matrices'][0] == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
