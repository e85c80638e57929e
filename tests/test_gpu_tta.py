"""Test-time augmentation on the GPU: the two kernels against their torch definitions bit for bit, TtaMcPredictStep against McPredictStep,
against itself under the group action, against the oracle forward composed with numpy transforms, and through the drop-in scripts (one
process, other batch sizes, two ranks)."""
import glob
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

NAMES = ('identity', 'flip_h', 'flip_v', 'rot180', 'transpose', 'rot90', 'rot270', 'anti_transpose')
FLIPS = NAMES[:4]
NUMPY_OPS = {
    'identity': lambda a: a,
    'flip_h': lambda a: np.flip(a, -1),
    'flip_v': lambda a: np.flip(a, -2),
    'rot180': lambda a: np.flip(a, (-2, -1)),
    'transpose': lambda a: np.swapaxes(a, -2, -1),
    'rot90': lambda a: np.rot90(a, 1, (-2, -1)),
    'rot270': lambda a: np.rot90(a, 3, (-2, -1)),
    'anti_transpose': lambda a: np.swapaxes(np.rot90(a, 2, (-2, -1)), -2, -1),
}
NUMPY_INVERSE = {'rot90': 'rot270', 'rot270': 'rot90'}
OUTPUTS = ('probabilities', 'entropy', 'mutual_info', 'variance')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _model(params, state, dev):
    from rcu_amd.model import UNet
    m = UNet(**params)
    m.load_state_dict(state)
    return m.to(dev).eval()


def _run(step, model, x, do_mi=True, do_var=True, first=0):
    from rcu_amd import steps
    bc = steps.BatchContext({'images': x.clone()}, 0, first)
    ctx = steps.TorchTestContext('cuda', model)
    step(bc, None, ctx)
    steps.MultiPredictionSummary(do_mi=do_mi, do_var=do_var)(bc, None, ctx)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in bc.output.items()}


@pytest.mark.timeout(300)
def test_transform_kernel_is_the_torch_op_bit_for_bit(dev):
    from rcu_amd import steps
    g = torch.Generator().manual_seed(1)
    cases = [((2, 3, 240, 240), NAMES), ((3, 4, 16, 16), NAMES), ((2, 4, 192, 256), FLIPS), ((2, 3, 15, 17), FLIPS), ((1, 1, 33, 33), NAMES)]
    for shape, names in cases:
        x = torch.randn(*shape, generator=g).to(dev)
        for name in names:
            got = steps.tta_transform(x, name)
            torch.cuda.synchronize()
            assert torch.equal(got, steps.tta_torch(x, name).contiguous()), (shape, name)
    with pytest.raises(ValueError):
        steps.tta_transform(torch.zeros(1, 1, 4, 6, device=dev), 'rot90')


@pytest.mark.timeout(300)
@pytest.mark.parametrize('flags', ['EXACT|MI|VAR', 'EXACT', 'VAR', 'float32'])
def test_fold_kernel_is_dst_plus_the_permuted_src(dev, flags):
    from rcu_amd import _lib, steps
    bits = {'EXACT|MI|VAR': _lib.RCU_MC_EXACT | _lib.RCU_MC_MI | _lib.RCU_MC_VAR, 'EXACT': _lib.RCU_MC_EXACT, 'VAR': _lib.RCU_MC_VAR,
            'float32': _lib.RCU_MC_MI}[flags]
    do_mi, do_var, exact = bool(bits & _lib.RCU_MC_MI), bool(bits & _lib.RCU_MC_VAR), bool(bits & _lib.RCU_MC_EXACT)
    g = torch.Generator().manual_seed(2)
    for n, c, h, w in ((3, 2, 240, 240), (2, 3, 16, 16), (2, 2, 192, 256), (1, 2, 15, 17)):
        names = NAMES if h == w else FLIPS
        for name in names:
            src = steps.McStatistics(n, c, h, w, dev, do_mi, do_var, exact=exact)
            dst = steps.McStatistics(n, c, h, w, dev, do_mi, do_var, exact=exact)
            src.blob.copy_(torch.rand(src.blob.numel(), generator=g, dtype=torch.float64).to(src.blob.dtype).to(dev) * 4)
            dst.blob.copy_(torch.rand(dst.blob.numel(), generator=g, dtype=torch.float64).to(dst.blob.dtype).to(dev) * 4)
            src.count, dst.count = 3, 5
            planes = src.blob.numel() // (h * w)
            expected = dst.blob.view(planes, h, w) + steps.tta_torch(src.blob.view(planes, h, w), steps.TTA_INVERSE[steps.tta_element(name)])
            steps.fold_transformed(src, dst, name)
            torch.cuda.synchronize()
            assert torch.equal(dst.blob.view(planes, h, w), expected), (flags, (n, c, h, w), name)
            assert dst.count == 8


PARAMS = dict(nb_classes=2, in_channels=4, depth=3, start_filters=32, dropout=0.05)


@pytest.mark.timeout(300)
def test_identity_tta_is_mc_dropout_bit_for_bit(dev):
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    m = _model(PARAMS, uo.synthetic_state(31, **PARAMS), dev)
    x = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(3))
    mc = _run(steps.McPredictStep(4, do_mi=True, do_var=True, lanes=2, seed=7), m, x, first=10)
    tta = _run(steps.TtaMcPredictStep(['identity'], mc_steps=4, seed=7, lanes=2, do_mi=True, do_var=True), m, x, first=10)
    assert set(tta) == set(mc)
    for key in set(OUTPUTS) | {'ws_probabilities'}:
        assert torch.equal(tta[key], mc[key]), key
    # another element changes the samples (its keys differ), the counts stay
    other = _run(steps.TtaMcPredictStep(['flip_h'], mc_steps=4, seed=7, lanes=2, do_mi=True, do_var=True), m, x, first=10)
    assert not torch.equal(other['probabilities'], mc['probabilities'])


@pytest.mark.timeout(600)
@pytest.mark.parametrize('shape,group', [((2, 4, 32, 32), NAMES), ((2, 4, 32, 48), FLIPS)], ids=['d4-square', 'flips-rect'])
def test_tta_over_the_whole_group_is_equivariant(dev, shape, group):
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    m = _model(PARAMS, uo.synthetic_state(32, **PARAMS), dev)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(4))
    base = _run(steps.TtaMcPredictStep(group, ws_pass=False, do_mi=True, do_var=True), m, x)
    for name in group:
        moved = _run(steps.TtaMcPredictStep(group, ws_pass=False, do_mi=True, do_var=True), m, steps.tta_torch(x, name).contiguous())
        for key in OUTPUTS:
            assert torch.equal(moved[key], steps.tta_torch(base[key], name).contiguous()), (name, key)


def _oracle_summary(per_sample_probs):
    ps = torch.stack(per_sample_probs)
    p_mean = ps.mean(0)
    ent = -(torch.where(p_mean > 0, p_mean * p_mean.log(), torch.zeros_like(p_mean))).sum(1, keepdim=True)
    ent_t = torch.stack([-(torch.where(p > 0, p * p.log(), torch.zeros_like(p))).sum(1, keepdim=True) for p in ps]).mean(0)
    var = ps.var(0, unbiased=True).mean(1, keepdim=True) if len(per_sample_probs) > 1 else None
    return {'probabilities': p_mean, 'entropy': ent, 'mutual_info': ent - ent_t, 'variance': var}


def _back(p, name):
    """numpy: map a [N, C, H, W] prediction of transformed images back (g^-1)."""
    return torch.from_numpy(np.ascontiguousarray(NUMPY_OPS[NUMPY_INVERSE.get(name, name)](p.numpy())))


@pytest.mark.timeout(900)
@pytest.mark.parametrize('case', ['eval-64', 'mc-64', 'eval-240'])
def test_tta_against_the_oracle_forward_on_transformed_inputs(dev, case):
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    params = dict(PARAMS, depth=4) if case == 'eval-240' else dict(PARAMS)
    st = uo.synthetic_state(33, **params)
    m = _model(params, st, dev)
    n, hw = (1, 240) if case == 'eval-240' else (2, 64)
    names = ('identity', 'flip_h', 'transpose', 'rot90') if case == 'eval-240' else NAMES
    T = 2 if case == 'mc-64' else 0
    x = torch.randn(n, 4, hw, hw, generator=torch.Generator().manual_seed(5))
    first = 3
    got = _run(steps.TtaMcPredictStep(names, mc_steps=T, seed=11, do_mi=True, do_var=True), m, x, first=first)
    sites = m.dropout_sites()
    probs = []
    for name in names:
        xt = torch.from_numpy(np.ascontiguousarray(NUMPY_OPS[name](x.numpy())))
        for t in range(1, max(T, 1) + 1):
            mk = None
            if T:
                steps.set_dropout_mode(m, True)
                flat = m.seeded_masks(n, dev, [steps.tta_pass_seed(11, name, t)], first)
                steps.set_dropout_mode(m, False)
                mk = [f.view(n, -1).cpu() for f in torch.split(flat, [n * c for _, c in sites])]      # [site][n][C_site]
            logits = uo.unet_forward(st, xt, mk, **params)
            probs.append(_back(torch.softmax(logits.double(), 1), name))
    ref = _oracle_summary(probs)
    tol = 1e-6 if hw == 64 else 1e-4         # (the padded-level comparisons: PROB_TOL)
    for key in OUTPUTS:
        d = float((got[key].double() - ref[key]).abs().max())
        assert d < tol, (case, key, d)
    lg0 = uo.unet_forward(st, x, None, **params)
    assert float((got['ws_probabilities'].double() - torch.softmax(lg0.double(), 1)).abs().max()) < tol
    # the replayed recipe: V x T volumes in canonical orientation, transform-major
    bc = steps.BatchContext({'images': x.clone()}, 0, first)
    steps.TtaMcPredictStep(names, mc_steps=T, seed=11)(bc, None, steps.TorchTestContext('cuda', m))
    multi = bc.output['multi_probabilities'].as_tensor()
    assert tuple(multi.shape) == (len(names) * max(T, 1), n, 2, hw, hw)
    for i, p in enumerate(probs):
        assert float((multi[i].cpu().double() - p).abs().max()) < tol, i


@pytest.mark.timeout(600)
def test_transform_order_lanes_and_pass_groups_do_not_change_the_bytes(dev):
    from oracle import unet_oracle as uo
    from rcu_amd import steps
    m = _model(PARAMS, uo.synthetic_state(34, **PARAMS), dev)
    x = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(6))
    names = ['identity', 'flip_h', 'rot90', 'anti_transpose']

    def run(order, lanes, group_pixels=None):
        return _run(steps.TtaMcPredictStep(order, mc_steps=3, seed=5, lanes=lanes, group_pixels=group_pixels, do_mi=True, do_var=True), m, x)

    base = run(names, 2)
    for other in (run(names[::-1], 2), run(names, 1), run(['rot90', 'identity', 'anti_transpose', 'flip_h'], 1), run(names, 2, 2 * 32 * 32),
                  run(names, 1, 2 * 32 * 32)):
        for key in set(OUTPUTS) | {'ws_probabilities'}:
            assert other[key].numpy().tobytes() == base[key].numpy().tobytes(), key


# ------------------------------------------------------------------------------------------------------------- the drop-in scripts
def _free_port():
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        return sock.getsockname()[1]


def _launch_ranks(script, cfg, env, ranks=2):
    """`python -m torch.distributed.run --nproc-per-node <ranks> <script> -config_file <cfg>` (ranks on the one GPU: the scripts take gloo)."""
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(ranks), '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), script, '-config_file', cfg]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=500, cwd=ROOT, env=env)


def _written(out_root):
    dirs = glob.glob(os.path.join(out_root, '*'))
    assert len(dirs) == 1, dirs
    return {os.path.basename(f): open(f, 'rb').read() for f in sorted(glob.glob(os.path.join(dirs[0], '*')))
            if f.endswith(('.nii.gz', 'metrics.csv'))}


def _brats_cfgs(tmp_path, tags):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_gpu_scripts as tgs
    cfg, vols, _, _ = tgs._setup(tmp_path, mc=2)
    text = open(cfg).read()
    assert '    mc: 2\n' in text and 'batch_size: 4' in text
    text = text.replace('    mc: 2\n', '    mc: 2\n    tta: [identity, flip_h, flip_v, rot180]\n')
    out = {}
    for tag, batch in tags:
        path = str(tmp_path / 'cfg_{}.yaml'.format(tag))
        with open(path, 'w') as f:
            f.write(text.replace(str(tmp_path / 'out'), str(tmp_path / 'out_{}'.format(tag))).replace('batch_size: 4', 'batch_size: {}'.format(batch)))
        out[tag] = path
    return out, vols


@pytest.mark.timeout(1500)
def test_brats_script_with_tta_and_mc_batch_sizes_and_two_ranks(tmp_path):
    cfgs, vols = _brats_cfgs(tmp_path, [('b8', 8), ('b32', 32), ('two', 8)])
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('WORLD_SIZE', None)
    path = os.path.join(ROOT, 'bin-dl', 'brats_test_default.py')
    for tag in ('b8', 'b32'):
        r = subprocess.run([sys.executable, path, '-config_file', cfgs[tag]], capture_output=True, text=True, timeout=500, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    b8, b32 = _written(str(tmp_path / 'out_b8')), _written(str(tmp_path / 'out_b32'))
    assert len(b8) == 2 * len(vols) + 1 and sorted(b8) == sorted(b32)
    for name in b8:
        assert b8[name] == b32[name], name
    r = _launch_ranks(path, cfgs['two'], env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    two = _written(str(tmp_path / 'out_two'))
    assert sorted(two) == sorted(b8)
    for name in b8:
        assert two[name] == b8[name], name


@pytest.mark.timeout(900)
def test_isic_script_with_tta_alone_writes_its_files(tmp_path):
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
        Image.fromarray(rng.randint(0, 255, (64, 96, 3)).astype(np.uint8)).save(os.path.join(img_dir, id_ + '.jpg'))
        Image.fromarray(((rng.rand(64, 96) > 0.6) * 255).astype(np.uint8)).save(os.path.join(lab_dir, id_ + '_segmentation.png'))
    mf = mgt.ModelFiles(str(tmp_path / 'train'), 'isic')
    mgt.save_model(mf, 'unet', params, uo.synthetic_state(21, **params))
    text = tgs.ISIC_MC_YAML.format(test_dir=str(tmp_path / 'out'), model_dir=mf.model_dir, dataset=str(prefix))
    assert '    mc: 2\n' in text
    cfg = str(tmp_path / 'test_isic_tta.yaml')
    with open(cfg, 'w') as f:
        f.write(text.replace('    mc: 2\n', '    tta: [identity, flip_h, flip_v]\n'))
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bin-dl', 'isic_test_default.py'), '-config_file', cfg], capture_output=True, text=True,
                       timeout=500, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    files = _written(str(tmp_path / 'out'))
    for id_ in ids:
        p = nifti.read(os.path.join(glob.glob(str(tmp_path / 'out' / '*'))[0], id_ + '_probabilities.nii.gz'))[0]
        assert p.shape == (64, 96) and p.dtype == np.float32 and np.all((p >= 0) & (p <= 1))
        assert id_ + '_prediction.nii.gz' in files
    # a transposing element on rectangular images is refused at the first batch, naming the element and the shape
    from rcu_amd import steps
    m = _model(params, uo.synthetic_state(21, **params), torch.device('cuda:0'))
    bc = steps.BatchContext({'images': torch.zeros(1, 3, 64, 96)}, 0)
    with pytest.raises(ValueError, match='rot90.*64 x 96'):
        steps.TtaMcPredictStep(['identity', 'rot90'])(bc, None, steps.TorchTestContext('cuda', m))
