"""bench.py's plain run and its --dump-outputs files: the headline line alone, the outputs of the last timed step as .npy files
within the size budget, the same files from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_the_same_rows_of_every_array_within_the_budget(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    gen = torch.Generator().manual_seed(3)
    out = {'probabilities': torch.rand(40, 2, 8, 8, generator=gen), 'entropy': torch.rand(40, 8, 8, generator=gen),
           'variance': torch.rand(40, 8, 8, generator=gen, dtype=torch.float64), 'half': torch.rand(40, 4, generator=gen).half()}
    total = sum(t.numel() * (8 if t.dtype == torch.float64 else 4) for t in out.values())
    # under the budget: every array whole
    written = bench.dump_outputs(out, str(tmp_path / 'whole'), budget=total)
    assert written == {k: list(t.shape) for k, t in out.items()}
    for k, t in out.items():
        a = np.load(str(tmp_path / 'whole' / (k + '.npy')))
        assert a.dtype == (np.float64 if t.dtype == torch.float64 else np.float32)
        assert np.array_equal(a, t.double().numpy() if t.dtype == torch.float64 else t.float().numpy())
    # over the budget: the same seeded rows of every array, the same rows on every call, the files within the budget
    budget = total // 3
    first = bench.dump_outputs(out, str(tmp_path / 'a'), budget=budget)
    bench.dump_outputs(out, str(tmp_path / 'b'), budget=budget)
    rows = first['entropy'][0]
    assert 1 <= rows < 40 and all(shape[0] == rows for shape in first.values())
    assert sum(os.path.getsize(str(tmp_path / 'a' / (k + '.npy'))) - 128 for k in out) <= budget
    ent = np.load(str(tmp_path / 'a' / 'entropy.npy'))
    idx = [int(np.flatnonzero((out['entropy'].numpy() == r).all(axis=(1, 2)))[0]) for r in ent]
    assert idx == sorted(idx) and len(set(idx)) == rows
    assert np.array_equal(np.load(str(tmp_path / 'a' / 'probabilities.npy')), out['probabilities'].numpy()[idx])
    for k in out:
        assert np.array_equal(np.load(str(tmp_path / 'a' / (k + '.npy'))), np.load(str(tmp_path / 'b' / (k + '.npy'))))


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_bench_prints_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    lines, dirs = [], []
    for run in ('a', 'b'):
        d = str(tmp_path / run)
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '2', '--warmup', '1', '--mc', '3', '--dump-outputs', d]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        found = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
        assert len(found) == 1
        lines.append(json.loads(found[0]))
        dirs.append(d)
    b = lines[0]
    assert b['steps'] == 2 and b['warmup'] == 1 and b['n_gpus'] == 1 and b['higher_is_better'] is True and b['dtype'] == 'f32'
    assert b['unit'] == 'MC-sample-volumes/s' and b['ms_per_step'] > 0
    assert abs(b['value'] - 3 * 1e3 / b['ms_per_step']) < 1e-6 * b['value']        # T = 3 sample-volumes per step
    assert b['forwards_per_rank'] == [2 * 4]                                          # 2 steps x (3 MC passes + the weight-scaling pass)
    for key in ('roofline', 'resident', 'cpu_baseline', 'parity', 'all_outputs', 'calibration_kernels', 'native_shapes'):
        assert key not in b                                                           # what --full measures
    names = sorted(os.listdir(dirs[0]))
    assert names == ['entropy.npy', 'probabilities.npy', 'ws_probabilities.npy'] and sorted(os.listdir(dirs[1])) == names
    assert sum(os.path.getsize(os.path.join(dirs[0], n)) for n in names) <= 64000000
    p = np.load(os.path.join(dirs[0], 'probabilities.npy'))
    e = np.load(os.path.join(dirs[0], 'entropy.npy'))
    assert p.dtype == np.float32 and p.ndim == 4 and p.shape[1:] == (2, 192, 128) and e.shape == (p.shape[0], 1, 192, 128)
    assert np.abs(p.sum(axis=1) - 1).max() < 1e-5 and float(e.min()) >= 0 and float(p.std()) > 0
    for n in names:
        assert np.array_equal(np.load(os.path.join(dirs[0], n)), np.load(os.path.join(dirs[1], n))), n
