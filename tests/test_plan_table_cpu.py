"""The planner's decisions against the snapshot tests/golden/g30_plan_table.npz (tests/golden/generate_plan_table.py; no GPU): every case of the
fixture is planned again, and every exact field of every rcu_layer_info row -- through the stored hash -- and the executed-work figures must be
what the library that recorded the fixture gave."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import generate_plan_table as gen  # noqa: E402


def test_planner_reproduces_the_plan_table():
    g = load_golden('g30_plan_table')
    case_list = json.loads(str(g['cases']))
    assert len(case_list) == len(g['hashes']) == len(g['counts']) >= 500 + 4 * 2 * 6 * 12
    assert [list(c) for c in gen.cases()] == case_list     # the fixture holds the generator's cases
    hashes, counts, mfma, seen = gen.compute(case_list)
    bad = [case_list[i] for i in np.nonzero((hashes != g['hashes']) | (counts != g['counts']))[0]]
    assert not bad, (len(bad), bad[:5])
    assert mfma.shape == g['mfma'].shape and mfma == pytest.approx(g['mfma'], rel=1e-12)
    # every kernel that can be a plan entry is pinned by at least one case
    assert sorted(seen) == [str(k) for k in g['kernels']] == gen.KERNELS and len(seen) == 28
    assert os.path.getsize(os.path.join(GOLDEN, 'g30_plan_table.npz')) < 256 * 1024
