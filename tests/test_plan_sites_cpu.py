"""The plan's dropout sites against the snapshot tests/golden/g35_plan_sites.json (tests/golden/generate_plan_sites.py; no GPU): every case of
G30 is planned again, and the hash over the sites' names and channels, rcu_unet_mask_floats_per_sample and rcu_unet_num_layers must be what the
library that recorded the fixture gave.  G30 (test_plan_table_cpu.py) pins the rcu_layer_info rows of the same cases; this is what they do not show."""
import json
import os
import sys

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import generate_plan_sites as gen  # noqa: E402
import generate_plan_table as table  # noqa: E402


def test_planner_reproduces_the_plan_sites():
    path = os.path.join(GOLDEN, 'g35_plan_sites.json')
    with open(path) as f:
        g = json.load(f)
    case_list = table.cases()
    assert g['fields'] == ['sites_hash', 'mask_floats_per_sample', 'num_layers']
    assert len(g['rows']) == len(case_list) >= 500 + 4 * 2 * 6 * 12      # one row per G30 case
    rows = gen.compute(case_list)
    bad = [(case_list[i], rows[i], g['rows'][i]) for i in range(len(rows)) if rows[i] != g['rows'][i]]
    assert not bad, (len(bad), bad[:5])
    assert os.path.getsize(path) < 256 * 1024
