#!/usr/bin/env python3
"""G25: the host metric arithmetic, bit for bit.

`ue_curve_metrics`, `component_metrics`, `boundary_metrics` and `surface_distance_metrics` turn integer tables into the floats that the
evaluation actions write into their CSV files with `str()`.  This fixture pins every one of those floats as `float.hex()`, so that a
rearrangement of the arithmetic that moves a last bit (another order of summation, a second rounding) shows up without a GPU:
  ue_curves    the level histograms (1000 levels) of G22's cases a, b, c, whole volume and inside the mask, and the sum of the three whole ones
  components   every table pair of G23 (5 cases x 2 connectivities) at 1000 and 7 levels, and per connectivity the five pairs concatenated
  boundary     G24's boundary tables (5 cases x 3 and 10 bands) and per band count the sum of the five
  surface      the surface-distance histograms of G24's five cases
Integers are stored as integers, floats as hex strings ('nan' for NaN), arrays as nested lists.  `compute()` is what the test calls.
Output: tests/golden/g25_metric_floats.json.

    python tests/golden/generate_metric_floats.py
"""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for path in (os.path.dirname(TESTS), TESTS):
    if path not in sys.path:
        sys.path.insert(0, path)
PATH = os.path.join(HERE, 'g25_metric_floats.json')


def encode(value):
    """float -> float.hex() ('nan' for any NaN), integer -> int, array / sequence -> nested lists, dict -> dict."""
    if isinstance(value, dict):
        return {str(k): encode(v) for k, v in value.items()}
    if isinstance(value, np.ndarray):
        return [encode(v) for v in value.tolist()]
    if isinstance(value, (list, tuple)):
        return [encode(v) for v in value]
    if isinstance(value, (bool, np.bool_)):
        return bool(value)
    if isinstance(value, (int, np.integer)):
        return int(value)
    value = float(value)
    return 'nan' if math.isnan(value) else value.hex()


def compute():
    from conftest import load_golden
    import test_boundary_cpu as tb
    import test_components_cpu as tc
    import test_ue_curves_cpu as tu
    from rcu_amd import evaluation as ev

    out = {'ue_curves': {}, 'components': {}, 'boundary': {}, 'surface': {}}
    g = load_golden('g22_ue_curves')
    whole = []
    for tag in 'abc':
        pr, tg, unc, mask = (g['{}_{}'.format(tag, k)] for k in ('prediction', 'target', 'uncertainty', 'mask'))
        whole.append(tu.numpy_histogram(pr, tg, unc, 1000))
        out['ue_curves'][tag] = ev.ue_curve_metrics(whole[-1])
        out['ue_curves'][tag + '_masked'] = ev.ue_curve_metrics(tu.numpy_histogram(pr, tg, unc, 1000, mask=mask))
    out['ue_curves']['sum'] = ev.ue_curve_metrics(whole[0] + whole[1] + whole[2])

    pairs = {6: [], 26: []}
    for name, conn, _, _, _, ref in tc.fixture_cases():
        pair = (tc.as_table(ref['pred_table']), tc.as_table(ref['target_table']))
        pairs[conn].append(pair)
        for levels in (1000, 7):
            out['components']['{}_c{}_l{}'.format(name, conn, levels)] = ev.component_metrics(*pair, levels)
    for conn, of_conn in pairs.items():
        out['components']['concatenated_c{}'.format(conn)] = ev.component_metrics(np.concatenate([p[0] for p in of_conn]),
                                                                                   np.concatenate([p[1] for p in of_conn]))

    g = tb.golden()
    for bands in (3, 10):
        tables = [tb.as_table(g['{}_table_r{}'.format(name, bands)]) for name in tb.CASES]
        for name, table in zip(tb.CASES, tables):
            out['boundary']['{}_r{}'.format(name, bands)] = ev.boundary_metrics(table)
        out['boundary']['sum_r{}'.format(bands)] = ev.boundary_metrics(ev.add_boundary_tables(tables))
    for name in tb.CASES:
        out['surface'][name] = ev.surface_distance_metrics(tb.histogram_of(g[name + '_sq_p_to_t'], g[name + '_sq_t_to_p']))
    return encode(out)


def main():
    out = compute()
    with open(PATH, 'w') as f:          # one line per table: small, and a diff names the table
        f.write('{\n' + ',\n'.join('"{}": {{\n{}\n}}'.format(section, ',\n'.join(
            '"{}": {}'.format(k, json.dumps(v, sort_keys=True, separators=(',', ':'))) for k, v in sorted(out[section].items())))
            for section in sorted(out)) + '\n}\n')
    with open(PATH) as f:
        assert json.load(f) == out
    print('wrote {} ({:.1f} KiB)'.format(PATH, os.path.getsize(PATH) / 1024))


if __name__ == '__main__':
    main()
