#!/usr/bin/env python3
"""G35: the parts of a plan that rcu_layer_info does not show but the ABI can read (no GPU): per case of G30 (generate_plan_table.cases) the
dropout sites of the rcu_unet_plan handle -- a 64-bit hash over their names and channel counts, in order --, rcu_unet_mask_floats_per_sample and
rcu_unet_num_layers.  The sites decide which rows of a mask tensor a layer reads (csrc/rcu_plan.hip builds them with the layers), so a planner
that kept every rcu_layer_info row and lost or reordered a site would pass G30 and fail here.

Run once against a library of the commit whose planner is to be pinned:
    RCU_HIP_LIBRARY=/path/to/librcu_hip.so python tests/golden/generate_plan_sites.py
Output: tests/golden/g35_plan_sites.json.
"""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for path in (os.path.dirname(TESTS), TESTS, HERE):
    if path not in sys.path:
        sys.path.insert(0, path)
PATH = os.path.join(HERE, 'g35_plan_sites.json')


def plan_sites(height, width, max_batch, options=None, **desc):
    """(sites hash, mask floats per sample, layers) of the plan plan_rows reads its rows from"""
    from plan_rows import DESC_DEFAULTS
    from rcu_amd import _lib
    lib = _lib.load()
    fields = dict(DESC_DEFAULTS, **desc)
    d = _lib.UnetDesc(height=height, width=width, max_batch=max_batch, **{k: int(v) for k, v in fields.items()})
    opts = _lib.UnetOptions()
    lib.rcu_unet_default_options(ctypes.byref(opts))
    for key, value in (options or {}).items():
        assert hasattr(opts, key), key
        setattr(opts, key, value)
    handle = ctypes.c_void_p()
    _lib.check(lib.rcu_unet_plan(ctypes.byref(d), ctypes.byref(opts), ctypes.byref(handle)))
    try:
        sites = [(lib.rcu_unet_dropout_site_name(handle, s).decode(), lib.rcu_unet_dropout_site_channels(handle, s))
                 for s in range(lib.rcu_unet_num_dropout_sites(handle))]
        digest = hashlib.sha256(repr(sites).encode()).digest()
        return int.from_bytes(digest[:8], 'little'), lib.rcu_unet_mask_floats_per_sample(handle), lib.rcu_unet_num_layers(handle)
    finally:
        lib.rcu_unet_destroy(handle)


def compute(case_list):
    """[[sites hash as hex, mask floats per sample, layers]] per case"""
    out = []
    for h, w, n, desc, options in case_list:
        sites, mask_floats, layers = plan_sites(h, w, n, options, **desc)
        out.append(['{:016x}'.format(sites), mask_floats, layers])
    return out


def main():
    import generate_plan_table as table
    rows = compute(table.cases())
    assert all(r[1] > 0 for r in rows) and len({r[0] for r in rows}) > 20, 'every case has dropout sites, and the cases differ in them'
    with open(PATH, 'w') as f:
        json.dump(dict(cases='tests/golden/generate_plan_table.py cases()', fields=['sites_hash', 'mask_floats_per_sample', 'num_layers'], rows=rows), f,
                  separators=(',', ':'))
        f.write('\n')
    print('{}: {} cases, {} distinct site tables, {} bytes'.format(PATH, len(rows), len({r[0] for r in rows}), os.path.getsize(PATH)))


if __name__ == '__main__':
    main()
