#!/usr/bin/env python3
"""G29: yardsticks of the input corruptions (include/rcu.h, "Input corruptions").

Everything comes from tests/corruption_reference.py, the float64 numpy / scipy restatement of the eight definitions (the Gaussian blur is
scipy.ndimage.gaussian_filter itself, the normals are Philox4x32-10 of oracle.mask_oracle with float64 transcendentals).

  x_<C>x<H>x<W>          the seeded float32 inputs [3, C, H, W] of the four shapes of the GPU tests
  y_<case>               the expected output of every (kind, amount) of corruption_reference.CASES on the smallest shape, 4 x 15 x 16, under
                         KEY at first_sample 2^32 + 5: float64 (float32 for intensity_shift and channel_drop, which are bit-exact)
  cases, key, first_sample, golden_shape

The expected outputs of the three larger shapes are computed by the same restatement when the tests run: as float64 arrays of every case
they would take several megabytes.

    python tests/golden/generate_corruptions.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import corruption_reference as cr  # noqa: E402

GOLDEN_SHAPE = cr.SHAPES[0]


def main():
    out = {}
    for shape in cr.SHAPES:
        out['x_{}x{}x{}'.format(*shape)] = cr.make_input(shape)
    x = out['x_{}x{}x{}'.format(*GOLDEN_SHAPE)]
    names = []
    for kind, amount in cr.CASES:
        amount = cr.case_amount(kind, amount, GOLDEN_SHAPE[0])
        name = cr.case_name(kind, None if kind == 'channel_drop' else amount)
        names.append(name)
        out['y_' + name] = cr.reference(kind, x, amount, cr.KEY, cr.FIRST_SAMPLE)
    out['cases'] = np.array(names)
    out['key'] = np.uint64(cr.KEY)
    out['first_sample'] = np.uint64(cr.FIRST_SAMPLE)
    out['golden_shape'] = np.array(GOLDEN_SHAPE, dtype=np.int64)
    path = os.path.join(HERE, 'g29_corruptions.npz')
    np.savez_compressed(path, **out)
    print('wrote {} ({} bytes)'.format(path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
