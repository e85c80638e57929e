#!/usr/bin/env python3
"""G24: yardsticks of the squared distance transform, the border shell, the surface distances and the boundary table.

Run in the build container only: the border shell and the distance map come from the REFERENCE's own labelhelper.boarder_mask
(common/utils/labelhelper.py:12-20, imported from RCU_REFERENCE_ROOT), everything else from scipy.ndimage and numpy.  What is committed is
data (masks, maps and the arrays the reference and scipy produced for them).

Cases (target mask ``<case>_target``, prediction ``<case>_prediction`` = the target shifted and perturbed, float64 ``<case>_uncertainty``):
  box     10 x 24 x 30   a box with a hole and a one-voxel island
  blobs   10 x 32 x 40   two touching blobs
  face     8 x 20 x 22   a blob that touches the volume face
  rand     6 x 15 x 17   random, 50 % foreground
  img         48 x 64    a 2-D image (depth 1): an ellipse with noise
Every mask holds both classes -- the condition under which the reference's output is meaningful; asserted for every case, none left out.

Per case:
  _dist11, _mask11, _dist23, _mask23   labelhelper.boarder_mask(target, 1, 1) and (target, 2, 3): float64 distance, bool mask
  _edt_sq_in, _edt_sq_out              rint(distance_transform_edt(target) ** 2), rint(distance_transform_edt(~target) ** 2), uint32
  _surface_prediction, _surface_target A & ~binary_erosion(A, border_value=1)
  _sq_p_to_t, _sq_t_to_p               sorted int64 squared distances of the prediction's surface voxels to the target's surface and back
  _hd, _hd95, _assd                    max / numpy.percentile(.., 95) / mean of both directions' float64 distances together
  _table_r3, _table_r10                int64 [2, R + 1, 4]: voxels, errors, unc_sum, unc_err_sum per (side, band), q as in G23's generator
Output: tests/golden/g24_boundary.npz (arrays and numbers only).

    python tests/golden/generate_boundary.py
"""
import os
import sys

import scipy                    # (before the np.bool shim: the other order breaks numpy)
from scipy import ndimage
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get('RCU_REFERENCE_ROOT', '/root/reference')
ONE = 1 << 24


def quantise(u):
    with np.errstate(invalid='ignore'):
        q = np.rint(np.clip(np.asarray(u, dtype=np.float64), 0.0, 1.0) * np.float64(ONE))
    return np.where(np.isnan(q), 0, q).astype(np.int64)


def surface(a):
    a = a != 0
    return a & ~ndimage.binary_erosion(a, border_value=1)


def boundary_table(prediction, target, d_sq, q, bands):
    """d_sq: the squared distance to the nearest voxel of the other class of the target."""
    side = (target != 0).astype(np.int64)
    error = (prediction != 0) != (target != 0)
    band = np.full(target.shape, bands, dtype=np.int64)
    for k in range(bands - 1, -1, -1):
        band[d_sq <= (k + 1) ** 2] = k
    table = np.zeros((2, bands + 1, 4), dtype=np.int64)
    for s in range(2):
        for b in range(bands + 1):
            cell = (side == s) & (band == b)
            table[s, b] = [cell.sum(), (cell & error).sum(), q[cell].sum(), q[cell & error].sum()]
    return table


def make_cases(rng):
    cases = {}
    t = np.zeros((10, 24, 30), dtype=np.uint8)
    t[2:8, 4:18, 5:22] = 1
    t[4:6, 8:12, 10:15] = 0          # the hole
    t[8, 21, 27] = 1                 # the island
    cases['box'] = t
    z, y, x = np.indices((10, 32, 40))
    t = (((z - 5) ** 2 + (y - 14) ** 2 + (x - 12) ** 2 <= 64) | ((z - 4) ** 2 * 2 + (y - 18) ** 2 + (x - 27) ** 2 <= 81)).astype(np.uint8)
    cases['blobs'] = t
    z, y, x = np.indices((8, 20, 22))
    cases['face'] = ((z ** 2 + (y - 9) ** 2 + (x - 21) ** 2 <= 49)).astype(np.uint8) * 2
    cases['rand'] = (rng.rand(6, 15, 17) < 0.5).astype(np.uint8)
    y, x = np.indices((48, 64))
    t = (((y - 22) / 14.0) ** 2 + ((x - 30) / 21.0) ** 2 <= 1).astype(np.uint8)
    t ^= (rng.rand(48, 64) < 0.02).astype(np.uint8)
    cases['img'] = t
    return cases


def main():
    sys.path.insert(0, REFERENCE_ROOT)
    if not hasattr(np, 'bool'):      # the reference uses np.bool (labelhelper.py:13)
        np.bool = bool
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')       # scipy.ndimage.morphology is a deprecated namespace
        from common.utils import labelhelper

    rng = np.random.RandomState(24)
    arrays = {'scipy_version': np.array(scipy.__version__), 'numpy_version': np.array(np.__version__)}
    cases = make_cases(rng)
    arrays['cases'] = np.array(list(cases))
    checked = 0
    for name, target in cases.items():
        shift = np.roll(target != 0, 1, axis=target.ndim - 1)
        prediction = ((shift & (rng.rand(*target.shape) < 0.95)) | (rng.rand(*target.shape) < 0.01)).astype(np.uint8)
        for m in (target, prediction):
            assert (m != 0).any() and (m == 0).any(), name      # both classes: the reference is meaningful
        checked += 1
        u = np.rint(rng.rand(*target.shape) * 4096) / 4096     # (few mantissa bits: the file stays small) ...
        flat = u.reshape(-1)
        flat[:160] = rng.rand(160)                                 # ... a run of full-precision values
        flat[161:201:5] = (np.arange(8) + 0.5) / ONE              # exact ties of the rounding: to even
        flat[203], flat[207], flat[212], flat[217] = -0.25, 1.5, np.nan, 1.0
        arrays.update({name + '_target': target, name + '_prediction': prediction, name + '_uncertainty': u})

        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            dist11, mask11 = labelhelper.boarder_mask(target, 1, 1)
            dist23, mask23 = labelhelper.boarder_mask(target, 2, 3)
        edt_in = ndimage.distance_transform_edt(target != 0)
        edt_out = ndimage.distance_transform_edt(target == 0)
        sq_in, sq_out = np.rint(edt_in ** 2), np.rint(edt_out ** 2)
        assert np.array_equal(np.sqrt(sq_in), edt_in) and np.array_equal(np.sqrt(sq_out), edt_out)      # sqrt of the exact integer IS scipy's value
        assert np.array_equal(np.sqrt(sq_in + sq_out), dist11) and np.array_equal(dist11, dist23)
        assert mask11.dtype == bool and dist11.dtype == np.float64
        arrays.update({name + '_dist11': dist11, name + '_mask11': mask11, name + '_dist23': dist23, name + '_mask23': mask23,
                       name + '_edt_sq_in': sq_in.astype(np.uint32), name + '_edt_sq_out': sq_out.astype(np.uint32)})

        sp, st = surface(prediction), surface(target)
        assert sp.any() and st.any()
        assert np.array_equal(st, (target != 0) & (sq_in == 1))          # the inner half of the border shell
        d_pt = ndimage.distance_transform_edt(~st)[sp]
        d_tp = ndimage.distance_transform_edt(~sp)[st]
        both = np.concatenate([d_pt, d_tp])
        arrays.update({name + '_surface_prediction': sp, name + '_surface_target': st,
                       name + '_sq_p_to_t': np.sort(np.rint(d_pt ** 2).astype(np.int64)), name + '_sq_t_to_p': np.sort(np.rint(d_tp ** 2).astype(np.int64)),
                       name + '_hd': np.array(both.max()), name + '_hd95': np.array(np.percentile(both, 95)), name + '_assd': np.array(both.mean())})
        q = quantise(u)
        for bands in (3, 10):
            arrays['{}_table_r{}'.format(name, bands)] = boundary_table(prediction, target, (sq_in + sq_out).astype(np.int64), q, bands)
        t3 = arrays[name + '_table_r3']
        assert t3[:, 0, 0].sum() == mask11.sum()                        # band 0 of both sides is the reference's shell
        print('{:6s} {:14s} shell {:5d}  surfaces {:4d} / {:4d}  hd {:.4f} hd95 {:.4f} assd {:.4f}'.format(
            name, str(target.shape), int(mask11.sum()), int(sp.sum()), int(st.sum()), float(both.max()), float(np.percentile(both, 95)), float(both.mean())))
    assert checked == len(cases)      # 100 % of the cases hold both classes
    path = os.path.join(HERE, 'g24_boundary.npz')
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print('wrote {} ({:.1f} KiB)'.format(path, size / 1024))
    assert size < 300 * 1024


if __name__ == '__main__':
    main()
