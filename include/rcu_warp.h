/* C ABI of the affine test-time augmentation kernels of librcu_hip.so: the fourth public header, beside include/rcu.h, include/rcu_fit.h and
 * include/rcu_knn.h (status codes, rcu_last_error() and the conventions are those of rcu.h: device pointers end in _dev, all device work is
 * enqueued on `stream`, nothing is allocated, nothing blocks the host).
 *
 * Affine test-time augmentation
 * -----------------------------
 * EXTENSION: rcu.h's test-time augmentation is the eight pixel permutations of D4, whose statistics blob folds back with one add per element.
 * Small rotations, scalings and shifts (Wang et al. 2019, Aleatoric uncertainty estimation with test-time augmentation for medical image
 * segmentation with CNNs) resample, and the entropy of a resampled probability is not the resampled entropy: every sample is resampled BEFORE it
 * enters the statistics (rcu_amd.steps.AffineTtaMcPredictStep, the `others.tta_affine` key of the two default test scripts).
 * tests/warp_reference.py restates this section in float64.
 *
 * Transform.  Six float64 numbers M = [[m00, m01, m02], [m10, m11, m12]] in pixel units about the plane centre, rows (y, x); it maps an OUTPUT
 * pixel to its SOURCE position.  For output pixel (i, j) of an H x W plane:
 *     yc = i - (H-1)/2,  xc = j - (W-1)/2
 *     sy = (m00*yc + m01*xc) + ty,   ty = m02 + (H-1)/2
 *     sx = (m10*yc + m11*xc) + tx,   tx = m12 + (W-1)/2
 * every product, sum and difference ONE IEEE float64 operation rounded to nearest, nothing contracted ((H-1)/2 is exact; ty and tx carry the bits
 * of the host's float64 additions).  Then, border mode: sy is clamped to [0, H-1], sx to [0, W-1] (edge values are replicated);
 *     i0 = floor(sy), i1 = min(i0 + 1, H-1), fy = (float)(sy - i0);  j0, j1, fx likewise from sx
 *     lerp(a, b, t) = fmaf(t, b - a, a)
 *     out = lerp(lerp(v[i0][j0], v[i0][j1], fx), lerp(v[i1][j0], v[i1][j1], fx), fy)          in float32.
 * This is F.grid_sample(x, F.affine_grid(theta), mode='bilinear', padding_mode='border', align_corners=False) with
 * theta = [[m11, m10*H/W, 2*m12/W], [m01*W/H, m00, 2*m02/H]].  A matrix with integer taps has fx = fy = 0: the output is a bit copy of its taps
 * (the identity, the flips on any plane, the D4 elements on square planes).  The entries must be finite (the Python layer refuses others; the
 * kernels clamp whatever they compute, so no entry can make them read outside the plane).
 *
 * Error.  With u = 2^-24, against the same expression evaluated exactly from the float32 taps and the float32 weights: three lerps, each a rounded
 * difference and a rounded fmaf, |out_dev - out| <= 12 u max|tap|.
 *
 * Warped statistics.  rcu_mc_accumulate_warped adds `groups` samples to the rcu_mc_stats_bytes blob of n canonical slices.  For every canonical
 * voxel and for g = 0 .. groups-1 in that order: the probability vector is the warp with M_g of each class plane of p[g][slice] (from logits:
 * softmax of each tap's logit vector first, the operations of rcu_softmax), and it is added exactly as rcu_mc_accumulate adds a pass (p, p^2,
 * entropy; quantised under RCU_MC_EXACT).  The caller passes the INVERSE of the matrices its inputs were warped with; the library applies what it
 * is given.  From logits the result is bit for bit rcu_softmax followed by the RCU_MC_INPUT_PROBS form; one call with G groups is bit for bit G
 * calls with one group each in ascending order; under RCU_MC_EXACT any split and any order give the same blob.  One lane owns one voxel: no
 * atomics.  A voxel's result does not depend on n, the slice's position, the alignment, the launch geometry or the stream.
 *
 * Every argument is checked before the device is touched (RCU_ERR_INVALID, rcu_last_error() names it): null pointers, n_mats / groups outside
 * 1 .. RCU_WARP_MAX_MATRICES, empty batches or planes, planes above 2^30 pixels, channels < 1, nb_classes outside 1..8, unknown flags. */
#ifndef RCU_WARP_H
#define RCU_WARP_H

#include "rcu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RCU_WARP_MAX_MATRICES 64

/* out[m][i] = warp(x[i], M_m): x [n][channels][H][W], mats_dev float64 [n_mats][6], out [n_mats][n][channels][H][W]; out must not overlap x */
int rcu_warp_affine(const float* x_dev, size_t n, int channels, int height, int width, const double* mats_dev, int n_mats, float* out_dev,
                    void* stream);

/* in_dev: float32 [groups][n][nb_classes][H*W] logits, or probabilities with RCU_MC_INPUT_PROBS; stats_dev: the blob of the n canonical slices;
 * flags as for rcu_mc_accumulate; mats_dev float64 [groups][6] */
int rcu_mc_accumulate_warped(const float* in_dev, void* stats_dev, size_t n, int height, int width, int nb_classes, int flags,
                             const double* mats_dev, int groups, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCU_WARP_H */
