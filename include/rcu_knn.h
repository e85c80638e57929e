/* C ABI of the nearest-neighbour kernels of librcu_hip.so: the third public header, beside include/rcu.h and include/rcu_fit.h (status codes,
 * rcu_last_error() and the conventions are those of rcu.h: device pointers end in _dev, all device work is enqueued on `stream`, nothing is
 * allocated, nothing blocks the host).
 *
 * Nearest-neighbour feature uncertainty
 * -------------------------------------
 * EXTENSION: the reference has no non-parametric single-pass uncertainty (rcu_amd.knn, rcu_amd.steps.KnnPredictStep, the fit_knn scripts and the
 * `others.knn` key of the two default test scripts -- Sun et al., ICML 2022, Out-of-distribution detection with deep nearest neighbors).
 * tests/knn_reference.py restates this section in float64.
 *
 * Bank.  M rows b_m in R^F, F = start_filters, 1 <= F <= RCU_KNN_MAX_FEATURES (one channel block), 1 <= M <= RCU_KNN_MAX_BANK, float32 [M][F]
 * without padding.  1 <= k <= RCU_KNN_MAX_K and k <= M.  bank_sq[m] = |b_m|^2 is made by the host: summed in float64 from the float32 rows, rounded
 * once.  With normalize on, the bank holds ALREADY normalised rows: the host divides each tapped row by max(|row|, 2^-40) in float64 and rounds once
 * to float32 (a zero row stays zero); with normalize off the rows are the tapped features as they are.
 *
 * Features.  phi(v) in R^F is rcu_unet_features of an eval-mode forward: F real channels at channel_pitch floats per voxel, channel_pitch >= F and a
 * multiple of 4, features_dev 16-byte aligned.  Channels F .. pitch - 1 are never used as data: they may hold anything, NaN included.
 *   normalize on:   xhat = phi / max(|phi|, 2^-40), |phi| = sqrtf(sum phi_c^2) in float32, each division correctly rounded (a zero vector stays zero;
 *                   a vector whose squares underflow float32 is outside the contract);
 *   normalize off:  xhat = phi.
 *
 * Distance.  d2(v, m) = max(0, |xhat_v|^2 + |b_m|^2 - 2 xhat_v . b_m).  On the device: xx = sum xhat_c^2 in float32 (two fmaf chains over the
 * channels a lane holds, then one add), dot = the fp32 MFMA's k-ordered fmaf chain over the 32 channel slots from 0 (slots >= F hold zeros),
 * d2 = fmaxf(0, fmaf(-2, dot, xx + bank_sq[m])).
 * Neighbours.  d2_(1) <= ... <= d2_(k): the k smallest of d2(v, .) over m = 0 .. M - 1 as a multiset (a duplicated bank row counts twice).
 * Score.  knn(v) = sqrtf(d2_(k)(v)), float32; optionally the k sorted squared distances, float32 [n_voxels][k].
 *
 * Purity.  d2(v, m) is bit for bit a function of the F values of voxel v, the F values and bank_sq of row m, F and normalize.  It does not depend on
 * m's position, M, k, the tile a row falls in, the pitch, the contents of channels F .. pitch - 1, the voxel's position, n_voxels, the launch
 * geometry or the stream.  Hence: permuting the voxels permutes the outputs bit for bit; permuting the bank rows changes no bit; a NULL d2_dev
 * changes no other bit.  No atomics.
 *
 * Error.  With u = 2^-24, against d2 evaluated exactly from the float32 inputs (phi, b, bank_sq):
 *     |d2_dev - d2| <= (2 F + 8) u (|xhat_v| + |b_m|)^2,
 * and, sorting being 1-Lipschitz in the sup norm, |d2_dev,(j) - d2_(j)| <= max_m of that bound for every j.  DESIGN.md ("Nearest-neighbour feature
 * uncertainty") derives it.  score is sqrtf of the kernel's own d2_(k): within 2^-23 relative of its exact square root.
 *
 * Sampling keys.  The bank is a seeded sample of the held-out voxels that does not depend on batching: voxel (global slice index g, pixel v) has
 *     key63 = ((r0 << 32 | r1) >> 1),  (r0, r1, ., .) = Philox4x32-10(counter (v, g mod 2^32, g >> 32, 0x6b6e6e), key (key mod 2^32, key >> 32)),
 * and the bank of a class is its voxels with the smallest triples (key63, g, v) (rcu_amd.knn.merge_candidates).  rcu_knn_sample_keys draws the keys
 * of n slices of hw pixels: keys_dev[i * hw + v] for slice_index_dev[i] = g >= 0.  1 <= n, 1 <= hw <= 2^31, n * hw <= 2^31.
 *
 * Every argument is checked before the device is touched (RCU_ERR_INVALID, rcu_last_error() names it). */
#ifndef RCU_KNN_H
#define RCU_KNN_H

#include "rcu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RCU_KNN_MAX_FEATURES 32
#define RCU_KNN_MAX_BANK 65536
#define RCU_KNN_MAX_K 8

/* one int64 key63 per voxel of n slices of hw pixels; asynchronous */
int rcu_knn_sample_keys(size_t n, size_t hw, const int64_t* slice_index_dev /* [n] */, uint64_t key, int64_t* keys_dev /* [n][hw] */, void* stream);

/* score_dev: float32 [n_voxels]; d2_dev: float32 [n_voxels][k] or NULL; 1 <= n_voxels <= 2^40; normalize is 0 or 1; asynchronous */
int rcu_knn_distances(const float* features_dev, int channel_pitch, int F, size_t n_voxels, const float* bank_dev /* [M][F] */,
                      const float* bank_sq_dev /* [M] */, int M, int k, int normalize, float* score_dev, float* d2_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCU_KNN_H */
