/* C ABI of the fit kernels of librcu_hip.so: the second public header, beside include/rcu.h (status codes, rcu_last_error() and the
 * conventions are those of rcu.h: device pointers end in _dev, all device work is enqueued on `stream`, nothing is allocated, nothing blocks the host).
 *
 * Auxiliary fit
 * -------------
 * The train-mode loss of the auxiliary PostNet (rcu.h "PostNet"; the reference's common/model/postnet.py under *_train_auxiliary_feat.py) on the
 * feature map of a FROZEN U-Net, and the gradient of that loss with respect to every PostNet parameter.  One call is one optimisation step's
 * forward and backward; the optimiser is the caller's.
 *
 * Inputs.  phi: the feature map, NHWC float32 [n * hw][channel_pitch] as rcu_unet_features hands it out; e(v) in {0, 1}: uint8 [n][hw], the
 * error target; the raw (unfolded) parameters of a PostNet with L = nb_convs hidden units of F channels and C = 2 classes; N = n * hw voxels.
 *
 * Forward, BatchNorm in train mode over the whole batch.  For l = 1 .. L, with a_0 = phi:
 *     u_l = W_l a_{l-1} + b_l            mu_l = mean_v u_l            var_l = mean_v (u_l - mu_l)^2   (biased)
 *     xhat_l = (u_l - mu_l) / sqrt(var_l + 1e-5)     y_l = gamma_l xhat_l + beta_l     a_l = max(y_l, 0)
 *     z = W_o a_L + b_o                  loss = (1 / N) sum_v [logsumexp_c z_c(v) - z_{e(v)}(v)]
 * Backward, the exact derivative of that loss:
 *     dz = (softmax(z) - onehot(e)) / N          da_L = W_o^T dz          dy_l = da_l where y_l > 0, else 0
 *     du_l = (gamma_l / sigma_l) (dy_l - mean_v dy_l - xhat_l mean_v(dy_l xhat_l)),  sigma_l = sqrt(var_l + 1e-5)       da_{l-1} = W_l^T du_l
 *     dW_l = sum_v du_l(v) a_{l-1}(v)^T     db_l = sum_v du_l  (zero in exact arithmetic: a bias in front of a train-mode BatchNorm)
 *     dgamma_l = sum_v dy_l xhat_l          dbeta_l = sum_v dy_l          dW_o = sum_v dz a_L^T          db_o = sum_v dz
 * Outputs.  The loss (float64); the gradient of every parameter (float32, each rounded once from a float64 sum); mu_l and var_l (float32 [L][F]).
 * BatchNorm's running statistics are the caller's to update, as torch does: running_mean = 0.9 rm + 0.1 mu,
 * running_var = 0.9 rv + 0.1 var N / (N - 1), num_batches_tracked += 1 (rcu_amd.auxiliary does it).  N >= 2 is required.
 *
 * Packing.  Parameters and gradients are ONE flat float32 array each, in this order (state_dict names of the PostNet), with
 * rcu_postnet_fit_param_count(F, nb_convs) = nb_convs (F F + 3 F) + 2 F + 2 elements:
 *     for k = 0 .. nb_convs - 1:   convs.k.conv2d_batch_relu.conv.weight [F][F]     convs.k.conv2d_batch_relu.conv.bias [F]
 *                                  convs.k.conv2d_batch_relu.bn.weight [F]          convs.k.conv2d_batch_relu.bn.bias [F]
 *     conv_logits.weight [2][F]    conv_logits.bias [2]
 *
 * Determinism.  The outputs are a function of (phi, e, parameters, n, hw, F, L) bit for bit: they do not depend on the launch geometry, the stream,
 * the alignment of any pointer or the channel pitch.  No float atomics.  The voxels are partitioned by index as rcu_density_moments partitions
 * them: chunk q of slice s = voxels [q m, (q + 1) m) of the slice, m = RCU_DENSITY_CHUNK; every sum over voxels is a float32 sum over one chunk
 * (weight gradients: the fp32 MFMA's k-ordered fmaf chain over the chunk's voxel pairs; per-channel sums: 32 voxel columns added in voxel order,
 * then one fixed butterfly over the columns), and the chunks' sums are promoted to float64 and added in a fixed order that depends on the number
 * of chunks alone (64 stripes q mod 64, each in chunk order, then the stripes in stripe order).  BatchNorm's statistics couple every voxel of the
 * batch, so unlike the density fit the result depends on the batch as a whole: no independence of batching is claimed.
 * The variance is accumulated about a per-channel shift known before the pass (the mean of u_l over count = min(N, 1024) voxels spread over the
 * batch, voxel i * stride with stride = floor(N / count), less one where that is even and above 1: an odd stride does not line the samples up in
 * columns of an image of even width), var = sum (u - shift)^2 / N - (mu - shift)^2 in float64: nothing cancels where |mu| >> sigma.  The first
 * layer runs on phi - c, c the mean of phi over the same voxels, with the bias b_1 + W_1 c: its products are then of the size of sigma, not of
 * |mu|, and so is the rounding of u_1 (a constant error of that bias is in mu_1 too and cancels).  dW_1 is formed with phi itself.
 *
 * Limits.  1 <= F <= 32 (one channel block); channels >= F of a voxel are never read as data; channel_pitch >= 32 and a multiple of 4; C = 2;
 * 1 <= nb_convs <= RCU_POSTNET_FIT_MAX_CONVS; n >= 1, hw >= 1, 2 <= n * hw < 2^40, n * ceil(hw / RCU_DENSITY_CHUNK) < 2^31.  features_dev,
 * params_dev, grads_dev, batch_mean_dev, batch_var_dev and flags_dev are 4-byte aligned, loss_dev and workspace_dev 8-byte aligned.
 * A label >= 2 sets flags_dev[0] = 1 (uint32; the call never clears it, the caller zeroes it and reads it with the loss); such a voxel counts
 * with logsumexp alone.  Every argument is checked before the device is touched (RCU_ERR_INVALID, rcu_last_error() names it). */
#ifndef RCU_FIT_H
#define RCU_FIT_H

#include "rcu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RCU_POSTNET_FIT_MAX_CONVS 4

/* elements of the flat parameter / gradient array (see "Packing"); 0 for F or nb_convs outside the limits */
size_t rcu_postnet_fit_param_count(int F, int nb_convs);

/* bytes of workspace_dev for one rcu_postnet_loss_grad call; 0 for arguments outside the limits */
size_t rcu_postnet_fit_workspace_bytes(int F, int nb_convs, size_t n, size_t hw);

/* loss_dev: float64 [1]; grads_dev: float32 [rcu_postnet_fit_param_count]; batch_mean_dev, batch_var_dev: float32 [nb_convs][F]; flags_dev:
 * uint32 [1]; 2 nb_convs + 1 passes over features_dev and nothing of size N x F written.  Asynchronous: returns with the work enqueued. */
int rcu_postnet_loss_grad(const float* features_dev, int channel_pitch, int F, size_t n, size_t hw, const uint8_t* labels_dev, int nb_convs,
                          const float* params_dev, float* grads_dev, double* loss_dev, float* batch_mean_dev, float* batch_var_dev,
                          uint32_t* flags_dev, void* workspace_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCU_FIT_H */
