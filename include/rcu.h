/* rcu.h -- C ABI of librcu_hip.so: the MI355X (gfx950) implementation of the repeated-stochastic-
 * inference uncertainty path of alainjungo/reliability-challenges-uncertainty.
 *
 * The reference is pure Python and has no FFI of its own; the path sits behind three Python call
 * protocols.  Each group of entry points below names the reference
 * interface it stands behind (paths relative to the reference root):
 *
 *   model seam   context.model(images) -> logits | (logits, sigma)
 *                common/model/unet.py:123-186, called from rechun/dl/customsteps.py:23,32,
 *                common/trainloop/steps.py:84, bin-dl/brats_test_ensemble.py:85,89,
 *                bin-dl/brats_test_aleatoric.py:63
 *   step seam    BatchStep.__call__(batch_context, task_context, context)
 *                common/trainloop/steps.py:14-17; McPredictStep / MultiPredictionSummary
 *                rechun/dl/customsteps.py:10-71
 *   metric seam  EvaluationStrategy.__call__(to_evaluate, results)
 *                common/evalutation/eval.py:9-16; numpy kernels common/evalutation/numpyfunctions.py:6-107
 *
 * Conventions: every function returns 0 on success and a negative rcu_status otherwise and never
 * throws; rcu_last_error() gives the message of the calling thread's last failure.  Pointers
 * named *_dev are device pointers (e.g. torch tensor.data_ptr()), *_host are host pointers.
 * `stream` is a hipStream_t passed as void* (0 = the null stream); all device work is enqueued on
 * it and no call synchronises unless documented.  A handle is not thread-safe; distinct handles
 * are independent.  Tensors at the boundary use the reference's layout: float32, NCHW, contiguous.
 */
#ifndef RCU_H
#define RCU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rcu_status {
    RCU_OK = 0,
    RCU_ERR_INVALID = -1,   /* bad argument / unsupported shape */
    RCU_ERR_HIP = -2,       /* a HIP runtime call failed */
    RCU_ERR_WEIGHTS = -3,   /* missing / mis-sized weight tensor */
    RCU_ERR_STATE = -4      /* call order violated (e.g. forward before finalize_weights) */
} rcu_status;

const char* rcu_last_error(void);
/* "librcu_hip <version> gfx950" */
const char* rcu_version(void);

/* ------------------------------------------------------------------------------------------
 * Model seam: UNet(nb_classes, in_channels, depth, start_filters, dropout, dropout_center,
 *                  residual=False, sigma_out, provide_features=False, bn)   (unet.py:128-130)
 * ------------------------------------------------------------------------------------------ */
typedef struct rcu_unet rcu_unet;

typedef struct rcu_unet_desc {
    int32_t nb_classes;      /* 1..8 */
    int32_t in_channels;
    int32_t depth;           /* number of down / up levels */
    int32_t start_filters;
    int32_t has_dropout;     /* 0 <=> dropout=None: the model has no Dropout2d modules at all */
    int32_t dropout_center;  /* -1 <=> None (dropout in every conv unit), else unet.py:74-82 */
    int32_t sigma_out;       /* 1: twin head, forward returns (logits, sigma) */
    int32_t bn;              /* 1: BatchNorm2d in every conv unit (folded, eval mode) */
    int32_t height, width;   /* per-slice size, each >= 2^depth; sizes not divisible by 2^depth take the reference's centre pad
                                (common/model/unet.py:110-116) and the direct kernels on the levels with odd sizes */
    int32_t max_batch;       /* largest N a forward call may pass; sizes the workspace */
    int32_t residual;        /* 1: ConvResidualBlock (common/model/unet.py:42-60) instead of ConvBlock: a block's second unit has no
                                ReLU and a 1x1 conv of the block input ("<block>.residual") is added to its output */
    int32_t provide_features; /* 1: rcu_unet_features will be called (unet.py:135-136, 178-179): the input of conv_cls.0 is kept
                                channels-last; otherwise the library is free to hold it in its channel-blocked layout */
} rcu_unet_desc;

int rcu_unet_create(const rcu_unet_desc* desc, rcu_unet** out);
int rcu_unet_destroy(rcu_unet* h);
/* bytes of device memory the handle OWNS: its packed weights, plus the activation workspace unless that is borrowed from a donor
 * (rcu_unet_create_with) */
int64_t rcu_unet_workspace_bytes(const rcu_unet* h);

/* Plan options: which kernel family / activation layout the planner may choose.  The defaults are the shipped path; the other
 * values exist for A/B measurements and for the parity tests that compare the kernel families on the same input (they replace the
 * RCU_CONV_WINO / RCU_CONV_WINO4 / RCU_CONV_FIRST / RCU_ACT_LAYOUT / RCU_FUSE_HEAD environment switches of earlier rounds: the library
 * reads no environment variable on the product path). */
typedef struct rcu_unet_options {
    int32_t conv_winograd;    /* 1 (default): Winograd kernels wherever their tiles fit; 0: the direct kernels everywhere */
    int32_t conv_winograd4;   /* 1 (default): F(4x4,3x3) wherever its tiles fit -- at the 12x8 level where, for the batch the plan is sized for, its few long
                                 work items fill the chip's rounds of workgroups (pick_config) --; 2: wherever its tiles fit, whatever the fill (parity
                                 tests on small batches); 0: F(2x2,3x3) only; 3: F(4x4,3x3) for the units with >= 64 output channels only (the round-2 selection) */
    int32_t conv_first;       /* 1 (default): the unpadded first-unit kernel; 0: the tiled kernel + channels-last input copy */
    int32_t act_layout;       /* 0 (default): channel-blocked activations between Winograd kernels, and the pixel-pair form of that layout
                                 ([N][C/8][H][W/2][4 channel pairs][2 pixels][2 channels]) for the tensors only F(4x4,3x3) kernels touch on unpadded
                                 levels; 1: channels-last everywhere; 2: channel-blocked, never paired (A/B measurements, bitwise tests).  A layout is
                                 an addressing choice: the results have the same bits under every value */
    int32_t fuse_head;        /* 1 (default): 1x1 classifier + softmax + statistics in conv_cls.0's epilogue where the shapes allow;
                                 0: the standalone head kernel (also settable per handle at run time: rcu_unet_set_fuse_head) */
    int32_t head_winograd4;   /* 1 (default): conv_cls.0 -- with the classifier fused into its epilogue or not -- takes F(4x4,3x3) where the 32x32 tile
                                 fits (and conv_winograd4 is 1 or 2); 0: it stays on F(2x2,3x3), the plan of rounds 1-4 (A/B measurements) */
    int32_t pad_levels;       /* 1 (default): a level whose real extent (height >> l) x (width >> l) is not a whole number of Winograd tiles is ALLOCATED with
                                 a padded extent -- the padding holds zeros no kernel writes, which is the conv's own zero padding -- and runs on the Winograd
                                 kernels (the reference's BraTS slices are 240 x 240: levels 240, 120, 60, 30, 15; ISIC's 192 x 256 ends in a 12 x 16 level);
                                 0: real extents only, such levels take the direct kernels (the plans of rounds 1-5; A/B measurements) */
    int32_t upconv_winograd4; /* the 25-product F(4x4,3x3) up-convolutions (csrc/rcu_wino4_up.hip; the slot was reserved[0] -- a caller that zeroes it keeps
                                 the sub-pixel F(2x2,2x2) kernels).  0: never; 1 (default): per layer where the plan's work items fill the chip and the
                                 kernel measured faster at that plan size (pick_config); 2: wherever its tiles fit, whatever the fill (parity tests on
                                 small batches).  Padded levels (pad_levels) keep the sub-pixel kernels under every value */
} rcu_unet_options;
/* fills *opts with the defaults above */
void rcu_unet_default_options(rcu_unet_options* opts);
/* rcu_unet_create with explicit options (NULL = defaults) and an optional workspace DONOR: a handle of the same shape (desc and options
 * equal, max_batch <= the donor's) whose activation workspace the new handle shares instead of allocating its own -- the members of
 * an ensemble (bin-dl/brats_test_ensemble.py:44-57: K models resident at once) differ in 35 MB of packed weights, not in their
 * 6 GB of activations.  Handles that share a workspace must not run concurrently (launch them on ONE stream); the workspace is
 * freed when its last user is destroyed, in any order. */
int rcu_unet_create_with(const rcu_unet_desc* desc, const rcu_unet_options* opts, rcu_unet* workspace_donor, rcu_unet** out);
/* The plan alone -- which kernel runs which layer on which grid (rcu_unet_num_layers / rcu_unet_layer_info) -- without any device memory: a handle
 * that can be inspected and destroyed, nothing else (weights and forwards fail with RCU_ERR_STATE / RCU_ERR_HIP).  What a caller sizes its launches
 * by, and what the planner's tests read without a GPU. */
int rcu_unet_plan(const rcu_unet_desc* desc, const rcu_unet_options* opts, rcu_unet** out);
/* Run-time form of rcu_unet_options.fuse_head (benchmarks time the standalone head kernel on the plan of the timed run). */
int rcu_unet_set_fuse_head(rcu_unet* h, int on);

/* Dropout sites in execution order (= torch named_modules order of the Dropout2d modules). */
int rcu_unet_num_dropout_sites(const rcu_unet* h);
int rcu_unet_dropout_site_channels(const rcu_unet* h, int site);
/* state_dict-style name of the site, e.g. "down_convs.0.block.block.0.conv2d_batch_relu.dropout" */
const char* rcu_unet_dropout_site_name(const rcu_unet* h, int site);
/* sum of the sites' channel counts = floats of mask per sample and pass */
int rcu_unet_mask_floats_per_sample(const rcu_unet* h);

/* Weights: one call per state_dict tensor (torch.load(checkpoint)['state_dict'],
 * common/model/management.py:56-64), by its key (a leading "module." is ignored,
 * common/trainloop/context.py:167).  float32 host data in torch layout (conv: [Cout][Cin][kh][kw]).
 * Keys the path does not need (num_batches_tracked) are accepted and ignored. */
int rcu_unet_load_weight(rcu_unet* h, const char* name, const float* data_host, size_t count);
/* Folds BatchNorm (A = gamma / sqrt(var + 1e-5), B = beta - A * mean), repacks every conv into the
 * kernel layout and uploads.  Synchronous.  Fails with RCU_ERR_WEIGHTS naming the first missing key. */
int rcu_unet_finalize_weights(rcu_unet* h);

/* One forward pass of n <= max_batch slices.
 *   x_dev       [n][in_channels][H][W]
 *   masks_dev   NULL = eval mode (set_dropout_mode(model, False), common/utils/torchhelper.py:44-50);
 *               else the Dropout2d factors {0, 1/(1-p)} of this pass, sites concatenated:
 *               [site 0: n x C_0][site 1: n x C_1]...  (n * mask_floats_per_sample floats)
 *   logits_dev  [n][nb_classes][H][W] or NULL
 *   sigma_dev   [n][nb_classes][H][W] raw sigma head output, or NULL (must be NULL without sigma_out)
 */
int rcu_unet_forward(rcu_unet* h, const float* x_dev, int n, const float* masks_dev, float* logits_dev,
                     float* sigma_dev, void* stream);

/* Forward + softmax + accumulation into MC statistics, fused so that neither logits nor the
 * probability volume reach HBM (one pass of McPredictStep's loop body, customsteps.py:30-34, or one
 * ensemble member, brats_test_ensemble.py:85-92).  stats_dev / flags as for rcu_mc_accumulate. */
int rcu_unet_forward_accumulate(rcu_unet* h, const float* x_dev, int n, const float* masks_dev, void* stats_dev,
                                int flags, void* stream);
/* The same for `passes` stochastic passes at once: the n images run as one batch of n * passes samples (sample
 * t*n + i = image i under mask rows [site][t*n + i][C_site], masks_dev holds n * passes rows per site) and all passes
 * are added to the n statistics entries in pass order -- bit-identical to `passes` calls of
 * rcu_unet_forward_accumulate, but a small batch (the reference's batch_size 32, customsteps.py:30-34) fills the GPU.
 * n * passes <= max_batch. */
int rcu_unet_forward_accumulate_passes(rcu_unet* h, const float* x_dev, int n, int passes, const float* masks_dev,
                                       void* stats_dev, int flags, void* stream);

/* EXTENSION (BASELINE.json config "BraTS aleatoric + MC"; the reference has no such path: its McPredictStep cannot take the
 * (logits, sigma) tuple of a sigma_out model, customsteps.py:32-33, and bin-dl/brats_test_aleatoric.py:57-73 does ONE forward).
 * One stochastic pass of a sigma_out model: softmax(logits) goes into the MC statistics exactly as in
 * rcu_unet_forward_accumulate, and the pass's sigma = |raw| (exp(raw) with is_log_sigma, as brats_test_aleatoric.py:66-69)
 * is ADDED to sigma_sum_dev [n][nb_classes][H][W] (float32; zero it before the first pass, divide by T after the last). */
int rcu_unet_forward_accumulate_sigma(rcu_unet* h, const float* x_dev, int n, const float* masks_dev, void* stats_dev,
                                      int flags, float* sigma_sum_dev, int is_log_sigma, void* stream);

/* The same for a pass group (see rcu_unet_forward_accumulate_passes): `passes` stochastic passes of the n images as one batch of
 * n * passes samples; statistics and sigma sums are added to in pass order -- the bits of `passes` calls of
 * rcu_unet_forward_accumulate_sigma. */
int rcu_unet_forward_accumulate_sigma_passes(rcu_unet* h, const float* x_dev, int n, int passes, const float* masks_dev,
                                             void* stats_dev, int flags, float* sigma_sum_dev, int is_log_sigma, void* stream);

/* Per-layer introspection for benchmarks: canonical FLOPs (2*Cin*Cout*9*H*W per slice, real
 * channel counts) and the kernel configuration chosen. */
typedef struct rcu_layer_info {
    char name[96];
    char kernel[64];
    int32_t cin, cout, height, width;
    int32_t grid_height, grid_width; /* the grid the kernel's tiles walk: the ALLOCATED extent of the layer's level (an up-convolution's low-resolution
                                        level), larger than the real one on a padded level (rcu_unet_options.pad_levels) */
    int32_t upsample, pooled, dual_source;
    int32_t head_fusable;         /* 1: forwards that want logits or statistics (no sigma) run this unit with the classifier head in the kernel's epilogue
                                     while rcu_unet_options.fuse_head is on -- profilers see that kernel as `kernel` + "+head"; rcu_unet_run_layer runs the plain one */
    double flops_per_slice;       /* algorithmic: 2*cin*cout*9*H*W of the layer as the reference computes it */
    double mfma_flops_per_slice;  /* what the kernel issues to the MFMA pipe (padded channels; 4 of 9 taps for the
                                     sub-pixel up-convolution; whole tiles) */
} rcu_layer_info;
int rcu_unet_num_layers(const rcu_unet* h);
int rcu_unet_layer_info(const rcu_unet* h, int layer, rcu_layer_info* out);
/* The activation layouts the planner chose (rcu_unet_options.act_layout) for the tensors of layer `layer`: its source, its second source (the
 * skip tensor of a cat-free decoder unit), its output and its pooled output; -1 where the layer has no such tensor.  Any pointer may be NULL. */
enum { RCU_LAYOUT_NHWC = 0, RCU_LAYOUT_BLOCKED = 1, RCU_LAYOUT_PAIRED = 2 };
int rcu_unet_layer_layouts(const rcu_unet* h, int layer, int32_t* src1, int32_t* src2, int32_t* out, int32_t* pooled);
/* Runs only conv layer `layer` on the handle's current workspace contents (benchmark aid; layer 0 then reads the
   workspace's channels-last input copy, which a forward pass only fills when its first-layer kernel does not read the
   caller's NCHW input directly -- timing only). */
int rcu_unet_run_layer(rcu_unet* h, int layer, int n, const float* masks_dev, void* stream);

/* Per-kernel timing of the next `max_forwards` forward calls with HIP events recorded on the caller's
 * stream between launches (slot 0 = input re-layout, slots 1..L = conv layers in rcu_unet_layer_info
 * order, slot L+1 = head kernel).  collect() waits for the recorded work, writes the summed
 * milliseconds per slot (L+2 doubles) and the number of forwards covered, and re-arms the pool. */
int rcu_unet_profile_begin(rcu_unet* h, int max_forwards);
int rcu_unet_profile_collect(rcu_unet* h, double* ms_sum, int* forwards);

/* Feature map of the last forward call = the input of conv_cls (UNet.features when provide_features is set,
 * common/model/unet.py:178-179): NHWC float32 in the handle's workspace, `channels` real channels at a pitch
 * of `channel_pitch` floats per voxel; valid until the next forward call on this handle. */
int rcu_unet_features(const rcu_unet* h, const float** features_dev, int* channels, int* channel_pitch);

/* Input of the 1x1 classifier conv_cls.1 in the last forward call = the output of conv_cls.0 after BN and ReLU (UNet.head_features when
 * provide_head_features is set; "Last-layer Laplace" below): a compact channels-last [n * H * W][channel_pitch] float32 tensor in the handle's
 * workspace, `channels` = start_filters real channels.  Valid after a forward that did not fuse the head (rcu_unet_set_fuse_head(h, 0), or any
 * forward that takes the separate head kernel), until the next forward on this handle or on one that shares its workspace.  RCU_ERR_STATE
 * otherwise -- before the first forward, after a forward that fused the head -- and for a sigma_out handle (its head tensor interleaves the sigma
 * twin's channels). */
int rcu_unet_head_features(const rcu_unet* h, const float** features_dev, int* channels, int* channel_pitch);

/* ------------------------------------------------------------------------------------------
 * PostNet -- auxiliary confidence network on the U-Net features
 *   (common/model/postnet.py:6-18; bin-dl/brats_test_auxiliary_feat.py:74-77, isic_test_auxiliary_feat.py)
 *   nb_convs x [Conv2d 1x1 C->C, BatchNorm2d (eval), ReLU] + Conv2d 1x1 C->nb_classes, C <= 32, nb_classes <= 32.
 *   Weights by state_dict name: convs.<i>.conv2d_batch_relu.{conv.weight,conv.bias,bn.weight,bn.bias,
 *   bn.running_mean,bn.running_var}, conv_logits.{weight,bias}.
 * ------------------------------------------------------------------------------------------ */
typedef struct rcu_postnet rcu_postnet;
int rcu_postnet_create(int in_channels, int nb_classes, int nb_convs, int bn, rcu_postnet** out);
void rcu_postnet_destroy(rcu_postnet* h);
int rcu_postnet_load_weight(rcu_postnet* h, const char* name, const float* host_data, size_t count);
int rcu_postnet_finalize_weights(rcu_postnet* h);
/* in_channels <= 96.  features: NHWC float32 [n*hw][channel_pitch] (channel_pitch >= in_channels rounded up to 32, a multiple of 4;
 * the padding channels up to the next multiple of 32 must hold zeros or finite values -- their weights are zero);
 * masks_dev: NULL (eval / no Dropout2d) or the factors {0, 1/(1-p)} of one MC pass, float32 [nb_convs][n][in_channels]
 * (Dropout2d sits between conv and BatchNorm in every hidden unit, common/model/unet.py:14-15); logits_dev: float32 [n][nb_classes][hw]. */
int rcu_postnet_forward(rcu_postnet* h, const float* features_dev, int channel_pitch, int n, int hw, const float* masks_dev,
                        float* logits_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Step seam: per-voxel sufficient statistics over T passes / K members
 *   (McPredictStep + MultiPredictionSummary, customsteps.py:16-71; torchhelper.py:53-54)
 * ------------------------------------------------------------------------------------------ */
#define RCU_MC_MI 1           /* also track sum_t H(p_t)  -> mutual_info available */
#define RCU_MC_VAR 2          /* statistics in float64 incl. sum p^2 -> variance available */
#define RCU_MC_INPUT_PROBS 4  /* rcu_mc_accumulate input is already softmax-ed */
#define RCU_MC_EXACT 8        /* statistics in float64, every addend rounded to a multiple of 2^-40 first: all additions are exact */
#define RCU_MC_EXACT_MAX_PASSES 2048

/* Size of the statistics blob for n*hw voxels.  Layout: planes over voxel v = n_idx*hw + pix;
 * with neither RCU_MC_VAR nor RCU_MC_EXACT float32 planes [sum p_c (C)] [sum H (if MI)]; with either, float64 planes
 * [sum p_c (C)] [sum p_c^2 (C) (if VAR)] [sum H (if MI)].  The blob is plain additive: partial blobs of
 * disjoint pass subsets are merged by element-wise addition (one RCCL sum-reduce).
 * RCU_MC_EXACT (what the predict steps of the product use): an addend x (a pass's p_c, p_c^2 or entropy, all <= log 8) enters as
 * (x + 6144.0) - 6144.0 in float64, i.e. rounded to the nearest multiple of 2^-40; sums of such multiples below 2^13 are exactly
 * representable, so every addition -- in a kernel, between stream lanes, in the collective -- is exact and the merged statistics of
 * up to RCU_MC_EXACT_MAX_PASSES passes do not depend on the order, the pass groups, the lanes, the number of ranks or the
 * collective's reduction tree: a run on 8 GPUs writes the bytes a run on one GPU writes.  Cost against the reference's float32
 * mean: |delta p| <= 2^-41 per pass on probabilities below 2^-17. */
size_t rcu_mc_stats_bytes(size_t n, size_t hw, int nb_classes, int flags);
int rcu_mc_begin(void* stats_dev, size_t n, size_t hw, int nb_classes, int flags, void* stream);
/* in_dev: [n][C][hw] logits (softmax applied here) or probabilities (RCU_MC_INPUT_PROBS). */
int rcu_mc_accumulate(const float* in_dev, void* stats_dev, size_t n, size_t hw, int nb_classes, int flags,
                      void* stream);
/* T = number of accumulated passes.  Outputs (any may be NULL): mean [n][C][hw]; entropy, mutual_info,
 * variance [n][1][hw].  mutual_info needs RCU_MC_MI, variance needs RCU_MC_VAR. */
int rcu_mc_finalize(const void* stats_dev, size_t n, size_t hw, int nb_classes, int T, int flags, float* mean_dev,
                    float* entropy_dev, float* mutual_info_dev, float* variance_dev, void* stream);

/* F.softmax(logits, 1) (customsteps.py:24; steps.py:88) */
int rcu_softmax(const float* logits_dev, float* probs_dev, size_t n, size_t hw, int nb_classes, void* stream);
/* AleatoricPredictStep (bin-dl/brats_test_aleatoric.py:63-73) plus the writer's selection of the
 * predicted class' sigma (same file :95-97).  Outputs may be NULL. */
int rcu_aleatoric(const float* logits_dev, const float* sigma_raw_dev, size_t n, size_t hw, int nb_classes,
                  int is_log_sigma, float* probs_dev, float* sigma_dev, uint8_t* prediction_dev,
                  float* sigma_pred_dev, void* stream);
/* argmax over classes (first maximum) and the foreground-class probability map, as written to
 * *_prediction / *_probabilities.nii.gz (bin-dl/brats_test_default.py:96-99). */
int rcu_prediction_and_foreground(const float* probs_dev, size_t n, size_t hw, int nb_classes,
                                  uint8_t* prediction_dev, float* p_foreground_dev, void* stream);

/* Dropout2d factors of the MC passes of a launch, drawn on the device in one kernel: the `masks_dev` argument of
 * rcu_unet_forward_accumulate_passes (passes == 1: of rcu_unet_forward / rcu_unet_forward_accumulate) for seeded passes.
 * seeds_host[t]: the seed of pass t (the predict steps use job_seed(YAML seed, pass)); first_sample: the GLOBAL index of the batch's sample 0 --
 * its position in the run's stream of slices / images, whatever batches the loader cuts that stream into; site_channels_host / site_keep_host:
 * channels and 1 - p of the n_sites Dropout2d sites in execution order (site_keep < 0: the site is not active -- factor 1; 0: p = 1 -- factor 0).
 * out_dev: float32 [site][passes * n + i][C_site], sample t * n + i = image i in pass t.  The factor of (pass t, image i, site s, channel c) is
 * 1 / keep where the 24-bit uniform from word e & 3 of Philox4x32-10(key = seeds[t], counter = e >> 2) is below keep, else 0, with
 * e = (first_sample + i) * sum_s C_s + (C_0 + ... + C_{s-1}) + c: Bernoulli(1 - p) / (1 - p), the law of torch's Dropout2d
 * (common/model/unet.py:16), and a function of (seed, global sample index, site, channel) alone -- a slice's MC sample does not depend on the
 * batch_size it is loaded with (round 6; rounds 1-5 keyed the draw by the batch and the position in it), nor on the group, lane or rank the
 * pass is launched in. */
int rcu_dropout_masks(const uint64_t* seeds_host, int passes, int n, uint64_t first_sample, const int32_t* site_channels_host,
                      const float* site_keep_host, int n_sites, float* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Metric seam: calibration histograms (numpyfunctions.py:6-107)
 * ------------------------------------------------------------------------------------------ */
#define RCU_MAX_BINS 32
#define RCU_MAX_THRESHOLDS 16

typedef struct rcu_ece_result {           /* raw histogram of one volume, all RCU_MAX_BINS slots */
    uint64_t count[RCU_MAX_BINS];
    double sum_conf[RCU_MAX_BINS];
    uint64_t sum_pos[RCU_MAX_BINS];
} rcu_ece_result;

/* float32 thresholds t_k (k = 1..n_bins-1) with  sum_k [p >= t_k] == np.digitize(p, linspace(0,
 * 1+1e-8, n_bins+1)) - 1  for every float32 p in [0, 1]  (numpyfunctions.py:53-54). */
int rcu_ece_thresholds(int n_bins, float* thr_host);
size_t rcu_ece_workspace_bytes(size_t n_per_volume, int n_volumes);
/* Reliability histogram of n_volumes independent volumes of n_per_volume voxels each (volume v at
 * offset v * n_per_volume in every array).  mask_dev NULL = all voxels (ISIC), else voxels with
 * mask != 0 (BraTS brain mask, rechun/eval/analysis.py:118-125).  result_dev: n_volumes results. */
int rcu_ece_hist(const float* p_dev, const uint8_t* target_dev, const uint8_t* mask_dev, size_t n_per_volume,
                 int n_volumes, const float* thr_host, int n_bins, rcu_ece_result* result_dev, void* workspace_dev,
                 void* stream);
/* raw bin index per voxel (test aid: pins the binning bit-for-bit) */
int rcu_ece_bin_ids(const float* p_dev, size_t n, const float* thr_host, int n_bins, uint8_t* ids_dev, void* stream);

/* Test / tuning aid: consecutive 16,384-voxel blocks a workgroup of the histogram (ece) and of the count kernel (unc) takes;
 * 0 = the launcher's choice (default).  Integer sums: every value gives the same results.  Process-wide. */
int rcu_calib_set_blocks_per_workgroup(int ece_blocks, int unc_blocks);

size_t rcu_unc_workspace_bytes(size_t n_per_volume, int n_volumes);
/* counts_dev: [n_volumes][n_thr][8] uint64 = tp, tn, fp, fn, tpu, tnu, fpu, fnu with
 * "uncertain" := uncertainty > thr (compared in float64), numpyfunctions.py:86-107 for every
 * threshold of bin-eval/eval_uncertainty.py:239 in one pass.  unc_dev is float64 (unc_is_f64=1, what
 * ToEntropy yields) or float32. */
int rcu_unc_counts(const void* unc_dev, int unc_is_f64, const uint8_t* prediction_dev, const uint8_t* target_dev,
                   const uint8_t* mask_dev, size_t n_per_volume, int n_volumes, const double* thr_host, int n_thr,
                   uint64_t* counts_dev, void* workspace_dev, void* stream);
/* The same counts straight from the float32 foreground-probability map p, for the evaluation of the 'probabilities' confidence entry
 * (bin-eval/eval_uncertainty.py:176-202 on analysis.py:249-252: uncertainty = ToEntropy([1 - p, p])): that uncertainty is a function of the
 * float32 p alone, so {p : uncertainty(p) > thr} is a set of float32 values -- found for the script's 11 thresholds (eval_uncertainty.py:239)
 * by running the REFERENCE over every float32 in [0, 1] (tests/golden/generate_ue_boundaries.py, fixture g20, compiled in as
 * csrc/rcu_ue_table.inc): an interval of bit patterns per threshold with a ragged window of 0-3 values at either end.  The kernel looks p
 * up in that table: the counts equal the reference's integer for integer (no device log to disagree with numpy's in the last ulp) and the
 * 8-byte-per-voxel entropy map is never made (6 bytes per voxel instead of 7 + 12 for making the map).
 * thr_host: strictly ascending, every value one of rcu_unc_from_p_threshold(0 .. rcu_unc_from_p_num_thresholds() - 1), else RCU_ERR_INVALID
 * (rcu_unc_from_p_supported tells beforehand; other thresholds take rcu_normalised_entropy + rcu_unc_counts).  The table (4.4 KB) is
 * copied to the workspace with every call, stream-ordered.
 * "The reference's sets" are those of the build that made the table: numpy 2.2.6's float32 log on a CPU with AVX512 (the fixture records
 * numpy_version / cpu_features); a numpy that rounds log differently in the last ulp (another SIMD path) can disagree on the one to three
 * float32 values right at a boundary.  tests/test_oracle_golden.py::test_uncertain_voxel_table_holds_under_the_local_numpy re-evaluates
 * every probe value on the host it runs on, and bench.py re-checks the counts of its timed output on the GPU box's host (parity.ue_counts_equal);
 * where they differ, rcu_normalised_entropy + rcu_unc_counts (the map-based path) is the reference-of-that-host's arithmetic. */
int rcu_unc_from_p_num_thresholds(void);
double rcu_unc_from_p_threshold(int i);
int rcu_unc_from_p_supported(const double* thr_host, int n_thr);
/* number of the thresholds the probability p exceeds per the table (host side: tests pin the table against the fixture without a GPU); -1 = unsupported thresholds */
int rcu_unc_from_p_exceeded(float p, const double* thr_host, int n_thr);
size_t rcu_unc_from_p_workspace_bytes(size_t n_per_volume, int n_volumes);
int rcu_unc_counts_from_p(const float* p_foreground_dev, const uint8_t* prediction_dev, const uint8_t* target_dev, const uint8_t* mask_dev,
                          size_t n_per_volume, int n_volumes, const double* thr_host, int n_thr, uint64_t* counts_dev, void* workspace_dev,
                          void* stream);
/* ToEntropy (rechun/eval/analysis.py:196-203) on a foreground-probability map: float32 products,
 * float64 sum, / log 2.  Either output may be NULL. */
int rcu_normalised_entropy(const float* p_foreground_dev, size_t n, double* out_f64_dev, float* out_f32_dev,
                           void* stream);

/* EXTENSION (the reference thresholds the uncertainty at 11 hand-picked values; rcu_amd.evaluation.uncertainty_histogram, ue_curve_metrics):
 * the joint histogram of (uncertainty level, confusion cell) of n_volumes volumes of n_per_volume voxels each (volume v at offset
 * v * n_per_volume in every array, which need not be a multiple of 4), from which the threshold-free uncertainty-error metrics (AUROC / AUPRC
 * of error detection, risk-coverage area, the uncertainty-error Dice at its best threshold) are host arithmetic on integers.
 *   levels B        2 <= B <= RCU_UNC_HIST_MAX_LEVELS
 *   boundaries      t_k = (double)k / (double)B, k = 1 .. B-1: one correctly rounded float64 division each (for B = 1000 the doubles of the
 *                   script's literals 0.05, 0.1, ... 0.95: k / 1000 equals the decimal exactly, and both are rounded once)
 *   level(u)        #{k : u > t_k}, compared in float64 exactly as rcu_unc_counts compares: u <= t_1, negative u and NaN -> 0; u exactly t_k -> k-1;
 *                   u > t_{B-1} (also u > 1) -> B-1
 *   cells           tp = 0, tn = 1, fp = 2, fn = 3 (prediction != 0, target != 0); voxels with mask == 0 are skipped (mask_dev NULL = all voxels)
 *   hist_dev        [n_volumes][4][B] uint64, written (not added to)
 * Hence, for every k in 1..B-1, sum_{l >= k} hist[v][c][l] is the "uncertain" count and sum_l hist[v][c][l] the base count that rcu_unc_counts
 * returns for thr = t_k.  Integer sums: the histogram does not depend on the launch geometry, and histograms of disjoint voxel sets add.
 * rcu_unc_hist takes the prepared uncertainty map (float64 with unc_is_f64 = 1, what ToEntropy yields, or float32), like rcu_unc_counts.
 * rcu_unc_hist_from_p takes the float32 foreground-probability map and computes the normalised entropy in registers with the arithmetic of
 * rcu_normalised_entropy (one device function, csrc/rcu_entropy.h): rcu_unc_hist_from_p(p) == rcu_unc_hist(rcu_normalised_entropy(p)) integer
 * for integer, and the 8-byte-per-voxel map is never made (6 bytes read per voxel instead of 4 read + 8 written + 10 read).  It is NOT
 * table-based like rcu_unc_counts_from_p: right at a level boundary the device's logf may place one of the one to three float32 values there
 * differently from a host's numpy -- the caveat stated above for the map-based path.
 * Every argument is checked before the device is touched (RCU_ERR_INVALID, rcu_last_error() names it): levels outside
 * 2..RCU_UNC_HIST_MAX_LEVELS, a null pointer (mask_dev may be NULL), n_per_volume == 0, n_volumes outside 1..65535.
 * workspace_dev: rcu_unc_hist_workspace_bytes(...) bytes (the boundary table; 0 for levels out of range). */
#define RCU_UNC_HIST_MAX_LEVELS 4096
size_t rcu_unc_hist_workspace_bytes(size_t n_per_volume, int n_volumes, int levels);
int rcu_unc_hist(const void* unc_dev, int unc_is_f64, const uint8_t* prediction_dev, const uint8_t* target_dev, const uint8_t* mask_dev,
                 size_t n_per_volume, int n_volumes, int levels, uint64_t* hist_dev, void* workspace_dev, void* stream);
int rcu_unc_hist_from_p(const float* p_foreground_dev, const uint8_t* prediction_dev, const uint8_t* target_dev, const uint8_t* mask_dev,
                        size_t n_per_volume, int n_volumes, int levels, uint64_t* hist_dev, void* workspace_dev, void* stream);
/* Test / tuning aid (as rcu_calib_set_blocks_per_workgroup): consecutive blocks (16,384 voxels; 65,536 for levels > 1365) a workgroup of the level
 * histogram takes, at most 64; 0 = the launcher's choice (default).  Integer sums: every value gives the same histogram.  Process-wide. */
int rcu_unc_hist_set_blocks_per_workgroup(int blocks);

/* EXTENSION (the reference's calibration measure is one ECE over at most RCU_MAX_BINS equal-width bins; rcu_amd.evaluation.calibration_levels,
 * calibration_curve_metrics, isotonic_levels): the calibration level histogram of n_volumes volumes of n_per_volume voxels each (volume v at
 * offset v * n_per_volume in every array, which need not be a multiple of 4; the bases need not be 16-byte aligned), from which the proper
 * scoring rules (Brier, NLL), Murphy's decomposition, equal-width / equal-mass / maximum / Kolmogorov-Smirnov calibration errors, a reliability
 * curve and an isotonic recalibration map are host arithmetic on integers.  Integer sums: the outputs do not depend on the launch geometry,
 * and those of disjoint voxel sets add.
 *   levels B        2 <= B <= RCU_CALIB_CURVE_MAX_LEVELS
 *   thresholds      t_k, k = 1 .. B-1: exactly what rcu_ece_thresholds would give for n_bins = B -- the smallest float32 >= k * ((1 + 1e-8) / B),
 *                   the edges of np.linspace(0, 1 + 1e-8, B + 1) the reference's _binary_calibration digitises against.  For every divisor
 *                   n of B the thresholds t_{k B / n} of B levels are bit-equal to the thresholds t_k of n bins (checked for every B in
 *                   2..4096): merging B / n consecutive levels gives the reference's n-bin histogram for every float32 p.
 *   level(p)        #{k : p >= t_k}: p = 1 (and anything above) -> B-1; NaN and negative p -> 0; p = 0.5 -> level 499 of 1000, bin 4 of 10
 *   levels_dev      [n_volumes][3][B] uint64, written (not added to): plane 0 the voxels with target == 0 per level, plane 1 those with
 *                   target != 0, plane 2 the sum of Q(p) over all voxels of the level,
 *                   Q(p) = rint(c(p) * 2^32), c(p) = clamp((double)p, 0, 1), ties to even, NaN -> 0.  (double)p * 2^32 is an integer for
 *                   float32 p >= 2^-9: the confidence sums are exact there; below, each voxel is off by at most 2^-33.
 *   totals_dev      [n_volumes][2][4] uint64, written: per target class y (0: target == 0) n_y, sum Q(p), sum Q2(p), sum N(p, y) with
 *                   Q2(p) = rint(c(p) * c(p) * 2^32) (the product is exact in float64; for p in [0, 1] c(p) is p itself) and the NLL term
 *                   N = rint(l * 2^20), l = -logf(fmaxf(p_y, 2^-23)) clamped to [0, 23 ln 2], p_y = y ? p : 1.0f - p in float32 --
 *                   the convention of rcu_temperature_nll (NaN p: p_y counts as 2^-23)
 *   mask            voxels with mask == 0 are skipped; mask_dev NULL = all voxels
 * Every argument is checked before the device is touched (RCU_ERR_INVALID, rcu_last_error() names it): levels outside
 * 2..RCU_CALIB_CURVE_MAX_LEVELS, a null pointer (mask_dev may be NULL), n_per_volume == 0, n_volumes outside 1..65535.
 * workspace_dev: rcu_calib_curve_workspace_bytes(...) bytes (the threshold table; 0 for levels out of range).
 * rcu_calib_curve_thresholds writes the levels - 1 thresholds to host memory and touches no device.
 * rcu_calib_curve_terms (test aid, as rcu_ece_bin_ids and rcu_temperature_nll_terms) writes every voxel's level and its float32 l (clamped,
 * before the rounding to N) with the scan's arithmetic bit for bit; it takes no mask. */
#define RCU_CALIB_CURVE_MAX_LEVELS 4096
int rcu_calib_curve_thresholds(int levels, float* thr_host);
size_t rcu_calib_curve_workspace_bytes(size_t n_per_volume, int n_volumes, int levels);
int rcu_calib_curve(const float* p_foreground_dev, const uint8_t* target_dev, const uint8_t* mask_dev, size_t n_per_volume, int n_volumes,
                    int levels, uint64_t* levels_dev, uint64_t* totals_dev, void* workspace_dev, void* stream);
int rcu_calib_curve_terms(const float* p_foreground_dev, const uint8_t* target_dev, size_t n, int levels, int32_t* level_dev, float* nll_dev,
                          void* stream);
/* Test / tuning aid (as rcu_unc_hist_set_blocks_per_workgroup): consecutive blocks (16,384 voxels; 65,536 for levels > 1365) a workgroup of the
 * calibration level histogram takes, at most 64; 0 = the launcher's choice (default).  Integer sums: every value gives the same result.  Process-wide. */
int rcu_calib_curve_set_blocks_per_workgroup(int blocks);

/* ------------------------------------------------------------------------------------------
 * Test-time augmentation (EXTENSION: the reference has no TTA; rcu_amd.steps.TtaMcPredictStep)
 *   The network runs on transformed copies g(x) of every slice, the statistics of those passes are mapped back with g^-1 and added to
 *   the canonical statistics.  The transforms are the eight elements of the dihedral group D4 acting on the last two axes (H, W) of an
 *   NCHW tensor, each defined by its torch equivalent:
 *     0 identity        x                                      4 transpose        x.transpose(-2, -1)
 *     1 flip_h          x.flip(-1)                             5 rot90            torch.rot90(x, 1, (-2, -1))
 *     2 flip_v          x.flip(-2)                             6 rot270           torch.rot90(x, 3, (-2, -1))
 *     3 rot180          x.flip(-2, -1)                         7 anti_transpose   torch.rot90(x, 2, (-2, -1)).transpose(-2, -1)
 *   Codes 0-4 and 7 are their own inverses; rot90 and rot270 are each other's.  Codes 4-7 swap H and W: they are accepted for square
 *   planes only (BraTS 240 x 240 -- not ISIC 192 x 256), elsewhere the call fails with RCU_ERR_INVALID (never a silent skip).
 *   Dropout masks of a transformed pass: rcu_dropout_masks at first_sample = the slice's global index under a key of (seed, element,
 *   pass) alone -- the identity's key is the plain MC key of the pass, every other element's differs from all of those and from each
 *   other's for passes 1..RCU_MC_EXACT_MAX_PASSES (rcu_amd.steps.tta_pass_seed).
 * ------------------------------------------------------------------------------------------ */
#define RCU_TTA_IDENTITY 0
#define RCU_TTA_FLIP_H 1
#define RCU_TTA_FLIP_V 2
#define RCU_TTA_ROT180 3
#define RCU_TTA_TRANSPOSE 4
#define RCU_TTA_ROT90 5
#define RCU_TTA_ROT270 6
#define RCU_TTA_ANTI_TRANSPOSE 7

/* out = g(x), x and out [n][channels][H][W] float32, out != x (the two must not overlap); codes 4-7 need H == W.  n, channels, H, W >= 1. */
int rcu_tta_transform(const float* x_dev, size_t n, int channels, int height, int width, int element, float* out_dev, void* stream);
/* dst += g^-1(src), plane by plane, over the rcu_mc_stats_bytes layout (n entries, hw = H*W, flags as for rcu_mc_begin: a combination of
 * RCU_MC_MI, RCU_MC_VAR, RCU_MC_EXACT, anything else is RCU_ERR_INVALID): src holds statistics accumulated from images transformed by g.
 * Every plane of the layout is folded -- the C class sums, the C sums of p^2 (VAR), the entropy sum (MI) -- with one addition per element:
 * dst[v] + src[g(v)].  Under RCU_MC_EXACT the addition is exact, so the merged statistics do not depend on the order of the folds; in the
 * float32 and the plain float64 (VAR without EXACT) forms the result is that of the folds in call order, each one a single rounded addition
 * per element (rcu_amd.steps.TtaMcPredictStep folds a lane's transforms in the order the transforms are given, then adds the side lanes'
 * statistics into lane 0's in lane order).  src and dst must not overlap. */
int rcu_mc_fold_transformed(const void* src_stats_dev, void* dst_stats_dev, size_t n, int height, int width, int nb_classes, int flags,
                            int element, void* stream);

/* ------------------------------------------------------------------------------------------
 * Temperature scaling (EXTENSION: the reference has no calibration fitting; rcu_amd.calibration)
 *   Post-hoc scaling of the classifier by one scalar T: every pass's logits become z / T before the softmax (Guo et al. 2017 for one
 *   deterministic pass, Laves et al. 2019 for MC dropout), T fitted to minimise the NLL of the pass-averaged prediction on held-out volumes.
 * ------------------------------------------------------------------------------------------ */
/* Scale the classifier of the handle by 1 / temperature: at rcu_unet_finalize_weights, conv_cls.1.weight and .bias are packed as
 * (float)((double)w / temperature) -- conv_cls.1 is a 1x1 conv, so softmax((Wx + b) / T) = softmax((W / T) x + b / T) and every forward path
 * (fused and standalone head, MC statistics, TTA, pass groups) honours T with no kernel change.  The sigma head is not touched.
 * Call before rcu_unet_finalize_weights (afterwards: RCU_ERR_STATE; rcu_unet_load_weight re-opens the handle); temperature finite and > 0,
 * else RCU_ERR_INVALID; a sigma_out handle is RCU_ERR_INVALID (its sigma is in logit units: scaling the mean alone has no defined meaning).
 * T = 1 packs the bytes of a handle that never called this. */
int rcu_unet_set_temperature(rcu_unet* h, double temperature);

/* NLL sweep over n_candidates inverse temperatures beta_k (beta_host: finite, > 0).
 *   logits_dev  [passes][n][C][hw] float32: the pass-major output of ONE rcu_unet_forward over the batch repeated `passes` times (sample t * n + i),
 *               masks from rcu_dropout_masks with the passes' seeds -- or eval-mode logits with passes = 1
 *   target_dev  [n][hw] class indices; mask_dev [n][hw] (voxels with mask != 0) or NULL (all voxels)
 * For every voxel v inside the mask and every k:  l_k(v) = -log( (1/P) sum_t softmax(beta_k z_{t,v})[y_v] ), computed in float32 in the log
 * domain (correct when every pass's probability underflows float32), clamped to [0, 4096], rounded to the nearest multiple of 2^-20 (ties to
 * even) and ADDED as an unsigned 64-bit integer: out_dev[k] += sum_v round(l_k(v) * 2^20).  out_dev[n_candidates] += the number of voxels
 * summed, out_dev[n_candidates + 1] += the number of voxels inside the mask whose target is >= C (they are left out of the sums).  The caller
 * zeroes out_dev once; every call adds to it, stream-ordered.  Integer sums: the result does not depend on how the voxels are split over
 * workgroups or calls (the idea of RCU_MC_EXACT).
 * Limits: 2 <= C <= 8, 1 <= passes <= RCU_MC_EXACT_MAX_PASSES, 1 <= n_candidates <= 128, n >= 1, hw >= 1, n * hw < 2^32.  Every argument is
 * checked before the device is touched (RCU_ERR_INVALID).  workspace_dev: rcu_temperature_nll_workspace_bytes(n * hw, n_candidates) bytes. */
size_t rcu_temperature_nll_workspace_bytes(size_t voxels, int n_candidates);
int rcu_temperature_nll(const float* logits_dev, int passes, size_t n, size_t hw, int nb_classes, const uint8_t* target_dev,
                        const uint8_t* mask_dev, const float* beta_host, int n_candidates, uint64_t* out_dev, void* workspace_dev, void* stream);
/* Test aid (as rcu_ece_bin_ids): the float32 l(v) of every voxel for one beta, the arithmetic of rcu_temperature_nll bit for bit (before the
 * clamp); 0 outside the mask and where the target is >= C.  terms_dev: [n][hw] float32. */
int rcu_temperature_nll_terms(const float* logits_dev, int passes, size_t n, size_t hw, int nb_classes, const uint8_t* target_dev,
                              const uint8_t* mask_dev, float beta, float* terms_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Test-time logit sampling (EXTENSION: the reference writes softmax(mu) of its sigma-head models; rcu_amd.steps.AleatoricPredictStep /
 * AleatoricMcPredictStep with logit_samples = S)
 *   A sigma-head U-Net (sigma_out) is trained on the NLL of E_eps[softmax(mu + sigma * eps)] (Kendall & Gal 2017).  At test time the sampled
 *   predictive of a voxel with logits mu[c] and raw sigma raw[c] (c < C <= 8) is
 *       sig[c]   = is_log_sigma ? expf(raw[c]) : fabsf(raw[c])
 *       p_bar[c] = (1/S) sum_{s < S} softmax(mu + sig * z_s)[c]     (for s in order: x[c] = fmaf(sig[c], z, mu[c]), softmax, float32 sum; / S)
 *   with the normal z(K, g, p, s, c) of the pass key K, the slice's GLOBAL index g, the pixel p = y * W + x, the sample s and the class c:
 *       j = s * C + c;  w[0..3] = Philox4x32-10(key (K lo, K hi), counter (p, g lo, g hi, 2^31 | j >> 2))
 *       u[i] = ((w[i] >> 8) + 0.5f) * 2^-24 in float32;  (a, b) = (u0, u1) if (j & 3) < 2 else (u2, u3)
 *       r = sqrtf(-2 logf(a)),  sincospif(2 b, &sn, &cs),  z = (j & 1) ? r sn : r cs
 *   Bit 31 of counter word 3 keeps the noise apart from rcu_dropout_masks (words 2 and 3 are 0 there): a pass may use its mask key.  The first
 *   S samples do not depend on the total S.  With MC dropout pass t adds p_bar_t where it would add softmax(mu_t): entropy of the mean is the
 *   total uncertainty, the mutual information the epistemic part and entropy - mutual information = mean_t H(p_bar_t) the aleatoric part.
 * ------------------------------------------------------------------------------------------ */
#define RCU_LOGIT_MAX_SAMPLES 1024

/* Test aid: out_dev[v][s][c] = z(key, first_sample + v / hw, v % hw, s, c) for the n * hw voxels v, s < samples, c < nb_classes (float32,
 * n * hw * samples * nb_classes elements).  RCU_ERR_INVALID for a null out_dev, nb_classes outside 1..8, samples outside
 * 1..RCU_LOGIT_MAX_SAMPLES, n or hw of 0, hw >= 2^32. */
int rcu_logit_normals(uint64_t key, uint64_t first_sample, size_t n, size_t hw, int nb_classes, int samples, float* out_dev, void* stream);
/* The sampled predictive of materialised logits_dev and sigma_raw_dev ([n][nb_classes][hw] float32, the outputs of rcu_unet_forward) under
 * `key`, image i being slice first_sample + i: written to probs_dev ([n][nb_classes][hw], or NULL) and / or added to the statistics blob
 * stats_dev (rcu_mc_stats_bytes layout, flags a combination of RCU_MC_MI, RCU_MC_VAR, RCU_MC_EXACT -- the addition of rcu_mc_accumulate with
 * p_bar in place of the softmax; or NULL).  RCU_ERR_INVALID for null inputs, both outputs NULL, other flags, and the limits of
 * rcu_logit_normals. */
int rcu_logit_sampling(const float* logits_dev, const float* sigma_raw_dev, size_t n, size_t hw, int nb_classes, int is_log_sigma, int samples,
                       uint64_t key, uint64_t first_sample, float* probs_dev, void* stats_dev, int flags, void* stream);
/* rcu_unet_forward_accumulate_sigma_passes with the sampled predictive: pass t of the group (masks as there) adds p_bar_t under keys_host[t]
 * ([passes] on the host, read before the call returns) into stats_dev, and its sig to sigma_sum_dev exactly as
 * rcu_unet_forward_accumulate_sigma_passes adds it.  Image i is slice first_sample + i.  Neither mu nor sigma reaches HBM: the sampling runs
 * in the head kernel (a group of more than 32 passes as one head launch per 32 passes, in pass order -- the same bits).  RCU_ERR_INVALID for
 * a null handle or pointer, a handle without sigma_out, n * passes outside 1..max_batch, samples outside 1..RCU_LOGIT_MAX_SAMPLES. */
int rcu_unet_forward_sample_sigma_passes(rcu_unet* h, const float* x_dev, int n, int passes, const float* masks_dev, const uint64_t* keys_host,
                                         uint64_t first_sample, int samples, void* stats_dev, int flags, float* sigma_sum_dev, int is_log_sigma,
                                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Connected components (EXTENSION: every measure of the reference is per voxel; rcu_amd.evaluation.connected_components, component_table,
 * component_metrics and the 'components' evaluation action work on connected regions)
 *   Labelling.  n_volumes independent volumes of depth x height x width uint8 voxels each (volume v at offset v * depth * height * width; a voxel
 *   is foreground iff its value is not 0), connectivity 6 (face neighbours) or 26 (the 3 x 3 x 3 neighbourhood); with depth 1 these are the 2-D
 *   4- and 8-neighbourhoods.  Volumes never connect to each other.
 *     labels_dev   [n_volumes][depth * height * width] int32: 0 for background, for foreground 1 + the smallest linear index (C order within
 *                  the volume) of any voxel of the component -- a function of the mask alone, whatever the tiles, the launch order or the batch
 *   Block-based union-find (csrc/rcu_cc.hip): a tile-local pass in LDS, a seam pass and a flatten pass in global memory with agent-scope atomics,
 *   lock-free (no workgroup ever waits for another).
 *   Limits: depth, height, width >= 1, fewer than 2^31 - 1 voxels per volume, n_volumes in 1..65535, connectivity 6 or 26.
 *
 *   Table.  The components of the whole batch in increasing order of (volume, label) -- within a volume the raster order of the components' first
 *   voxels, the numbering of scipy.ndimage.label --, one rcu_cc_entry each:
 *     root           label - 1: the linear index of the component's first voxel
 *     voxels         its size
 *     other_voxels   its voxels where other_dev is not 0 (0 without other_dev)
 *     unc_sum        the sum of q(u) over its voxels,   q(u) = rint(clamp(u, 0, 1) * 2^24) in float64, ties to even, NaN -> 0
 *     unc_max        the maximum of q(u)
 *   Integer sums (the idea of RCU_MC_EXACT): the table carries the same bits whatever the launch geometry or batching.  u is a float32 map
 *   (RCU_CC_UNC_F32), a float64 map (RCU_CC_UNC_F64) or the normalised entropy of a float32 foreground-probability map computed in registers
 *   with the arithmetic of rcu_normalised_entropy (RCU_CC_UNC_P: the table equals the one of RCU_CC_UNC_F64 on rcu_normalised_entropy's output,
 *   integer for integer); RCU_CC_UNC_NONE with a null unc_dev leaves unc_sum and unc_max 0.
 *   Three calls, all stream-ordered, over labels in the format above:
 *     rcu_cc_compact   ranks the roots: counts_dev[v] (uint32, [n_volumes]) = the components of volume v; the ranks stay in workspace_dev
 *     rcu_cc_relabel   dense_dev [n_volumes][n_per_volume] int32 = 1 .. counts[v] in table order, 0 for background (may be labels_dev itself)
 *     rcu_cc_table     fills table_dev[0 .. table_entries), table_entries = the sum of counts (the caller reads the counts in between); volume
 *                      v's rows start at the sum of the counts in front of it.  Rows beyond table_entries are never written.
 *   workspace_dev: rcu_cc_workspace_bytes(n_per_volume, n_volumes) bytes, the same memory for the three calls (0 for arguments out of range).
 *   Limits: those of the labelling and n_per_volume * n_volumes < 2^32.
 *   Every argument is checked before the device is touched (RCU_ERR_INVALID, rcu_last_error() names it).
 * ------------------------------------------------------------------------------------------ */
#define RCU_CC_UNC_NONE 0
#define RCU_CC_UNC_F32 1
#define RCU_CC_UNC_F64 2
#define RCU_CC_UNC_P 3
typedef struct rcu_cc_entry {
    int32_t root;
    uint32_t voxels, other_voxels, unc_max;
    uint64_t unc_sum;
} rcu_cc_entry;      /* 24 bytes */

int rcu_cc_label(const uint8_t* mask_dev, int depth, int height, int width, int n_volumes, int connectivity, int32_t* labels_dev, void* stream);
size_t rcu_cc_workspace_bytes(size_t n_per_volume, int n_volumes);
int rcu_cc_compact(const int32_t* labels_dev, size_t n_per_volume, int n_volumes, uint32_t* counts_dev, void* workspace_dev, void* stream);
int rcu_cc_relabel(const int32_t* labels_dev, size_t n_per_volume, int n_volumes, const void* workspace_dev, int32_t* dense_dev, void* stream);
int rcu_cc_table(const int32_t* labels_dev, const uint8_t* other_dev, const void* unc_dev, int unc_kind, size_t n_per_volume, int n_volumes,
                 const void* workspace_dev, rcu_cc_entry* table_dev, size_t table_entries, void* stream);
/* Test / tuning aid (as rcu_unc_hist_set_blocks_per_workgroup): the tile of the labelling's LDS pass, every extent >= 1 and at most 1024 voxels
 * in all; 0, 0, 0 = the launcher's choice (4 x 8 x 32, or 1 x 16 x 64 for depth 1).  Every tile gives the same labels.  Process-wide. */
int rcu_cc_set_tile(int tile_depth, int tile_height, int tile_width);

/* ------------------------------------------------------------------------------------------
 * Component pairs (EXTENSION: the joint table of two labellings; rcu_amd.evaluation.component_pairs, lesion_tables, lesion_metrics and the
 * 'lesions' evaluation action: lesion-wise Dice, lesion F1, panoptic quality, one-to-one matching, filtering of lesions by uncertainty)
 *   a_dev, b_dev   [n_volumes][n_per_volume] int32 label maps: 0 (and every negative value) is background, positive values are ids.  The
 *                  outputs of rcu_cc_relabel and of rcu_cc_label are both valid; nothing is assumed about how dense the ids are.
 *   inside_dev     [n_volumes][n_per_volume] uint8 or null
 *   table_dev      rcu_cc_pairs_bytes(capacity, n_volumes) bytes (0 for arguments out of range): per volume `capacity` slots of one rcu_cc_pair
 *                  -- volume v's slots start at slot v * capacity --, then, 256-byte aligned behind the slots of all volumes, two uint32
 *                  counters per volume: used (slots claimed) and dropped (voxels whose pair found no slot after `capacity` probes)
 *   A slot is empty iff its a and b are 0 (a real pair has both above 0).  For a pair (a, b), voxels = the voxels of the volume that carry label
 *   a in A and b in B, inside_voxels = those of them where inside_dev is not 0 (0 without inside_dev).  The call clears table_dev itself,
 *   stream-ordered.  Open addressing with linear probing (csrc/rcu_cc_pairs.hip): the hashed key is (uint64) a << 32 | b, the slot's first
 *   eight bytes are claimed with one 64-bit compare-and-swap; per wave one insert per distinct pair; nobody waits for anybody.  The ORDER of
 *   the slots is the race's; the sorted list of the non-empty slots is a function of the inputs alone whenever dropped == 0 (integer adds: the
 *   same bits whatever the launch geometry, the batching or the hash).  With dropped != 0 the table is full and lacks pairs -- a voxel is
 *   either counted in the table or counted as dropped --: run again with a larger capacity (one of at least 2 * n_per_volume always suffices).
 *   Limits: capacity a power of two in 64..2^26; those of rcu_cc_table: n_per_volume in 1..2^31 - 2, n_volumes in 1..65535, n_per_volume *
 *   n_volumes < 2^32.  Every argument is checked before the device is touched (RCU_ERR_INVALID, rcu_last_error() names it).
 * ------------------------------------------------------------------------------------------ */
typedef struct rcu_cc_pair {
    uint32_t a, b, voxels, inside_voxels;
} rcu_cc_pair;      /* 16 bytes */

size_t rcu_cc_pairs_bytes(size_t capacity, int n_volumes);
int rcu_cc_pairs(const int32_t* a_dev, const int32_t* b_dev, const uint8_t* inside_dev, size_t n_per_volume, int n_volumes, size_t capacity,
                 void* table_dev, void* stream);
/* Test aid (as rcu_cc_set_tile): the hash of a pair is shifted right by `shift` bits (0..63; 0 = the whole hash) before it picks the start slot, so
 * that small inputs crowd into a few start slots and probe long chains.  Every shift gives the same sorted table.  Process-wide. */
int rcu_cc_pairs_set_hash_shift(int shift);

/* ------------------------------------------------------------------------------------------
 * Distance transform (EXTENSION: where in the image the errors and the uncertainty sit; rcu_amd.evaluation.distance_transform_sq, boarder_mask,
 * boundary_table, surface_distance_histograms and the 'boundary' evaluation action.  The reference builds its border shell with two host
 * distance transforms: common/utils/labelhelper.py:12-20)
 *   Transform.  n_volumes independent volumes of depth x height x width uint8 voxels, laid out as for rcu_cc_label; volumes never see each other.
 *   The feature set of a volume is its voxels with value 0 (zero_is_feature = 1: scipy.ndimage.distance_transform_edt(mask)) or with a value
 *   other than 0 (zero_is_feature = 0: the transform of ~mask, with no inverted copy made).
 *     out_dev   [n_volumes][depth * height * width] uint32: the minimum over the feature voxels w of the same volume of |v - w|^2, unit spacing:
 *               an exact integer, 0 on the feature voxels -- a function of the mask alone, whatever the launch geometry or the batch
 *   A volume without a feature voxel gets RCU_EDT_NONE everywhere.  (scipy's output there is an artefact -- distances to a virtual voxel in front
 *   of the array -- and is NOT copied.)  Depth 1 gives the 2-D transform.
 *   Three separable passes in place in out_dev (csrc/rcu_edt.hip): a two-sweep ballot scan per row, then min_j f(j) + (i - j)^2 along the height
 *   and the depth from a slab in LDS, every thread walking outward from its own voxel until (i - j)^2 reaches its best.  Integers only; sums with
 *   NONE saturate.
 *   Limits: every extent in 1..16384 (the three squares then add below 2^32 - 1), fewer than 2^31 - 1 voxels per volume, n_volumes in 1..65535,
 *   n_per_volume * n_volumes < 2^32, zero_is_feature 0 or 1.
 *
 *   Border shell.  From d_in = the transform of a label map with zero_is_feature = 1 (squared distance to the nearest background voxel) and d_out
 *   = the one with zero_is_feature = 0 (to the nearest foreground voxel), n entries each:
 *     mask_dev       uint8 (d_in <= distance_in^2) && (d_out <= distance_out^2), compared in integers: labelhelper.boarder_mask's mask
 *     distance_dev   float64 sqrt(d_in + d_out), correctly rounded (one of the two terms is 0): labelhelper.boarder_mask's distance, bit for bit
 *   RCU_EDT_NONE counts as +inf: no border on that side, and the distance is inf.  Either output may be null, not both.  distance_in and
 *   distance_out in 0..65535.
 *
 *   Boundary table.  Per volume 2 x (bands + 1) cells, cell (side, band) at index side * (bands + 1) + band:
 *     side   target != 0;     band   from d = d_in + d_out of the TARGET: band k < bands holds k^2 < d <= (k + 1)^2, band `bands` holds
 *            d > bands^2, RCU_EDT_NONE included.  Integer comparisons.  Band 0 of both sides together is the reference's border shell (1, 1).
 *     voxels, errors ((prediction != 0) != (target != 0)), unc_sum = the sum of q(u) over the cell's voxels, unc_err_sum = over its error voxels
 *   q and the uncertainty sources are rcu_cc_table's (RCU_CC_UNC_NONE / _F32 / _F64 / _P, the same arithmetic).  Integer sums, reduced per wave and
 *   per workgroup in LDS before they reach global memory: the same bits whatever the batching.  bands in 1..64; the limits of rcu_cc_table.
 *
 *   Surface distances.  The surface of a label map A is S(A) = {v in A : d_in_A(v) == 1}: the voxels of A that are face-adjacent to a voxel
 *   outside A INSIDE the volume (A & ~scipy.ndimage.binary_erosion(A, border_value=1); medpy's border_value=0 differs from it only where A touches
 *   the volume face, whose voxels medpy counts as surface).  For the maps P and T of every volume:
 *     hist_dev   [n_volumes][2][bins] uint32, bins = rcu_surface_distance_bins(depth, height, width) = (D-1)^2 + (H-1)^2 + (W-1)^2 + 2:
 *                direction 0 counts the voxels of S(P) by their squared distance to S(T) (rcu_edt_sq with the feature set S(T)), direction 1 the
 *                voxels of S(T) by their squared distance to S(P); the LAST bin counts the voxels whose other surface is empty (RCU_EDT_NONE)
 *   workspace_dev: rcu_surface_distance_workspace_bytes(n_per_volume, n_volumes) bytes (0 for arguments out of range).  The limits of rcu_edt_sq.
 *   Every argument is checked before the device is touched (RCU_ERR_INVALID, rcu_last_error() names it).
 * ------------------------------------------------------------------------------------------ */
#define RCU_EDT_NONE 0xFFFFFFFFu
typedef struct rcu_boundary_cell {
    uint64_t voxels, errors, unc_sum, unc_err_sum;
} rcu_boundary_cell;      /* 32 bytes */

int rcu_edt_sq(const uint8_t* mask_dev, int depth, int height, int width, int n_volumes, int zero_is_feature, uint32_t* out_dev, void* stream);
int rcu_border_mask(const uint32_t* d_in_dev, const uint32_t* d_out_dev, size_t n, int distance_in, int distance_out, uint8_t* mask_dev,
                    double* distance_dev, void* stream);
int rcu_boundary_table(const uint8_t* prediction_dev, const uint8_t* target_dev, const uint32_t* d_in_dev, const uint32_t* d_out_dev,
                       const void* unc_dev, int unc_kind, size_t n_per_volume, int n_volumes, int bands, rcu_boundary_cell* table_dev, void* stream);
size_t rcu_surface_distance_bins(int depth, int height, int width);
size_t rcu_surface_distance_workspace_bytes(size_t n_per_volume, int n_volumes);
int rcu_surface_distance_hist(const uint8_t* prediction_dev, const uint8_t* target_dev, int depth, int height, int width, int n_volumes,
                              uint32_t* hist_dev, void* workspace_dev, void* stream);
/* Test / tuning aid (as rcu_cc_set_tile): the run of adjacent x a workgroup of the height / depth passes stages per line, a power of two in
 * 1..64; 0 = the launcher's choice (32).  It is halved until a whole line fits the slab (16384 entries).  Every width gives the same distances.
 * Process-wide. */
int rcu_edt_set_slab_width(int slab_width);

/* ------------------------------------------------------------------------------------------
 * Sample agreement (EXTENSION: the reference's uncertainties are per-voxel moments of the pass probabilities; rcu_amd.steps.McPredictStep with
 * agreement=True, SampleAgreementStep, rcu_amd.evaluation.agreement_tables / agreement_metrics and the 'agreement' evaluation action look at
 * the T samples as whole segmentations -- the structure-wise uncertainties of Roy et al., Bayesian QuickNAT, 2019)
 *   Vote plane.  votes_dev is uint32 [n_words][V] over the voxels v = image * hw + pixel of a batch, V = n * hw, zeroed by its owner before the
 *   first pass.  Pass j (1-based) owns bit (j - 1) % 32 of word (j - 1) / 32; RCU_VOTES_MAX_PASSES = 64 passes, so n_words is 1 or 2.  The bit
 *   at v is set iff the arg-max of the vector the pass adds to the MC statistics at v is not class 0, ties going to the lower class as in
 *   rcu_prediction_and_foreground (two classes: p[1] > p[0]).  The entries below only ever OR bits in; they leave every other bit alone.
 *   Tables.  A volume is a run of n_per_volume consecutive voxels of the plane.  With A_i the set of voxels of the volume pass i + 1 voted for:
 *       hist[vol][c],      c = 0..T        voxels with exactly c of the bits 0..T-1 set                          (uint64 [n_volumes][T + 1])
 *       pairs[vol][i][j],  0 <= i <= j < T |A_i & A_j|, row-major upper triangle with the diagonal (= the |A_i|) (uint64 [n_volumes][T (T + 1) / 2])
 *   Bits at or above T are ignored.  All integers: the tables are a function of the plane alone and the tables of slices add up to their subject's.
 * ------------------------------------------------------------------------------------------ */
#define RCU_VOTES_MAX_PASSES 64

/* rcu_unet_forward_accumulate_passes that also votes: pass t of the group (masks as there; passes == 1: one pass) ORs bit bits_host[t] (int32
 * [passes] on the host, read before the call returns; bit b lives in word b / 32 at bit b % 32) of votes_dev.  The statistics receive what
 * rcu_unet_forward_accumulate_passes gives them, bit for bit.  The forward takes the separate head kernel (as under rcu_unet_set_fuse_head(h,
 * 0)); the voxel's word is read and written once per launch beside its statistics entries, a group whose bits straddle a word (or of more than
 * 32 passes) runs as one head launch per word, in pass order.  No atomics: launches that share a plane must share a stream.
 * RCU_ERR_INVALID, before anything is launched, for a null handle / x_dev / stats_dev / votes_dev / bits_host, n_words outside 1..2, a bit
 * outside [0, 32 * n_words), nb_classes outside 1..8 and n * passes outside 1..max_batch. */
int rcu_unet_forward_accumulate_votes(rcu_unet* h, const float* x_dev, int n, int passes, const float* masks_dev, void* stats_dev, int flags,
                                      uint32_t* votes_dev, int n_words, const int32_t* bits_host, void* stream);
/* The vote of one pass over a materialised [n][nb_classes][hw] float32 volume: probabilities (flags = RCU_MC_INPUT_PROBS), or logits (flags = 0),
 * which go through the softmax of rcu_mc_accumulate first -- the vote is the arg-max of what the statistics would receive.  ORs bit `bit` of
 * votes_dev ([n_words][n * hw]).  RCU_ERR_INVALID for null pointers, n_words outside 1..2, bit outside [0, 32 * n_words), nb_classes outside
 * 1..8; n * hw == 0 is a no-op. */
int rcu_mc_votes(const float* in_dev, size_t n, size_t hw, int nb_classes, int flags, uint32_t* votes_dev, int n_words, int bit, void* stream);
/* hist_dev and pairs_dev (zeroed here, then filled on `stream`) of the n_volumes volumes of n_per_volume voxels of votes_dev
 * ([n_words][n_per_volume * n_volumes]) for T = passes.  RCU_ERR_INVALID for null pointers, n_words outside 1..2, passes outside
 * 1..32 * n_words, n_per_volume outside 1..2^31-2, n_volumes outside 1..65535, n_per_volume * n_volumes >= 2^32. */
int rcu_agreement_tables(const uint32_t* votes_dev, int n_words, size_t n_per_volume, int n_volumes, int passes, uint64_t* hist_dev,
                         uint64_t* pairs_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Patch-level uncertainty (EXTENSION: the patch accuracy vs. patch uncertainty family of Mukhoti & Gal, Evaluating Bayesian Deep Learning Methods
 * for Semantic Segmentation, 2018 -- p(accurate | certain), p(uncertain | inaccurate), PAvPU; rcu_amd.evaluation.patch_table, patch_histogram,
 * pavpu_metrics and the 'patches' evaluation action)
 *   Grid.  n_volumes independent volumes of depth x height x width voxels, laid out as for rcu_cc_label.  A volume is cut into non-overlapping
 *   patches of pd x ph x pw voxels (each extent in 1..RCU_PATCH_MAX_EXTENT) anchored at the origin: patch (gz, gy, gx) holds the voxels with
 *   z / pd == gz, y / ph == gy, x / pw == gx; the patches at the far edges are partial.  rcu_patch_count = ceil(depth / pd) * ceil(height / ph) *
 *   ceil(width / pw) patches per volume, numbered in raster order (gx fastest); 0 for arguments out of range.  Depth 1 gives the 2-D grid.
 *   Table.  table_dev is uint64 [n_volumes][patches][4], the row of a patch {n, errors, foreground, sum_q} over its voxels whose mask byte is
 *   not 0 (every voxel with a null mask_dev):
 *       n            the number of such voxels                     errors   those with (prediction != 0) != (target != 0)
 *       foreground   those with prediction != 0 or target != 0     sum_q    the sum of q(u), q and the uncertainty sources being rcu_cc_table's
 *   (RCU_CC_UNC_NONE / _F32 / _F64 / _P, the same arithmetic and the same argument check; RCU_CC_UNC_NONE leaves sum_q 0).  A patch has at most
 *   4096 voxels, so sum_q <= 2^36.  Integers, one lane per patch (csrc/rcu_patch.hip): the table is a function of the inputs alone, whatever the
 *   launch geometry, the batching (volumes in one call or in several) or the alignment of a volume's first element.
 *   Histogram.  hist_dev is uint64 [n_volumes][3][levels], zeroed here: every table row with n != 0 adds 1 to hist[cell][level] with
 *       cell 0   accurate patch that holds foreground: 1000 (n - errors) > accuracy_per_mille n, and foreground > 0
 *       cell 1   inaccurate patch (it necessarily holds foreground)            cell 2   accurate patch of pure background
 *       level    the level of the patch's mean uncertainty sum_q / (n 2^24) under the rule of rcu_unc_hist, level(u) = #{k in 1..levels-1 : u > k /
 *                levels}, taken IN INTEGERS: #{k : sum_q levels > k n 2^24} = min(levels - 1, (sum_q levels - 1) div (n 2^24)) for sum_q > 0, else 0
 *   (rows of rcu_patch_table keep every product below 2^49).  Histograms of volumes add.
 *   Limits: depth * height * width and n_patches in 1..2^31 - 2, n_volumes in 1..65535, levels in 2..RCU_UNC_HIST_MAX_LEVELS, accuracy_per_mille in
 *   0..999.  Every argument is checked before the device is touched (RCU_ERR_INVALID, rcu_last_error() names it).
 * ------------------------------------------------------------------------------------------ */
#define RCU_PATCH_MAX_EXTENT 16
size_t rcu_patch_count(int depth, int height, int width, int pd, int ph, int pw);
int rcu_patch_table(const uint8_t* prediction_dev, const uint8_t* target_dev, const uint8_t* mask_dev /* may be null */, const void* unc_dev,
                    int unc_kind /* RCU_CC_UNC_* */, int depth, int height, int width, int n_volumes, int pd, int ph, int pw,
                    uint64_t* table_dev /* [n_volumes][patches][4] */, void* stream);
int rcu_patch_hist(const uint64_t* table_dev, size_t n_patches, int n_volumes, int levels, int accuracy_per_mille,
                   uint64_t* hist_dev /* [n_volumes][3][levels] */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Input corruptions (EXTENSION: the reference tests on clean, in-distribution volumes only; rcu_amd.corruption, rcu_amd.steps.CorruptInputStep and
 * the `others.corruption` key of the test scripts -- calibration and uncertainty under dataset shift, Ovadia et al. 2019, Mehrtash et al. 2020)
 *   Appearance corruptions of the network input: the labels stay valid, every writer and every evaluation action runs unchanged on the corrupted
 *   run.  x and out are float32 [n][channels][H][W]; image i is the slice with GLOBAL index g = first_sample + i.  The output of a slice is a
 *   function of (x of that slice, kind, amount, key, g) alone, bit for bit the same whatever n, the position in the batch, the launch geometry or
 *   the stream.  Arithmetic is float32 with fmaf in the stated order unless said otherwise; a = (float)amount, p = i * W + j, c the channel.
 *     0 gaussian_noise   y = fmaf(a, z, x), z the normal z(K = key, g, p, s = 0, class = c) of "Test-time logit sampling" above with C = channels
 *                        (element c & 3 of the block c >> 2).  a >= 0, channels <= 8.
 *     1 gaussian_blur    per plane scipy.ndimage.gaussian_filter(x, sigma = amount, mode='reflect', truncate=4.0): radius r = int(4 amount + 0.5),
 *                        taps w_k = exp(-k^2 / (2 amount^2)) / sum, k = -r..r, made on the HOST in float64, rounded to float32 and passed as
 *                        aux_host[k + r] (n_aux = 2 r + 1).  The H axis first, then the W axis on its float32 result; each pass is one chain
 *                        acc = fmaf(w_k, x[i + k], acc) over k = -r..r from acc = 0; an index i out of range is -i - 1, or 2 n - 1 - i at the far
 *                        end.  0 < amount <= 8, r < min(H, W).
 *     2 downsample       k = (int)amount; y[i][j] = the mean of the pixels that exist in block (i / k, j / k): their float32 sum in raster order
 *                        of the block, divided by their count.  2 <= k <= 16.
 *     3 contrast         m = the mean of the (slice, channel) plane in float64 (a fixed partition summed in a fixed order: a function of the
 *                        plane alone), m32 = (float)m, y = fmaf(a, x - m32, m32).  0 <= amount <= 4.
 *     4 intensity_shift  y = x + a.  amount finite.
 *     5 bias_field       y = x * expf(a * f_c(i, j)), f_c = sum over (u, v) in {0, 1, 2}^2 without (0, 0), in raster order, of
 *                        coef[c][3 u + v - 1] * (A_u[i] * B_v[j]): f = fmaf(coef, A_u[i] * B_v[j], f) from f = 0, with A_u[i] = cos(pi u (i + 0.5) / H),
 *                        B_v[j] = cos(pi v (j + 0.5) / W) made on the host in float64 and rounded to float32, and sum_e |coef[c][e]| = 1 (so |f| <= 1).
 *                        aux_host = coef [channels][8], A [3][H], B [3][W] back to back (n_aux = 8 channels + 3 H + 3 W).  One field per channel,
 *                        the same for every slice of a run (a coil profile); rcu_amd.corruption.bias_coefficients derives coef from the key.
 *                        0 <= amount <= 2.
 *     6 ghosting         y[i][j] = fmaf(a, x[(i + H / 2) mod H][j], x[i][j]) with the integer H / 2: the N/2 ghost along the phase-encode axis.
 *                        0 <= amount <= 1.
 *     7 channel_drop     y = 0 on the channels c whose bit (1 << c) is set in the mask passed as amount, y = x on the others (a missing MR sequence:
 *                        z-scored inputs have mean 0).  amount an integer in 1 .. 2^channels - 2, 2 <= channels <= 30.
 *   key and first_sample enter kind 0 only; kinds without aux_host take n_aux = 0.
 *   Severities 1..5 of rcu_amd.corruption (part of the definition; in input units, BraTS inputs being per-channel z-scores):
 *     gaussian_noise    0.1   0.2   0.3   0.5   0.8
 *     gaussian_blur     0.5   1     1.5   2     3
 *     downsample        2     3     4     6     8
 *     contrast          0.8   0.6   0.45  0.3   0.2
 *     intensity_shift   0.1   0.2   0.3   0.5   0.8
 *     bias_field        0.1   0.2   0.3   0.45  0.6
 *     ghosting          0.05  0.1   0.15  0.25  0.4
 *   (channel_drop has no severity: it names its channels.)
 *   Limits: n, channels, H, W >= 1, H * W <= 2^30, channels <= 4096.  Every argument is checked before the device is touched (RCU_ERR_INVALID,
 *   rcu_last_error() names it); a kind is never skipped silently.  x and out must not overlap.  workspace_dev: rcu_corrupt_workspace_bytes bytes
 *   (0 for the kinds that need none: NULL is accepted there); aux_host is read before the call returns.
 * ------------------------------------------------------------------------------------------ */
#define RCU_CORRUPT_GAUSSIAN_NOISE 0
#define RCU_CORRUPT_GAUSSIAN_BLUR 1
#define RCU_CORRUPT_DOWNSAMPLE 2
#define RCU_CORRUPT_CONTRAST 3
#define RCU_CORRUPT_INTENSITY_SHIFT 4
#define RCU_CORRUPT_BIAS_FIELD 5
#define RCU_CORRUPT_GHOSTING 6
#define RCU_CORRUPT_CHANNEL_DROP 7
size_t rcu_corrupt_workspace_bytes(size_t n, int channels, int height, int width, int kind);
int rcu_corrupt(const float* x_dev, size_t n, int channels, int height, int width, int kind, double amount, uint64_t key, uint64_t first_sample,
                const float* aux_host, int n_aux, float* out_dev, void* workspace_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Adaptive MC (EXTENSION: the reference runs T passes over every slice; rcu_amd.steps.McPredictStep(adaptive=...), rcu_amd.steps.AdaptiveMcStatistics
 * and the `others.mc_adaptive` key of the two default test scripts)
 *   Slices on which more passes cannot change the answer are retired at pass checkpoints and finalised from the passes they have seen.  Opt-in and
 *   approximate by design; without the key nothing changes.
 *   Schedule: checkpoints t_1 < t_2 < ... (at most RCU_ADAPTIVE_MAX_CHECKPOINTS, 2 <= t_1, the last below T), a tolerance 0 <= eps < 1 and
 *   max_unsettled >= 0; nb_classes >= 2.  At checkpoint t, with S_c(v) the RCU_MC_EXACT sum of p_c(v) over the t passes a still-active slice has seen
 *   (a multiple of 2^-40 below 2^13: S_c * 2^40 is an integer float64 holds exactly),
 *     voxel v is SETTLED    iff  (int64)(max_c S_c(v) * 2^40) >= thr_q,
 *     thr_q = ceil((1.0 - eps) * t * 2^40), computed by the HOST in exact rational arithmetic on the float64 value of 1.0 - eps
 *             (rcu_amd.steps.adaptive_threshold; tests/adaptive_reference.py) and passed as an int64 -- nothing on the device rounds;
 *     in words: the mean probability of the leading class over the t passes is at least 1 - eps;
 *     a slice is RETIRED at t iff its number of unsettled voxels is <= max_unsettled.  It keeps the statistics of its t passes and is finalised with
 *     count t; the other slices go on to pass t + 1, and after the last checkpoint to T.
 *   The decision is a comparison of integers that are exact sums: it cannot depend on the pass groups, the stream lanes, the batch a slice arrives in
 *   or the geometry of the launch that scores it.  Pass j keeps its mask key whatever span it runs in, and the masks are keyed by the slice's global
 *   index (rcu_dropout_masks), so a slice moved into a smaller batch keeps its samples.
 * ------------------------------------------------------------------------------------------ */
#define RCU_ADAPTIVE_MAX_CHECKPOINTS 4
/* Per slice i of an RCU_MC_EXACT blob (flags without RCU_MC_EXACT are refused: RCU_ERR_INVALID): unsettled_dev[i] = the number of voxels with
 * (int64)(max_c S_c * 2^40) < thr_q, margin_q_dev[i] = the minimum of that integer over the slice.  Reads the nb_classes class-sum planes once
 * (8 * nb_classes bytes per voxel), 16 bytes per lane where hw is even and the blob is 16-byte aligned, one value otherwise -- the same integers
 * either way.  Reduction: in-wave, one LDS step per workgroup, one 32-bit integer add and one 64-bit integer min per workgroup and slice.
 * n <= 2^20, hw <= 2^30, thr_q >= 0. */
int rcu_mc_slice_scores(const void* stats_dev, size_t n, size_t hw, int nb_classes, int flags, int64_t thr_q, uint32_t* unsettled_dev,
                        int64_t* margin_q_dev, void* stream);
/* rcu_dropout_masks with a DEVICE array of n global sample indices in place of first_sample: row i of every pass is drawn at the counter of sample
 * sample_index_dev[i] (>= 0) -- bit for bit the row of that sample in a contiguous draw that covers it.  Same output layout. */
int rcu_dropout_masks_indexed(const uint64_t* seeds_host, int passes, int n, const int64_t* sample_index_dev, const int32_t* site_channels_host,
                              const float* site_keep_host, int n_sites, float* out_dev, void* stream);
/* A compact blob of m slices added into a blob of n slices (same hw, nb_classes, flags): for every plane
 * dst[plane * n*hw + index[i]*hw + pix] += src[plane * m*hw + i*hw + pix].  An entry index[i] < 0 (or >= n) is skipped.  The other entries of a call
 * MUST be distinct: there are no atomics, and the entry point cannot check a device array cheaply.  With RCU_MC_EXACT the additions are exact, so the
 * order of merges is irrelevant.  Moves are 16 bytes where hw and the blobs' alignment allow.  src and dst must not overlap. */
int rcu_mc_merge_slices(const void* src_stats_dev, size_t m, void* dst_stats_dev, size_t n, size_t hw, int nb_classes, int flags,
                        const int32_t* index_dev, void* stream);
/* rcu_mc_finalize with the pass count of slice i read from counts_dev[i] (DEVICE array of n entries, each >= 1; >= 2 for the variance; not checked)
 * in place of T: the same arithmetic per voxel, so with all counts equal to T it writes the bits rcu_mc_finalize writes. */
int rcu_mc_finalize_counts(const void* stats_dev, size_t n, size_t hw, int nb_classes, const int32_t* counts_dev, int flags, float* mean_dev,
                           float* entropy_dev, float* mutual_info_dev, float* variance_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Feature-space density (EXTENSION: the reference has no single-pass epistemic uncertainty; rcu_amd.density, rcu_amd.steps.DensityPredictStep, the
 * fit_density scripts and the `others.density` key of the two default test scripts -- Mukhoti et al. 2021, Deep Deterministic Uncertainty; Lee et
 * al. 2018 for the shared covariance)
 *   Features.  phi(v) in R^F is rcu_unet_features of an eval-mode forward: F real channels at channel_pitch floats per voxel.  1 <= F <=
 *   RCU_DENSITY_MAX_FEATURES, channel_pitch >= F and a multiple of 4.  Channels F .. pitch - 1 are ignored: they may hold any finite value.
 *   Classes.  y(v) in {0 .. K - 1}, K <= 8, one uint8 per voxel.
 *   Moments, per slice s and class c:  n[s][c] = #{v : y(v) = c} (int64),  S[s][c][:] = sum phi (float64 [F]),  G[s][c][:][:] = sum phi phi^T
 *   (float64 [F][F], BOTH triangles filled, bitwise symmetric).  A float32 accumulator covers one chunk of RCU_DENSITY_CHUNK consecutive voxels of
 *   the slice (chunk q = voxels [q m, (q + 1) m) of the slice, m = RCU_DENSITY_CHUNK; G: the fp32 MFMA's k-ordered fmaf chain over the chunk's
 *   voxels; S: the voxels of even and of odd index summed separately); the chunk sums are promoted and added in float64 in chunk order.  The rows of
 *   slice s are bit for bit a function of that slice's features, labels, hw, F and K: not of n, the slice's position in the batch, the alignment of
 *   the pointers, the launch geometry or the stream.  Error: |G_ij - exact| <= (m + 1) 2^-24 sum_v |phi_i phi_j|, |S_i - exact| <= (m + 1) 2^-24
 *   sum_v |phi_i|.
 *   A label >= K is refused: RCU_ERR_INVALID after the kernels have run (such voxels are left out of every sum); the call reads one word back, so it
 *   returns with the stream drained.  Classes beyond four (two above 32 channels) cost one more pass over the features each four (two).
 *   Fit (host, float64; rcu_amd.density.fit_from_moments, tests/density_reference.py).  Per class every entry of n, S and G is summed over all slices
 *   with an exactly rounded sum (math.fsum; integers for n): the fit does not depend on batching or slice order.  mu_c = S_c / n_c,
 *   Sigma_c = G_c / n_c - mu_c mu_c^T + ridge (tr Sigma_c / F) I (ridge 1e-6 by default; shared_covariance: the pooled sum_c n_c Sigma_c / sum n
 *   before the ridge, for every class), L_c = chol(Sigma_c), A_c = L_c^-1 (lower triangular), b_c = A_c mu_c,
 *   k_c = log(n_c / sum n) - sum log diag L_c - (F / 2) log 2 pi.  A class with n_c <= F is refused.
 *   Energy.  e(v) = -log sum_c exp(k_c - d2_c(v) / 2), d2_c(v) = |A_c phi(v) - b_c|^2: the negative log density, float32, from A, b, k rounded once
 *   to float32.  Per class the rows y_i = fma chain over j = 0 .. F - 1 (in the MFMA's order) from -b_i, then d2 = sum y_i^2 in float32, t_c =
 *   fmaf(-0.5, d2, k_c), and a running logsumexp that subtracts the maximum so far.  A voxel's energy is a function of its F feature values and the
 *   parameters alone, whatever n_voxels, its position or the presence of d2_dev.  With s_i = sum_j |A_ij phi_j| + |b_i|:
 *   |d2_c - exact| <= (3 F + 8) 2^-24 sum_i s_i^2.  features_dev must be 16-byte aligned.
 *   Every argument is checked before the device is touched (RCU_ERR_INVALID, rcu_last_error() names it).
 * ------------------------------------------------------------------------------------------ */
#define RCU_DENSITY_MAX_FEATURES 64
#define RCU_DENSITY_CHUNK 1024
size_t rcu_density_moments_workspace_bytes(size_t n, size_t hw, int F, int K);
int rcu_density_moments(const float* features_dev, int channel_pitch, int F, const uint8_t* labels_dev /* [n][hw] */, size_t n, size_t hw, int K,
                        int64_t* n_out_dev /* [n][K] */, double* S_out_dev /* [n][K][F] */, double* G_out_dev /* [n][K][F][F] */, void* workspace_dev,
                        void* stream);
int rcu_density_energy(const float* features_dev, int channel_pitch, int F, size_t n_voxels, int K, const float* A_dev /* [K][F][F] */,
                       const float* b_dev /* [K][F] */, const float* k_dev /* [K] */, float* energy_dev /* [n_voxels] */,
                       float* d2_dev /* [n_voxels][K] or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Last-layer Laplace (EXTENSION: the reference has no post-hoc Bayesian estimate; rcu_amd.laplace, rcu_amd.steps.LaplacePredictStep -- Daxberger et
 * al. 2021, Laplace Redux; MacKay 1992 for the probit predictive; tests/laplace_reference.py restates this section in float64)
 *   Symbols.  F = start_filters, D = F + 1.  C = nb_classes, 2 <= C <= RCU_LAPLACE_MAX_CLASSES.  P = C (C + 1) / 2 pairs q = (c, c'), c <= c', in
 *   row-major order (0,0), (0,1), ..., (1,1), ....  psi(v) in R^F is the output of conv_cls.0 (after BN and ReLU) in an eval-mode forward:
 *   rcu_unet_head_features, F real channels at channel_pitch floats per voxel (channels F .. pitch - 1 are ignored: they may hold any finite value).
 *   z(v) = W psi + w0 are the logits the model writes, p(v) its float32 softmax as the default step writes it.  theta* = (W, w0) / temperature, as
 *   the model applies them, ordered class-major: F weights, then the bias.
 *   Curvature weights (float32, no contraction).  omega_cc = p_c * (1 - p_c): one float32 subtraction, then one float32 multiplication;
 *   omega_cc' = -(p_c * p_c'): one multiplication.  numpy in float32 reproduces every omega bit for bit.
 *   Moments, per slice s and pair q:  w[s][q] = sum_v omega_q,  S[s][q][:] = sum_v omega_q psi,  G[s][q][:][:] = sum_v omega_q psi psi^T (both
 *   triangles, bitwise symmetric), float64 all.  Accumulated as rcu_density_moments accumulates: a wave owns one chunk of RCU_DENSITY_CHUNK = m
 *   consecutive voxels of the slice, by voxel index within the slice, and accumulates in float32 -- G_ij, i <= j, by the fp32 MFMA's k-ordered fmaf
 *   chain of psi_i * fl(omega_q psi_j) over the chunk's voxels (the B operand omega_q psi_j is rounded once; the entry is mirrored to (j, i)); S_i
 *   adds fl(omega_q psi_i) and w adds omega_q, the voxels of even and of odd index summed separately -- the chunk sums are promoted and added in
 *   float64 in chunk order (even before odd), no atomics.  The rows of slice s are bit for bit a function of that slice's psi, p, hw, F and C alone:
 *   not of n, the slice's position in the batch, the alignment of the pointers, the launch geometry or the stream.  Up to four pairs take one pass
 *   over the features (two above 32 channels): C = 2 is one pass up to 32 channels, two above.
 *   Error of the moments against float64 sums of the same float32 omega:  |G_ij - exact| <= (m + 2) 2^-24 sum_v |omega_q psi_i psi_j| (density's
 *   bound plus the one rounding of the B operand), S the same with |omega_q psi_i|, w with |omega_q|.
 *   Fit (host, float64; rcu_amd.laplace.fit_from_moments).  Every entry is summed over the slices with an exactly rounded sum (math.fsum): the
 *   same slices in any batches or order give the same bits.  Per pair M_q = [[G_q, S_q], [S_q^T, w_q]] is D x D; H[(c,i),(c',j)] = M_(c,c')[i][j],
 *   mirrored for c' < c; H_eff = hessian_scale * H (default 1.0, > 0); Sigma = (H_eff + tau I)^-1 by Cholesky.  tau is prior_precision: a float
 *   > 0, default 1.0, or the string `evidence`: the first maximiser over tau_k = 2^(k/4), k = -80 .. 80, of -(tau/2) |theta*|^2 + (C D / 2) log
 *   tau - (1/2) sum_i log(max(lambda_i, 0) + tau) with lambda_i the eigenvalues of H_eff (the log-likelihood at theta* does not depend on tau and
 *   is left out).  Per class c: L = chol(Sigma_cc), lower, Sigma_cc the D x D diagonal block; A_c = (L^T)[:F, :F], b_c = -(L^T)[:F, F], kappa_c =
 *   L[F][F]^2, so that s2_c(v) = psi~^T Sigma_cc psi~ = |A_c psi - b_c|^2 + kappa_c with psi~ = (psi, 1): density's form plus a constant.
 *   Voxels are not independent observations: hessian_scale is the user's knob for that.
 *   Predictive (device, float32, from A, b, kappa rounded once to float32).  s2_c as rcu_density_energy computes d2_c (the fma chain from -b_i in
 *   the MFMA's order, then the squares added in float32), then + kappa_c.  t_c = fmaf((float)(pi / 8), s2_c, 1.0f), zt_c = z_c / sqrt(t_c) (both
 *   correctly rounded), p~ = the project's softmax of zt, std_c = sqrt(s2_c): the mean-field probit link of the `laplace` package, the diagonal of
 *   the logit covariance.  prediction is the first maximum of p~, std_pred the std of that class.  A voxel's outputs are a function of its F
 *   feature values, its C logits and the parameters alone, whatever n, hw, its position or the presence of the optional outputs.  Error of s2_c
 *   against float64 on the same float32 parameters: (3 F + 8) 2^-24 sum_i s_i^2 with s_i = sum_j |A_ij psi_j| + |b_i|, plus 2^-23 kappa_c.
 *   Every argument is checked before the device is touched (RCU_ERR_INVALID, rcu_last_error() names it): F in 1..64, channel_pitch >= F and a
 *   multiple of 4, C in 2..4, features_dev (and the moments' workspace_dev) 16-byte aligned, n in 1..2^20, hw in 1..2^30.
 * ------------------------------------------------------------------------------------------ */
#define RCU_LAPLACE_MAX_CLASSES 4
size_t rcu_laplace_moments_workspace_bytes(size_t n, size_t hw, int F, int nb_classes);
int rcu_laplace_moments(const float* features_dev, int channel_pitch, int F, const float* probabilities_dev /* NCHW [n][C][hw] */, size_t n,
                        size_t hw, int nb_classes, double* w_out_dev /* [n][P] */, double* S_out_dev /* [n][P][F] */,
                        double* G_out_dev /* [n][P][F][F] */, void* workspace_dev, void* stream);
int rcu_laplace_predict(const float* features_dev, int channel_pitch, int F, const float* logits_dev /* NCHW [n][C][hw] */, size_t n, size_t hw,
                        int nb_classes, const float* A_dev /* [C][F][F] */, const float* b_dev /* [C][F] */, const float* kappa_dev /* [C] */,
                        float* probabilities_dev /* [n][C][hw] */, float* std_dev /* [n][C][hw] or NULL */, float* std_pred_dev /* [n][hw] or NULL */,
                        uint8_t* prediction_dev /* [n][hw] or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Quantile rescale (EXTENSION: the reference brings an unbounded uncertainty map -- the aleatoric sigma, the density energy -- into [0, 1] with the
 * run's global min / max, so one outlier voxel fixes the scale; this is the rank transform of the run instead.  rcu_amd.evaluation.quantile_table /
 * quantile_rescale / RescaleQuantile, the `quantiles` action and `--rescale quantile` of the evaluation script; tests/quantile_reference.py)
 *   Key.  key(u) is the order-preserving uint32 of the float32 value u: -0.0 is taken as +0.0 first; with b the bit pattern, key = ~b if the sign bit
 *   is set, else b | 0x80000000.  key is non-decreasing in u over all of float32, the infinities included.  A map stored in another dtype is cast to
 *   float32 first (round to nearest: monotone, so the result is still a rank transform).  NaN has no key: NaNs are counted, and a run with any NaN
 *   is refused by the host (ValueError naming the subject).
 *   Population.  The voxels inside the T2 brain mask where the dataset evaluates inside one (ece_details == 'foreground': BraTS), every voxel
 *   otherwise (ISIC) -- the rule `calib` follows.  N = the population size over all subjects of the run (a BraTS volume is about 85 % constant
 *   background: over all voxels about 850 of 1000 boundaries would coincide on that one value).
 *   Table.  Q boundaries, 2 <= Q <= RCU_UNC_HIST_MAX_LEVELS.  For k = 1 .. Q-1: the rank r_k = ceil(k N / Q) in integers, b_k = the key of the
 *   r_k-th smallest population value (1-based).  Coinciding boundaries (ties) are kept as they are.  This is
 *   numpy.quantile(x, k / Q, method='inverted_cdf').
 *   Level.  l(u) = #{k in 1..Q-1 : key(u) > b_k}, in 0 .. Q-1, for every voxel, inside the population or not.  For distinct values level l holds
 *   exactly r_{l+1} - r_l population voxels (r_0 = 0, r_Q = N).
 *   Rescaled value.  (l + 0.5) / Q in float64, stored as float32: it lies in (0, 1), and under level(u) = #{k in 1..B-1 : u > k / B} (rcu_unc_hist)
 *   with B = Q it gives back l for every l -- the float32 rounding error stays below 2^-24, against 0.5 / Q to the nearest threshold.
 *   Selection.  Exact, by radix passes over the keys from the top: a pass counts, for every selected prefix, the population voxels per next digit
 *   (rcu_key_hist); the host finds each boundary's digit and its rank inside that digit from the integer table (evaluation.quantile_refine) and
 *   selects the distinct prefixes of the next pass.  The digit widths of the passes (the plan) add up to 32.
 * ------------------------------------------------------------------------------------------ */
#define RCU_KEY_HIST_MAX_PREFIXES 4095
/* One radix pass over n_volumes float32 volumes of n_per_volume voxels (volume v at maps_dev + v * n_per_volume; mask_dev: uint8 in the same layout,
 * not 0 = in the population, or NULL = every voxel).  For every population voxel that is not NaN: hi = key >> (shift + bits) (0 where shift + bits =
 * 32), slot = the index of hi in prefixes_host -- n_prefixes strictly increasing values below 2^(32 - shift - bits), a HOST array; n_prefixes == 0:
 * every voxel is slot 0 -- voxels whose hi is not listed are skipped; digit = (key >> shift) & (2^bits - 1); hist_dev[slot][digit] += 1.
 * hist_dev: int64 [max(n_prefixes, 1)][2^bits], ADDED to (the caller zeroes it once: one resident table collects a whole run).  counts_dev: uint64
 * [2], added to as well: [0] += the NaNs among the population voxels, [1] += the population voxels (NaNs included).  All integers: the same bits
 * whatever the launch geometry, the batching, the alignment of the pointers or the order of the volumes.  workspace_dev: at least
 * rcu_key_hist_workspace_bytes(n_prefixes) bytes (the prefix table on the device).  1 <= bits <= 16, shift >= 0, shift + bits <= 32, n_per_volume in
 * 1..2^31-2, n_volumes in 1..65535; every argument is checked before the device is touched (RCU_ERR_INVALID, rcu_last_error() names it). */
size_t rcu_key_hist_workspace_bytes(int n_prefixes);
/* Testing aid: blocks of 16,384 (32,768 in the packed LDS form) voxels one workgroup of rcu_key_hist takes (1..8; larger values count as 8; 0 = the
 * launcher's own rule).  The counts do not depend on it. */
int rcu_key_hist_set_blocks_per_workgroup(int blocks);
int rcu_key_hist(const float* maps_dev, const uint8_t* mask_dev, size_t n_per_volume, int n_volumes, const uint32_t* prefixes_host, int n_prefixes,
                 int shift, int bits, int64_t* hist_dev, uint64_t* counts_dev, void* workspace_dev, void* stream);
/* The rank transform of n float32 values under the quantiles - 1 non-decreasing boundary keys bounds_host (HOST array): out_dev[i] =
 * (float)((l + 0.5) / quantiles) with l = l(map_dev[i]) as above, and levels_dev[i] = l (uint16, or NULL).  NaN -> level 0.  A voxel's output is a
 * function of its value and the table alone.  workspace_dev: at least rcu_quantile_apply_workspace_bytes(quantiles) bytes.  out_dev must not overlap map_dev. */
size_t rcu_quantile_apply_workspace_bytes(int quantiles);
int rcu_quantile_apply(const float* map_dev, size_t n, const uint32_t* bounds_host, int quantiles, float* out_dev, uint16_t* levels_dev,
                       void* workspace_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RCU_H */
