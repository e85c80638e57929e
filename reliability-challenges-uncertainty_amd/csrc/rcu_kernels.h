// Internal declarations shared by the HIP translation units of librcu_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/rcu.h"

namespace rcu {

// rcu_last_error() of the calling thread := msg; returns code (defined in rcu_api.hip; every translation unit's entry points report through it)
int report_error(int code, const std::string& msg);

// host helpers of the entry points that live next to their kernels
inline int hip_failed(const char* fn, hipError_t e) { return report_error(RCU_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e)); }
inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int check_n_volumes(const std::string& f, int n_volumes, int max_volumes)
{
    if (n_volumes >= 1 && n_volumes <= max_volumes) return RCU_OK;
    return report_error(RCU_ERR_INVALID, f + "n_volumes must be in 1.." + std::to_string(max_volumes) + ", got " + std::to_string(n_volumes));
}
// a batch of label / distance maps: n_per_volume < 2^31 - 1, n_volumes in 1..max_volumes, the batch below 2^32 voxels (ranks and offsets are u32)
inline bool batch_n_ok(size_t n) { return n != 0 && n < (size_t)0x7fffffff; }
inline bool batch_total_ok(size_t n, int n_volumes) { return (unsigned long long)n * (unsigned long long)n_volumes <= 0xffffffffull; }
inline bool batch_ok(size_t n, int n_volumes, int max_volumes)
{
    return batch_n_ok(n) && n_volumes >= 1 && n_volumes <= max_volumes && batch_total_ok(n, n_volumes);
}
inline int check_batch(const std::string& f, size_t n, int n_volumes, int max_volumes)
{
    if (!batch_n_ok(n)) return report_error(RCU_ERR_INVALID, f + "n_per_volume must be in 1..2^31-2, got " + std::to_string(n));
    if (int st = check_n_volumes(f, n_volumes, max_volumes)) return st;
    if (!batch_total_ok(n, n_volumes)) return report_error(RCU_ERR_INVALID, f + "n_per_volume * n_volumes must be below 2^32");
    return RCU_OK;
}

// ---------------------------------------------------------------------------------------------
// conv3x3 implicit GEMM (rcu_conv.hip)
// ---------------------------------------------------------------------------------------------
// Activations are fp32 with the channel count padded to a multiple of 32 (the network input to a multiple of 8); padded
// channels hold zeros.  One launch covers every slice of the batch.  Two layouts of a [N][H][W][C] tensor:
//   NHWC     a pixel's C channels are contiguous                                   (every kernel)
//   blocked  [N][C/8][H][W][8]: a pixel's 8-channel group (the Cin chunk of the Winograd kernels) is 32 contiguous bytes and
//            the groups of neighbouring pixels follow each other, so an LDS-DMA instruction that stages 8 channels of 32..64
//            pixels touches 8..16 whole 128-byte lines instead of 32..64 quarter lines (Winograd kernels + rcu_first.hip only)
//   paired   [N][C/8][H][W/2][4 channel pairs][2 pixels][2 channels]: the blocked layout with the 64 bytes of each aligned pixel pair permuted, so
//            that a lane of the F(4x4,3x3) epilogues -- two couts of adjacent pixels -- stores 16 contiguous bytes without trading with its
//            neighbour (rcu_wino4_geom.h; rcu_wino4.hip, rcu_wino4_up.hip, rcu_first.hip only; even W, unpadded levels)
// NHWC and blocked are addressed as  sample * (H W C 4) + chunk * chunk_bytes + (y W + x) * pix_bytes + (c mod 8) * 4  with
//   NHWC: pix_bytes = 4 C, chunk_bytes = 32;   blocked: pix_bytes = 32, chunk_bytes = 32 H W.
// A paired tensor has the strides of the blocked one and in_paired / out_paired set: inside a chunk plane
//   ((y W + x) >> 1) * 64 + ((c mod 8) >> 1) * 16 + (x & 1) * 8 + (c & 1) * 4.
struct ConvArgs {
    const float* src1;   // [N][H][W][C1]   first  K-range (channels [0, C1))
    const float* src2;   // [N][H][W][C2]   second K-range (cat-free decoder), may be null (C2 = 0)
    const float* wpack;  // [Cin/KC][NTW_total] tiles of [TAPS][BN][KC+4] floats, each padded to 1024-float multiples
    const float* alpha;  // [CoutP]  folded BN scale               (1 for bias-only convs)
    const float* betab;  // [CoutP]  alpha * conv bias
    const float* beta;   // [CoutP]  folded BN shift               (0 for bias-only convs)
    const float* mask;   // [N][Cmask] dropout factors {0, 1/(1-p)} of this site, or null (eval / no site)
    const float* mask2;  // second site for output channels >= Csplit (fused cls+sigma head unit), or null
    float* out;          // [N][H][W][CoutP]; sub-pixel up-conv kernels: [N][2H][2W][CoutP]
    float* pooled;       // [N][H/2][W/2][CoutP] or null
    int out_H, out_W;    // sub-pixel up-conv (direct kernels): extent of the output tensor when it is larger than 2H x 2W -- the
    int out_y0, out_x0;  //   reference's centre pad (common/model/unet.py:110-116) -- and where the 2H x 2W image sits in it; 0: 2H x 2W
    int N, H, W;         // input grid = pixel-tile grid
    // Padded levels (`part` = 1; Winograd kernels + rcu_first.hip; rcu_plan.hip, plan_unet): the tensors of a level are allocated with
    // extents rounded up to whole tiles, H x W above are those ALLOCATED extents of the source level, and the pixels beyond the real image hold
    // zeros that no kernel ever writes -- so a tile that hangs over the real border reads exactly the zero padding the reference's conv applies
    // (common/model/unet.py:13: padding=1) and the load side of the kernels is the whole-tile one.  What changes is the store side:
    int part;            //   1: the fields below are set and the kernel's store side honours them
    int Hr, Wr;          //   real extent of the OUTPUT grid (up-convolutions: of the up-sampled grid): pixels at or beyond it are not stored
    int pool_H, pool_W;  //   allocated extent of `pooled` (out_H, out_W above: of `out`) -- a level's padding is its own, not half its parent's
    int C1, C2;          // padded channel counts of the two sources
    int cin_real;        // first-layer kernel (rcu_first.hip): input channels that are not padding
    const float* x_nchw; // first-layer kernel: when set, the caller's [n_images][cin_real][H][W] input is read in place of src1
    int n_images;        //   (sample n is image n % n_images: pass groups replicate the images)
    int CoutP;           // padded output channels (multiple of 32)
    int Cmask;           // real channel count of the dropout site (mask row length)
    int Csplit, Cmask2;  // mask2 row = [N][Cmask2], applies to channel co - Csplit
    int relu;            // 1: max(0, .) epilogue
    int accumulate;      // direct kernels: 1 = the unit's result is ADDED to what `out` holds (ConvResidualBlock: the 1x1 residual
                         // conv has been written there), before the 2x2 max-pool
    int tiles_y, tiles_x, slice_groups;
    int NT;              // output-channel tiles
    uint32_t magic_ntw, magic_tx, magic_ty;   // ceil(2^32 / d) for d = NTW_total, tiles_x, tiles_y (0: divide): the Winograd kernels
                                              // split a work item into tile coordinates with s_mul_hi instead of three divisions
    int NTW_total;       // weight tiles per Cin chunk = NT (3x3) or 4 * NT (sub-pixel: one set per parity class)
    uint32_t src1_bytes, src2_bytes, wpack_bytes;   // buffer-resource ranges (Winograd kernels)
    // layout of the sources (both alike), of `out` and of `pooled` (see above); 0 / 0 = NHWC for the kernels that know nothing else
    uint32_t in_pix_bytes, in_chunk_bytes;
    uint32_t out_pix_bytes, out_chunk_bytes;
    uint32_t pool_pix_bytes, pool_chunk_bytes;
    // fused 1x1 head of conv_cls.0 (rcu_wino.hip, rcu_wino4.hip; two classes): when head_w is set the conv unit's output stays on chip
    const float* head_w;   // [2][32] 1x1 weights, head_b[2] bias
    const float* head_b;
    float* head_logits;    // NCHW [N][2][H*W] or null
    void* head_stats;      // MC statistics blob or null
    int head_flags;        // MC_MI | MC_VAR
    size_t head_V;         // voxels of one pass = images * H * W
    int head_passes;       // MC passes in this launch: sample t * head_images + i is image i (pass groups); its statistics entry is i's
    int head_images;
    int in_paired;         // the sources (both alike) are paired tensors
    int out_paired;        // `out` and `pooled` (both alike) are paired tensors
};

enum ConvConfig {
    CONV_CFG_T8x16_N64 = 0,          // 8x16-pixel tile, 64 couts, Cin chunks of 8, LDS double-buffered (workhorse)
    CONV_CFG_T8x16_N32 = 1,          // 8x16-pixel tile, 32 couts, Cin chunks of 8, double-buffered (32-channel layers)
    CONV_CFG_T8x16_N32_FIRST = 2,    // first layer: Cin padded to 8 = a single chunk
    CONV_CFG_S2T12x8_N64 = 3,        // two whole 12x8 slices per workgroup (BraTS bottom level)
    CONV_CFG_UP_T8x16_N64 = 4,       // sub-pixel up-conv (2x2 taps on the low-res grid), 64 couts
    CONV_CFG_UP_T8x16_N32 = 5,       // sub-pixel up-conv, 32 couts
    CONV_CFG_UP_S2T12x8_N64 = 6,     // sub-pixel up-conv out of the 12x8 bottom level, chunks of 8
    CONV_CFG_T16x16_N32 = 7,         // 16x16-pixel tile, 32 couts: halves the weight staging per MFMA of the 32-channel layers
    CONV_CFG_UP_T16x16_N32 = 8,      // sub-pixel up-conv, 32 couts, 16x16 low-res tile
    CONV_CFG_T16x16_N64 = 9,         // 256 pixels x 64 couts: half the staging / barriers / fragment reads per MFMA
    CONV_CFG_S2T8x16_N64 = 10,       // the same tile as two 8x16 pieces of consecutive slices (heights not divisible by 16)
    CONV_CFG_COUNT,
    // Winograd F(2x2,3x3) kernels (rcu_wino.hip): 16 positions instead of 9 taps, weights host-transformed
    CONV_CFG_WINO_T16x16_N64 = CONV_CFG_COUNT,   // 16x16-pixel tile (64 Winograd tiles) x 64 couts
    CONV_CFG_WINO_T16x32_N32,                    // 16x32-pixel tile x 32 couts (32-channel layers)
    CONV_CFG_WINO_S2T8x16_N64,                   // two 8x16 pieces of consecutive slices x 64 couts
    CONV_CFG_WINO_S8T4x8_N64,                    // 4x8 strips of eight consecutive slices x 64 couts (8-pixel-wide level)
    CONV_CFG_WINO_T16x32_N32_HEAD,               // T16x32_N32 with the 1x1 head + softmax + statistics in the epilogue
    // Winograd F(2x2,2x2) sub-pixel up-convolutions (rcu_wino_up.hip): 18 positions = two parity classes per work item
    CONV_CFG_UPW_T16x16_N64,
    CONV_CFG_UPW_T16x32_N32,
    CONV_CFG_UPW_S2T8x16_N64,
    CONV_CFG_UPW_S8T4x8_N64,
    // first conv unit of the network, K = 9 taps x 4 (8) channels unpadded (rcu_first.hip)
    CONV_CFG_FIRST_T8x32,
    // Winograd F(4x4,3x3) kernels (rcu_wino4.hip): 36 positions, one wave per SIMD (288 accumulator registers), 32 couts
    CONV_CFG_WINO4_T32x32_N32,                   // 32x32-pixel tile (64 Winograd tiles of 4x4)
    CONV_CFG_WINO4_S2T16x32_N32,                 // 16x32 pixels of two consecutive slices
    CONV_CFG_WINO4_S8T8x16_N32,                  // 8x16 pixels of eight consecutive slices, images 16 pixels wide
    CONV_CFG_WINO4_S8T12x8_N32,                  // 12x8 pixels of TEN consecutive slices (their 60 tiles in the 64 tile slots of a workgroup; S8 names the block geometry the tile descends from), images 8 wide
    CONV_CFG_WINO4_T32x32_N32_HEAD,              // T32x32_N32 with the 1x1 head + softmax + statistics in the epilogue (run-time choice of forward_impl, never a plan entry)
    CONV_CFG_WINO4_S4T8x32_N32,                  // 8x32 pixels of four consecutive slices, images 32 pixels wide (round 6: ISIC's 24x32 level without padding)
    // Winograd F(4x4,3x3) up-convolutions on the up-sampled grid without the vanishing point (rcu_wino4_up.hip): 25 positions, one wave per SIMD
    // (200 accumulator registers), 32 couts; the names give the OUTPUT tile.  Unpadded levels only (no ConvArgs::part)
    CONV_CFG_UPW4_T32x32_N32,                    // 32x32 output pixels of one slice
    CONV_CFG_UPW4_S2T16x32_N32,                  // 16x32 output pixels of two consecutive slices
    CONV_CFG_UPW4_S8T8x16_N32,                   // 8x16 output pixels of eight consecutive slices, output images 16 pixels wide
    CONV_CFG_END
};

enum class ConvFamily {
    Direct,      // 3x3 taps as they are (rcu_conv.hip)
    DirectUp,    // sub-pixel up-convolution: 2x2 taps on the low-resolution grid per output parity class (rcu_conv.hip)
    First,       // the network's first conv unit (rcu_first.hip); weights packed like Direct
    Wino2,       // F(2x2,3x3), TAPS = 16 positions (rcu_wino.hip)
    Wino2Up,     // F(2x2,2x2) up-convolution, TAPS = 18 = two parity classes of 9 (rcu_wino_up.hip)
    Wino4,       // F(4x4,3x3), TAPS = 36 positions (rcu_wino4.hip)
    Wino4Up,     // F(4x4,3x3) up-convolution without the vanishing point, TAPS = 25 positions (rcu_wino4_up.hip)
};
// What the host has to know about a kernel family; each family's file defines its record next to its ConvConfigInfo table.  Up-convolutions:
// TH x TW of a row is the low-resolution tile, the grid the tiles walk.
struct ConvFamilyTraits {
    ConvFamily id;
    bool winograd;        // packed weight tile = [position][channel pair][cout][2], the LDS image; else [tap][cout][KCP] (rcu_wpack.h)
    bool reads_blocked;   // takes its sources in the channel-blocked layout as well as in NHWC (ConvArgs)
    bool writes_blocked;  // ... its output and pooled output
    bool part;            // store side honours ConvArgs::part: may read or write the tensors of a padded level
    int weight_sets;      // weight-tile sets per (Cin chunk, cout tile): 1, 2 or 4 (one per parity class or pair of classes)
    double mults;         // multiplications executed per pixel of the walked grid and (cin, cout) pair
    bool reads_paired = false;    // takes its sources in the paired layout too (whole tiles of unpadded levels)
    bool writes_paired = false;   // ... its output and pooled output
};
struct ConvConfigInfo {
    int TS, TH, TW, BN, KC, TAPS;
    const char* kernel_name;
    int KCP;   // floats per [tap][channel] row of a packed weight tile (KC, or KC + 4 in the padded layout)
    int SWZ;   // 1: the two 16-byte units of a row are swapped for output channels 16..31 (mod 32), see ConvTile
    ConvFamilyTraits family;
    double slot_factor = 1.0;   // tile slots executed per tile held: 64 / 60 for the folded 12x8 tile of rcu_wino4.hip
    int head_cfg = -1;          // the ConvConfig of this kernel with the 1x1 head fused into its epilogue, or -1
};
// the only function that knows the order of the ConvConfig values
const ConvConfigInfo& conv_config_info(int cfg);
const ConvConfigInfo& wino_config_info(int cfg);
const ConvConfigInfo& wino_up_config_info(int cfg);
const ConvConfigInfo& wino4_config_info(int cfg);
const ConvConfigInfo& wino4_up_config_info(int cfg);
const ConvConfigInfo& first_config_info();
hipError_t launch_conv3x3(int cfg, const ConvArgs& a, hipStream_t stream);
hipError_t launch_conv_wino(int cfg, const ConvArgs& a, hipStream_t stream);
hipError_t launch_upconv_wino(int cfg, const ConvArgs& a, hipStream_t stream);
hipError_t launch_conv_wino4(int cfg, const ConvArgs& a, hipStream_t stream);
hipError_t launch_upconv_wino4(int cfg, const ConvArgs& a, hipStream_t stream);
hipError_t launch_conv_first(const ConvArgs& a, hipStream_t stream);

// Loads of data a kernel reads exactly once (activation / logits / probability / label streams of the per-voxel kernels): non-temporal, so that the
// stream does not push the lines that ARE reused -- statistics planes that are read-modify-written, weights -- out of L2 and the memory-side cache.
// Measured round 4 (profiles/r04_nt_loads.txt): head kernel 116 -> 98 us (0.61 -> 0.72 of the HBM peak), ece_hist / unc_counts 0.72 / 0.74 -> 0.79 /
// 0.82.  NOT for the conv kernels' input staging (their input was written by the previous kernel and neighbouring tiles re-read its halo: +4..5 %
// time with nt there) and NOT for mc_accumulate / mc_finalize (their logits and statistics were written by the kernel before them and one volume's
// worth sits in the 256 MB memory-side cache: finalize 13.3 -> 15.3 us with nt).
#if defined(__HIPCC__)
template <class V>
__device__ __forceinline__ V stream_load_as(const void* p)
{
    return __builtin_nontemporal_load(reinterpret_cast<const V*>(p));
}
__device__ __forceinline__ float stream_load(const float* p) { return stream_load_as<float>(p); }
__device__ __forceinline__ unsigned stream_load(const unsigned* p) { return stream_load_as<unsigned>(p); }
__device__ __forceinline__ float4 stream_load(const float4* p)
{
    typedef float v4 __attribute__((ext_vector_type(4)));
    const v4 v = stream_load_as<v4>(p);
    return float4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ double2 stream_load(const double2* p)
{
    typedef double v2 __attribute__((ext_vector_type(2)));
    const v2 v = stream_load_as<v2>(p);
    return double2{v.x, v.y};
}
// four consecutive values of a 16-byte-aligned float32 / float64 stream
__device__ __forceinline__ void load4(const float* src, float (&q)[4])
{
    const float4 v = stream_load(reinterpret_cast<const float4*>(src));
    q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
}
__device__ __forceinline__ void load4(const double* src, double (&q)[4])
{
    const double2 a = stream_load(reinterpret_cast<const double2*>(src)), b = stream_load(reinterpret_cast<const double2*>(src + 2));
    q[0] = a.x, q[1] = a.y, q[2] = b.x, q[3] = b.y;
}
#endif

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device attribute of a kernel: set once per (kernel, device), so that one
// process driving several GPUs gets it on every one of them.
hipError_t set_max_dynamic_lds(const void* kernel, int bytes);

// ---------------------------------------------------------------------------------------------
// layout / head / aggregation kernels (rcu_pointwise.hip)
// ---------------------------------------------------------------------------------------------
// out_nhwc is allocated PH x PW >= H x W per image (a padded level 0): only the H x W real pixels are written
hipError_t launch_pack_input(const float* x_nchw, float* out_nhwc, int N, int C, int CP, int H, int W, int PH, int PW, int replicas,
                             hipStream_t stream);

// the H x W real pixels of an NHWC tensor allocated PH x PW per image -> a compact [N][H][W][CP] tensor (rcu_unet_features on a padded level 0)
hipError_t launch_crop_nhwc(const float* src, float* dst, int N, int H, int W, int PH, int PW, int CP, hipStream_t stream);

// MC statistics blob: planes over the voxel index v = n*HW + hw.
//   neither RCU_MC_VAR nor RCU_MC_EXACT : float planes  [sum_p[0..C-1]] [sum_H if MI]
//   RCU_MC_VAR and / or RCU_MC_EXACT    : double planes [sum_p[0..C-1]] [sum_p^2[0..C-1] if VAR] [sum_H if MI]
//   RCU_MC_EXACT: the addends are rounded to multiples of 2^-40 first, which makes every addition exact (rcu_head_common.h)
constexpr int MC_MI = 1;
constexpr int MC_VAR = 2;
constexpr int MC_INPUT_PROBS = 4;   // accumulate: input already holds probabilities (ensemble seam)
constexpr int MC_EXACT = 8;
constexpr int MAX_CLASSES = 8;
inline int check_classes(int c)
{
    if (c < 1 || c > MAX_CLASSES) return report_error(RCU_ERR_INVALID, "nb_classes must be in 1..8");
    return RCU_OK;
}

struct HeadArgs {
    const float* act;     // [V][CP] NHWC activations of the (fused) head conv unit
    const float* w_cls;   // [C][CPh]  1x1 weights (zero padded), bias b_cls[C]
    const float* b_cls;
    const float* w_sig;   // optional twin (reads channels [CPh, 2*CPh) of act)
    const float* b_sig;
    float* logits;        // NCHW [N][C][HW] or null
    float* sigma;         // NCHW or null
    float* sigma_sum;     // NCHW or null: += |sigma| (or exp(sigma), sigma_log) of this pass (aleatoric + MC extension)
    int sigma_log;
    void* stats;          // MC stats blob or null
    int C, CP, CPh, stats_flags;
    size_t V, HW;         // V = voxels of ONE pass (n * HW)
    int passes;           // > 1 (statistics only): act holds `passes` consecutive groups of V voxels, all accumulated
                          // into the same V statistics entries, in pass order
};
hipError_t launch_head(const HeadArgs& a, hipStream_t stream);
// test-time logit sampling of a sigma head (rcu_head_common.h, logit_sample_predictive): the head kernels with softmax(mu) replaced by the sampled
// predictive of (mu, sigma) under keys[t] for pass t.  launch_head_sampled runs a pass group of more than SAMPLE_MAX_PASSES passes as one launch per
// SAMPLE_MAX_PASSES passes, in pass order (keys_host: a.passes keys, or one for a single pass); a.stats is required.
constexpr int LOGIT_MAX_SAMPLES = 1024;
constexpr int SAMPLE_MAX_PASSES = 32;
struct SampleArgs {
    unsigned long long keys[SAMPLE_MAX_PASSES];   // key of pass t of the launch
    unsigned long long first_sample;              // global index of the batch's image 0
    int samples;                                  // S, 1..LOGIT_MAX_SAMPLES
};
hipError_t launch_head_sampled(const HeadArgs& a, const unsigned long long* keys_host, unsigned long long first_sample, int samples,
                               hipStream_t stream);
// sample votes (include/rcu.h "Sample agreement"): the head kernels' VOTES variant also ORs, for every pass of the launch, the bit "this pass's
// arg-max at the voxel is not class 0" into the voxel's word of a vote plane.  All passes of one launch vote into ONE word;
// launch_head_votes splits a pass group at word boundaries (and at SAMPLE_MAX_PASSES passes), in pass order.  bits_host: a.passes bit
// indices in [0, 32 * n_words).  a.stats is required, logits / sigma outputs and the sigma sum are not part of this form.
constexpr int VOTES_MAX_PASSES = RCU_VOTES_MAX_PASSES;
struct VoteArgs {
    uint32_t* plane;                              // [n_words][V]
    int n_words;
    int word;                                     // the word the passes of this launch vote into
    unsigned char bit[SAMPLE_MAX_PASSES];         // bit of pass t of the launch inside that word
};
hipError_t launch_head_votes(const HeadArgs& a, uint32_t* votes, int n_words, const int32_t* bits_host, hipStream_t stream);
// RCU_ERR_INVALID (with its message) unless 1 <= nb_classes <= 8, 1 <= samples <= LOGIT_MAX_SAMPLES, n, hw >= 1 and hw < 2^32
int check_logit_sampling_shape(const char* fn, size_t n, size_t hw, int nb_classes, int samples);   // (rcu_logit_sampling.hip)
// a vote plane of n_words words / a bit index inside it, or RCU_ERR_INVALID with its message (rcu_pointwise.hip)
int check_vote_plane(const std::string& fn, int n_words);
int check_vote_bit(const std::string& fn, int bit, int n_words);

// Dropout2d factors of the passes of a pass group, drawn in one launch (include/rcu.h: rcu_dropout_masks)
constexpr int MASK_MAX_PASSES = 32;      // seeds per launch (kernel arguments)
constexpr int MASK_MAX_SITES = 40;       // 2 * (2 * 8 + 1) + the head units: depth <= 8
struct MaskArgs {
    unsigned long long seed[MASK_MAX_PASSES];
    int site_end[MASK_MAX_SITES];        // exclusive prefix sums of n * C_site: site s covers [site_end[s - 1], site_end[s]) of a pass's own mask
    float site_keep[MASK_MAX_SITES];     // 1 - p of the site; < 0: the site is not active (factor 1); 0: p = 1 (factor 0)
    int passes;                          // passes of the whole group: rows per site of the output layout
    int first, count;                    // this launch draws passes first .. first + count - 1 (seed[0 .. count - 1])
    int sites, per_pass;
    int site_ch[MASK_MAX_SITES];         // channels of the site
    int site_off[MASK_MAX_SITES];        // offset of the site in ONE sample's factors (prefix sums of site_ch); per_sample = their total
    int per_sample;
    unsigned long long first_sample;     // global index of the batch's sample 0 (include/rcu.h, rcu_dropout_masks)
};

// ---------------------------------------------------------------------------------------------
// adaptive MC (rcu_adaptive.hip; include/rcu.h "Adaptive MC")
// ---------------------------------------------------------------------------------------------
// launch_dropout_masks with row i drawn at the global sample sample_index[i] (device array of a.site_end[0] / a.site_ch[0] entries); a.first_sample unused
hipError_t launch_dropout_masks_indexed(const MaskArgs& a, const long long* sample_index, float* out, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// calibration kernels (rcu_calib.hip)
// ---------------------------------------------------------------------------------------------
constexpr int MAX_BINS = 32;
constexpr int MAX_THR = 16;
struct EceResult {           // one per volume
    unsigned long long count[MAX_BINS];
    double sum_conf[MAX_BINS];
    unsigned long long sum_pos[MAX_BINS];
};

// ---------------------------------------------------------------------------------------------
// temperature scaling: NLL sweep over candidate inverse temperatures (rcu_temperature.hip; entry points rcu_temperature_nll*)
// ---------------------------------------------------------------------------------------------
constexpr int TN_MAX_CANDIDATES = 128;
// bytes of the per-workgroup partials of one rcu_temperature_nll call over `voxels` voxels
size_t temperature_nll_workspace_bytes(size_t voxels, int n_candidates);

// ---------------------------------------------------------------------------------------------
// PostNet: fused 1x1-conv stack on the U-Net feature map (rcu_postnet.hip)
// ---------------------------------------------------------------------------------------------
// packed layer of CB x CB blocks of 32 channels: weight tiles + accumulator start values + constants behind the dropout factor
constexpr int pn_layer_floats(int cb) { return cb * cb * 1024 + 2 * cb * 32; }
constexpr int PN_MAX_LAYERS = 12;
constexpr int PN_MAX_BLOCKS = 3;   // up to 96 feature channels (the packed layers live in LDS: n_layers * pn_layer_floats <= 160 KB)

}  // namespace rcu
