// Affine test-time augmentation (include/rcu_warp.h): the bilinear warp of an NCHW float32 batch under a list of 2 x 3 matrices
// (rcu_warp_affine) and the accumulate that reads every sample through a warp on its way into the MC statistics (rcu_mc_accumulate_warped).
// Both are gathers of four taps per output pixel, memory-bound.  One lane owns one output pixel of a plane: its taps and weights are six
// float64 operations per axis (under `fp contract(off)`: nothing is fused, the bits are those of the host's float64) and are
// reused over every plane the lane walks.  A wave covers WARP_BX x (64 / WARP_BX) pixels: under a rotation the taps of a 16 x 4 footprint stay
// within a few cache lines, where those of 64 pixels of one row spread over as many source rows as the row climbs.
// Nothing here can read outside a plane: the source position is clamped before the taps are formed, whatever the matrix holds.
#include "../../include/rcu_warp.h"
#include "rcu_head_common.h"
#include "rcu_kernels.h"

#include <string>

namespace rcu {
namespace {

#ifndef RCU_WARP_BX
#define RCU_WARP_BX 16      // pixels of a workgroup along W (experiment builds override the footprint; 64 x 4 is the row form)
#endif
#ifndef RCU_WARP_BY
#define RCU_WARP_BY 16
#endif
constexpr int WARP_BX = RCU_WARP_BX, WARP_BY = RCU_WARP_BY;
constexpr int WARP_THREADS = WARP_BX * WARP_BY;
static_assert(WARP_THREADS == 256, "a workgroup of the warp kernels is four waves");
constexpr unsigned WARP_MAX_PLANE_BLOCKS = 1024;      // grid extent over planes / slices; more are walked by a grid stride

struct Taps {
    int o00, o01, o10, o11;      // offsets of the four taps within the plane (a plane holds at most 2^30 pixels)
    float fx, fy;
};

// one axis: position = (a * yc + b * xc) + (t + centre), clamped to [0, extent - 1] -> lower tap, upper tap, weight.
// contract(off): hipcc fuses a * b + c by default -- through __dmul_rn / __dadd_rn too, which are plain operators in HIP's headers (the ISA showed
// v_fma_f64 with them) -- and the definition has no fused float64 operation; the pragma covers the operators written in its block.
__device__ __forceinline__ void axis_taps(double a, double b, double t, double yc, double xc, double centre, int extent, int& lo, int& hi, float& f)
{
#pragma clang fp contract(off)
    const double pa = a * yc, pb = b * xc;
    const double lin = pa + pb, shift = t + centre;
    double s = lin + shift;
    s = fmin(fmax(s, 0.0), (double)(extent - 1));      // border mode (fmax(NaN, 0) is 0: no value of s leaves the plane)
    const double fl = floor(s);
    lo = (int)fl;
    hi = lo + 1 < extent ? lo + 1 : extent - 1;
    f = (float)(s - fl);
}

__device__ __forceinline__ Taps taps_of(const double* __restrict__ m, int i, int j, int H, int W)
{
#pragma clang fp contract(off)
    const double cy = 0.5 * (double)(H - 1), cx = 0.5 * (double)(W - 1);      // exact
    const double yc = (double)i - cy, xc = (double)j - cx;
    int i0, i1, j0, j1;
    Taps t;
    axis_taps(m[0], m[1], m[2], yc, xc, cy, H, i0, i1, t.fy);
    axis_taps(m[3], m[4], m[5], yc, xc, cx, W, j0, j1, t.fx);
    t.o00 = i0 * W + j0;
    t.o01 = i0 * W + j1;
    t.o10 = i1 * W + j0;
    t.o11 = i1 * W + j1;
    return t;
}

__device__ __forceinline__ float lerp(float a, float b, float t)
{
#pragma clang fp contract(off)
    return fmaf(t, b - a, a);
}

__device__ __forceinline__ float bilinear(float v00, float v01, float v10, float v11, float fx, float fy)
{
    return lerp(lerp(v00, v01, fx), lerp(v10, v11, fx), fy);
}

// the output pixel of this lane: tiles of WARP_BX x WARP_BY pixels, row-major over the plane, along grid.x
__device__ __forceinline__ bool lane_pixel(int H, int W, int& i, int& j)
{
    const unsigned tiles_x = ((unsigned)W + WARP_BX - 1) / WARP_BX;
    const unsigned ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    i = (int)(ty * WARP_BY + threadIdx.y);
    j = (int)(tx * WARP_BX + threadIdx.x);
    return i < H && j < W;
}

// grid.x: tiles of a plane, grid.y: planes (strided), grid.z: matrices
__global__ __launch_bounds__(WARP_THREADS) void warp_affine_kernel(const float* __restrict__ x, const double* __restrict__ mats,
                                                                   float* __restrict__ out, size_t planes, int H, int W)
{
    int i, j;
    if (!lane_pixel(H, W, i, j)) return;
    const Taps t = taps_of(mats + 6 * (size_t)blockIdx.z, i, j, H, W);
    const size_t hw = (size_t)H * W;
    const size_t o = (size_t)i * W + j;
    float* dst = out + (size_t)blockIdx.z * planes * hw;
    for (size_t p = blockIdx.y; p < planes; p += gridDim.y) {
        const float* src = x + p * hw;
        dst[p * hw + o] = bilinear(src[t.o00], src[t.o01], src[t.o10], src[t.o11], t.fx, t.fy);
    }
}

// grid.x: tiles of a plane, grid.y: canonical slices (strided).  The voxel's statistics are loaded once, every group is added in ascending
// order with the operations of accumulate_voxel (VoxelStats, rcu_head_common.h), and stored once.
template <int C>
__global__ __launch_bounds__(WARP_THREADS) void mc_accumulate_warped_kernel(const float* __restrict__ in, void* stats,
                                                                            const double* __restrict__ mats, int groups, size_t n, int H, int W,
                                                                            int flags)
{
    int i, j;
    if (!lane_pixel(H, W, i, j)) return;
    const size_t hw = (size_t)H * W, V = n * hw;
    const size_t o = (size_t)i * W + j;
    const bool probs = (flags & MC_INPUT_PROBS) != 0;
    for (size_t s = blockIdx.y; s < n; s += gridDim.y) {
        VoxelStats<C> st;
        st.load(stats, s * hw + o, V, flags);
        for (int g = 0; g < groups; ++g) {
            const Taps t = taps_of(mats + 6 * (size_t)g, i, j, H, W);
            const float* src = in + ((size_t)g * n + s) * C * hw;
            float v00[C], v01[C], v10[C], v11[C], p[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float* plane = src + (size_t)c * hw;
                v00[c] = plane[t.o00];
                v01[c] = plane[t.o01];
                v10[c] = plane[t.o10];
                v11[c] = plane[t.o11];
            }
            if (!probs) {      // rcu_softmax of every tap, then the warp of the probabilities
                softmax_inplace<C>(v00);
                softmax_inplace<C>(v01);
                softmax_inplace<C>(v10);
                softmax_inplace<C>(v11);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) p[c] = bilinear(v00[c], v01[c], v10[c], v11[c], t.fx, t.fy);
            st.add(flags, p);
        }
        st.store(stats, s * hw + o, V, flags);
    }
}

inline dim3 warp_grid(int H, int W, size_t planes, unsigned z)
{
    const unsigned tiles = (((unsigned)W + WARP_BX - 1) / WARP_BX) * (((unsigned)H + WARP_BY - 1) / WARP_BY);      // <= 2^30 / 16 + ...: fits
    return dim3(tiles, (unsigned)(planes < WARP_MAX_PLANE_BLOCKS ? planes : WARP_MAX_PLANE_BLOCKS), z);
}

template <int C>
hipError_t launch_accumulate_warped(const float* in, void* stats, const double* mats, int groups, size_t n, int H, int W, int flags, hipStream_t stream)
{
    hipLaunchKernelGGL(mc_accumulate_warped_kernel<C>, warp_grid(H, W, n, 1), dim3(WARP_BX, WARP_BY), 0, stream, in, stats, mats, groups, n, H, W,
                       flags);
    return hipGetLastError();
}

int check_plane(const std::string& fn, size_t n, int height, int width, int count, const char* count_name)
{
    if (count < 1 || count > RCU_WARP_MAX_MATRICES)
        return report_error(RCU_ERR_INVALID, fn + ": " + count_name + " must be in 1.." + std::to_string(RCU_WARP_MAX_MATRICES) + ", got " +
                                                 std::to_string(count));
    if (n < 1 || height < 1 || width < 1) return report_error(RCU_ERR_INVALID, fn + ": empty batch or plane (n, height, width >= 1)");
    if ((size_t)height * (size_t)width > (size_t)1 << 30) return report_error(RCU_ERR_INVALID, fn + ": plane larger than 2^30 pixels");
    return RCU_OK;
}

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}

}  // namespace
}  // namespace rcu

using namespace rcu;

extern "C" int rcu_warp_affine(const float* x_dev, size_t n, int channels, int height, int width, const double* mats_dev, int n_mats, float* out_dev,
                               void* stream)
{
    if (!x_dev || !mats_dev || !out_dev) return report_error(RCU_ERR_INVALID, "rcu_warp_affine: null argument");
    if (int st = check_plane("rcu_warp_affine", n, height, width, n_mats, "n_mats")) return st;
    if (channels < 1) return report_error(RCU_ERR_INVALID, "rcu_warp_affine: channels must be >= 1");
    const size_t planes = n * (size_t)channels;
    const size_t bytes = planes * (size_t)height * width * sizeof(float);
    if (overlap(x_dev, bytes, out_dev, bytes * (size_t)n_mats))
        return report_error(RCU_ERR_INVALID, "rcu_warp_affine: out must not overlap x (out == x is not supported)");
    hipLaunchKernelGGL(warp_affine_kernel, warp_grid(height, width, planes, (unsigned)n_mats), dim3(WARP_BX, WARP_BY), 0,
                       static_cast<hipStream_t>(stream), x_dev, mats_dev, out_dev, planes, height, width);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_warp_affine", e);
}

extern "C" int rcu_mc_accumulate_warped(const float* in_dev, void* stats_dev, size_t n, int height, int width, int nb_classes, int flags,
                                        const double* mats_dev, int groups, void* stream)
{
    if (!in_dev || !stats_dev || !mats_dev) return report_error(RCU_ERR_INVALID, "rcu_mc_accumulate_warped: null argument");
    if (int st = check_plane("rcu_mc_accumulate_warped", n, height, width, groups, "groups")) return st;
    if (nb_classes < 1 || nb_classes > MAX_CLASSES) return report_error(RCU_ERR_INVALID, "rcu_mc_accumulate_warped: nb_classes must be in 1..8");
    if (flags & ~(RCU_MC_MI | RCU_MC_VAR | RCU_MC_INPUT_PROBS | RCU_MC_EXACT))
        return report_error(RCU_ERR_INVALID, "rcu_mc_accumulate_warped: flags must be a combination of RCU_MC_MI, RCU_MC_VAR, RCU_MC_INPUT_PROBS and "
                                             "RCU_MC_EXACT, got " + std::to_string(flags));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipErrorInvalidValue;
    switch (nb_classes) {
#define RCU_WARP_CASE(C_) case C_: e = launch_accumulate_warped<C_>(in_dev, stats_dev, mats_dev, groups, n, height, width, flags, s); break;
        RCU_WARP_CASE(1) RCU_WARP_CASE(2) RCU_WARP_CASE(3) RCU_WARP_CASE(4) RCU_WARP_CASE(5) RCU_WARP_CASE(6) RCU_WARP_CASE(7) RCU_WARP_CASE(8)
#undef RCU_WARP_CASE
    }
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_mc_accumulate_warped", e);
}
