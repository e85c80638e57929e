// Adaptive MC dropout (include/rcu.h "Adaptive MC"): the device glue between the pass spans of rcu_amd.steps.McPredictStep(adaptive=...).
//   mc_slice_scores         per slice: the number of unsettled voxels and the smallest leading class sum, both integers
//   dropout_masks_indexed   the mask draw of rcu_dropout_masks at scattered global sample indices
//   mc_merge_slices         a compact statistics blob added into the rows of the full one
//   mc_finalize_counts      rcu_mc_finalize with a pass count per slice
// All four are memory-bound streams over statistics planes (rcu_kernels.h: the blob layout); none touches a conv, head or aggregation kernel.
// The per-voxel arithmetic they share with those -- entropy_of, mc_is_f64 / mc_h_plane, Philox -- is rcu_head_common.h's.
#include <initializer_list>

#include "rcu_head_common.h"

namespace rcu {

static constexpr int AD_THREADS = 256;
static constexpr int AD_WAVES = AD_THREADS / 64;
static constexpr int AD_UNROLL = 4;      // units a lane of the score kernel has in flight

static inline bool aligned16(std::initializer_list<const void*> ptrs)
{
    for (const void* p : ptrs)
        if (p != nullptr && (reinterpret_cast<uintptr_t>(p) & 15u) != 0) return false;
    return true;
}

// ------------------------------------------------------------------------------- slice scores
// q(v) = (int64)(max_c S_c(v) * 2^40): S_c is a multiple of 2^-40 below 2^13 (RCU_MC_EXACT), so the product is an integer below 2^53 and the
// conversion is exact -- nothing here rounds.  A voxel is unsettled iff q(v) < thr_q.  Per slice: the count of unsettled voxels (an integer add)
// and min_v q(v) (an integer min); both are associative and commutative, so neither depends on the launch geometry.
__device__ __forceinline__ long long score_of(double leading) { return (long long)(leading * 1099511627776.0); }

__global__ __launch_bounds__(AD_THREADS) void mc_scores_init_kernel(uint32_t* __restrict__ unsettled, long long* __restrict__ margin_q, int n)
{
    const int i = blockIdx.x * AD_THREADS + threadIdx.x;
    if (i >= n) return;
    unsettled[i] = 0u;
    margin_q[i] = 0x7fffffffffffffffll;
}

// VEC = 2: 16 bytes (two voxels) per lane and class plane; VEC = 1: one voxel.  Workgroup b of a slice walks the slice's rounds of
// AD_UNROLL * AD_THREADS units b, b + bps, ...
template <int C, int VEC>
__global__ __launch_bounds__(AD_THREADS) void mc_slice_scores_kernel(const double* __restrict__ stats, uint32_t units, size_t HW, size_t V, uint32_t bps,
                                                                      long long thr_q, uint32_t* __restrict__ unsettled, long long* __restrict__ margin_q)
{
    const uint32_t slice = blockIdx.x / bps, b = blockIdx.x - slice * bps;
    const double* base = stats + (size_t)slice * HW;
    uint32_t count = 0u;
    long long lowest = 0x7fffffffffffffffll;
    // AD_UNROLL units per lane and round, their loads issued together: a unit past the end of the slice reads the slice's last unit again (an
    // address inside the blob, no branch in front of the loads) and is left out of the count and of the minimum
    for (uint32_t first = b * (AD_UNROLL * AD_THREADS) + threadIdx.x; first < units; first += bps * (AD_UNROLL * AD_THREADS)) {
        long long q[AD_UNROLL][VEC];
#pragma unroll
        for (int k = 0; k < AD_UNROLL; ++k) {
            const uint32_t u = first + k * AD_THREADS, at = u < units ? u : units - 1;
            if constexpr (VEC == 2) {
                double2 m = reinterpret_cast<const double2*>(base)[at];
#pragma unroll
                for (int c = 1; c < C; ++c) {
                    const double2 s = reinterpret_cast<const double2*>(base + (size_t)c * V)[at];
                    m.x = fmax(m.x, s.x);
                    m.y = fmax(m.y, s.y);
                }
                q[k][0] = score_of(m.x);
                q[k][VEC - 1] = score_of(m.y);
            } else {
                double m = base[at];
#pragma unroll
                for (int c = 1; c < C; ++c) m = fmax(m, base[(size_t)c * V + at]);
                q[k][0] = score_of(m);
            }
        }
#pragma unroll
        for (int k = 0; k < AD_UNROLL; ++k) {
            const bool inside = first + k * AD_THREADS < units;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                count += (inside && q[k][e] < thr_q) ? 1u : 0u;
                lowest = (inside && q[k][e] < lowest) ? q[k][e] : lowest;
            }
        }
    }
    // in-wave butterfly, then one LDS step per workgroup, then one integer add and one integer min per workgroup and slice
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        count += __shfl_xor(count, off);
        const long long other = __shfl_xor(lowest, off);
        lowest = other < lowest ? other : lowest;
    }
    __shared__ uint32_t s_count[AD_WAVES];
    __shared__ long long s_lowest[AD_WAVES];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_count[wave] = count;
        s_lowest[wave] = lowest;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < AD_WAVES; ++k) {
            count += s_count[k];
            lowest = s_lowest[k] < lowest ? s_lowest[k] : lowest;
        }
        if (count != 0u) atomicAdd(&unsettled[slice], count);
        atomicMin(&margin_q[slice], lowest);
    }
}

#define RCU_AD_DISPATCH_C(Cval, ...)                                 \
    switch (Cval) {                                                  \
        case 1: { constexpr int C_ = 1; __VA_ARGS__; break; }        \
        case 2: { constexpr int C_ = 2; __VA_ARGS__; break; }        \
        case 3: { constexpr int C_ = 3; __VA_ARGS__; break; }        \
        case 4: { constexpr int C_ = 4; __VA_ARGS__; break; }        \
        case 5: { constexpr int C_ = 5; __VA_ARGS__; break; }        \
        case 6: { constexpr int C_ = 6; __VA_ARGS__; break; }        \
        case 7: { constexpr int C_ = 7; __VA_ARGS__; break; }        \
        case 8: { constexpr int C_ = 8; __VA_ARGS__; break; }        \
        default: return hipErrorInvalidValue;                        \
    }

// float64 statistics only (MC_EXACT): unsettled[i] = #{v in slice i : (int64)(max_c S_c(v) * 2^40) < thr_q}, margin_q[i] = the smallest such integer
static hipError_t launch_mc_slice_scores(const void* stats, int C, size_t N, size_t HW, long long thr_q, uint32_t* unsettled, long long* margin_q,
                                         hipStream_t stream)
{
    hipLaunchKernelGGL(mc_scores_init_kernel, dim3((unsigned)((N + AD_THREADS - 1) / AD_THREADS)), dim3(AD_THREADS), 0, stream, unsettled, margin_q,
                       (int)N);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const double* sd = static_cast<const double*>(stats);
    const size_t V = N * HW;
    const bool vec = HW % 2 == 0 && aligned16({stats});      // every slice of every plane then starts on 16 bytes
    const uint32_t units = (uint32_t)(vec ? HW / 2 : HW);
    // AD_UNROLL units per lane and workgroup: enough loads in flight per lane, enough workgroups per slice to fill the device from a few slices on
    uint32_t bps = (units + AD_UNROLL * AD_THREADS - 1) / (AD_UNROLL * AD_THREADS);
    bps = bps < 1u ? 1u : bps > 64u ? 64u : bps;
    const dim3 grid((unsigned)(N * bps));
    if (vec) {
        RCU_AD_DISPATCH_C(C, hipLaunchKernelGGL((mc_slice_scores_kernel<C_, 2>), grid, dim3(AD_THREADS), 0, stream, sd, units, HW, V, bps, thr_q,
                                                unsettled, margin_q));
    } else {
        RCU_AD_DISPATCH_C(C, hipLaunchKernelGGL((mc_slice_scores_kernel<C_, 1>), grid, dim3(AD_THREADS), 0, stream, sd, units, HW, V, bps, thr_q,
                                                unsettled, margin_q));
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------- indexed mask draw
// dropout_masks_kernel (rcu_pointwise.hip) with the global index of row i read from sample_index[i] instead of first_sample + i: the same element
// number e, the same Philox block and word, the same factor -- bit for bit the row the contiguous draw gives that sample.
__global__ __launch_bounds__(AD_THREADS) void dropout_masks_indexed_kernel(const MaskArgs a, const long long* __restrict__ sample_index,
                                                                            float* __restrict__ out)
{
    const int r = blockIdx.x * AD_THREADS + threadIdx.x;      // element of the pass's own mask [site][n][C_site]
    const int t = blockIdx.y;
    if (r >= a.per_pass) return;
    int s = 0;
    while (r >= a.site_end[s]) ++s;
    const int begin = s ? a.site_end[s - 1] : 0, len = a.site_end[s] - begin;
    const int ch = a.site_ch[s], i = (r - begin) / ch, c = (r - begin) - i * ch;
    const unsigned long long e = (unsigned long long)sample_index[i] * (unsigned long long)a.per_sample + (unsigned long long)(a.site_off[s] + c);
    uint32_t w[4];
    philox4x32_10((uint32_t)a.seed[t], (uint32_t)(a.seed[t] >> 32), (uint32_t)(e >> 2), (uint32_t)(e >> 34), 0u, 0u, w);
    const uint32_t word = (e & 3) == 0 ? w[0] : (e & 3) == 1 ? w[1] : (e & 3) == 2 ? w[2] : w[3];
    const float keep = a.site_keep[s];
    const float u = (float)(word >> 8) * (1.0f / 16777216.0f);
    const float factor = keep < 0.f ? 1.f : (keep > 0.f && u < keep) ? 1.f / keep : 0.f;
    out[(size_t)a.passes * begin + (size_t)(a.first + t) * len + (r - begin)] = factor;
}

hipError_t launch_dropout_masks_indexed(const MaskArgs& a, const long long* sample_index, float* out, hipStream_t stream)
{
    hipLaunchKernelGGL(dropout_masks_indexed_kernel, dim3((a.per_pass + AD_THREADS - 1) / AD_THREADS, a.count), dim3(AD_THREADS), 0, stream, a,
                       sample_index, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------- merge of a compact blob
// dst[plane][index[i]][pix] += src[plane][i][pix] for every plane; T: the element of a move (16 bytes where rows and bases allow, else one value).
// Row r = plane * m + i is walked by the workgroups blockIdx.x = r * bpr .. r * bpr + bpr - 1.  No atomics: the indices of a call are distinct.
template <typename T>
__device__ __forceinline__ T add_elements(T a, T b) { return a + b; }
template <>
__device__ __forceinline__ double2 add_elements<double2>(double2 a, double2 b) { return double2{a.x + b.x, a.y + b.y}; }
template <>
__device__ __forceinline__ float4 add_elements<float4>(float4 a, float4 b) { return float4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }

template <typename T>
__global__ __launch_bounds__(AD_THREADS) void mc_merge_slices_kernel(const T* __restrict__ src, T* __restrict__ dst, uint32_t units, uint32_t m, uint32_t n,
                                                                      uint32_t bpr, const int32_t* __restrict__ index)
{
    const uint32_t r = blockIdx.x / bpr, b = blockIdx.x - r * bpr;
    const uint32_t plane = r / m, i = r - plane * m;
    const int32_t to = index[i];
    if (to < 0 || (uint32_t)to >= n) return;      // a skipped entry (and never a store outside dst)
    const T* s = src + ((size_t)plane * m + i) * units;
    T* d = dst + ((size_t)plane * n + (uint32_t)to) * units;
    for (uint32_t u = b * AD_THREADS + threadIdx.x; u < units; u += bpr * AD_THREADS) d[u] = add_elements<T>(d[u], s[u]);
}

template <typename T>
static hipError_t launch_merge_as(const void* src, void* dst, size_t units, size_t rows, size_t m, size_t n, const int32_t* index, hipStream_t stream)
{
    uint32_t bpr = (uint32_t)((units + 4 * AD_THREADS - 1) / (4 * AD_THREADS));
    bpr = bpr < 1u ? 1u : bpr > 64u ? 64u : bpr;
    hipLaunchKernelGGL(mc_merge_slices_kernel<T>, dim3((unsigned)(rows * bpr)), dim3(AD_THREADS), 0, stream, static_cast<const T*>(src), static_cast<T*>(dst),
                       (uint32_t)units, (uint32_t)m, (uint32_t)n, bpr, index);
    return hipGetLastError();
}

// every plane: dst[plane][index[i]] += src[plane][i], i < M; entries outside [0, N) are skipped; the others must be distinct
static hipError_t launch_mc_merge_slices(const void* src, size_t M, void* dst, size_t N, size_t HW, int C, int flags, const int32_t* index, hipStream_t stream)
{
    const size_t planes = (size_t)C + ((flags & MC_VAR) ? (size_t)C : 0) + ((flags & MC_MI) ? 1 : 0);
    const size_t rows = planes * M;
    const bool f64 = (flags & (MC_VAR | MC_EXACT)) != 0;
    const bool al = aligned16({src, dst});
    if (f64) {
        if (al && HW % 2 == 0) return launch_merge_as<double2>(src, dst, HW / 2, rows, M, N, index, stream);
        return launch_merge_as<double>(src, dst, HW, rows, M, N, index, stream);
    }
    if (al && HW % 4 == 0) return launch_merge_as<float4>(src, dst, HW / 4, rows, M, N, index, stream);
    return launch_merge_as<float>(src, dst, HW, rows, M, N, index, stream);
}

// ------------------------------------------------------------------------------- finalize with a count per slice
// mc_finalize_kernel / mc_finalize4_kernel (rcu_pointwise.hip) with T = counts[slice]: the same operations in the same order on every voxel, so
// equal counts give the bits rcu_mc_finalize gives.
template <int C>
__global__ __launch_bounds__(AD_THREADS) void mc_finalize_counts_kernel(const void* stats, size_t HW, size_t V, const int32_t* __restrict__ counts,
                                                                         int flags, float* __restrict__ mean, float* __restrict__ entropy,
                                                                         float* __restrict__ mi, float* __restrict__ var)
{
    const size_t v = (size_t)blockIdx.x * AD_THREADS + threadIdx.x;
    if (v >= V) return;
    const size_t n = v / HW, hw = v % HW;
    const int T = counts[n];
    float p[C];
    float sum_h = 0.f;
    if (mc_is_f64(flags)) {
        const double* sd = reinterpret_cast<const double*>(stats);
        double vsum = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double s = sd[(size_t)c * V + v];
            p[c] = (float)(s / (double)T);
            if (flags & MC_VAR) {
                const double q = sd[(size_t)(C + c) * V + v];
                vsum += (q - s * s / (double)T) / (double)(T - 1);
            }
        }
        if (var != nullptr && (flags & MC_VAR)) var[v] = (float)fmax(vsum / (double)C, 0.0);
        if (flags & MC_MI) sum_h = (float)sd[(size_t)mc_h_plane(flags, C) * V + v];
    } else {
        const float* sf = reinterpret_cast<const float*>(stats);
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = sf[(size_t)c * V + v] / (float)T;
        if (flags & MC_MI) sum_h = sf[(size_t)C * V + v];
    }
    if (mean != nullptr) {
#pragma unroll
        for (int c = 0; c < C; ++c) mean[(n * C + c) * HW + hw] = p[c];
    }
    const float h = entropy_of<C>(p);
    if (entropy != nullptr) entropy[v] = h;
    if (mi != nullptr && (flags & MC_MI)) mi[v] = h - sum_h / (float)T;
}

template <int C>
__global__ __launch_bounds__(AD_THREADS) void mc_finalize_counts4_kernel(const void* stats, uint32_t HW4, uint32_t V4, const int32_t* __restrict__ counts,
                                                                          int flags, float4* __restrict__ mean, float4* __restrict__ entropy,
                                                                          float4* __restrict__ mi, float4* __restrict__ var)
{
    const uint32_t i = blockIdx.x * AD_THREADS + threadIdx.x;
    if (i >= V4) return;
    const uint32_t n = i / HW4, q = i - n * HW4;
    const int T = counts[n];
    float p[4][C], sum_h[4] = {0.f, 0.f, 0.f, 0.f}, vr[4] = {0.f, 0.f, 0.f, 0.f};
    if (mc_is_f64(flags)) {
        const double2* sd = reinterpret_cast<const double2*>(stats);
        const size_t P2 = 2 * (size_t)V4;
        double vsum[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const double2 s2 = sd[(size_t)c * P2 + 2 * (size_t)i + h];
                p[2 * h][c] = (float)(s2.x / (double)T);
                p[2 * h + 1][c] = (float)(s2.y / (double)T);
                if (flags & MC_VAR) {
                    const double2 q2 = sd[(size_t)(C + c) * P2 + 2 * (size_t)i + h];
                    vsum[2 * h] += (q2.x - s2.x * s2.x / (double)T) / (double)(T - 1);
                    vsum[2 * h + 1] += (q2.y - s2.y * s2.y / (double)T) / (double)(T - 1);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) vr[k] = (float)fmax(vsum[k] / (double)C, 0.0);
        if (flags & MC_MI) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const double2 e = sd[(size_t)mc_h_plane(flags, C) * P2 + 2 * (size_t)i + h];
                sum_h[2 * h] = (float)e.x;
                sum_h[2 * h + 1] = (float)e.y;
            }
        }
    } else {
        const float4* sf = reinterpret_cast<const float4*>(stats);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float4 a = sf[(size_t)c * V4 + i];
            p[0][c] = a.x / (float)T; p[1][c] = a.y / (float)T; p[2][c] = a.z / (float)T; p[3][c] = a.w / (float)T;
        }
        if (flags & MC_MI) {
            const float4 e = sf[(size_t)C * V4 + i];
            sum_h[0] = e.x; sum_h[1] = e.y; sum_h[2] = e.z; sum_h[3] = e.w;
        }
    }
    if (mean != nullptr) {
#pragma unroll
        for (int c = 0; c < C; ++c) mean[(size_t)(n * C + c) * HW4 + q] = float4{p[0][c], p[1][c], p[2][c], p[3][c]};
    }
    float h[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] = entropy_of<C>(p[k]);
    if (entropy != nullptr) entropy[i] = float4{h[0], h[1], h[2], h[3]};
    if (mi != nullptr && (flags & MC_MI))
        mi[i] = float4{h[0] - sum_h[0] / (float)T, h[1] - sum_h[1] / (float)T, h[2] - sum_h[2] / (float)T, h[3] - sum_h[3] / (float)T};
    if (var != nullptr && (flags & MC_VAR)) var[i] = float4{vr[0], vr[1], vr[2], vr[3]};
}

// launch_mc_finalize (rcu_pointwise.hip) with T = counts[slice] (device array of N entries >= 1)
static hipError_t launch_mc_finalize_counts(const void* stats, int C, size_t N, size_t HW, const int32_t* counts, int flags, float* mean, float* entropy,
                                            float* mi, float* var, hipStream_t stream)
{
    const size_t V = N * HW;
    // the condition of launch_mc_finalize's four-voxel form (rcu_pointwise.hip, vec4_ok)
    if (HW % 4 == 0 && V / 4 < ((size_t)1 << 31) && aligned16({stats, mean, entropy, mi, var})) {
        RCU_AD_DISPATCH_C(C, hipLaunchKernelGGL(mc_finalize_counts4_kernel<C_>, dim3((unsigned)((V / 4 + AD_THREADS - 1) / AD_THREADS)), dim3(AD_THREADS), 0,
                                                stream, stats, (uint32_t)(HW / 4), (uint32_t)(V / 4), counts, flags, reinterpret_cast<float4*>(mean),
                                                reinterpret_cast<float4*>(entropy), reinterpret_cast<float4*>(mi), reinterpret_cast<float4*>(var)));
        return hipGetLastError();
    }
    RCU_AD_DISPATCH_C(C, hipLaunchKernelGGL(mc_finalize_counts_kernel<C_>, dim3((unsigned)((V + AD_THREADS - 1) / AD_THREADS)), dim3(AD_THREADS), 0, stream,
                                            stats, HW, V, counts, flags, mean, entropy, mi, var));
    return hipGetLastError();
}

}  // namespace rcu

// ------------------------------------------------------------------------------------------------
// entry points (include/rcu.h "Adaptive MC").  A HIP error is reported under the text of the call that returned it.
// ------------------------------------------------------------------------------------------------
using namespace rcu;

// slices of hw voxels whose rows, row blocks and voxel quads stay inside the kernels' 32-bit indices
static int check_adaptive_shape(const char* fn, size_t n, size_t hw, int C)
{
    if (check_classes(C)) return RCU_ERR_INVALID;
    if (n < 1 || hw < 1 || n > ((size_t)1 << 20) || hw > ((size_t)1 << 30))
        return report_error(RCU_ERR_INVALID, std::string(fn) + ": n must be in 1..2^20 and hw in 1..2^30");
    return RCU_OK;
}

extern "C" int rcu_mc_slice_scores(const void* stats_dev, size_t n, size_t hw, int C, int flags, int64_t thr_q, uint32_t* unsettled_dev,
                                   int64_t* margin_q_dev, void* stream)
{
    if (!stats_dev || !unsettled_dev || !margin_q_dev) return report_error(RCU_ERR_INVALID, "rcu_mc_slice_scores: null argument");
    if (check_adaptive_shape("rcu_mc_slice_scores", n, hw, C)) return RCU_ERR_INVALID;
    if (!(flags & RCU_MC_EXACT) || (flags & ~(RCU_MC_MI | RCU_MC_VAR | RCU_MC_EXACT)))
        return report_error(RCU_ERR_INVALID, "rcu_mc_slice_scores: needs RCU_MC_EXACT statistics (the decision is made on exact integer sums), got flags " +
                                                 std::to_string(flags));
    if (thr_q < 0) return report_error(RCU_ERR_INVALID, "rcu_mc_slice_scores: thr_q must be >= 0");
    if (reinterpret_cast<uintptr_t>(stats_dev) % 8 != 0) return report_error(RCU_ERR_INVALID, "rcu_mc_slice_scores: stats must be 8-byte aligned");
    const hipError_t e = launch_mc_slice_scores(stats_dev, C, n, hw, (long long)thr_q, unsettled_dev, reinterpret_cast<long long*>(margin_q_dev),
                                                static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RCU_OK
                           : hip_failed("launch_mc_slice_scores(stats_dev, C, n, hw, (long long)thr_q, unsettled_dev, reinterpret_cast<long long*>(margin_q_dev), "
                                        "static_cast<hipStream_t>(stream))", e);
}

extern "C" int rcu_mc_merge_slices(const void* src_stats_dev, size_t m, void* dst_stats_dev, size_t n, size_t hw, int C, int flags,
                                   const int32_t* index_dev, void* stream)
{
    if (!src_stats_dev || !dst_stats_dev || !index_dev) return report_error(RCU_ERR_INVALID, "rcu_mc_merge_slices: null argument");
    if (check_adaptive_shape("rcu_mc_merge_slices", n, hw, C) || check_adaptive_shape("rcu_mc_merge_slices", m, hw, C)) return RCU_ERR_INVALID;
    if (flags & ~(RCU_MC_MI | RCU_MC_VAR | RCU_MC_EXACT))
        return report_error(RCU_ERR_INVALID, "rcu_mc_merge_slices: flags must be a combination of RCU_MC_MI, RCU_MC_VAR and RCU_MC_EXACT, got " +
                                                 std::to_string(flags));
    const uintptr_t s = reinterpret_cast<uintptr_t>(src_stats_dev), d = reinterpret_cast<uintptr_t>(dst_stats_dev);
    const size_t element = (flags & (RCU_MC_VAR | RCU_MC_EXACT)) ? 8 : 4;
    if (s % element != 0 || d % element != 0) return report_error(RCU_ERR_INVALID, "rcu_mc_merge_slices: blobs must be aligned to their element");
    if (s < d + rcu_mc_stats_bytes(n, hw, C, flags) && d < s + rcu_mc_stats_bytes(m, hw, C, flags))
        return report_error(RCU_ERR_INVALID, "rcu_mc_merge_slices: src and dst must not overlap");
    const hipError_t e = launch_mc_merge_slices(src_stats_dev, m, dst_stats_dev, n, hw, C, flags, index_dev, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RCU_OK
                           : hip_failed("launch_mc_merge_slices(src_stats_dev, m, dst_stats_dev, n, hw, C, flags, index_dev, static_cast<hipStream_t>(stream))", e);
}

extern "C" int rcu_mc_finalize_counts(const void* stats, size_t n, size_t hw, int C, const int32_t* counts_dev, int flags, float* mean,
                                      float* entropy, float* mi, float* var, void* stream)
{
    if (!stats || !counts_dev) return report_error(RCU_ERR_INVALID, "rcu_mc_finalize_counts: null argument");
    if (check_classes(C)) return RCU_ERR_INVALID;
    if (mi && !(flags & RCU_MC_MI)) return report_error(RCU_ERR_INVALID, "mutual_info requested without RCU_MC_MI statistics");
    if (var && !(flags & RCU_MC_VAR)) return report_error(RCU_ERR_INVALID, "variance requested without RCU_MC_VAR statistics");
    if (n * hw == 0) return RCU_OK;
    const hipError_t e = launch_mc_finalize_counts(stats, C, n, hw, counts_dev, flags, mean, entropy, mi, var, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RCU_OK
                           : hip_failed("launch_mc_finalize_counts(stats, C, n, hw, counts_dev, flags, mean, entropy, mi, var, static_cast<hipStream_t>(stream))", e);
}
