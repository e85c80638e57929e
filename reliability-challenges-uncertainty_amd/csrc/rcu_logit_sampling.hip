// Test-time logit sampling of a sigma head over materialised logits (include/rcu.h, "Test-time logit sampling"): rcu_logit_normals dumps the
// normals z of the definition, rcu_logit_sampling writes and / or accumulates the sampled predictive
//     p_bar[c] = (1/S) sum_s softmax(mu + sig * z_s)[c],   sig = |raw| or exp(raw)
// of every voxel.  Both call the device functions of the fused head (rcu_head_common.h: logit_normals4, logit_sample_predictive), so the
// materialised and the fused paths produce the same bits.  One thread per voxel, voxel index fastest across lanes: the [n][C][hw] planes are
// read and written coalesced; the arithmetic (S softmaxes and S * C / 4 Philox blocks per voxel) dominates from S of a few on.
#include "../../include/rcu.h"
#include "rcu_head_common.h"

#include <string>

namespace rcu {
namespace {

constexpr int LS_THREADS = 256;

inline unsigned ls_grid(size_t n) { return (unsigned)((n + LS_THREADS - 1) / LS_THREADS); }

#define RCU_LS_DISPATCH_C(Cval, ...)                                 \
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

// out[v][s][c] = z(key, first_sample + v / hw, v % hw, s, c), one thread per voxel (a test aid: the stores are strided by S * C)
__global__ __launch_bounds__(LS_THREADS) void logit_normals_kernel(unsigned long long key, unsigned long long first_sample, size_t hw, size_t V,
                                                                   int C, int S, float* __restrict__ out)
{
    const size_t v = (size_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (v >= V) return;
    const size_t n = v / hw, p = v % hw;
    const uint32_t J = (uint32_t)S * (uint32_t)C;
    float* o = out + v * J;
    for (uint32_t q = 0; q * 4 < J; ++q) {
        float z[4];
        logit_normals4(key, first_sample + n, (uint32_t)p, q, z);
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e)
            if (q * 4 + e < J) o[q * 4 + e] = z[e];
    }
}

template <int C>
__global__ __launch_bounds__(LS_THREADS) void logit_sampling_kernel(const float* __restrict__ logits, const float* __restrict__ sigma_raw, size_t hw,
                                                                    size_t V, int is_log_sigma, int S, unsigned long long key,
                                                                    unsigned long long first_sample, float* __restrict__ probs, void* stats, int flags)
{
    const size_t v = (size_t)blockIdx.x * LS_THREADS + threadIdx.x;
    if (v >= V) return;
    const size_t n = v / hw, p = v % hw;
    VoxelStats<C> st;
    if (stats != nullptr) st.load(stats, v, V, flags);
    float l[C], sg[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        l[c] = logits[(n * C + c) * hw + p];
        sg[c] = sigma_of_raw(sigma_raw[(n * C + c) * hw + p], is_log_sigma);
    }
    logit_sample_predictive<C>(l, sg, key, first_sample + n, (uint32_t)p, S);
    if (probs != nullptr) {
#pragma unroll
        for (int c = 0; c < C; ++c) probs[(n * C + c) * hw + p] = l[c];
    }
    if (stats != nullptr) {
        st.add(flags, l);
        st.store(stats, v, V, flags);
    }
}

}  // namespace

static hipError_t launch_logit_normals(unsigned long long key, unsigned long long first_sample, size_t n, size_t hw, int C, int samples, float* out,
                                       hipStream_t stream)
{
    const size_t V = n * hw;
    hipLaunchKernelGGL(logit_normals_kernel, dim3(ls_grid(V)), dim3(LS_THREADS), 0, stream, key, first_sample, hw, V, C, samples, out);
    return hipGetLastError();
}

static hipError_t launch_logit_sampling(const float* logits, const float* sigma_raw, size_t n, size_t hw, int C, int is_log_sigma, int samples,
                                        unsigned long long key, unsigned long long first_sample, float* probs, void* stats, int flags, hipStream_t stream)
{
    const size_t V = n * hw;
    RCU_LS_DISPATCH_C(C, hipLaunchKernelGGL(logit_sampling_kernel<C_>, dim3(ls_grid(V)), dim3(LS_THREADS), 0, stream, logits, sigma_raw, hw, V,
                                            is_log_sigma, samples, key, first_sample, probs, stats, flags));
    return hipGetLastError();
}

// the argument checks both entry points share; every one before the device is touched
int check_logit_sampling_shape(const char* fn, size_t n, size_t hw, int nb_classes, int samples)
{
    if (nb_classes < 1 || nb_classes > MAX_CLASSES) return report_error(RCU_ERR_INVALID, std::string(fn) + ": nb_classes must be in 1..8");
    if (samples < 1 || samples > RCU_LOGIT_MAX_SAMPLES)
        return report_error(RCU_ERR_INVALID, std::string(fn) + ": samples must be in 1.." + std::to_string(RCU_LOGIT_MAX_SAMPLES) + ", got " +
                                                 std::to_string(samples));
    if (n < 1 || hw < 1) return report_error(RCU_ERR_INVALID, std::string(fn) + ": empty batch (n, hw >= 1)");
    if (hw >= ((size_t)1 << 32)) return report_error(RCU_ERR_INVALID, std::string(fn) + ": hw must be below 2^32 (the pixel is one counter word)");
    return RCU_OK;
}

}  // namespace rcu

using namespace rcu;

extern "C" int rcu_logit_normals(uint64_t key, uint64_t first_sample, size_t n, size_t hw, int nb_classes, int samples, float* out_dev, void* stream)
{
    if (!out_dev) return report_error(RCU_ERR_INVALID, "rcu_logit_normals: null out_dev");
    if (int st = check_logit_sampling_shape("rcu_logit_normals", n, hw, nb_classes, samples)) return st;
    hipError_t e = launch_logit_normals(key, first_sample, n, hw, nb_classes, samples, out_dev, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return report_error(RCU_ERR_HIP, std::string("rcu_logit_normals: ") + hipGetErrorString(e));
    return RCU_OK;
}

extern "C" int rcu_logit_sampling(const float* logits_dev, const float* sigma_raw_dev, size_t n, size_t hw, int nb_classes, int is_log_sigma,
                                  int samples, uint64_t key, uint64_t first_sample, float* probs_dev, void* stats_dev, int flags, void* stream)
{
    if (!logits_dev || !sigma_raw_dev) return report_error(RCU_ERR_INVALID, "rcu_logit_sampling: null logits_dev / sigma_raw_dev");
    if (!probs_dev && !stats_dev) return report_error(RCU_ERR_INVALID, "rcu_logit_sampling: probs_dev and stats_dev are both null (no output)");
    if (int st = check_logit_sampling_shape("rcu_logit_sampling", n, hw, nb_classes, samples)) return st;
    if (stats_dev && (flags & ~(RCU_MC_MI | RCU_MC_VAR | RCU_MC_EXACT)))
        return report_error(RCU_ERR_INVALID, "rcu_logit_sampling: flags must be a combination of RCU_MC_MI, RCU_MC_VAR and RCU_MC_EXACT, got " +
                                                 std::to_string(flags));
    hipError_t e = launch_logit_sampling(logits_dev, sigma_raw_dev, n, hw, nb_classes, is_log_sigma ? 1 : 0, samples, key, first_sample, probs_dev,
                                         stats_dev, stats_dev ? flags : 0, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return report_error(RCU_ERR_HIP, std::string("rcu_logit_sampling: ") + hipGetErrorString(e));
    return RCU_OK;
}
