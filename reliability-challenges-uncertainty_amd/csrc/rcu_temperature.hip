// Temperature scaling (include/rcu.h, "Temperature scaling"): the NLL of the pass-averaged prediction under every candidate inverse
// temperature beta_k, summed over voxels as exact integers (rcu_temperature_nll), and the per-voxel terms of one beta (rcu_temperature_nll_terms).
//
//   l_k(v) = -log( (1/P) sum_t softmax(beta_k z_{t,v})[y_v] ),   clamped to [0, 4096], added as round(l * 2^20) in uint64
//
// One workgroup = 4 waves over a tile of 64 voxels (lane l = voxel l of the tile).  The tile's P x (C-1) logit differences
// d_{t,c} = z_{t,c} - z_{t,y} are read from HBM once, by the whole workgroup, into LDS ([j][64] floats, j = t * (C-1) + c'); wave w then runs
// candidates k = w, w + 4, ... over them, each lane adding its voxel's rounded term into a per-candidate register (at most 32 per lane).  The
// registers are reduced over the wave once, when the workgroup has walked all its tiles, and written to the workspace as one partial per
// (workgroup, slot); a second kernel adds the partials of a slot and adds the total to out (Guideline 12's store-and-sum).  Integer sums: the
// result does not depend on the tiles, the workgroups or the calls the voxels are split into.  When P x (C-1) exceeds the LDS stage
// (TN_STAGE_MAX floats per voxel: binary models up to 256 passes), the differences are read from global memory per candidate instead.
//
// Binary models (C = 2), with d_t = z_other - z_y and delta = min_t d_t, one exp and one reciprocal per (voxel, candidate, pass):
//   delta > 0  (every pass prefers the other class; p_t may all underflow):  v_t = exp(beta (delta - d_t)) in (0, 1], g = exp(-beta delta)
//              p_t = g v_t / (1 + g v_t)  ->  l = beta delta - log( (1/P) sum_t v_t / (1 + g v_t) ),  the sum >= 1 / (2P)
//   delta <= 0 (some pass has p_t >= 1/2):  E_t = exp(-beta d_t),  1 - p_t = 1 / (1 + E_t)  ->  l = -log1p( -(1/P) sum_t 1 / (1 + E_t) )
// Both forms add non-negative quantities only, so l keeps its relative accuracy from 0 up to the clamp.
// More classes: a_t = -LSE_c(beta d_{t,c}) (the argmax class' term taken out of the sum, log1p of the rest), m = max_t a_t,
//   l = -m - log1p( (1/P) sum_t expm1(a_t - m) )  (two sweeps over the passes).
#include "../../include/rcu.h"
#include "rcu_kernels.h"

#include <cmath>
#include <string>

namespace rcu {
namespace {

constexpr int TN_THREADS = 256;         // 4 waves
constexpr int TN_TILE = 64;             // voxels per tile: one per lane
constexpr int TN_WAVES = TN_THREADS / 64;
constexpr int TN_PER_WAVE = (TN_MAX_CANDIDATES + TN_WAVES - 1) / TN_WAVES;   // candidates a wave owns (k = wave + 4 j)
constexpr int TN_STAGE_MAX = 256;       // LDS stage: floats per voxel (64 KB per workgroup)
constexpr unsigned TN_MAX_GROUPS = 2048;
constexpr float TN_CLAMP = 4096.f;
constexpr float TN_SCALE = 1048576.f;   // 2^20
constexpr size_t TN_MAX_VOXELS = 0xFFFFFFFFull;   // per call: voxel indices are 32-bit

struct Betas {
    float b[TN_MAX_CANDIDATES];
};

struct NllArgs {
    const float* logits;     // [P][n][C][hw]
    const uint8_t* target;   // [n][hw]
    const uint8_t* mask;     // [n][hw] or null
    unsigned nvox, hw;
    unsigned n;
    int P, C, K;
};

__device__ inline float load_d(const NllArgs& a, unsigned i, unsigned pix, int y, int t, int cc)
{
    // cc-th class other than y (cc < C - 1)
    const int c = cc + (cc >= y);
    const float* base = a.logits + ((size_t)t * a.n + i) * a.C * a.hw + pix;
    return base[(size_t)c * a.hw] - base[(size_t)y * a.hw];
}

// the differences of pass t, other class cc of the lane's voxel: from the LDS stage or from global memory
template <bool STAGED>
__device__ inline float get_d(const NllArgs& a, const float* stage, int lane, unsigned i, unsigned pix, int y, int t, int cc)
{
    if (STAGED) return stage[(t * (a.C - 1) + cc) * TN_TILE + lane];
    return load_d(a, i, pix, y, t, cc);
}

// l of a binary voxel at beta; delta = min_t d_t
template <bool STAGED>
__device__ inline float term_binary(const NllArgs& a, const float* stage, int lane, unsigned i, unsigned pix, int y, float delta, float beta)
{
    const bool against = delta > 0.f;
    const float shift = against ? delta : 0.f;
    const float g = against ? __expf(-beta * delta) : 1.f;
    float A = 0.f, R = 0.f;
    for (int t = 0; t < a.P; ++t) {
        const float d = get_d<STAGED>(a, stage, lane, i, pix, y, t, 0);
        const float v = __expf(beta * (shift - d));
        const float r = __builtin_amdgcn_rcpf(fmaf(g, v, 1.f));
        A = fmaf(v, r, A);
        R += r;
    }
    const float invP = 1.f / (float)a.P;
    return against ? fmaf(beta, delta, -logf(A * invP)) : -log1pf(-R * invP);
}

// -LSE_c(beta d_{t,c}) over all classes (d_y = 0) of pass t
template <bool STAGED>
__device__ inline float log_p_pass(const NllArgs& a, const float* stage, int lane, unsigned i, unsigned pix, int y, int t, float beta)
{
    float mx = 0.f;
    int arg = -1;     // -1: class y
    for (int cc = 0; cc < a.C - 1; ++cc) {
        const float s = beta * get_d<STAGED>(a, stage, lane, i, pix, y, t, cc);
        if (s > mx) { mx = s; arg = cc; }
    }
    float u = arg >= 0 ? expf(-mx) : 0.f;    // class y's term when it is not the argmax
    for (int cc = 0; cc < a.C - 1; ++cc)
        if (cc != arg) u += expf(beta * get_d<STAGED>(a, stage, lane, i, pix, y, t, cc) - mx);
    return -(mx + log1pf(u));
}

template <bool STAGED>
__device__ inline float term_general(const NllArgs& a, const float* stage, int lane, unsigned i, unsigned pix, int y, float beta)
{
    float m = -INFINITY;
    for (int t = 0; t < a.P; ++t) m = fmaxf(m, log_p_pass<STAGED>(a, stage, lane, i, pix, y, t, beta));
    float s = 0.f;
    for (int t = 0; t < a.P; ++t) s += expm1f(log_p_pass<STAGED>(a, stage, lane, i, pix, y, t, beta) - m);
    return -m - log1pf(s / (float)a.P);
}

template <bool STAGED, bool BINARY>
__device__ inline float voxel_term(const NllArgs& a, const float* stage, int lane, unsigned i, unsigned pix, int y, float delta, float beta)
{
    if (BINARY) return term_binary<STAGED>(a, stage, lane, i, pix, y, delta, beta);
    return term_general<STAGED>(a, stage, lane, i, pix, y, beta);
}

__device__ inline unsigned long long fixed_point(float l)
{
    l = fminf(fmaxf(l, 0.f), TN_CLAMP);
    return (unsigned long long)rintf(l * TN_SCALE);     // exact: l * 2^20 <= 2^32, rounded to nearest, ties to even
}

__device__ inline unsigned long long wave_sum(unsigned long long x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// BINARY: C == 2.  TERMS: K == 1, write the float l of every voxel (0 outside the mask or with an invalid target) to terms[] instead of summing.
template <bool STAGED, bool BINARY, bool TERMS>
__global__ __launch_bounds__(TN_THREADS) void temperature_nll_kernel(NllArgs a, Betas betas, unsigned long long* __restrict__ partials,
                                                                     float* __restrict__ terms)
{
    extern __shared__ float stage[];     // [P * (C - 1)][TN_TILE] when STAGED
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per_voxel = a.P * (a.C - 1);
    unsigned long long acc[TN_PER_WAVE];
#pragma unroll
    for (int j = 0; j < TN_PER_WAVE; ++j) acc[j] = 0;
    unsigned long long valid = 0, invalid = 0;
    const unsigned tiles = (unsigned)(((size_t)a.nvox + TN_TILE - 1) / TN_TILE);
    for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t v64 = (size_t)tile * TN_TILE + lane;
        const unsigned v = (unsigned)v64;
        const bool inside = v64 < a.nvox && (a.mask == nullptr || a.mask[v] != 0);
        const int y = inside ? (int)a.target[v] : 0;
        const bool active = inside && y < a.C;
        const unsigned i = v / a.hw, pix = v - i * a.hw;
        if (wave == 0) {
            valid += active;
            invalid += inside && !active;
        }
        if (STAGED) {
            __syncthreads();             // the previous tile's stage has been read by every wave
            for (int j = wave; j < per_voxel; j += TN_WAVES) {
                const int t = j / (a.C - 1), cc = j - t * (a.C - 1);
                stage[j * TN_TILE + lane] = active ? load_d(a, i, pix, y, t, cc) : 0.f;
            }
            __syncthreads();
        }
        float delta = 0.f;
        if (BINARY && active) {
            delta = INFINITY;
            for (int t = 0; t < a.P; ++t) delta = fminf(delta, get_d<STAGED>(a, stage, lane, i, pix, y, t, 0));
        }
#pragma unroll
        for (int j = 0; j < TN_PER_WAVE; ++j) {
            const int k = wave + TN_WAVES * j;
            if (k >= a.K) break;         // uniform over the wave
            if (active) {
                const float l = voxel_term<STAGED, BINARY>(a, stage, lane, i, pix, y, delta, betas.b[k]);
                if (TERMS)
                    terms[v] = l;
                else
                    acc[j] += fixed_point(l);
            } else if (TERMS && v64 < a.nvox) {
                terms[v] = 0.f;
            }
        }
    }
    if (TERMS) return;
    const int slots = a.K + 2;
    unsigned long long* out = partials + (size_t)blockIdx.x * slots;
#pragma unroll
    for (int j = 0; j < TN_PER_WAVE; ++j) {
        const int k = wave + TN_WAVES * j;
        if (k >= a.K) break;
        const unsigned long long s = wave_sum(acc[j]);
        if (lane == 0) out[k] = s;
    }
    if (wave == 0) {
        const unsigned long long sv = wave_sum(valid), si = wave_sum(invalid);
        if (lane == 0) {
            out[a.K] = sv;
            out[a.K + 1] = si;
        }
    }
}

// one workgroup per slot: out[slot] += sum over the workgroups' partials
__global__ __launch_bounds__(TN_THREADS) void temperature_sum_kernel(const unsigned long long* __restrict__ partials, unsigned groups, int slots,
                                                                     unsigned long long* __restrict__ out)
{
    __shared__ unsigned long long wave_part[TN_WAVES];
    const int slot = blockIdx.x, tid = threadIdx.x;
    unsigned long long s = 0;
    for (unsigned g = tid; g < groups; g += TN_THREADS) s += partials[(size_t)g * slots + slot];
    s = wave_sum(s);
    if ((tid & 63) == 0) wave_part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned long long total = 0;
        for (int w = 0; w < TN_WAVES; ++w) total += wave_part[w];
        atomicAdd(out + slot, total);
    }
}

unsigned groups_for(size_t nvox)
{
    const size_t tiles = (nvox + TN_TILE - 1) / TN_TILE;
    return (unsigned)std::max<size_t>(1, std::min<size_t>(tiles, TN_MAX_GROUPS));
}

template <bool BINARY, bool TERMS>
void launch_as(const NllArgs& a, const Betas& b, unsigned long long* partials, float* terms, hipStream_t stream)
{
    const unsigned groups = groups_for(a.nvox);
    const int per_voxel = a.P * (a.C - 1);
    if (per_voxel <= TN_STAGE_MAX) {
        const size_t lds = (size_t)per_voxel * TN_TILE * sizeof(float);
        hipLaunchKernelGGL((temperature_nll_kernel<true, BINARY, TERMS>), dim3(groups), dim3(TN_THREADS), lds, stream, a, b, partials, terms);
    } else {
        hipLaunchKernelGGL((temperature_nll_kernel<false, BINARY, TERMS>), dim3(groups), dim3(TN_THREADS), 0, stream, a, b, partials, terms);
    }
}

template <bool TERMS>
hipError_t launch(const NllArgs& a, const Betas& b, unsigned long long* partials, float* terms, hipStream_t stream)
{
    if (a.C == 2)
        launch_as<true, TERMS>(a, b, partials, terms, stream);
    else
        launch_as<false, TERMS>(a, b, partials, terms, stream);
    return hipGetLastError();
}

int check_args(const char* fn, const float* logits, int passes, size_t n, size_t hw, int C, const uint8_t* target)
{
    if (!logits || !target) return report_error(RCU_ERR_INVALID, std::string(fn) + ": null argument");
    if (C < 2 || C > 8) return report_error(RCU_ERR_INVALID, std::string(fn) + ": nb_classes must be in 2..8, got " + std::to_string(C));
    if (passes < 1 || passes > RCU_MC_EXACT_MAX_PASSES)
        return report_error(RCU_ERR_INVALID, std::string(fn) + ": passes must be in 1.." + std::to_string(RCU_MC_EXACT_MAX_PASSES) + ", got " +
                                                 std::to_string(passes));
    if (n < 1 || hw < 1) return report_error(RCU_ERR_INVALID, std::string(fn) + ": empty batch (n, hw >= 1)");
    if (hw > TN_MAX_VOXELS || n > TN_MAX_VOXELS / hw)
        return report_error(RCU_ERR_INVALID, std::string(fn) + ": more than 2^32 - 1 voxels in one call");
    return RCU_OK;
}

bool valid_beta(float b) { return std::isfinite(b) && b > 0.f; }

}  // namespace

size_t temperature_nll_workspace_bytes(size_t voxels, int n_candidates)
{
    return (size_t)groups_for(voxels) * (size_t)(std::max(n_candidates, 1) + 2) * sizeof(unsigned long long);
}

}  // namespace rcu

using namespace rcu;

extern "C" size_t rcu_temperature_nll_workspace_bytes(size_t voxels, int n_candidates)
{
    return temperature_nll_workspace_bytes(voxels, n_candidates);
}

extern "C" int rcu_temperature_nll(const float* logits_dev, int passes, size_t n, size_t hw, int nb_classes, const uint8_t* target_dev,
                                   const uint8_t* mask_dev, const float* beta_host, int n_candidates, uint64_t* out_dev, void* workspace_dev,
                                   void* stream)
{
    if (int st = check_args("rcu_temperature_nll", logits_dev, passes, n, hw, nb_classes, target_dev)) return st;
    if (!beta_host || !out_dev || !workspace_dev) return report_error(RCU_ERR_INVALID, "rcu_temperature_nll: null argument");
    if (n_candidates < 1 || n_candidates > TN_MAX_CANDIDATES)
        return report_error(RCU_ERR_INVALID, "rcu_temperature_nll: n_candidates must be in 1.." + std::to_string(TN_MAX_CANDIDATES) + ", got " +
                                                 std::to_string(n_candidates));
    Betas b{};
    for (int k = 0; k < n_candidates; ++k) {
        if (!valid_beta(beta_host[k]))
            return report_error(RCU_ERR_INVALID, "rcu_temperature_nll: beta[" + std::to_string(k) + "] is not a finite positive number");
        b.b[k] = beta_host[k];
    }
    const NllArgs a{logits_dev, target_dev, mask_dev, (unsigned)(n * hw), (unsigned)hw, (unsigned)n, passes, nb_classes, n_candidates};
    const hipStream_t s = static_cast<hipStream_t>(stream);
    auto* partials = static_cast<unsigned long long*>(workspace_dev);
    hipError_t e = launch<false>(a, b, partials, nullptr, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(temperature_sum_kernel, dim3(n_candidates + 2), dim3(TN_THREADS), 0, s, partials, groups_for(n * hw), n_candidates + 2,
                           reinterpret_cast<unsigned long long*>(out_dev));
        e = hipGetLastError();
    }
    if (e != hipSuccess) return report_error(RCU_ERR_HIP, std::string("rcu_temperature_nll: ") + hipGetErrorString(e));
    return RCU_OK;
}

extern "C" int rcu_temperature_nll_terms(const float* logits_dev, int passes, size_t n, size_t hw, int nb_classes, const uint8_t* target_dev,
                                         const uint8_t* mask_dev, float beta, float* terms_dev, void* stream)
{
    if (int st = check_args("rcu_temperature_nll_terms", logits_dev, passes, n, hw, nb_classes, target_dev)) return st;
    if (!terms_dev) return report_error(RCU_ERR_INVALID, "rcu_temperature_nll_terms: null argument");
    if (!valid_beta(beta)) return report_error(RCU_ERR_INVALID, "rcu_temperature_nll_terms: beta is not a finite positive number");
    Betas b{};
    b.b[0] = beta;
    const NllArgs a{logits_dev, target_dev, mask_dev, (unsigned)(n * hw), (unsigned)hw, (unsigned)n, passes, nb_classes, 1};
    hipError_t e = launch<true>(a, b, nullptr, terms_dev, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return report_error(RCU_ERR_HIP, std::string("rcu_temperature_nll_terms: ") + hipGetErrorString(e));
    return RCU_OK;
}
