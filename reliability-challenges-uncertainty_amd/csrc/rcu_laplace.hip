// Last-layer Laplace (include/rcu.h "Last-layer Laplace"): the two kernels of the GGN fit and the probit predictive on the classifier's input, both
// on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain, one rounding per product), in the forms of rcu_density.hip.
//
// laplace_moments_kernel -- the curvature-weighted Gram matrix of a slice, G_q = sum_v omega_q(v) psi psi^T for the class pairs q = (c, c'), c <= c'.
//   The lane map is density_moments_kernel's: lane (i = lane % 32, h = lane / 32) holds channel i of voxel 2 t + h in ONE register that is the A
//   operand as it is and, multiplied once by omega_q of its voxel (__fmul_rn), the B operand of pair q.  The features are read once for up to QC
//   pairs (four, two above 32 channels; one launch per pass, the pairs' classes compile-time); a voxel's C probabilities are read once per pass, one
//   broadcast dword per class and lane half, and omega is computed with __fmul_rn / __fsub_rn: no contraction, numpy's float32 bits.  One WAVE
//   owns one chunk of RCU_DENSITY_CHUNK voxels of one slice, accumulates it in float32 (the MFMA chain for G; for S and w the voxels of even and of
//   odd index apart, one add per voxel), and leaves the chunk's sums in the workspace.  laplace_finalize_kernel promotes them and adds the chunks of
//   a slice in float64, in chunk order.  No atomics, nothing depends on n, the slice's position, the alignment or the launch geometry.
// laplace_predict_kernel -- s2_c = |A_c psi - b_c|^2 + kappa_c exactly as density_energy_kernel computes d2_c (weights as A, 32 voxels as B, the
//   accumulator started at -b_c, the squares added in register order, one exchange with lane ^ 32), for all C classes from one read of the features;
//   then the probit link, the project's softmax (rcu_head_common.h), the first maximum.  Lane half 0 of a voxel stores the probabilities and the
//   prediction, half 1 the standard deviations: both halves hold the same values.
#include "rcu_head_common.h"
#include "rcu_kernels.h"

#include <cmath>
#include <type_traits>

namespace rcu {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LM_CHUNK = RCU_DENSITY_CHUNK;
constexpr int LM_AHEAD = 8;         // steps (voxel pairs) whose loads are in flight together

constexpr int lm_blocks(int cb) { return cb == 1 ? 1 : 3; }
constexpr int lm_pairs(int C) { return C * (C + 1) / 2; }
// floats of one chunk's record: G [P][NB][16][64], S [P][CB][64] (the two voxel parities side by side), w [P][2]; a multiple of 64
constexpr size_t lm_g_floats(int P, int cb) { return (size_t)P * lm_blocks(cb) * 1024; }
constexpr size_t lm_s_floats(int P, int cb) { return (size_t)P * cb * 64; }
constexpr size_t lm_record_floats(int P, int cb) { return (lm_g_floats(P, cb) + lm_s_floats(P, cb) + 2 * (size_t)P + 63) / 64 * 64; }

// the classes (c, c') of pair q, row-major over c <= c'
constexpr int lm_pair_first(int C, int q)
{
    int c = 0;
    while (q >= C - c) q -= C - c, ++c;
    return c;
}
constexpr int lm_pair_second(int C, int q)
{
    int c = 0;
    while (q >= C - c) q -= C - c, ++c;
    return c + q;
}

// f(integral_constant<int, K>) for K = 0 .. N - 1: the index is a constant expression inside f
template <int K, int N, typename Fn>
__device__ __forceinline__ void static_for(Fn&& f)
{
    if constexpr (K < N) {
        f(std::integral_constant<int, K>{});
        static_for<K + 1, N>(f);
    }
}

// PASS: the pairs PASS * QC .. PASS * QC + QC - 1 (a launch per pass: the pairs' classes are compile-time, every array stays in registers)
template <int CB, int QC, int C, int PASS>
__global__ __launch_bounds__(256) void laplace_moments_kernel(const float* __restrict__ x, int pitch, int F, const float* __restrict__ probs,
                                                              size_t total, unsigned hw, unsigned chunks, float* __restrict__ records,
                                                              size_t record_floats)
{
    constexpr int NB = lm_blocks(CB), P = lm_pairs(C);
    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= total) return;
    const size_t s = w / chunks;
    const unsigned q = (unsigned)(w % chunks);
    constexpr int q0 = PASS * QC;
    const unsigned v0 = q * LM_CHUNK, v1 = v0 + LM_CHUNK < hw ? v0 + LM_CHUNK : hw;
    const float* xs = x + s * (size_t)hw * pitch + i;
    const float* ps = probs + s * (size_t)C * hw;
    bool on[CB];
#pragma unroll
    for (int ib = 0; ib < CB; ++ib) on[ib] = i + 32 * ib < F;

    f32x16 acc[QC][NB];
    float sacc[QC][CB], wacc[QC];
#pragma unroll
    for (int k = 0; k < QC; ++k) {
        wacc[k] = 0.f;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[k][nb][r] = 0.f;
#pragma unroll
        for (int ib = 0; ib < CB; ++ib) sacc[k][ib] = 0.f;
    }
    // LM_AHEAD steps per trip, their loads issued together in front of the MFMAs; the steps are consumed in voxel order, so the sums are those of
    // the one-step loop.  A voxel beyond the chunk has omega = 0 and features 0: it adds +-0 to sums that start at +0, which changes no bit.
    for (unsigned t0 = v0; t0 < v1; t0 += 2 * LM_AHEAD) {
        float pv[LM_AHEAD][C];
        float a[LM_AHEAD][CB];
        bool ok[LM_AHEAD];
#pragma unroll
        for (int u = 0; u < LM_AHEAD; ++u) {
            const unsigned v = t0 + 2 * u + h;
            ok[u] = v < v1;
#pragma unroll
            for (int c = 0; c < C; ++c) pv[u][c] = ok[u] ? ps[(size_t)c * hw + v] : 0.f;
#pragma unroll
            for (int ib = 0; ib < CB; ++ib) a[u][ib] = (ok[u] && on[ib]) ? xs[(size_t)v * pitch + 32 * ib] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < LM_AHEAD; ++u) {
            static_for<0, (P - q0 < QC ? P - q0 : QC)>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                constexpr int ca = lm_pair_first(C, q0 + k), cb = lm_pair_second(C, q0 + k);
                const float p1 = pv[u][ca], p2 = pv[u][cb];
                float om = ca == cb ? __fmul_rn(p1, __fsub_rn(1.f, p1)) : -__fmul_rn(p1, p2);
                om = ok[u] ? om : 0.f;
                float bm[CB];
#pragma unroll
                for (int ib = 0; ib < CB; ++ib) {
                    bm[ib] = __fmul_rn(om, a[u][ib]);
                    sacc[k][ib] = __fadd_rn(sacc[k][ib], bm[ib]);
                }
                wacc[k] = __fadd_rn(wacc[k], om);
                acc[k][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][0], bm[0], acc[k][0], 0, 0, 0);
                if constexpr (CB == 2) {
                    acc[k][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][0], bm[1], acc[k][1], 0, 0, 0);
                    acc[k][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][1], bm[1], acc[k][2], 0, 0, 0);
                }
            });
        }
    }
    float* rec = records + w * record_floats;
    float* rec_s = rec + lm_g_floats(P, CB);
    float* rec_w = rec_s + lm_s_floats(P, CB);
#pragma unroll
    for (int k = 0; k < QC; ++k) {
        if (q0 + k >= P) continue;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) rec[(((size_t)(q0 + k) * NB + nb) * 16 + r) * 64 + lane] = acc[k][nb][r];
#pragma unroll
        for (int ib = 0; ib < CB; ++ib) rec_s[((q0 + k) * CB + ib) * 64 + lane] = sacc[k][ib];
        if (i == 0) rec_w[(q0 + k) * 2 + h] = wacc[k];
    }
}

// one thread per output entry of a slice: the chunks' float32 sums promoted and added in float64 in chunk order (even voxels' sum, then odd)
template <int CB>
__global__ __launch_bounds__(256) void laplace_finalize_kernel(const float* __restrict__ records, size_t record_floats, unsigned chunks, int P, int F,
                                                               unsigned blocks_per_slice, double* __restrict__ w_out, double* __restrict__ S_out,
                                                               double* __restrict__ G_out)
{
    constexpr int NB = lm_blocks(CB);
    const size_t s = blockIdx.x / blocks_per_slice;
    const size_t e = (size_t)(blockIdx.x % blocks_per_slice) * 256 + threadIdx.x;
    const size_t EG = (size_t)P * NB * 1024, ES = (size_t)P * CB * 32;
    const float* rec = records + s * chunks * record_floats;
    if (e < EG) {
        const int c = (int)(e / (NB * 1024)), nb = (int)(e / 1024) % NB, r = (int)(e >> 6) & 15, lane = (int)e & 63;
        const int ib = nb == 2 ? 1 : 0, jb = nb == 0 ? 0 : 1;
        const int i = 32 * ib + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3), j = 32 * jb + (lane & 31);
        if (i >= F || j >= F) return;
        // the diagonal blocks are computed in full; the upper triangle is kept and mirrored, so the two triangles carry the same bits
        if (nb != 1 && j < i) return;
        double sum = 0.0;
        for (unsigned q = 0; q < chunks; ++q) sum += (double)rec[q * record_floats + e];
        double* G = G_out + (s * P + c) * (size_t)F * F;
        G[(size_t)i * F + j] = sum;
        G[(size_t)j * F + i] = sum;
    } else if (e < EG + ES) {
        const int idx = (int)(e - EG), c = idx / (CB * 32), ch = idx % (CB * 32);
        if (ch >= F) return;
        const size_t at = EG + (size_t)(c * CB + ch / 32) * 64 + ch % 32;
        double sum = 0.0;
        for (unsigned q = 0; q < chunks; ++q) {
            sum += (double)rec[q * record_floats + at];
            sum += (double)rec[q * record_floats + at + 32];
        }
        S_out[(s * P + c) * (size_t)F + ch] = sum;
    } else if (e < EG + ES + P) {
        const int c = (int)(e - EG - ES);
        const size_t at = EG + 2 * ES + 2 * (size_t)c;
        double sum = 0.0;
        for (unsigned q = 0; q < chunks; ++q) {
            sum += (double)rec[q * record_floats + at];
            sum += (double)rec[q * record_floats + at + 1];
        }
        w_out[s * P + c] = sum;
    }
}

// LDS image per class, as rcu_density.hip: CB x CB weight tiles [cob][cib][j = 0..3][lane][4] (float4 = A_c[32 cob + lane % 32][32 cib + 8 j + 4
// (lane / 32) .. + 3]), then the accumulators' start values [cob][j][h][4] = -b_c[32 cob + 8 j + 4 h .. + 3]; zeros at rows and columns >= F.
// kappa_c follows the classes.
constexpr int lp_class_floats(int cb) { return cb * cb * 1024 + cb * 32; }

struct PredictOut {
    float* probs;        // [n][C][hw]
    float* std;          // [n][C][hw] or null
    float* std_pred;     // [n][hw] or null
    uint8_t* prediction; // [n][hw] or null
};

template <int CB, int C>
__global__ __launch_bounds__(256) void laplace_predict_kernel(const float* __restrict__ x, int pitch, int F, const float* __restrict__ logits,
                                                              size_t nvox, unsigned hw, const float* __restrict__ A, const float* __restrict__ b,
                                                              const float* __restrict__ kappa, const PredictOut out)
{
    extern __shared__ __attribute__((aligned(16))) float lp_smem[];
    constexpr int W_FLOATS = CB * CB * 1024, B_FLOATS = CB * 32, CLS = lp_class_floats(CB);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    for (int e = tid; e < C * W_FLOATS; e += 256) {
        const int c = e / W_FLOATS, rest = e % W_FLOATS, blk = rest >> 10, j = (rest >> 8) & 3, ln = (rest >> 2) & 63, q = rest & 3;
        const int row = 32 * (blk / CB) + (ln & 31), col = 32 * (blk % CB) + 8 * j + 4 * (ln >> 5) + q;
        lp_smem[c * CLS + rest] = (row < F && col < F) ? A[((size_t)c * F + row) * F + col] : 0.f;
    }
    for (int e = tid; e < C * B_FLOATS; e += 256) {
        const int c = e / B_FLOATS, rest = e % B_FLOATS;      // rest = ((cob * 4 + j) * 2 + h) * 4 + q
        const int ch = 32 * (rest >> 5) + 8 * ((rest >> 3) & 3) + 4 * ((rest >> 2) & 1) + (rest & 3);
        lp_smem[c * CLS + W_FLOATS + rest] = ch < F ? -b[(size_t)c * F + ch] : 0.f;
    }
    if (tid < C) lp_smem[C * CLS + tid] = kappa[tid];
    __syncthreads();

    const size_t ngroups = (nvox + 31) / 32;
    const size_t stride = (size_t)gridDim.x * 4;
    size_t g = (size_t)blockIdx.x * 4 + wave;
    if (g >= ngroups) return;

    auto load = [&](size_t grp, f32x4 (&q)[CB][4]) {
        size_t v = grp * 32 + n;
        v = v < nvox ? v : nvox - 1;            // tail lanes read a valid voxel, their results are not stored
        const float* src = x + v * pitch + 4 * h;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ch = 32 * cb + 8 * j + 4 * h;     // ch < F implies ch + 3 < pitch (a multiple of 4 that is >= F)
                f32x4 t = {0.f, 0.f, 0.f, 0.f};
                if (ch < F) {
                    t = *reinterpret_cast<const f32x4*>(src + 32 * cb + 8 * j);
                    t.y = ch + 1 < F ? t.y : 0.f, t.z = ch + 2 < F ? t.z : 0.f, t.w = ch + 3 < F ? t.w : 0.f;
                }
                q[cb][j] = t;
            }
    };
    f32x4 cur[CB][4], nxt[CB][4];
    load(g, cur);
    for (; g < ngroups; g += stride) {
        const bool more = g + stride < ngroups;
        load(more ? g + stride : g, nxt);       // next group's features are in flight during this group's MFMAs
        const size_t v = g * 32 + n;
        const bool live = v < nvox;
        const size_t vc = live ? v : nvox - 1;
        const size_t img = nvox <= 0xFFFFFFFFull ? (size_t)((unsigned)vc / hw) : vc / hw;
        const size_t base = img * (size_t)C * hw + (vc - img * hw);     // class 0 of the voxel in an [n][C][hw] tensor
        float z[C];
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = logits[base + (size_t)c * hw];
        f32x16 act[CB];
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                act[cb][4 * j + 0] = cur[cb][j].x, act[cb][4 * j + 1] = cur[cb][j].y, act[cb][4 * j + 2] = cur[cb][j].z,
                               act[cb][4 * j + 3] = cur[cb][j].w;
            }
        float s2[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float* wl = lp_smem + (size_t)c * CLS;
            float part = 0.f;
#pragma unroll
            for (int cob = 0; cob < CB; ++cob) {
                f32x16 acc;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(wl + W_FLOATS + ((cob * 4 + j) * 2 + h) * 4);
                    acc[4 * j + 0] = b4.x, acc[4 * j + 1] = b4.y, acc[4 * j + 2] = b4.z, acc[4 * j + 3] = b4.w;
                }
#pragma unroll
                for (int cib = 0; cib < CB; ++cib)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x4 a = *reinterpret_cast<const f32x4*>(wl + (((cob * CB + cib) * 4 + j) * 64 + lane) * 4);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, act[cib][4 * j + 0], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, act[cib][4 * j + 1], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, act[cib][4 * j + 2], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, act[cib][4 * j + 3], acc, 0, 0, 0);
                    }
#pragma unroll
                for (int r = 0; r < 16; ++r) part = fmaf(acc[r], acc[r], part);
            }
            const float other = __shfl_xor(part, 32);
            const float d2 = h == 0 ? __fadd_rn(part, other) : __fadd_rn(other, part);      // rows of half 0 first, in both lanes
            s2[c] = __fadd_rn(d2, lp_smem[C * CLS + c]);
        }
        float sd[C], p[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float t = fmaf(0.39269908169872414f, s2[c], 1.0f);      // (float)(pi / 8)
            p[c] = __fdiv_rn(z[c], __fsqrt_rn(t));
            sd[c] = __fsqrt_rn(s2[c]);
        }
        softmax_inplace<C>(p);
        int best = 0;
        float best_p = p[0], best_sd = sd[0];
#pragma unroll
        for (int c = 1; c < C; ++c) {
            const bool up = p[c] > best_p;      // strictly: the first maximum stays
            best = up ? c : best, best_p = up ? p[c] : best_p, best_sd = up ? sd[c] : best_sd;
        }
        if (live && h == 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) out.probs[base + (size_t)c * hw] = p[c];
            if (out.prediction != nullptr) out.prediction[v] = (uint8_t)best;
        }
        if (live && h == 1) {
            if (out.std != nullptr) {
#pragma unroll
                for (int c = 0; c < C; ++c) out.std[base + (size_t)c * hw] = sd[c];
            }
            if (out.std_pred != nullptr) out.std_pred[v] = best_sd;
        }
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int j = 0; j < 4; ++j) cur[cb][j] = nxt[cb][j];
    }
}

template <int CB, int C>
hipError_t launch_predict(const float* x, int pitch, int F, const float* logits, size_t nvox, unsigned hw, const float* A, const float* b,
                          const float* kappa, const PredictOut& out, hipStream_t stream)
{
    const size_t ngroups = (nvox + 31) / 32;
    const size_t wgs = (ngroups + 3) / 4;
    const unsigned grid = (unsigned)(wgs < 2048 ? wgs : 2048);
    const size_t lds = ((size_t)C * lp_class_floats(CB) + 8) * sizeof(float);
    hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void*>(&laplace_predict_kernel<CB, C>), (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((laplace_predict_kernel<CB, C>), dim3(grid), dim3(256), lds, stream, x, pitch, F, logits, nvox, hw, A, b, kappa, out);
    return hipGetLastError();
}

template <int CB, int QC, int C, int PASS>
hipError_t launch_moment_passes(const float* x, int pitch, int F, const float* probs, size_t total, unsigned hw, unsigned chunks, float* records,
                                size_t rf, hipStream_t stream)
{
    hipLaunchKernelGGL((laplace_moments_kernel<CB, QC, C, PASS>), dim3((unsigned)((total + 3) / 4)), dim3(256), 0, stream, x, pitch, F, probs, total,
                       hw, chunks, records, rf);
    if (hipError_t e = hipGetLastError()) return e;
    if constexpr ((PASS + 1) * QC < lm_pairs(C))
        return launch_moment_passes<CB, QC, C, PASS + 1>(x, pitch, F, probs, total, hw, chunks, records, rf, stream);
    return hipSuccess;
}

template <int CB, int QC, int C>
hipError_t launch_moments(const float* x, int pitch, int F, const float* probs, size_t n, unsigned hw, double* w_out, double* S_out, double* G_out,
                          void* workspace, hipStream_t stream)
{
    constexpr int P = lm_pairs(C);
    const unsigned chunks = (hw + LM_CHUNK - 1) / LM_CHUNK;
    const size_t total = n * chunks, rf = lm_record_floats(P, CB);
    float* records = static_cast<float*>(workspace);
    if (hipError_t e = launch_moment_passes<CB, QC, C, 0>(x, pitch, F, probs, total, hw, chunks, records, rf, stream)) return e;
    const size_t entries = lm_g_floats(P, CB) + (size_t)P * CB * 32 + P;
    const unsigned bps = (unsigned)((entries + 255) / 256);
    hipLaunchKernelGGL(laplace_finalize_kernel<CB>, dim3((unsigned)(n * bps)), dim3(256), 0, stream, records, rf, chunks, P, F, bps, w_out, S_out,
                       G_out);
    return hipGetLastError();
}

int invalid(const char* fn, const std::string& msg) { return report_error(RCU_ERR_INVALID, std::string(fn) + ": " + msg); }

// the contract both kernels share: 1 <= F <= 64, channel_pitch >= F and a multiple of 4, 2 <= C <= 4, 16-byte aligned features
int check_shape(const char* fn, const float* features, int channel_pitch, int F, int C)
{
    if (F < 1 || F > RCU_DENSITY_MAX_FEATURES) return invalid(fn, "F must be in 1..64, got " + std::to_string(F));
    if (channel_pitch < F || channel_pitch % 4) return invalid(fn, "channel_pitch must be >= F and a multiple of 4, got " + std::to_string(channel_pitch));
    if (C < 2 || C > RCU_LAPLACE_MAX_CLASSES) return invalid(fn, "nb_classes must be in 2..4, got " + std::to_string(C));
    if (reinterpret_cast<uintptr_t>(features) % 16) return invalid(fn, "features_dev must be 16-byte aligned");
    return RCU_OK;
}

bool misaligned(const void* p, size_t to) { return reinterpret_cast<uintptr_t>(p) % to != 0; }

}  // namespace
}  // namespace rcu

using namespace rcu;

extern "C" size_t rcu_laplace_moments_workspace_bytes(size_t n, size_t hw, int F, int nb_classes)
{
    if (n < 1 || hw < 1 || F < 1 || F > RCU_DENSITY_MAX_FEATURES || nb_classes < 2 || nb_classes > RCU_LAPLACE_MAX_CLASSES) return 0;
    const size_t chunks = (hw + LM_CHUNK - 1) / LM_CHUNK;
    return round256(n * chunks * lm_record_floats(lm_pairs(nb_classes), F > 32 ? 2 : 1) * sizeof(float));
}

extern "C" int rcu_laplace_moments(const float* features_dev, int channel_pitch, int F, const float* probabilities_dev, size_t n, size_t hw,
                                   int nb_classes, double* w_out_dev, double* S_out_dev, double* G_out_dev, void* workspace_dev, void* stream)
{
    static const char* fn = "rcu_laplace_moments";
    if (!features_dev || !probabilities_dev || !w_out_dev || !S_out_dev || !G_out_dev || !workspace_dev)
        return invalid(fn, "null argument (features_dev, probabilities_dev, w_out_dev, S_out_dev, G_out_dev, workspace_dev)");
    if (int st = check_shape(fn, features_dev, channel_pitch, F, nb_classes)) return st;
    if (n < 1 || n > ((size_t)1 << 20) || hw < 1 || hw > ((size_t)1 << 30)) return invalid(fn, "n must be in 1..2^20 and hw in 1..2^30");
    const size_t chunks = (hw + LM_CHUNK - 1) / LM_CHUNK;
    if (n * chunks > ((size_t)1 << 31) - 4) return invalid(fn, "n * ceil(hw / RCU_DENSITY_CHUNK) must be below 2^31");
    if (misaligned(probabilities_dev, 4) || misaligned(workspace_dev, 16) || misaligned(w_out_dev, 8) || misaligned(S_out_dev, 8) ||
        misaligned(G_out_dev, 8))
        return invalid(fn, "probabilities_dev must be 4-byte, the outputs 8-byte and workspace_dev 16-byte aligned");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned uhw = (unsigned)hw;
    hipError_t e = hipSuccess;
#define RCU_LM(C_)                                                                                                                         \
    e = F <= 32 ? launch_moments<1, 4, C_>(features_dev, channel_pitch, F, probabilities_dev, n, uhw, w_out_dev, S_out_dev, G_out_dev,     \
                                           workspace_dev, s)                                                                               \
                : launch_moments<2, 2, C_>(features_dev, channel_pitch, F, probabilities_dev, n, uhw, w_out_dev, S_out_dev, G_out_dev,     \
                                           workspace_dev, s)
    if (nb_classes == 2) RCU_LM(2);
    else if (nb_classes == 3) RCU_LM(3);
    else RCU_LM(4);
#undef RCU_LM
    if (e != hipSuccess) return hip_failed(fn, e);
    return RCU_OK;
}

extern "C" int rcu_laplace_predict(const float* features_dev, int channel_pitch, int F, const float* logits_dev, size_t n, size_t hw, int nb_classes,
                                   const float* A_dev, const float* b_dev, const float* kappa_dev, float* probabilities_dev, float* std_dev,
                                   float* std_pred_dev, uint8_t* prediction_dev, void* stream)
{
    static const char* fn = "rcu_laplace_predict";
    if (!features_dev || !logits_dev || !A_dev || !b_dev || !kappa_dev || !probabilities_dev)
        return invalid(fn, "null argument (features_dev, logits_dev, A_dev, b_dev, kappa_dev, probabilities_dev)");
    if (int st = check_shape(fn, features_dev, channel_pitch, F, nb_classes)) return st;
    if (n < 1 || n > ((size_t)1 << 20) || hw < 1 || hw > ((size_t)1 << 30)) return invalid(fn, "n must be in 1..2^20 and hw in 1..2^30");
    if (misaligned(logits_dev, 4) || misaligned(A_dev, 4) || misaligned(b_dev, 4) || misaligned(kappa_dev, 4) || misaligned(probabilities_dev, 4) ||
        misaligned(std_dev, 4) || misaligned(std_pred_dev, 4))
        return invalid(fn, "the float arrays must be 4-byte aligned");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const PredictOut out{probabilities_dev, std_dev, std_pred_dev, prediction_dev};
    const size_t nvox = n * hw;
    const unsigned uhw = (unsigned)hw;
    hipError_t e = hipSuccess;
#define RCU_LP(C_)                                                                                                                          \
    e = F <= 32 ? launch_predict<1, C_>(features_dev, channel_pitch, F, logits_dev, nvox, uhw, A_dev, b_dev, kappa_dev, out, s)             \
                : launch_predict<2, C_>(features_dev, channel_pitch, F, logits_dev, nvox, uhw, A_dev, b_dev, kappa_dev, out, s)
    if (nb_classes == 2) RCU_LP(2);
    else if (nb_classes == 3) RCU_LP(3);
    else RCU_LP(4);
#undef RCU_LP
    if (e != hipSuccess) return hip_failed(fn, e);
    return RCU_OK;
}
