// Per-voxel arithmetic shared by the head kernel (rcu_pointwise.hip) and the head fused into the Winograd epilogue of
// conv_cls.0 (rcu_wino.hip): softmax, entropy, the update of the MC statistics planes.  Same functions, same bits.
#pragma once
#include "rcu_kernels.h"

namespace rcu {

// ------------------------------------------------------------------------------- shared device helpers
template <int C>
__device__ __forceinline__ void softmax_inplace(float (&l)[C])
{
    float mx = l[0];
#pragma unroll
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, l[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        l[c] = expf(l[c] - mx);
        s += l[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) l[c] = l[c] / s;
}

template <int C>
__device__ __forceinline__ float entropy_of(const float (&p)[C])
{
    float h = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) h += (p[c] > 0.f) ? p[c] * logf(p[c]) : 0.f;
    return -h;
}

// ---- float64 statistics (MC_VAR and / or MC_EXACT): planes [sum p_c (C)] [sum p_c^2 (C) if MC_VAR] [sum H if MC_MI]
__device__ __forceinline__ bool mc_is_f64(int flags) { return (flags & (MC_VAR | MC_EXACT)) != 0; }
__device__ __forceinline__ int mc_h_plane(int flags, int C) { return (flags & MC_VAR) ? 2 * C : C; }   // float64 layouts only

// MC_EXACT: every addend is rounded (to nearest even) to a multiple of 2^-40 before it is added -- 1.5 * 2^12 has the float64 ulp 2^-40
// and x + 6144 stays inside [4096, 8192) for the addends here (p, p^2 <= 1, H <= log 8), so the sum of the two roundings is that multiple
// exactly.  Sums of multiples of 2^-40 below 2^13 are representable in float64's 53 bits: every addition is EXACT, hence associative and
// commutative -- the statistics of T <= 2048 passes carry the same bits whatever the order, the pass groups, the stream lanes, the ranks
// and the reduction tree of the collective that merges them.  (No fast-math: hipcc does not reassociate (x + c) - c away; the GPU test
// test_exact_statistics_* checks the quantum.)
__device__ __forceinline__ double mc_quantise(double x)
{
    const double shifted = __dadd_rn(x, 6144.0);
    return __dsub_rn(shifted, 6144.0);
}

template <int C>
__device__ __forceinline__ void accumulate_voxel(void* stats, size_t v, size_t V, int flags, const float (&p)[C])
{
    if (mc_is_f64(flags)) {
        double* sd = reinterpret_cast<double*>(stats);
        const bool exact = (flags & MC_EXACT) != 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double pc = (double)p[c];
            sd[(size_t)c * V + v] += exact ? mc_quantise(pc) : pc;
            if (flags & MC_VAR) sd[(size_t)(C + c) * V + v] += exact ? mc_quantise(pc * pc) : pc * pc;
        }
        if (flags & MC_MI) {
            const double h = (double)entropy_of<C>(p);
            sd[(size_t)mc_h_plane(flags, C) * V + v] += exact ? mc_quantise(h) : h;
        }
    } else {
        float* sf = reinterpret_cast<float*>(stats);
#pragma unroll
        for (int c = 0; c < C; ++c) sf[(size_t)c * V + v] += p[c];
        if (flags & MC_MI) sf[(size_t)C * V + v] += entropy_of<C>(p);
    }
}

// The statistics entries of one voxel held in registers across the passes of a group: load, add pass after pass in
// the same order and with the same operations as accumulate_voxel, store -- bit-identical to one launch per pass.
template <int C>
struct VoxelStats {
    double d[2 * C + 1];      // [sum p_c] [sum p_c^2] [sum H], whatever the planes of the blob
    float f[C + 1];
    __device__ __forceinline__ void load(const void* stats, size_t v, size_t V, int flags)
    {
        if (mc_is_f64(flags)) {
            const double* sd = reinterpret_cast<const double*>(stats);
#pragma unroll
            for (int k = 0; k < C; ++k) d[k] = sd[(size_t)k * V + v];
#pragma unroll
            for (int k = 0; k < C; ++k) d[C + k] = (flags & MC_VAR) ? sd[(size_t)(C + k) * V + v] : 0.0;
            d[2 * C] = (flags & MC_MI) ? sd[(size_t)mc_h_plane(flags, C) * V + v] : 0.0;
        } else {
            const float* sf = reinterpret_cast<const float*>(stats);
#pragma unroll
            for (int k = 0; k < C; ++k) f[k] = sf[(size_t)k * V + v];
            f[C] = (flags & MC_MI) ? sf[(size_t)C * V + v] : 0.f;
        }
    }
    __device__ __forceinline__ void add(int flags, const float (&p)[C])
    {
        if (mc_is_f64(flags)) {
            const bool exact = (flags & MC_EXACT) != 0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const double pc = (double)p[c];
                d[c] += exact ? mc_quantise(pc) : pc;
                if (flags & MC_VAR) d[C + c] += exact ? mc_quantise(pc * pc) : pc * pc;
            }
            if (flags & MC_MI) {
                const double h = (double)entropy_of<C>(p);
                d[2 * C] += exact ? mc_quantise(h) : h;
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) f[c] += p[c];
            if (flags & MC_MI) f[C] += entropy_of<C>(p);
        }
    }
    __device__ __forceinline__ void store(void* stats, size_t v, size_t V, int flags) const
    {
        if (mc_is_f64(flags)) {
            double* sd = reinterpret_cast<double*>(stats);
#pragma unroll
            for (int k = 0; k < C; ++k) sd[(size_t)k * V + v] = d[k];
            if (flags & MC_VAR) {
#pragma unroll
                for (int k = 0; k < C; ++k) sd[(size_t)(C + k) * V + v] = d[C + k];
            }
            if (flags & MC_MI) sd[(size_t)mc_h_plane(flags, C) * V + v] = d[2 * C];
        } else {
            float* sf = reinterpret_cast<float*>(stats);
#pragma unroll
            for (int k = 0; k < C; ++k) sf[(size_t)k * V + v] = f[k];
            if (flags & MC_MI) sf[(size_t)C * V + v] = f[C];
        }
    }
};

// ------------------------------------------------------------------------------- counter-based random numbers
// Philox4x32-10 (Salmon et al., SC'11) under key (k0, k1) at the 128-bit counter (c0, c1, c2, c3).  The dropout masks draw with c2 = c3 = 0
// (rcu_pointwise.hip, dropout_masks_kernel); the logit noise below sets bit 31 of c3, so the two never share a counter under one key.
__device__ __forceinline__ void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t (&out)[4])
{
    uint32_t c[4] = {c0, c1, c2, c3};
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n1 = lo1, n2 = hi0 ^ c[3] ^ k1, n3 = lo0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
}

// ------------------------------------------------------------------------------- test-time logit sampling (sigma-head models)
// include/rcu.h "Test-time logit sampling".  The normal z of (key K, slice g, pixel p, sample s, class c), j = s * C + c, is element j & 3 of
// the block j >> 2: Philox4x32-10 under (K lo, K hi) at counter (p, g lo, g hi, 2^31 | j >> 2) gives four words w, u = ((w >> 8) + 0.5f) * 2^-24
// in float32, and Box-Muller turns (u0, u1) into the block's elements 0 and 1 (r cos, r sin) and (u2, u3) into 2 and 3.
__device__ __forceinline__ void logit_normals4(unsigned long long key, unsigned long long g, uint32_t p, uint32_t q, float (&z)[4])
{
    uint32_t w[4];
    philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), p, (uint32_t)g, (uint32_t)(g >> 32), 0x80000000u | q, w);
    float u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = ((float)(w[i] >> 8) + 0.5f) * 5.9604644775390625e-8f;     // 2^-24
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float r = sqrtf(-2.f * logf(u[2 * k]));
        float sn, cs;
        sincospif(2.f * u[2 * k + 1], &sn, &cs);
        z[2 * k] = r * cs;
        z[2 * k + 1] = r * sn;
    }
}

// l: the logits mu in, the sampled predictive p_bar = (1/S) sum_s softmax(mu + sig * z_s) out (float32 sums in sample order).
// sig: the voxel's sigma (|raw| or exp(raw)).  S, g and key are the same on every lane of a wave: the branches below are uniform.
template <int C>
__device__ __forceinline__ void logit_sample_predictive(float (&l)[C], const float (&sig)[C], unsigned long long key, unsigned long long g,
                                                        uint32_t p, int S)
{
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t block = 0xFFFFFFFFu;
    for (int s = 0; s < S; ++s) {
        float x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const uint32_t j = (uint32_t)(s * C + c);
            if ((j >> 2) != block) {
                block = j >> 2;
                logit_normals4(key, g, p, block, z);
            }
            const uint32_t e = j & 3u;
            const float zj = e == 0 ? z[0] : e == 1 ? z[1] : e == 2 ? z[2] : z[3];
            x[c] = fmaf(sig[c], zj, l[c]);
        }
        softmax_inplace<C>(x);
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += x[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) l[c] = acc[c] / (float)S;
}

// sigma of a raw sigma-head output: what rcu_aleatoric writes and the sigma sums add
__device__ __forceinline__ float sigma_of_raw(float raw, int is_log_sigma) { return is_log_sigma ? expf(raw) : fabsf(raw); }


}  // namespace rcu
