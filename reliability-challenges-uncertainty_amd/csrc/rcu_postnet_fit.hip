// Auxiliary fit (include/rcu_fit.h "Auxiliary fit"): the train-mode loss of the PostNet on the U-Net feature map and its gradient, the first
// gradient kernel of the library.  The per-voxel MLP runs on the fp32 matrix cores (v_mfma_f32_32x32x2_f32) in the orientation of rcu_postnet.hip:
// D[cout][voxel] = W[cout][cin] X[cin][voxel], a lane (voxel n = lane % 32, half h = lane / 32) owns the 16 channels perm(r, h) = 8 (r / 4) + 4 h +
// r % 4 of ITS voxel in accumulator element r, and because the k index of an MFMA step is only a label the accumulator of one layer is the B operand
// of the next as it stands.  The backward chain da_{l-1} = W_l^T du_l is the same product with the transposed weight image, so the whole forward
// and backward chain of a group of 32 voxels lives in registers.
//
// Train-mode BatchNorm makes the forward sequential in the layers' statistics and the backward in the per-channel sums of dy and dy xhat, so the
// call is 2 L + 1 passes over phi, each of which recomputes the chain it needs from the 128 bytes it reads per voxel:
//   stats pass l = 1 .. L   u_l from the finished layers below it; sum (u_l - shift_l) and sum (u_l - shift_l)^2      -> mu_l, var_l
//                           (in front of it the same kernel over <= 1024 voxels spread over the batch gives shift_l, see rcu_fit.h; in front of
//                           everything fit_center_kernel gives the centre c of phi over those voxels: the chain runs on phi - c)
//   top pass                loss, dW_o, db_o, and sum dy_L, sum dy_L xhat_L (= dbeta_L, dgamma_L)
//   down pass l = L .. 1    du_l from the sums of layer l; dW_l, db_l; sum dy_{l-1}, sum dy_{l-1} xhat_{l-1}
// Nothing of size N x F is written: a pass leaves one record of float32 sums per chunk, and a finalising kernel adds the records in float64.
//
// The weight gradient dW_l = sum_v du_l(v) a_{l-1}(v)^T contracts over VOXELS: its operands want a lane to own a channel with the voxels along k.
// Both du_l and a_{l-1} cross a wave-local 32 x 32 LDS tile (rows of 33 floats: the column writes and the row reads are both conflict-free), with
// no workgroup barrier: a wave's LDS operations are served in order, the fences only keep the compiler from moving them.
//
// A wave owns one chunk of RCU_DENSITY_CHUNK voxels of one slice (rcu_density.hip's partition), so every float32 sum is a function of the chunk's
// voxels alone and the grid is never capped.
#include "rcu_kernels.h"

#include "../../include/rcu_fit.h"

#include <cmath>

namespace rcu {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // a feature pointer is 4-byte aligned, no more

constexpr int PF_CHUNK = RCU_DENSITY_CHUNK;
constexpr int PF_MAX_L = RCU_POSTNET_FIT_MAX_CONVS;
constexpr double PF_EPS = 1e-5;

// per-layer state in the workspace, float32 [L][5][32], written by the finalising kernels for the passes behind them
enum { ST_SHIFT = 0, ST_MU = 32, ST_RSTD = 64, ST_MDY = 96, ST_MDYX = 128, ST_FLOATS = 160 };
// LDS image of a layer: forward weight tile, transposed weight tile ([j][lane][4], float4 = W[lane % 32][8 j + 4 (lane / 32) .. + 3]), bias, gamma,
// beta in channel order, the layer's state; zeros at channels >= F.  The output layer follows the layers: W_o[0][32], W_o[1][32], b_o[2].
enum { LY_WF = 0, LY_WB = 1024, LY_BIAS = 2048, LY_GAMMA = 2080, LY_BETA = 2112, LY_STATE = 2144, LY_FLOATS = LY_STATE + ST_FLOATS };
constexpr int OUT_FLOATS = 160;   // W_o, b_o (padded to 96), then the centre of phi [32] and the first layer's bias about it [32]
enum { OUT_CENTER = 96, OUT_BIASC = 128, EXTRA_FLOATS = 64 };
constexpr int TR_ROW = 33, TR_FLOATS = 32 * TR_ROW;   // one transposed tile; two per wave
constexpr size_t lds_floats(int L) { return (size_t)L * LY_FLOATS + OUT_FLOATS + 4 * 2 * TR_FLOATS; }

// floats of a chunk's record
constexpr int REC_STATS = 64;      // S1 [32], S2 [32]
constexpr int REC_TOP = 192;       // dW_o[0] [32], dW_o[1] [32], sum dy [32], sum dy xhat [32], db_o [2], loss
constexpr int REC_DOWN = 1152;     // dW in accumulator layout [16][64], sum du [32], sum dy [32], sum dy xhat [32]

constexpr size_t layer_params(int F) { return (size_t)F * F + 3 * (size_t)F; }

struct FitArgs {
    const float* x;
    int pitch, F;
    const uint8_t* labels;
    unsigned hw, chunks;
    size_t total;             // waves = chunks of the launch
    const float* params;
    const float* state;
    float* records;
    unsigned* flag;
    float inv_n;
    unsigned sample_count;    // > 0: the shift form of a stats pass -- ONE wave over voxels i * sample_stride, i < sample_count, about shift 0
    size_t sample_stride;
};

__device__ __forceinline__ f32x16 chan16(const float* p, int h)
{
    f32x16 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p + 8 * j + 4 * h);
        o[4 * j + 0] = t.x, o[4 * j + 1] = t.y, o[4 * j + 2] = t.z, o[4 * j + 3] = t.w;
    }
    return o;
}

// acc + W x for the 32 voxels of the wave: 16 steps of two channels
__device__ __forceinline__ f32x16 layer_product(const float* img, int lane, const f32x16& x, f32x16 acc)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(img + (j * 64 + lane) * 4);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, x[4 * j + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, x[4 * j + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, x[4 * j + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, x[4 * j + 3], acc, 0, 0, 0);
    }
    return acc;
}

// the sum over the 32 voxel columns of a half wave, in every lane of the half: one fixed butterfly
__device__ __forceinline__ float half_sum(float v)
{
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ void store_chan16(float* dst, const f32x16& v, int n, int h)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float s = half_sum(v[r]);
        if (n == 0) dst[8 * (r >> 2) + 4 * h + (r & 3)] = s;
    }
}

// MODE 0: statistics of u_T;  MODE 1: loss, output layer, sums of layer L (T = L);  MODE 2: gradient of layer T, sums of layer T - 1
template <int L, int MODE, int T>
__global__ __launch_bounds__(256) void fit_pass_kernel(const FitArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float pf_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    const int F = a.F;
    const size_t lp = layer_params(F);
    for (int k = 0; k < L; ++k) {
        const float* p = a.params + (size_t)k * lp;
        float* ly = pf_smem + k * LY_FLOATS;
        for (int e = tid; e < 1024; e += 256) {
            const int j = e >> 8, ln = (e >> 2) & 63, q = e & 3;
            const int row = ln & 31, col = 8 * j + 4 * (ln >> 5) + q;
            const bool in = row < F && col < F;
            ly[LY_WF + e] = in ? p[(size_t)row * F + col] : 0.f;
            ly[LY_WB + e] = in ? p[(size_t)col * F + row] : 0.f;
        }
        for (int e = tid; e < 96; e += 256) ly[LY_BIAS + e] = (e & 31) < F ? p[(size_t)F * F + (size_t)(e >> 5) * F + (e & 31)] : 0.f;
        for (int e = tid; e < ST_FLOATS; e += 256) ly[LY_STATE + e] = a.state[k * ST_FLOATS + e];
    }
    float* const out0 = pf_smem + L * LY_FLOATS;
    {
        float* const out = out0;
        const float* p = a.params + (size_t)L * lp;
        for (int e = tid; e < 64; e += 256) out[e] = (e & 31) < F ? p[(size_t)(e >> 5) * F + (e & 31)] : 0.f;
        if (tid < 2) out[64 + tid] = p[2 * (size_t)F + tid];
        for (int e = tid; e < EXTRA_FLOATS; e += 256) out[OUT_CENTER + e] = a.state[L * ST_FLOATS + e];
    }
    __syncthreads();

    const size_t w = (size_t)blockIdx.x * 4 + wave;
    if (w >= a.total) return;
    size_t base, stride;
    unsigned count;
    const bool sample = MODE == 0 && a.sample_count != 0;
    if (sample) {
        base = 0, stride = a.sample_stride, count = a.sample_count;
    } else {
        const size_t s = w / a.chunks;
        const unsigned q = (unsigned)(w % a.chunks);
        base = s * a.hw + (size_t)q * PF_CHUNK, stride = 1;
        count = a.hw - q * PF_CHUNK < (unsigned)PF_CHUNK ? a.hw - q * PF_CHUNK : (unsigned)PF_CHUNK;
    }
    const unsigned groups = (count + 31) / 32;

    auto voxel = [&](unsigned g) {
        const unsigned i = 32 * g + n;
        return base + (size_t)(i < count ? i : count - 1) * stride;     // tail lanes read a valid voxel, their sums take nothing from it
    };
    auto load = [&](unsigned g, f32x4 (&q)[4]) {
        const float* src = a.x + voxel(g) * a.pitch + 4 * h;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ch = 8 * j + 4 * h;      // channel_pitch >= 32: the 16 bytes exist; what lies at channels >= F is never used as data
            const f32x4u t = *reinterpret_cast<const f32x4u*>(src + 8 * j);
            q[j].x = ch < F ? t.x : 0.f, q[j].y = ch + 1 < F ? t.y : 0.f, q[j].z = ch + 2 < F ? t.z : 0.f, q[j].w = ch + 3 < F ? t.w : 0.f;
        }
    };

    f32x16 zero16;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero16[r] = 0.f;
    // the chunk's float32 sums
    f32x16 s_a = zero16, s_b = zero16, s_c = zero16, s_d = zero16;
    float s_loss = 0.f, s_dz0 = 0.f, s_dz1 = 0.f;
    bool bad = false;
    float* const tr = out0 + OUT_FLOATS + wave * 2 * TR_FLOATS;

    constexpr int NF = MODE == 0 ? T - 1 : L;     // finished layers of the forward chain
    f32x4 cur[4], nxt[4];
    load(0, cur);
    for (unsigned g = 0; g < groups; ++g) {
        load(g + 1 < groups ? g + 1 : g, nxt);    // the next group's features are in flight during this group's MFMAs
        // The per-channel constants are re-read from LDS in every group: an offset the compiler cannot see through keeps it from hoisting
        // the ~20 loop-invariant vectors of 16 registers out of the loop (which cost the second wave per SIMD and, for L = 4, spilled).
        int opaque = 0;
        asm volatile("" : "+s"(opaque));
        const float* const sm = pf_smem + opaque;
        const float* const out = sm + L * LY_FLOATS;
        const bool valid = 32 * g + n < count;
        f32x16 act, aprev = zero16;
#pragma unroll
        for (int j = 0; j < 4; ++j) act[4 * j + 0] = cur[j].x, act[4 * j + 1] = cur[j].y, act[4 * j + 2] = cur[j].z, act[4 * j + 3] = cur[j].w;
        if (MODE == 2 && T == 1) aprev = act;      // dW_1 takes phi as it is
        {
            // the chain runs on phi - c, c a per-channel centre known before the call's passes, and the first layer's bias is b + W c: where a
            // channel's |mean| >> sigma the products of the first layer are then of the size of sigma, and so is the rounding of u_1
            const f32x16 cen = chan16(out + OUT_CENTER, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) act[r] -= cen[r];
        }
        f32x16 xh[L + 1];
#pragma unroll
        for (int k = 1; k <= NF; ++k) {
            const float* ly = sm + (k - 1) * LY_FLOATS;
            if (MODE == 2 && k == T && k > 1) aprev = act;
            const f32x16 u = layer_product(ly + LY_WF, lane, act, chan16(k == 1 ? out + OUT_BIASC : ly + LY_BIAS, h));
            const f32x16 mu = chan16(ly + LY_STATE + ST_MU, h), rs = chan16(ly + LY_STATE + ST_RSTD, h);
            const f32x16 ga = chan16(ly + LY_GAMMA, h), be = chan16(ly + LY_BETA, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                xh[k][r] = (u[r] - mu[r]) * rs[r];
                act[r] = fmaxf(fmaf(ga[r], xh[k][r], be[r]), 0.f);
            }
        }
        if constexpr (MODE == 0) {
            const float* ly = sm + (T - 1) * LY_FLOATS;
            const f32x16 u = layer_product(ly + LY_WF, lane, act, chan16(T == 1 ? out + OUT_BIASC : ly + LY_BIAS, h));
            const f32x16 sh = chan16(ly + LY_STATE + ST_SHIFT, h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float d = valid ? u[r] - (sample ? 0.f : sh[r]) : 0.f;
                s_a[r] += d;
                s_b[r] = fmaf(d, d, s_b[r]);
            }
        } else {
            // the two logits: 16 channels in this lane, 16 in lane ^ 32; half 0 first in both lanes
            const f32x16 wo0 = chan16(out, h), wo1 = chan16(out + 32, h);
            float p0 = 0.f, p1 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) p0 = fmaf(wo0[r], act[r], p0), p1 = fmaf(wo1[r], act[r], p1);
            const float o0 = __shfl_xor(p0, 32), o1 = __shfl_xor(p1, 32);
            const float z0 = (h == 0 ? p0 + o0 : o0 + p0) + out[64], z1 = (h == 0 ? p1 + o1 : o1 + p1) + out[65];
            const int e = valid ? (int)a.labels[voxel(g)] : 0;
            bad |= e >= 2;
            const float m = fmaxf(z0, z1), e0 = expf(z0 - m), e1 = expf(z1 - m), ssum = e0 + e1;
            const float dz0 = valid ? (e0 / ssum - (e == 0 ? 1.f : 0.f)) * a.inv_n : 0.f;
            const float dz1 = valid ? (e1 / ssum - (e == 1 ? 1.f : 0.f)) * a.inv_n : 0.f;
            f32x16 dy;
            {
                const float* ly = sm + (L - 1) * LY_FLOATS;
                const f32x16 ga = chan16(ly + LY_GAMMA, h), be = chan16(ly + LY_BETA, h);
#pragma unroll
                for (int r = 0; r < 16; ++r) dy[r] = fmaf(ga[r], xh[L][r], be[r]) > 0.f ? fmaf(wo1[r], dz1, wo0[r] * dz0) : 0.f;
            }
            if constexpr (MODE == 1) {
                const float loss = m + logf(ssum) - (e == 0 ? z0 : e == 1 ? z1 : 0.f);
                if (valid && h == 0) s_loss += loss, s_dz0 += dz0, s_dz1 += dz1;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s_a[r] = fmaf(dz0, act[r], s_a[r]);
                    s_b[r] = fmaf(dz1, act[r], s_b[r]);
                    s_c[r] += dy[r];
                    s_d[r] = fmaf(dy[r], xh[L][r], s_d[r]);
                }
            } else {
#pragma unroll
                for (int k = L; k >= T; --k) {
                    const float* ly = sm + (k - 1) * LY_FLOATS;
                    const f32x16 ga = chan16(ly + LY_GAMMA, h), rs = chan16(ly + LY_STATE + ST_RSTD, h);
                    const f32x16 mdy = chan16(ly + LY_STATE + ST_MDY, h), mdyx = chan16(ly + LY_STATE + ST_MDYX, h);
                    f32x16 du;
#pragma unroll
                    for (int r = 0; r < 16; ++r) du[r] = valid ? ga[r] * rs[r] * (dy[r] - mdy[r] - xh[k][r] * mdyx[r]) : 0.f;
                    if (k == T) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) s_b[r] += du[r];
                        // du and a_{T-1} to "lane = channel, voxels along k"
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the reads of the last group are in order in front of these writes
                        __builtin_amdgcn_wave_barrier();
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int c = 8 * (r >> 2) + 4 * h + (r & 3);
                            tr[c * TR_ROW + n] = du[r];
                            tr[TR_FLOATS + c * TR_ROW + n] = aprev[r];
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                        for (int s = 0; s < 16; ++s)
                            s_a = __builtin_amdgcn_mfma_f32_32x32x2f32(tr[n * TR_ROW + 2 * s + h], tr[TR_FLOATS + n * TR_ROW + 2 * s + h], s_a, 0, 0, 0);
                    }
                    if (k > 1) {
                        const f32x16 da = layer_product(ly + LY_WB, lane, du, zero16);
                        const float* lb = sm + (k - 2) * LY_FLOATS;
                        const f32x16 gb = chan16(lb + LY_GAMMA, h), bb = chan16(lb + LY_BETA, h);
#pragma unroll
                        for (int r = 0; r < 16; ++r) dy[r] = fmaf(gb[r], xh[k - 1][r], bb[r]) > 0.f ? da[r] : 0.f;
                        if (k == T) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                s_c[r] += dy[r];
                                s_d[r] = fmaf(dy[r], xh[k - 1][r], s_d[r]);
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
    }

    float* rec = a.records + w * (MODE == 0 ? REC_STATS : MODE == 1 ? REC_TOP : REC_DOWN);
    if constexpr (MODE == 0) {
        store_chan16(rec, s_a, n, h);
        store_chan16(rec + 32, s_b, n, h);
    } else if constexpr (MODE == 1) {
        store_chan16(rec, s_a, n, h);
        store_chan16(rec + 32, s_b, n, h);
        store_chan16(rec + 64, s_c, n, h);
        store_chan16(rec + 96, s_d, n, h);
        const float l = half_sum(s_loss), d0 = half_sum(s_dz0), d1 = half_sum(s_dz1);
        if (lane == 0) rec[128] = d0, rec[129] = d1, rec[130] = l;
        if (bad) *a.flag = 1u;
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) rec[r * 64 + lane] = s_a[r];
        store_chan16(rec + 1024, s_b, n, h);
        if (T > 1) {
            store_chan16(rec + 1056, s_c, n, h);
            store_chan16(rec + 1088, s_d, n, h);
        }
    }
}

// c_j = the mean of phi_j over the sampled voxels i * stride, i < count (8 stripes i mod 8 in voxel order, then the stripes in order, float64), and
// the first layer's bias about it, b + W c (float64, rounded once): extra[0..31] = c, extra[32..63] = b + W c, zeros at channels >= F.  A constant
// error of that bias is in mu_1 as it is in every u_1: it cancels in u_1 - mu_1.
__global__ __launch_bounds__(256) void fit_center_kernel(const float* __restrict__ x, int pitch, int F, unsigned count, size_t stride,
                                                         const float* __restrict__ params, float* __restrict__ extra)
{
    __shared__ double part[8][32];
    __shared__ float cen[32];
    const int j = threadIdx.x & 31, stripe = threadIdx.x >> 5;
    double sum = 0.0;
    if (j < F)
        for (unsigned i = stripe; i < count; i += 8) sum += (double)x[(size_t)i * stride * pitch + j];
    part[stripe][j] = sum;
    __syncthreads();
    if (threadIdx.x < 32) {
        double t = 0.0;
        for (int k = 0; k < 8; ++k) t += part[k][j];
        const float c = j < F ? (float)(t / (double)count) : 0.f;
        cen[j] = c;
        extra[j] = c;
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        double b = 0.0;
        if (j < F) {
            b = (double)params[(size_t)F * F + j];
            for (int k = 0; k < F; ++k) b += (double)params[(size_t)j * F + k] * (double)cen[k];
        }
        extra[32 + j] = (float)b;
    }
}

struct FinArgs {
    const float* records;
    size_t total;          // records
    int F, L, T;
    double n_voxels;       // N; the shift form of a stats pass: the number of sampled voxels
    int sample;
    float* state;
    float* grads;
    double* loss;
    float* batch_mean;
    float* batch_var;
};

// sums of 16 consecutive record entries over all records: stripe t takes records t, t + 64, ... in order, then the stripes are added in stripe
// order, all in float64.  1024 threads = 16 entries x 64 stripes; the result is valid in threads 0 .. 15.
__device__ __forceinline__ double entry_sum(const float* rec, size_t rf, size_t total, double (*part)[16])
{
    const int el = threadIdx.x & 15, stripe = threadIdx.x >> 4;
    double s = 0.0;
    for (size_t q = stripe; q < total; q += 64) s += (double)rec[q * rf + el];
    __syncthreads();
    part[stripe][el] = s;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x < 16)
        for (int k = 0; k < 64; ++k) t += part[k][threadIdx.x];
    return t;
}

template <int MODE>
__global__ __launch_bounds__(1024) void fit_finalize_kernel(const FinArgs a)
{
    __shared__ double part[64][16];
    const int e0 = blockIdx.x * 16, e = e0 + (threadIdx.x & 15);
    const bool lead = threadIdx.x < 16;
    const int F = a.F;
    const size_t lp = layer_params(F);
    if constexpr (MODE == 0) {       // 2 blocks: channel e
        const double s1 = entry_sum(a.records + e0, REC_STATS, a.total, part);
        const double s2 = entry_sum(a.records + 32 + e0, REC_STATS, a.total, part);
        if (!lead) return;
        float* st = a.state + (a.T - 1) * ST_FLOATS;
        if (a.sample) {
            st[ST_SHIFT + e] = (float)(s1 / a.n_voxels);
            return;
        }
        const double d = s1 / a.n_voxels, mu = (double)st[ST_SHIFT + e] + d;
        double var = s2 / a.n_voxels - d * d;
        var = var > 0.0 ? var : 0.0;
        st[ST_MU + e] = (float)mu;
        st[ST_RSTD + e] = (float)(1.0 / sqrt(var + PF_EPS));
        if (e < F) a.batch_mean[(a.T - 1) * F + e] = (float)mu, a.batch_var[(a.T - 1) * F + e] = (float)var;
    } else if constexpr (MODE == 1) {   // 9 blocks: entries 0 .. 130 of REC_TOP
        const double s = entry_sum(a.records + e0, REC_TOP, a.total, part);
        if (!lead) return;
        float* g_out = a.grads + (size_t)a.L * lp;
        float* g_l = a.grads + (size_t)(a.L - 1) * lp + (size_t)F * F;      // bias, gamma, beta of layer L
        float* st = a.state + (a.L - 1) * ST_FLOATS;
        const int c = e & 31;
        if (e < 64) {
            if (c < F) g_out[(size_t)(e >> 5) * F + c] = (float)s;
        } else if (e < 96) {
            st[ST_MDY + c] = (float)(s / a.n_voxels);
            if (c < F) g_l[2 * F + c] = (float)s;
        } else if (e < 128) {
            st[ST_MDYX + c] = (float)(s / a.n_voxels);
            if (c < F) g_l[F + c] = (float)s;
        } else if (e < 130) {
            g_out[2 * (size_t)F + (e - 128)] = (float)s;
        } else if (e == 130) {
            a.loss[0] = s / a.n_voxels;
        }
    } else {                            // 66 or 70 blocks: entries of REC_DOWN
        const double s = entry_sum(a.records + e0, REC_DOWN, a.total, part);
        if (!lead) return;
        float* g_t = a.grads + (size_t)(a.T - 1) * lp;
        const int c = e & 31;
        if (e < 1024) {
            const int r = e >> 6, ln = e & 63;
            const int i = 8 * (r >> 2) + 4 * (ln >> 5) + (r & 3), j = ln & 31;
            if (i < F && j < F) g_t[(size_t)i * F + j] = (float)s;
        } else if (e < 1056) {
            if (c < F) g_t[(size_t)F * F + c] = (float)s;
        } else if (a.T > 1) {
            float* g_b = a.grads + (size_t)(a.T - 2) * lp + (size_t)F * F;
            float* st = a.state + (a.T - 2) * ST_FLOATS;
            if (e < 1088) {
                st[ST_MDY + c] = (float)(s / a.n_voxels);
                if (c < F) g_b[2 * F + c] = (float)s;
            } else if (e < 1120) {
                st[ST_MDYX + c] = (float)(s / a.n_voxels);
                if (c < F) g_b[F + c] = (float)s;
            }
        }
    }
}

template <int L, int MODE, int T>
hipError_t launch_pass_lt(const FitArgs& a, hipStream_t stream)
{
    if constexpr (T <= L && (MODE != 1 || T == L)) {      // the top pass exists for T = L alone
        const size_t lds = lds_floats(L) * sizeof(float);
        hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void*>(&fit_pass_kernel<L, MODE, T>), (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((fit_pass_kernel<L, MODE, T>), dim3((unsigned)((a.total + 3) / 4)), dim3(256), lds, stream, a);
        return hipGetLastError();
    } else {
        return hipErrorInvalidValue;
    }
}

template <int L, int MODE>
hipError_t launch_pass_l(int T, const FitArgs& a, hipStream_t stream)
{
    switch (T) {
        case 1: return launch_pass_lt<L, MODE, 1>(a, stream);
        case 2: return launch_pass_lt<L, MODE, 2>(a, stream);
        case 3: return launch_pass_lt<L, MODE, 3>(a, stream);
        default: return launch_pass_lt<L, MODE, 4>(a, stream);
    }
}

template <int MODE>
hipError_t launch_pass(int L, int T, const FitArgs& a, hipStream_t stream)
{
    switch (L) {
        case 1: return launch_pass_l<1, MODE>(T, a, stream);
        case 2: return launch_pass_l<2, MODE>(T, a, stream);
        case 3: return launch_pass_l<3, MODE>(T, a, stream);
        default: return launch_pass_l<4, MODE>(T, a, stream);
    }
}

template <int MODE>
hipError_t launch_finalize(const FinArgs& a, int entries, hipStream_t stream)
{
    hipLaunchKernelGGL(fit_finalize_kernel<MODE>, dim3((unsigned)((entries + 15) / 16)), dim3(1024), 0, stream, a);
    return hipGetLastError();
}

int invalid(const char* fn, const std::string& msg) { return report_error(RCU_ERR_INVALID, std::string(fn) + ": " + msg); }

bool shape_ok(int F, int L, size_t n, size_t hw)
{
    if (F < 1 || F > 32 || L < 1 || L > PF_MAX_L || n < 1 || hw < 1 || n > ((size_t)1 << 31) || hw > ((size_t)1 << 31)) return false;
    const size_t chunks = (hw + PF_CHUNK - 1) / PF_CHUNK;
    return n * hw >= 2 && n * hw < ((size_t)1 << 40) && n * chunks < ((size_t)1 << 31);
}

}  // namespace
}  // namespace rcu

using namespace rcu;

extern "C" size_t rcu_postnet_fit_param_count(int F, int nb_convs)
{
    if (F < 1 || F > 32 || nb_convs < 1 || nb_convs > PF_MAX_L) return 0;
    return (size_t)nb_convs * layer_params(F) + 2 * (size_t)F + 2;
}

extern "C" size_t rcu_postnet_fit_workspace_bytes(int F, int nb_convs, size_t n, size_t hw)
{
    if (!shape_ok(F, nb_convs, n, hw)) return 0;
    const size_t chunks = (hw + PF_CHUNK - 1) / PF_CHUNK;
    return round256(((size_t)nb_convs * ST_FLOATS + EXTRA_FLOATS) * sizeof(float)) + round256(n * chunks * REC_DOWN * sizeof(float));
}

extern "C" int rcu_postnet_loss_grad(const float* features_dev, int channel_pitch, int F, size_t n, size_t hw, const uint8_t* labels_dev, int nb_convs,
                                     const float* params_dev, float* grads_dev, double* loss_dev, float* batch_mean_dev, float* batch_var_dev,
                                     uint32_t* flags_dev, void* workspace_dev, void* stream)
{
    static const char* fn = "rcu_postnet_loss_grad";
    if (!features_dev || !labels_dev || !params_dev || !grads_dev || !loss_dev || !batch_mean_dev || !batch_var_dev || !flags_dev || !workspace_dev)
        return invalid(fn, "null argument (features_dev, labels_dev, params_dev, grads_dev, loss_dev, batch_mean_dev, batch_var_dev, flags_dev, "
                           "workspace_dev)");
    if (F < 1 || F > 32) return invalid(fn, "F must be in 1..32, got " + std::to_string(F));
    if (channel_pitch < 32 || channel_pitch % 4)
        return invalid(fn, "channel_pitch must be >= 32 and a multiple of 4, got " + std::to_string(channel_pitch));
    if (nb_convs < 1 || nb_convs > PF_MAX_L)
        return invalid(fn, "nb_convs must be in 1.." + std::to_string(PF_MAX_L) + ", got " + std::to_string(nb_convs));
    if (n < 1 || hw < 1 || n > ((size_t)1 << 31) || hw > ((size_t)1 << 31)) return invalid(fn, "n and hw must be in 1..2^31");
    if (n * hw < 2) return invalid(fn, "train-mode BatchNorm needs N = n * hw >= 2 voxels");
    if (!shape_ok(F, nb_convs, n, hw)) return invalid(fn, "n * hw must be below 2^40 and n * ceil(hw / RCU_DENSITY_CHUNK) below 2^31");
    auto off = [](const void* p, size_t m) { return reinterpret_cast<uintptr_t>(p) % m != 0; };
    if (off(features_dev, 4) || off(params_dev, 4) || off(grads_dev, 4) || off(batch_mean_dev, 4) || off(batch_var_dev, 4) || off(flags_dev, 4))
        return invalid(fn, "features_dev, params_dev, grads_dev, batch_mean_dev, batch_var_dev and flags_dev must be 4-byte aligned");
    if (off(loss_dev, 8) || off(workspace_dev, 8)) return invalid(fn, "loss_dev and workspace_dev must be 8-byte aligned");

    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int L = nb_convs;
    const size_t N = n * hw;
    const unsigned chunks = (unsigned)((hw + PF_CHUNK - 1) / PF_CHUNK);
    float* state = static_cast<float*>(workspace_dev);      // [L][ST_FLOATS], then the centre and the first bias about it
    float* records = reinterpret_cast<float*>(static_cast<char*>(workspace_dev) + round256(((size_t)L * ST_FLOATS + EXTRA_FLOATS) * sizeof(float)));

    FitArgs a{};
    a.x = features_dev, a.pitch = channel_pitch, a.F = F, a.labels = labels_dev, a.hw = (unsigned)hw, a.chunks = chunks, a.total = n * chunks;
    a.params = params_dev, a.state = state, a.records = records, a.flag = flags_dev, a.inv_n = (float)(1.0 / (double)N);
    FinArgs f{};
    f.records = records, f.total = a.total, f.F = F, f.L = L, f.n_voxels = (double)N, f.state = state, f.grads = grads_dev, f.loss = loss_dev;
    f.batch_mean = batch_mean_dev, f.batch_var = batch_var_dev;

    hipError_t e = hipSuccess;
    // the sampled voxels i * stride: an odd stride, so that it shares no factor with an even row width and the samples do not line up in image columns
    const unsigned sample_count = (unsigned)(N < (size_t)PF_CHUNK ? N : (size_t)PF_CHUNK);
    size_t sample_stride = N / sample_count;
    if (sample_stride > 1 && sample_stride % 2 == 0) --sample_stride;
    hipLaunchKernelGGL(fit_center_kernel, dim3(1), dim3(256), 0, s, features_dev, channel_pitch, F, sample_count, sample_stride, params_dev,
                       state + (size_t)L * ST_FLOATS);
    e = hipGetLastError();
    for (int t = 1; t <= L && e == hipSuccess; ++t) {
        FitArgs sa = a;
        sa.total = 1, sa.sample_count = sample_count, sa.sample_stride = sample_stride;
        FinArgs sf = f;
        sf.total = 1, sf.T = t, sf.sample = 1, sf.n_voxels = (double)sample_count;
        e = launch_pass<0>(L, t, sa, s);
        if (e == hipSuccess) e = launch_finalize<0>(sf, 32, s);
        f.T = t;
        if (e == hipSuccess) e = launch_pass<0>(L, t, a, s);
        if (e == hipSuccess) e = launch_finalize<0>(f, 32, s);
    }
    f.T = L;
    if (e == hipSuccess) e = launch_pass<1>(L, L, a, s);
    if (e == hipSuccess) e = launch_finalize<1>(f, 131, s);
    for (int t = L; t >= 1 && e == hipSuccess; --t) {
        f.T = t;
        e = launch_pass<2>(L, t, a, s);
        if (e == hipSuccess) e = launch_finalize<2>(f, t > 1 ? 1120 : 1056, s);
    }
    if (e != hipSuccess) return hip_failed(fn, e);
    return RCU_OK;
}
