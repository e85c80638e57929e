// Feature-space density (include/rcu.h "Feature-space density"): the two kernels of the class-Gaussian uncertainty on the U-Net feature map, both
// on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain, one rounding per product).
//
// density_moments_kernel -- the class-conditioned Gram matrix of a slice.  D[i][j] = sum_v phi_i(v) * [y(v) = c] phi_j(v): a step of the MFMA sums
//   over TWO voxels (k = lane / 32), so lane (i = lane % 32, h = lane / 32) holds channel i of voxel 2 t + h in ONE register that is the A operand as
//   it is and, zeroed where the voxel's label is not c, the B operand of class c: the features are read once for up to KC classes (one MFMA per class
//   and 32 x 32 block), a dword per lane and step, 256 contiguous bytes per wave at pitch 32.  64 channels are the blocks (0,0), (0,1), (1,1); the
//   finalising kernel mirrors (0,1).  One WAVE owns one chunk of RCU_DENSITY_CHUNK voxels of one slice -- the partition is by voxel index within the
//   slice alone -- accumulates it in float32 (the MFMA chain for G, one add per voxel for S), and leaves the chunk's sums in the workspace.
//   density_finalize_kernel promotes them and adds the chunks of a slice in float64, in chunk order: ((c0 + c1) + c2) + ...  No atomics, nothing
//   depends on n, the slice's position, the alignment or the launch geometry.
// density_energy_kernel -- Y = A_c X in the orientation of rcu_postnet.hip (weights as A, 32 voxels as B, the accumulator started at -b_c): a lane
//   (voxel n = lane % 32, half h) receives rows 8 (r / 4) + 4 h + r % 4 of ITS voxel in accumulator element r, squares and adds its 16 (32) rows in
//   register order, and one cross-lane exchange with lane ^ 32 completes d^2.  The classes are looped with a running logsumexp in registers; the
//   features are read once (four float4 per lane and 32 channels), A_c lives in LDS for every class.  Channels >= F are never read as data: their
//   operand registers are zero-filled, and so are the rows and columns >= F of the LDS image of A.
#include "rcu_kernels.h"

#include <cmath>

namespace rcu {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int DM_CHUNK = RCU_DENSITY_CHUNK;
constexpr int DM_AHEAD = 8;         // steps (voxel pairs) whose loads are in flight together
constexpr int DM_FLAG_BYTES = 256;   // head of the workspace: the "label >= K seen" word

constexpr int dm_blocks(int cb) { return cb == 1 ? 1 : 3; }
// floats of one chunk's record: G [K][NB][16][64], S [K][CB][64] (the two voxel parities side by side), n [K][2] as uint32; a multiple of 64
constexpr size_t dm_g_floats(int K, int cb) { return (size_t)K * dm_blocks(cb) * 1024; }
constexpr size_t dm_s_floats(int K, int cb) { return (size_t)K * cb * 64; }
constexpr size_t dm_record_floats(int K, int cb) { return (dm_g_floats(K, cb) + dm_s_floats(K, cb) + 2 * (size_t)K + 63) / 64 * 64; }

template <int CB, int KC>
__global__ __launch_bounds__(256) void density_moments_kernel(const float* __restrict__ x, int pitch, int F, const uint8_t* __restrict__ labels,
                                                              size_t total, unsigned hw, unsigned chunks, int K, float* __restrict__ records,
                                                              size_t record_floats, unsigned* __restrict__ flag)
{
    constexpr int NB = dm_blocks(CB);
    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= total) return;
    const size_t s = w / chunks;
    const unsigned q = (unsigned)(w % chunks);
    const int c0 = blockIdx.y * KC;
    const unsigned v0 = q * DM_CHUNK, v1 = v0 + DM_CHUNK < hw ? v0 + DM_CHUNK : hw;
    const float* xs = x + s * (size_t)hw * pitch + i;
    const uint8_t* ls = labels + s * (size_t)hw;
    bool on[CB];
#pragma unroll
    for (int ib = 0; ib < CB; ++ib) on[ib] = i + 32 * ib < F;

    f32x16 acc[KC][NB];
    float sacc[KC][CB];
    unsigned cnt[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        cnt[c] = 0;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][nb][r] = 0.f;
#pragma unroll
        for (int ib = 0; ib < CB; ++ib) sacc[c][ib] = 0.f;
    }
    bool bad = false;
    // DM_AHEAD steps per trip, their loads issued together in front of the MFMAs (a step's dword load is a full memory latency); the steps are
    // consumed in voxel order, so the sums are those of the one-step loop
    for (unsigned t0 = v0; t0 < v1; t0 += 2 * DM_AHEAD) {
        int lab[DM_AHEAD];
        float a[DM_AHEAD][CB];
#pragma unroll
        for (int u = 0; u < DM_AHEAD; ++u) {
            const unsigned v = t0 + 2 * u + h;
            const bool valid = v < v1;
            lab[u] = valid ? (int)ls[v] : -1;      // -1: beyond the chunk, in no class
#pragma unroll
            for (int ib = 0; ib < CB; ++ib) a[u][ib] = (valid && on[ib]) ? xs[(size_t)v * pitch + 32 * ib] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < DM_AHEAD; ++u) {
            bad |= lab[u] >= K;
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                if (c0 + c >= K) continue;      // uniform over the launch
                const bool sel = lab[u] == c0 + c;
                float bm[CB];
#pragma unroll
                for (int ib = 0; ib < CB; ++ib) {
                    bm[ib] = sel ? a[u][ib] : 0.f;
                    sacc[c][ib] += bm[ib];
                }
                cnt[c] += sel ? 1u : 0u;
                acc[c][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][0], bm[0], acc[c][0], 0, 0, 0);
                if constexpr (CB == 2) {
                    acc[c][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][0], bm[1], acc[c][1], 0, 0, 0);
                    acc[c][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][1], bm[1], acc[c][2], 0, 0, 0);
                }
            }
        }
    }
    float* rec = records + w * record_floats;
    float* rec_s = rec + dm_g_floats(K, CB);
    unsigned* rec_n = reinterpret_cast<unsigned*>(rec_s + dm_s_floats(K, CB));
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        if (c0 + c >= K) continue;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) rec[(((size_t)(c0 + c) * NB + nb) * 16 + r) * 64 + lane] = acc[c][nb][r];
#pragma unroll
        for (int ib = 0; ib < CB; ++ib) rec_s[((c0 + c) * CB + ib) * 64 + lane] = sacc[c][ib];
        if (i == 0) rec_n[(c0 + c) * 2 + h] = cnt[c];
    }
    if (bad) *flag = 1u;
}

// one thread per output entry of a slice: the chunks' float32 sums promoted and added in float64 in chunk order
template <int CB>
__global__ __launch_bounds__(256) void density_finalize_kernel(const float* __restrict__ records, size_t record_floats, unsigned chunks, int K, int F,
                                                               unsigned blocks_per_slice, long long* __restrict__ n_out, double* __restrict__ S_out,
                                                               double* __restrict__ G_out)
{
    constexpr int NB = dm_blocks(CB);
    const size_t s = blockIdx.x / blocks_per_slice;
    const size_t e = (size_t)(blockIdx.x % blocks_per_slice) * 256 + threadIdx.x;
    const size_t EG = (size_t)K * NB * 1024, ES = (size_t)K * CB * 32;
    const float* rec = records + s * chunks * record_floats;
    if (e < EG) {
        const int c = (int)(e / (NB * 1024)), nb = (int)(e / 1024) % NB, r = (int)(e >> 6) & 15, lane = (int)e & 63;
        const int ib = nb == 2 ? 1 : 0, jb = nb == 0 ? 0 : 1;
        const int i = 32 * ib + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3), j = 32 * jb + (lane & 31);
        if (i >= F || j >= F) return;
        double sum = 0.0;
        for (unsigned q = 0; q < chunks; ++q) sum += (double)rec[q * record_floats + e];
        double* G = G_out + (s * K + c) * (size_t)F * F;
        G[(size_t)i * F + j] = sum;
        if (nb == 1) G[(size_t)j * F + i] = sum;
    } else if (e < EG + ES) {
        const int idx = (int)(e - EG), c = idx / (CB * 32), ch = idx % (CB * 32);
        if (ch >= F) return;
        const size_t at = EG + (size_t)(c * CB + ch / 32) * 64 + ch % 32;
        double sum = 0.0;
        for (unsigned q = 0; q < chunks; ++q) {
            sum += (double)rec[q * record_floats + at];
            sum += (double)rec[q * record_floats + at + 32];
        }
        S_out[(s * K + c) * (size_t)F + ch] = sum;
    } else if (e < EG + ES + K) {
        const int c = (int)(e - EG - ES);
        long long sum = 0;
        for (unsigned q = 0; q < chunks; ++q) {
            const unsigned* rn = reinterpret_cast<const unsigned*>(rec + q * record_floats + EG + 2 * ES);
            sum += (long long)rn[c * 2] + (long long)rn[c * 2 + 1];
        }
        n_out[s * K + c] = sum;
    }
}

// LDS image per class: CB x CB weight tiles [cob][cib][j = 0..3][lane][4] (float4 = A_c[32 cob + lane % 32][32 cib + 8 j + 4 (lane / 32) .. + 3]),
// then the accumulators' start values [cob][j][h][4] = -b_c[32 cob + 8 j + 4 h .. + 3]; zeros at rows and columns >= F.  k_c follows the classes.
constexpr int de_class_floats(int cb) { return cb * cb * 1024 + cb * 32; }

template <int CB>
__global__ __launch_bounds__(256) void density_energy_kernel(const float* __restrict__ x, int pitch, int F, size_t nvox, int K,
                                                             const float* __restrict__ A, const float* __restrict__ b, const float* __restrict__ kc,
                                                             float* __restrict__ energy, float* __restrict__ d2_out)
{
    extern __shared__ __attribute__((aligned(16))) float de_smem[];
    constexpr int W_FLOATS = CB * CB * 1024, B_FLOATS = CB * 32, CLS = de_class_floats(CB);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    for (int e = tid; e < K * W_FLOATS; e += 256) {
        const int c = e / W_FLOATS, rest = e % W_FLOATS, blk = rest >> 10, j = (rest >> 8) & 3, ln = (rest >> 2) & 63, q = rest & 3;
        const int row = 32 * (blk / CB) + (ln & 31), col = 32 * (blk % CB) + 8 * j + 4 * (ln >> 5) + q;
        de_smem[c * CLS + rest] = (row < F && col < F) ? A[((size_t)c * F + row) * F + col] : 0.f;
    }
    for (int e = tid; e < K * B_FLOATS; e += 256) {
        const int c = e / B_FLOATS, rest = e % B_FLOATS;      // rest = ((cob * 4 + j) * 2 + h) * 4 + q
        const int ch = 32 * (rest >> 5) + 8 * ((rest >> 3) & 3) + 4 * ((rest >> 2) & 1) + (rest & 3);
        de_smem[c * CLS + W_FLOATS + rest] = ch < F ? -b[(size_t)c * F + ch] : 0.f;
    }
    if (tid < K) de_smem[K * CLS + tid] = kc[tid];
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
        f32x16 act[CB];
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                act[cb][4 * j + 0] = cur[cb][j].x, act[cb][4 * j + 1] = cur[cb][j].y, act[cb][4 * j + 2] = cur[cb][j].z,
                               act[cb][4 * j + 3] = cur[cb][j].w;
            }
        const size_t v = g * 32 + n;
        const bool store = v < nvox && h == 0;
        float m = 0.f, ssum = 1.f;
        for (int c = 0; c < K; ++c) {
            const float* wl = de_smem + (size_t)c * CLS;
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
            const float d2 = h == 0 ? part + other : other + part;      // rows of half 0 first, in both lanes
            if (store && d2_out != nullptr) d2_out[v * K + c] = d2;
            const float t = fmaf(-0.5f, d2, de_smem[K * CLS + c]);
            if (c == 0) {
                m = t, ssum = 1.f;
            } else {                              // running logsumexp: the maximum so far is subtracted
                const float mn = fmaxf(m, t);
                ssum = ssum * expf(m - mn) + expf(t - mn);
                m = mn;
            }
        }
        if (store) energy[v] = -(m + logf(ssum));
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int j = 0; j < 4; ++j) cur[cb][j] = nxt[cb][j];
    }
}

template <int CB>
hipError_t launch_energy(const float* x, int pitch, int F, size_t nvox, int K, const float* A, const float* b, const float* kc, float* energy,
                         float* d2, hipStream_t stream)
{
    const size_t ngroups = (nvox + 31) / 32;
    const size_t wgs = (ngroups + 3) / 4;
    const unsigned grid = (unsigned)(wgs < 2048 ? wgs : 2048);
    const size_t lds = ((size_t)K * de_class_floats(CB) + 8) * sizeof(float);
    hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void*>(&density_energy_kernel<CB>), (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(density_energy_kernel<CB>, dim3(grid), dim3(256), lds, stream, x, pitch, F, nvox, K, A, b, kc, energy, d2);
    return hipGetLastError();
}

template <int CB, int KC>
hipError_t launch_moments(const float* x, int pitch, int F, const uint8_t* labels, size_t n, unsigned hw, int K, long long* n_out, double* S_out,
                          double* G_out, void* workspace, hipStream_t stream)
{
    const unsigned chunks = (hw + DM_CHUNK - 1) / DM_CHUNK;
    const size_t total = n * chunks, rf = dm_record_floats(K, CB);
    unsigned* flag = static_cast<unsigned*>(workspace);
    float* records = reinterpret_cast<float*>(static_cast<char*>(workspace) + DM_FLAG_BYTES);
    hipLaunchKernelGGL((density_moments_kernel<CB, KC>), dim3((unsigned)((total + 3) / 4), (unsigned)((K + KC - 1) / KC)), dim3(256), 0, stream, x,
                       pitch, F, labels, total, hw, chunks, K, records, rf, flag);
    if (hipError_t e = hipGetLastError()) return e;
    const size_t entries = dm_g_floats(K, CB) + (size_t)K * CB * 32 + K;
    const unsigned bps = (unsigned)((entries + 255) / 256);
    hipLaunchKernelGGL(density_finalize_kernel<CB>, dim3((unsigned)(n * bps)), dim3(256), 0, stream, records, rf, chunks, K, F, bps, n_out, S_out,
                       G_out);
    return hipGetLastError();
}

int invalid(const char* fn, const std::string& msg) { return report_error(RCU_ERR_INVALID, std::string(fn) + ": " + msg); }

// the contract both kernels share: 1 <= F <= 64, channel_pitch >= F and a multiple of 4, 1 <= K <= 8
int check_shape(const char* fn, int channel_pitch, int F, int K)
{
    if (F < 1 || F > RCU_DENSITY_MAX_FEATURES) return invalid(fn, "F must be in 1..64, got " + std::to_string(F));
    if (channel_pitch < F || channel_pitch % 4) return invalid(fn, "channel_pitch must be >= F and a multiple of 4, got " + std::to_string(channel_pitch));
    if (K < 1 || K > MAX_CLASSES) return invalid(fn, "K must be in 1..8, got " + std::to_string(K));
    return RCU_OK;
}

}  // namespace
}  // namespace rcu

using namespace rcu;

extern "C" size_t rcu_density_moments_workspace_bytes(size_t n, size_t hw, int F, int K)
{
    if (n < 1 || hw < 1 || F < 1 || F > RCU_DENSITY_MAX_FEATURES || K < 1 || K > MAX_CLASSES) return 0;
    const size_t chunks = (hw + DM_CHUNK - 1) / DM_CHUNK;
    return round256(DM_FLAG_BYTES + n * chunks * dm_record_floats(K, F > 32 ? 2 : 1) * sizeof(float));
}

extern "C" int rcu_density_moments(const float* features_dev, int channel_pitch, int F, const uint8_t* labels_dev, size_t n, size_t hw, int K,
                                   int64_t* n_out_dev, double* S_out_dev, double* G_out_dev, void* workspace_dev, void* stream)
{
    static const char* fn = "rcu_density_moments";
    if (!features_dev || !labels_dev || !n_out_dev || !S_out_dev || !G_out_dev || !workspace_dev)
        return invalid(fn, "null argument (features_dev, labels_dev, n_out_dev, S_out_dev, G_out_dev, workspace_dev)");
    if (int st = check_shape(fn, channel_pitch, F, K)) return st;
    if (n < 1 || n > ((size_t)1 << 20) || hw < 1 || hw > ((size_t)1 << 30)) return invalid(fn, "n must be in 1..2^20 and hw in 1..2^30");
    const size_t chunks = (hw + DM_CHUNK - 1) / DM_CHUNK;
    if (n * chunks > ((size_t)1 << 31) - 4) return invalid(fn, "n * ceil(hw / RCU_DENSITY_CHUNK) must be below 2^31");
    if (reinterpret_cast<uintptr_t>(features_dev) % 4 || reinterpret_cast<uintptr_t>(workspace_dev) % 8)
        return invalid(fn, "features_dev must be 4-byte and workspace_dev 8-byte aligned");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(workspace_dev, 0, DM_FLAG_BYTES, s);
    if (e != hipSuccess) return hip_failed(fn, e);
    long long* no = reinterpret_cast<long long*>(n_out_dev);
    if (F <= 32)
        e = launch_moments<1, 4>(features_dev, channel_pitch, F, labels_dev, n, (unsigned)hw, K, no, S_out_dev, G_out_dev, workspace_dev, s);
    else
        e = launch_moments<2, 2>(features_dev, channel_pitch, F, labels_dev, n, (unsigned)hw, K, no, S_out_dev, G_out_dev, workspace_dev, s);
    if (e != hipSuccess) return hip_failed(fn, e);
    // the label check: one word comes back, so the call returns with the stream drained
    unsigned flag = 0;
    e = hipMemcpyAsync(&flag, workspace_dev, sizeof(flag), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_failed(fn, e);
    if (flag) return invalid(fn, "labels_dev holds a label >= K = " + std::to_string(K) + " (the outputs leave such voxels out)");
    return RCU_OK;
}

extern "C" int rcu_density_energy(const float* features_dev, int channel_pitch, int F, size_t n_voxels, int K, const float* A_dev, const float* b_dev,
                                  const float* k_dev, float* energy_dev, float* d2_dev, void* stream)
{
    static const char* fn = "rcu_density_energy";
    if (!features_dev || !A_dev || !b_dev || !k_dev || !energy_dev) return invalid(fn, "null argument (features_dev, A_dev, b_dev, k_dev, energy_dev)");
    if (int st = check_shape(fn, channel_pitch, F, K)) return st;
    if (n_voxels < 1 || n_voxels > ((size_t)1 << 40)) return invalid(fn, "n_voxels must be in 1..2^40");
    if (reinterpret_cast<uintptr_t>(features_dev) % 16) return invalid(fn, "features_dev must be 16-byte aligned");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = F <= 32 ? launch_energy<1>(features_dev, channel_pitch, F, n_voxels, K, A_dev, b_dev, k_dev, energy_dev, d2_dev, s)
                                 : launch_energy<2>(features_dev, channel_pitch, F, n_voxels, K, A_dev, b_dev, k_dev, energy_dev, d2_dev, s);
    if (e != hipSuccess) return hip_failed(fn, e);
    return RCU_OK;
}
