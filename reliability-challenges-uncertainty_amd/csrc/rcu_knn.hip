// Nearest-neighbour feature uncertainty (include/rcu_knn.h): the voxels x bank distance product with a k-smallest selection per voxel, and the
// Philox keys the bank is sampled by.
//
// knn_distances_kernel -- X^T B in the orientation of density_energy_kernel (rcu_density.hip): 32 bank rows are the A operand of
//   v_mfma_f32_32x32x2_f32 (bit for bit a k-ordered fmaf chain, one rounding per product), 32 voxels the B operand.  A wave owns KNN_GROUPS groups
//   of 32 voxels and keeps their (normalised) features in registers for the whole sweep over the bank, so a tile's A operand -- four float4 per lane
//   from LDS -- serves KNN_GROUPS x 16 MFMAs.  The bank does not fit the LDS (2048 rows x 32 channels are 256 KB): the workgroup stages it in pieces of
//   KNN_STAGE_TILES tiles, already in operand order [tile][j][lane][4] with zeros at channels >= F and at rows >= M, beside |b_m|^2 with +inf at
//   rows >= M -- the rows beyond the bank are masked by index where they are staged, and an infinite distance is never selected.
//   A lane (voxel n = lane % 32, half h) receives rows 8 (r / 4) + 4 h + r % 4 of the tile for ITS voxel in accumulator element r: 16 candidates per
//   tile.  It keeps the K smallest so far sorted in registers (+inf at the start); the smallest of the 16 is compared with the current K-th first, so
//   once the list has warmed up a tile costs 16 x 3 VALU operations for the distances and 16 for the minimum, and the insertion network runs rarely.
//   One exchange with lane ^ 32 merges the two halves: both lanes insert the other's list and hold the same sorted multiset.
//   The workgroups stride over sets of 4 x KNN_GROUPS groups (the grid is capped); every wave of a workgroup takes part in every barrier, a wave
//   whose groups lie beyond the end computes on the last voxel and stores nothing.
// knn_keys_kernel -- one Philox4x32-10 block per voxel.
#include "rcu_kernels.h"

#include "../../include/rcu_knn.h"
#include "rcu_head_common.h"

#include <cmath>

namespace rcu {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int KNN_GROUPS = 4;            // voxel groups (of 32) a wave keeps in registers
constexpr int KNN_STAGE_TILES = 8;       // bank tiles (of 32 rows) staged in LDS at a time: 32 KB + 1 KB of norms
constexpr unsigned KNN_GRID_CAP = 2048;  // workgroups; a set of 4 * KNN_GROUPS * 32 = 512 voxels each per trip
constexpr int KNN_TILE_FLOATS = 1024;
constexpr float KNN_MIN_NORM = 9.094947017729282e-13f;      // 2^-40

template <int K>
__device__ __forceinline__ void knn_insert(float (&best)[K], float d)
{
    float c = d;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float lo = fminf(best[i], c);
        c = fmaxf(best[i], c);
        best[i] = lo;
    }
}

template <int K>
__global__ __launch_bounds__(256) void knn_distances_kernel(const float* __restrict__ x, int pitch, int F, size_t nvox, const float* __restrict__ bank,
                                                            const float* __restrict__ bank_sq, int M, int normalize, float* __restrict__ score,
                                                            float* __restrict__ d2_out)
{
    __shared__ __attribute__((aligned(16))) float tiles[KNN_STAGE_TILES * KNN_TILE_FLOATS];
    __shared__ __attribute__((aligned(16))) float norms[KNN_STAGE_TILES * 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    const size_t ngroups = (nvox + 31) / 32;
    const size_t nsets = (ngroups + 4 * KNN_GROUPS - 1) / (4 * KNN_GROUPS);
    const int ntiles = (M + 31) / 32;
    const float inf = __builtin_inff();

    for (size_t set = blockIdx.x; set < nsets; set += gridDim.x) {
        // this wave's voxels: channel 8 j + 4 h + q of voxel n of group g in act[g][4 j + q], zeros at channels >= F
        f32x16 act[KNN_GROUPS];
        float xx[KNN_GROUPS];
        float best[KNN_GROUPS][K];
#pragma unroll
        for (int g = 0; g < KNN_GROUPS; ++g) {
            size_t v = ((set * 4 + wave) * KNN_GROUPS + g) * 32 + n;
            v = v < nvox ? v : nvox - 1;            // lanes beyond the end read a valid voxel, their results are not stored
            const float* src = x + v * (size_t)pitch + 4 * h;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ch = 8 * j + 4 * h;       // ch < F implies ch + 3 < pitch (a multiple of 4 that is >= F)
                f32x4 t = {0.f, 0.f, 0.f, 0.f};
                if (ch < F) {
                    t = *reinterpret_cast<const f32x4*>(src + 8 * j);
                    t.y = ch + 1 < F ? t.y : 0.f, t.z = ch + 2 < F ? t.z : 0.f, t.w = ch + 3 < F ? t.w : 0.f;
                }
                act[g][4 * j + 0] = t.x, act[g][4 * j + 1] = t.y, act[g][4 * j + 2] = t.z, act[g][4 * j + 3] = t.w;
            }
            if (normalize) {
                float part = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) part = fmaf(act[g][r], act[g][r], part);
                const float other = __shfl_xor(part, 32);
                const float ss = h == 0 ? part + other : other + part;      // the channels of half 0 first, in both lanes
                const float norm = fmaxf(sqrtf(ss), KNN_MIN_NORM);
#pragma unroll
                for (int r = 0; r < 16; ++r) act[g][r] = act[g][r] / norm;
            }
            float part = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) part = fmaf(act[g][r], act[g][r], part);
            const float other = __shfl_xor(part, 32);
            xx[g] = h == 0 ? part + other : other + part;
#pragma unroll
            for (int i = 0; i < K; ++i) best[g][i] = inf;
        }

        for (int t0 = 0; t0 < ntiles; t0 += KNN_STAGE_TILES) {
            const int staged = ntiles - t0 < KNN_STAGE_TILES ? ntiles - t0 : KNN_STAGE_TILES;
            __syncthreads();                        // the previous piece has been consumed
            for (int e = tid; e < staged * KNN_TILE_FLOATS; e += 256) {
                const int t = e >> 10, j = (e >> 8) & 3, ln = (e >> 2) & 63, q = e & 3;
                const int row = 32 * (t0 + t) + (ln & 31), col = 8 * j + 4 * (ln >> 5) + q;
                tiles[e] = (row < M && col < F) ? bank[(size_t)row * F + col] : 0.f;
            }
            for (int e = tid; e < staged * 32; e += 256) {
                const int row = 32 * t0 + e;
                norms[e] = row < M ? bank_sq[row] : inf;
            }
            __syncthreads();
            for (int t = 0; t < staged; ++t) {
                f32x4 a[4], bs[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a[j] = *reinterpret_cast<const f32x4*>(tiles + t * KNN_TILE_FLOATS + (j * 64 + lane) * 4);
                    bs[j] = *reinterpret_cast<const f32x4*>(norms + t * 32 + 8 * j + 4 * h);
                }
#pragma unroll
                for (int g = 0; g < KNN_GROUPS; ++g) {
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].x, act[g][4 * j + 0], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].y, act[g][4 * j + 1], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].z, act[g][4 * j + 2], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].w, act[g][4 * j + 3], acc, 0, 0, 0);
                    }
                    float d[16];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        d[4 * j + 0] = fmaxf(0.f, fmaf(-2.f, acc[4 * j + 0], xx[g] + bs[j].x));
                        d[4 * j + 1] = fmaxf(0.f, fmaf(-2.f, acc[4 * j + 1], xx[g] + bs[j].y));
                        d[4 * j + 2] = fmaxf(0.f, fmaf(-2.f, acc[4 * j + 2], xx[g] + bs[j].z));
                        d[4 * j + 3] = fmaxf(0.f, fmaf(-2.f, acc[4 * j + 3], xx[g] + bs[j].w));
                    }
                    float least = d[0];
#pragma unroll
                    for (int r = 1; r < 16; ++r) least = fminf(least, d[r]);
                    if (least < best[g][K - 1]) {
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if (d[r] < best[g][K - 1]) knn_insert<K>(best[g], d[r]);
                    }
                }
            }
        }

#pragma unroll
        for (int g = 0; g < KNN_GROUPS; ++g) {
            float theirs[K];
#pragma unroll
            for (int i = 0; i < K; ++i) theirs[i] = __shfl_xor(best[g][i], 32);
#pragma unroll
            for (int i = 0; i < K; ++i) knn_insert<K>(best[g], theirs[i]);
            const size_t v = ((set * 4 + wave) * KNN_GROUPS + g) * 32 + n;
            if (v < nvox && h == 0) {
                score[v] = sqrtf(best[g][K - 1]);
                if (d2_out != nullptr) {
#pragma unroll
                    for (int i = 0; i < K; ++i) d2_out[v * K + i] = best[g][i];
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void knn_keys_kernel(size_t total, unsigned hw, const long long* __restrict__ slice_index, unsigned long long key,
                                                       long long* __restrict__ keys)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const size_t i = e / hw;
    const uint32_t v = (uint32_t)(e - i * hw);
    const unsigned long long g = (unsigned long long)slice_index[i];
    uint32_t w[4];
    philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), v, (uint32_t)g, (uint32_t)(g >> 32), 0x6b6e6eu, w);
    keys[e] = (long long)((((unsigned long long)w[0] << 32) | w[1]) >> 1);
}

template <int K>
hipError_t launch_distances(const float* x, int pitch, int F, size_t nvox, const float* bank, const float* bank_sq, int M, int normalize, float* score,
                            float* d2, hipStream_t stream)
{
    const size_t ngroups = (nvox + 31) / 32;
    const size_t nsets = (ngroups + 4 * KNN_GROUPS - 1) / (4 * KNN_GROUPS);
    const unsigned grid = (unsigned)(nsets < KNN_GRID_CAP ? nsets : KNN_GRID_CAP);
    hipLaunchKernelGGL(knn_distances_kernel<K>, dim3(grid), dim3(256), 0, stream, x, pitch, F, nvox, bank, bank_sq, M, normalize, score, d2);
    return hipGetLastError();
}

int invalid(const char* fn, const std::string& msg) { return report_error(RCU_ERR_INVALID, std::string(fn) + ": " + msg); }

}  // namespace
}  // namespace rcu

using namespace rcu;

extern "C" int rcu_knn_sample_keys(size_t n, size_t hw, const int64_t* slice_index_dev, uint64_t key, int64_t* keys_dev, void* stream)
{
    static const char* fn = "rcu_knn_sample_keys";
    if (!slice_index_dev || !keys_dev) return invalid(fn, "null argument (slice_index_dev, keys_dev)");
    const size_t limit = (size_t)1 << 31;
    if (n < 1 || hw < 1 || n > limit || hw > limit || n * hw > limit) return invalid(fn, "n and hw must be >= 1 and n * hw <= 2^31");
    if (reinterpret_cast<uintptr_t>(slice_index_dev) % 8 || reinterpret_cast<uintptr_t>(keys_dev) % 8)
        return invalid(fn, "slice_index_dev and keys_dev must be 8-byte aligned");
    const size_t total = n * hw;
    hipLaunchKernelGGL(knn_keys_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), total, (unsigned)hw,
                       reinterpret_cast<const long long*>(slice_index_dev), (unsigned long long)key, reinterpret_cast<long long*>(keys_dev));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_failed(fn, e);
    return RCU_OK;
}

extern "C" int rcu_knn_distances(const float* features_dev, int channel_pitch, int F, size_t n_voxels, const float* bank_dev, const float* bank_sq_dev,
                                 int M, int k, int normalize, float* score_dev, float* d2_dev, void* stream)
{
    static const char* fn = "rcu_knn_distances";
    if (!features_dev || !bank_dev || !bank_sq_dev || !score_dev) return invalid(fn, "null argument (features_dev, bank_dev, bank_sq_dev, score_dev)");
    if (F < 1 || F > RCU_KNN_MAX_FEATURES) return invalid(fn, "F must be in 1..32, got " + std::to_string(F));
    if (channel_pitch < F || channel_pitch % 4) return invalid(fn, "channel_pitch must be >= F and a multiple of 4, got " + std::to_string(channel_pitch));
    if (M < 1 || M > RCU_KNN_MAX_BANK) return invalid(fn, "M must be in 1..65536, got " + std::to_string(M));
    if (k < 1 || k > RCU_KNN_MAX_K) return invalid(fn, "k must be in 1..8, got " + std::to_string(k));
    if (k > M) return invalid(fn, "k = " + std::to_string(k) + " exceeds the bank's M = " + std::to_string(M) + " rows");
    if (normalize != 0 && normalize != 1) return invalid(fn, "normalize must be 0 or 1, got " + std::to_string(normalize));
    if (n_voxels < 1 || n_voxels > ((size_t)1 << 40)) return invalid(fn, "n_voxels must be in 1..2^40");
    if (reinterpret_cast<uintptr_t>(features_dev) % 16) return invalid(fn, "features_dev must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(bank_dev) % 4 || reinterpret_cast<uintptr_t>(bank_sq_dev) % 4 || reinterpret_cast<uintptr_t>(score_dev) % 4 ||
        reinterpret_cast<uintptr_t>(d2_dev) % 4)
        return invalid(fn, "bank_dev, bank_sq_dev, score_dev and d2_dev must be 4-byte aligned");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    switch (k) {
#define RCU_KNN_CASE(KK)                                                                                                                       \
    case KK:                                                                                                                                   \
        e = launch_distances<KK>(features_dev, channel_pitch, F, n_voxels, bank_dev, bank_sq_dev, M, normalize, score_dev, d2_dev, s);         \
        break;
        RCU_KNN_CASE(1) RCU_KNN_CASE(2) RCU_KNN_CASE(3) RCU_KNN_CASE(4) RCU_KNN_CASE(5) RCU_KNN_CASE(6) RCU_KNN_CASE(7) RCU_KNN_CASE(8)
#undef RCU_KNN_CASE
    }
    if (e != hipSuccess) return hip_failed(fn, e);
    return RCU_OK;
}
