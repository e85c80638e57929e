// Joint histogram of (uncertainty level, confusion cell) per volume (include/rcu.h, "Uncertainty-error level histogram"):
//   hist[volume][cell][level] += 1,   cell = tp 0, tn 1, fp 2, fn 3,   level(u) = #{k in 1..B-1 : u > (double)k / (double)B}
// for a prepared uncertainty map (float64 / float32: rcu_unc_hist) or for the normalised entropy of a float32 foreground-probability map,
// computed in registers with the arithmetic of rcu_normalised_entropy (rcu_entropy.h: rcu_unc_hist_from_p).  Everything is integer
// arithmetic: the result does not depend on how the voxels are split over lanes, waves, workgroups or launches.
//
// One workgroup = 4 waves (16 for B > 1365, see LDS) over `blocks_per_wg` consecutive blocks of 16,384 (65,536) voxels of one volume, read once with 16-byte non-temporal loads,
// 4 consecutive voxels per lane and round (the loads of 4 rounds in flight, the next 4 issued before these are worked on, as in
// unc_counts_sorted_kernel).  A volume starts at element v * n_per_volume, which need not be a multiple of 4: the 16-byte loads cover
// [head, head + body) with head = the 0..3 elements up to the first 16-byte boundary and body a multiple of 4; the head and the 0..3
// elements behind the body are read one by one by the volume's first workgroup.  Arrays whose base is not 16-byte (map) / 4-byte (labels)
// aligned are read element by element throughout.
//
// LDS: ONE histogram per workgroup, 4 x B u32 counters in the output's [cell][level] order (16 KB at B = 1000, 64 KB at B = 4096), and
// behind it the B + 1 float64 level boundaries (8 KB / 32 KB), copied from the table a small kernel writes into the workspace in front of
// the scan.  Of the CU's 160 KB that allows six workgroups per CU at B = 1000 (24 KB each; the kernel's ~100 registers allow four of 4
// waves: 16 waves per CU) and ONE at B = 4096 (96 KB): from B = 1366 on a workgroup therefore has 16 waves instead of 4 (and blocks of
// 65,536 voxels), so that the CU keeps its 16 waves.
//
// Levels.  bound[0] = -inf, bound[k] = t_k = k / B, bound[B] = +inf.  With y = x * scale - 0.5, c = clamp(int(y), 0, B - 1) is the level or
// the level below it (the real position lies in (level, level + 1], the arithmetic is good to 1e-12 of it and the margin is 0.5), so
// level = c + (x > bound[c + 1]):  one product, one LDS read, one compare -- the count of the definition, NaN and negatives at 0.
// From the probability map the entropy is compared IN NATS, before its division by log 2: h = s / log 2 is monotone in s (a correctly
// rounded division), so h > t_k <=> s > S_k with S_k = the largest float64 s whose quotient is <= t_k.  The table kernel finds S_k by
// stepping from t_k * log 2 to the neighbouring float64 values with that same division (rcu_entropy.h), and the scan saves a float64
// division per voxel while binning exactly what rcu_normalised_entropy + rcu_unc_hist bin.
//
// Aggregation rule (the input is peaked: nearly every voxel of a BraTS volume is a certain true negative, key [tn][0], tumour cores are
// certain true positives, and 64 lanes adding to one LDS address serialise): per voxel slot of the wave, the key of the wave's first
// lane is published, the lanes that hold the same key are counted with one ballot and lane 0 adds the count with ONE ds_add; the other
// lanes add 1 each with a plain LDS atomic in the same instruction (scattered keys: few collide).  A wave whose lanes share a key -- nearly
// all of a peaked volume -- costs one LDS add per slot; when the first lane happens to hold a rare key (3 % of the slots of a 97 %
// peaked, spatially unordered input) the others collide on one counter for that slot, which the average does not feel.
// At the end the workgroup adds its non-zero counters to the output with 64-bit global integer atomics (the launcher zeroes the output).
#include "../../include/rcu.h"
#include "rcu_kernels.h"
#include "rcu_entropy.h"

#include <cmath>
#include <string>
#include <type_traits>

namespace rcu {
namespace {

// Workgroup sizes: 4 waves, or 16 where the LDS of one workgroup (histogram + boundary table, 24 B + 8 bytes) leaves room for one or two
// workgroups per CU only -- B above UH_SMALL_LEVELS --, so that the CU still has 16 waves to hide the stream's latency with.
constexpr int UH_THREADS = 256, UH_THREADS_WIDE = 1024;
constexpr int UH_SMALL_LEVELS = 1365;       // 24 B + 8 <= 32 KB: five workgroups per CU by LDS, four by registers
constexpr int UH_ROUNDS = 16;               // rounds of 4 consecutive voxels per thread and block: a block is THREADS * 64 voxels
// Blocks one workgroup takes at most.  A u32 LDS counter holds at most every voxel of its workgroup: UH_MAX_BLOCKS blocks of at most
// 1024 * 64 voxels = 2^22, plus at most 6 head / tail voxels -- below 2^23, it cannot overflow.
constexpr unsigned UH_MAX_BLOCKS = 64;
constexpr unsigned UH_RULE_BLOCKS = 8;      // what the launcher's own rule gives at most (blocks_for)
constexpr int UH_MAX_VOLUMES = 65535;       // grid.y

enum Source { SRC_F32 = 0, SRC_F64 = 1, SRC_P = 2 };

int g_forced_blocks = 0;

// bound[0..B] = -inf, the boundaries of levels 1 .. B-1, +inf.  nats = 0: t_k = k / B itself (the map is compared as it is);
// nats = 1: S_k = max{s : s / log 2 <= t_k} (the entropy is compared before its division, see above)
__global__ __launch_bounds__(UH_THREADS) void unc_hist_bounds_kernel(double* __restrict__ bound, int B, int nats)
{
    const int k = blockIdx.x * UH_THREADS + threadIdx.x;
    if (k > B) return;
    double t = (double)k / (double)B;   // IEEE division: one rounding
    if (nats && k > 0 && k < B) {
        // t > 0, so is every candidate: the neighbouring float64 values are the neighbouring bit patterns
        auto next = [](double x) { return __longlong_as_double(__double_as_longlong(x) + 1); };
        auto prev = [](double x) { return __longlong_as_double(__double_as_longlong(x) - 1); };
        double s = t * ENTROPY_LOG2;
        for (int i = 0; i < 64 && normalised_entropy_of_nats(s) > t; ++i) s = prev(s);          // (a step or two: the product is within an ulp)
        for (int i = 0; i < 64 && normalised_entropy_of_nats(next(s)) <= t; ++i) s = next(s);
        t = s;
    }
    bound[k] = (k == 0) ? -INFINITY : (k == B) ? INFINITY : t;
}

// level = #{k in 1..B-1 : x > bound[k]} (NaN, negatives -> 0; x > bound[B-1] -> B - 1); scale = the levels per unit of x
__device__ __forceinline__ unsigned level_of(double x, double scale, int B, const double* bound)
{
    const unsigned c = (unsigned)(int)fmin(fmax(fma(x, scale, -0.5), 0.0), (double)(B - 1));   // fmax(NaN, 0) = 0
    return c + ((x > bound[c + 1]) ? 1u : 0u);
}

__device__ __forceinline__ void lds_add(unsigned* p, unsigned v)
{
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// One voxel slot of the wave into the workgroup's histogram (see the aggregation rule above).  Called by all 64 lanes together.  The
// published key is lane 0's own, so every adding lane adds at its own key: lane 0 the count of the lanes that share it, the others 1.
__device__ __forceinline__ void wave_add(unsigned* hist, unsigned key, bool active, int lane)
{
    const unsigned k0 = (unsigned)__builtin_amdgcn_readfirstlane((int)key);      // (lane 0 need not be active itself: its key is a guess)
    const bool same = active & (key == k0), other = active & !same;
    const unsigned count = (unsigned)__popcll(__ballot(same));
    const bool first = lane == 0;      // (lane 0 is never `other`: the published key is its own)
    if (other | (first & (count != 0u))) lds_add(hist + key, first ? count : 1u);
}

// MASK = false: no mask array (the evaluation's uncertainty-error scans use none): every voxel counts, and the compiler knows it
template <int SRC, int THREADS, bool MASK>
__global__ __launch_bounds__(THREADS) void unc_hist_kernel(const void* __restrict__ src, const uint8_t* __restrict__ pred,
                                                            const uint8_t* __restrict__ target, const uint8_t* __restrict__ mask, size_t n, int B,
                                                            double scale, const double* __restrict__ bound_dev, unsigned long long* __restrict__ out,
                                                            unsigned blocks_per_wg, unsigned nblocks, int vec)
{
    using T = typename std::conditional<SRC == SRC_F64, double, float>::type;
    constexpr size_t BLOCK = (size_t)THREADS * 4 * UH_ROUNDS;
    extern __shared__ double uh_lds[];                       // [B + 1] boundaries, then the histogram [cell][level]
    double* const bound = uh_lds;
    unsigned* const hist = reinterpret_cast<unsigned*>(uh_lds + B + 1);
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i <= B; i += THREADS) bound[i] = bound_dev[i];
    for (int i = tid; i < 4 * B; i += THREADS) hist[i] = 0u;
    __syncthreads();
    const size_t vol = blockIdx.y;
    const T* uv = reinterpret_cast<const T*>(src) + vol * n;
    const uint8_t* pv = pred + vol * n;
    const uint8_t* tv = target + vol * n;
    const uint8_t* mv = MASK ? mask + vol * n : nullptr;
    // [head, head + body): the elements read with 16-byte loads (vec); else everything goes element by element (head = 0, body = n)
    size_t head = 0, body = n;
    if (vec) {
        head = (4 - ((vol * n) & 3)) & 3;
        head = head < n ? head : n;
        body = (n - head) & ~(size_t)3;
    }
    // key = cell * B + level of a voxel whose cell is known
    auto key_of = [&](T x, unsigned cell) {
        double u;
        if constexpr (SRC == SRC_P) u = entropy_nats_of_p(x);      // compared before the division by log 2 (bound holds S_k)
        else u = (double)x;
        return __umul24(cell, (unsigned)B) + level_of(u, scale, B, bound);
    };
    // four voxels of a (prediction, target, mask) word triple, the byte logic done once per word: P, T, A = per byte 1 where the prediction /
    // target / mask byte is not 0; cell = 1 + 2 T + P - 4 P T per byte (tp 0, tn 1, fp 2, fn 3: no byte borrows).  The four keys first (their
    // table reads in flight together), then the four adds.
    auto nonzero_bytes = [](unsigned w) { return ((w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u; };
    auto add4 = [&](bool in, const T (&q)[4], unsigned p4, unsigned t4, unsigned m4) {
        const unsigned P = nonzero_bytes(p4), Tg = nonzero_bytes(t4), A = in ? (MASK ? nonzero_bytes(m4) : 0x01010101u) : 0u;
        const unsigned C = 0x01010101u + 2u * Tg + P - 4u * (P & Tg);
        unsigned key[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) key[k] = key_of(q[k], (C >> (8 * k)) & 0xffu);
#pragma unroll
        for (int k = 0; k < 4; ++k) wave_add(hist, key[k], ((A >> (8 * k)) & 1u) != 0u, lane);
    };
    auto add1 = [&](bool in, size_t e) {      // element e of the volume, read on its own (in: e < n)
        T x = (T)0;
        bool act = in, pr = false, tg = false;
        if (in) {
            x = uv[e];
            pr = pv[e] != 0;
            tg = tv[e] != 0;
            if (MASK) act = mv[e] != 0;
        }
        wave_add(hist, key_of(x, tg ? (pr ? 0u : 3u) : (pr ? 2u : 1u)), act, lane);
    };
    // the head and the tail around the 16-byte part: at most 3 + 3 elements, taken by the first wave of the volume's first workgroup
    if (vec && blockIdx.x == 0 && tid < 64) {
        const size_t tail = n - head - body;
        add1((size_t)tid < head + tail, (size_t)tid < head ? (size_t)tid : body + (size_t)tid);
    }
    constexpr int BATCH = (SRC == SRC_F64) ? 2 : 4;      // rounds whose loads are in flight together: 64 bytes of map per lane either way
    const unsigned blk_end = min((blockIdx.x + 1) * blocks_per_wg, nblocks);
    for (unsigned blk = blockIdx.x * blocks_per_wg; blk < blk_end; ++blk) {
        const size_t base = (size_t)blk * BLOCK;             // relative to the 16-byte part
        if (vec && base + BLOCK <= body) {
            // whole block: loads of BATCH rounds in flight together, those of the next BATCH rounds issued before this batch is worked on
            T q[2][BATCH][4];
            unsigned p4[2][BATCH], t4[2][BATCH], m4[2][BATCH];
            auto load = [&](int r0, int s) {
#pragma unroll
                for (int i = 0; i < BATCH; ++i) {
                    const size_t e = head + base + ((size_t)(r0 + i) * THREADS + tid) * 4;
                    load4(uv + e, q[s][i]);
                    p4[s][i] = stream_load(reinterpret_cast<const unsigned*>(pv + e));
                    t4[s][i] = stream_load(reinterpret_cast<const unsigned*>(tv + e));
                    m4[s][i] = MASK ? stream_load(reinterpret_cast<const unsigned*>(mv + e)) : 0x01010101u;
                }
            };
            load(0, 0);
#pragma unroll
            for (int g = 0; g < UH_ROUNDS / BATCH; ++g) {
                if (g + 1 < UH_ROUNDS / BATCH) load((g + 1) * BATCH, (g + 1) & 1);
#pragma unroll
                for (int i = 0; i < BATCH; ++i) add4(true, q[g & 1][i], p4[g & 1][i], t4[g & 1][i], m4[g & 1][i]);
            }
        } else if (vec) {
            for (int r = 0; r < UH_ROUNDS; ++r) {            // the last, partial block of the 16-byte part (body % 4 == 0)
                const size_t rel = base + ((size_t)r * THREADS + tid) * 4;
                const bool in = rel < body;
                T q[4] = {(T)0, (T)0, (T)0, (T)0};
                unsigned p4 = 0u, t4 = 0u, m4 = 0x01010101u;
                if (in) {
                    const size_t e = head + rel;
                    load4(uv + e, q);
                    p4 = *reinterpret_cast<const unsigned*>(pv + e);
                    t4 = *reinterpret_cast<const unsigned*>(tv + e);
                    if (MASK) m4 = *reinterpret_cast<const unsigned*>(mv + e);
                }
                add4(in, q, p4, t4, m4);
            }
        } else {
            for (int r = 0; r < 4 * UH_ROUNDS; ++r) {
                const size_t e = base + (size_t)r * THREADS + tid;
                add1(e < n, e);
            }
        }
    }
    __syncthreads();
    unsigned long long* const o = out + vol * 4 * (size_t)B;
    for (int i = tid; i < 4 * B; i += THREADS) {
        const unsigned c = hist[i];
        if (c != 0u) atomicAdd(o + i, (unsigned long long)c);      // integers: exact, whatever the order
    }
}

inline size_t lds_bytes(int levels) { return (size_t)(levels + 1) * sizeof(double) + (size_t)4 * levels * sizeof(unsigned); }

// Blocks per workgroup.  A workgroup zeroes and scans its 4 B counters once, whatever it streams, so a large launch lets it stream several
// blocks; a small one keeps the chip full: at least four rounds of workgroups stay.  `resident`: workgroups the chip holds at a time (256 CUs
// x what LDS and registers allow).  Measured at B = 1000 on 160 volumes (tools/ue_hist_bench.py --sweep-blocks): 1 block 1.05 ms, 2 to 8
// blocks 0.92-0.95, 16 blocks 0.98 (too few workgroups left for the tail): UH_RULE_BLOCKS caps the rule; forced values may go to UH_MAX_BLOCKS.
unsigned blocks_for(size_t total_blocks, int levels)
{
    if (g_forced_blocks >= 1) return (unsigned)g_forced_blocks < UH_MAX_BLOCKS ? (unsigned)g_forced_blocks : UH_MAX_BLOCKS;
    const size_t resident = 256 * (levels <= UH_SMALL_LEVELS ? 4 : 1);
    const size_t k = total_blocks / (4 * resident);
    return (unsigned)(k < 1 ? 1 : k > UH_RULE_BLOCKS ? UH_RULE_BLOCKS : k);
}

template <int SRC, int THREADS, bool MASK>
hipError_t launch_as(const void* src, const uint8_t* pred, const uint8_t* target, const uint8_t* mask, size_t n, int n_volumes, int B,
                     unsigned long long* out, double* bound, hipStream_t stream)
{
    const size_t lds = lds_bytes(B);
    if (lds > 48 * 1024) {
        const hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void*>(&unc_hist_kernel<SRC, THREADS, MASK>), (int)lds);
        if (e != hipSuccess) return e;
    }
    constexpr size_t BLOCK = (size_t)THREADS * 4 * UH_ROUNDS;
    const unsigned nblocks = (unsigned)((n + BLOCK - 1) / BLOCK);      // of the longest 16-byte part; a volume's own bounds are checked per round
    const unsigned bpw = blocks_for((size_t)nblocks * n_volumes, B);
    const unsigned gx = (nblocks + bpw - 1) / bpw;
    const int vec = (reinterpret_cast<uintptr_t>(src) % 16 == 0) && (reinterpret_cast<uintptr_t>(pred) % 4 == 0) &&
                    (reinterpret_cast<uintptr_t>(target) % 4 == 0) && (mask == nullptr || reinterpret_cast<uintptr_t>(mask) % 4 == 0);
    hipLaunchKernelGGL((unc_hist_kernel<SRC, THREADS, MASK>), dim3(gx, n_volumes), dim3(THREADS), lds, stream, src, pred, target, mask, n, B,
                       (SRC == SRC_P) ? (double)B / 0.6931471805599453 : (double)B, bound, out, bpw, nblocks, vec);
    return hipGetLastError();
}

template <int SRC>
hipError_t launch_src(const void* src, const uint8_t* pred, const uint8_t* target, const uint8_t* mask, size_t n, int n_volumes, int B,
                      unsigned long long* out, double* bound, hipStream_t stream)
{
    if (B <= UH_SMALL_LEVELS) {
        if (mask) return launch_as<SRC, UH_THREADS, true>(src, pred, target, mask, n, n_volumes, B, out, bound, stream);
        return launch_as<SRC, UH_THREADS, false>(src, pred, target, mask, n, n_volumes, B, out, bound, stream);
    }
    if (mask) return launch_as<SRC, UH_THREADS_WIDE, true>(src, pred, target, mask, n, n_volumes, B, out, bound, stream);
    return launch_as<SRC, UH_THREADS_WIDE, false>(src, pred, target, mask, n, n_volumes, B, out, bound, stream);
}

hipError_t launch(int source, const void* src, const uint8_t* pred, const uint8_t* target, const uint8_t* mask, size_t n, int n_volumes, int B,
                  unsigned long long* out, void* workspace, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(out, 0, (size_t)n_volumes * 4 * B * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    double* bound = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(unc_hist_bounds_kernel, dim3((unsigned)((B + 1 + UH_THREADS - 1) / UH_THREADS)), dim3(UH_THREADS), 0, stream, bound, B,
                       source == SRC_P ? 1 : 0);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    switch (source) {
    case SRC_F64: return launch_src<SRC_F64>(src, pred, target, mask, n, n_volumes, B, out, bound, stream);
    case SRC_F32: return launch_src<SRC_F32>(src, pred, target, mask, n, n_volumes, B, out, bound, stream);
    default: return launch_src<SRC_P>(src, pred, target, mask, n, n_volumes, B, out, bound, stream);
    }
}

// every argument, before anything touches the GPU
int check_args(const char* fn, const char* map_name, const void* map, const uint8_t* prediction, const uint8_t* target, size_t n, int n_volumes,
               int levels, const uint64_t* hist, const void* workspace)
{
    const std::string f = std::string(fn) + ": ";
    if (levels < 2 || levels > RCU_UNC_HIST_MAX_LEVELS)
        return report_error(RCU_ERR_INVALID, f + "levels must be in 2.." + std::to_string(RCU_UNC_HIST_MAX_LEVELS) + ", got " + std::to_string(levels));
    if (!map) return report_error(RCU_ERR_INVALID, f + "null " + map_name);
    if (!prediction) return report_error(RCU_ERR_INVALID, f + "null prediction_dev");
    if (!target) return report_error(RCU_ERR_INVALID, f + "null target_dev");
    if (!hist) return report_error(RCU_ERR_INVALID, f + "null hist_dev");
    if (!workspace) return report_error(RCU_ERR_INVALID, f + "null workspace_dev");
    if (n == 0) return report_error(RCU_ERR_INVALID, f + "n_per_volume must be >= 1");
    return check_n_volumes(f, n_volumes, UH_MAX_VOLUMES);
}

}  // namespace
}  // namespace rcu

using namespace rcu;

extern "C" size_t rcu_unc_hist_workspace_bytes(size_t n_per_volume, int n_volumes, int levels)
{
    (void)n_per_volume;
    (void)n_volumes;
    if (levels < 2 || levels > RCU_UNC_HIST_MAX_LEVELS) return 0;
    return (size_t)(levels + 1) * sizeof(double);      // the boundary table
}

extern "C" int rcu_unc_hist_set_blocks_per_workgroup(int blocks)
{
    if (blocks < 0) return report_error(RCU_ERR_INVALID, "rcu_unc_hist_set_blocks_per_workgroup: negative block count");
    g_forced_blocks = blocks;
    return RCU_OK;
}

extern "C" int rcu_unc_hist(const void* unc_dev, int unc_is_f64, const uint8_t* prediction_dev, const uint8_t* target_dev, const uint8_t* mask_dev,
                            size_t n_per_volume, int n_volumes, int levels, uint64_t* hist_dev, void* workspace_dev, void* stream)
{
    if (int st = check_args("rcu_unc_hist", "unc_dev", unc_dev, prediction_dev, target_dev, n_per_volume, n_volumes, levels, hist_dev, workspace_dev))
        return st;
    const hipError_t e = launch(unc_is_f64 ? SRC_F64 : SRC_F32, unc_dev, prediction_dev, target_dev, mask_dev, n_per_volume, n_volumes, levels,
                                reinterpret_cast<unsigned long long*>(hist_dev), workspace_dev, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_unc_hist", e);
}

extern "C" int rcu_unc_hist_from_p(const float* p_foreground_dev, const uint8_t* prediction_dev, const uint8_t* target_dev, const uint8_t* mask_dev,
                                   size_t n_per_volume, int n_volumes, int levels, uint64_t* hist_dev, void* workspace_dev, void* stream)
{
    if (int st = check_args("rcu_unc_hist_from_p", "p_foreground_dev", p_foreground_dev, prediction_dev, target_dev, n_per_volume, n_volumes, levels,
                            hist_dev, workspace_dev))
        return st;
    const hipError_t e = launch(SRC_P, p_foreground_dev, prediction_dev, target_dev, mask_dev, n_per_volume, n_volumes, levels,
                                reinterpret_cast<unsigned long long*>(hist_dev), workspace_dev, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_unc_hist_from_p", e);
}
