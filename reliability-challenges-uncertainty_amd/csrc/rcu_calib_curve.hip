// Calibration level histogram per volume (include/rcu.h, "Calibration level histogram"):
//   levels[volume][0 | 1][level] += 1  (target == 0 | target != 0),   levels[volume][2][level] += Q(p),   level(p) = #{k in 1..B-1 : p >= t_k}
//   totals[volume][y] += (1, Q(p), Q2(p), N(p, y))
// from a float32 foreground-probability map, with the float32 thresholds t_k of rcu_ece_thresholds extended to B levels.  Everything that is
// added is an integer: the result does not depend on how the voxels are split over lanes, waves, workgroups or launches.
//
// The plan is rcu_unc_hist.hip's (read its header first): one workgroup = 4 waves (16 for B > 1365) over `blocks_per_wg` consecutive blocks of
// 16,384 (65,536) voxels of one volume, read once with 16-byte non-temporal loads (4 consecutive voxels per lane and round, the loads of 4
// rounds in flight and the next 4 issued before these are worked on); the 0..3 elements in front of the first 16-byte boundary of a volume
// and the 0..3 behind the last are read one by one by the volume's first workgroup, arrays whose bases are not 16-byte (p) / 4-byte (target,
// mask) aligned element by element throughout.
//
// LDS: ONE histogram per workgroup -- B u64 sums of Q (plane 2), 2 x B u32 counters (planes 0, 1) and the B + 1 float32 thresholds
// (thr[0] = -inf, thr[k] = t_k, thr[B] = +inf; a small kernel writes them into the workspace in front of the scan): 20 B + 4 bytes, 20 KB at
// B = 1000, 80 KB at B = 4096.  The narrow / wide switch is kept where the uncertainty histogram has it (B > 1365: 16 waves and blocks of
// 65,536 voxels, so that a CU whose LDS holds one or two workgroups still has its 16 waves).
//
// Levels.  With y = p * (B / (1 + 1e-8)) - 0.5 in float32, c = clamp(int(y), 0, B - 1) is the level or the level below it (the real position
// lies in [level, level + 1), the float32 arithmetic is good to 3e-4 of it at B = 4096 and the margin is 0.5), so
// level = min(c + (p >= thr[c + 1]), B - 1): one fma, one LDS read, one compare -- NaN and negatives at 0, p >= 1 (and +inf) at B - 1.
//
// Aggregation rule.  The input is as peaked as the uncertainty histogram's (nearly every voxel of a BraTS volume has p near 0: level 0), and
// here a level takes a SUM of 64 different Q, not a count that one ballot gives.  Mechanism: a wave keeps one HOT level h (wave-uniform, it
// starts at 0).  Voxels of the hot level never touch LDS: their two counts are ballot pop-counts added to two scalars, their Q goes
// into a per-lane 64-bit register sum.  Voxels of other levels add 1 and Q with two plain LDS atomics (ds_add_u32, ds_add_u64: scattered
// keys, few collide).  Only when the hot level is given up, and at the end of the workgroup, the register sums are reduced over the wave with
// a butterfly of six __shfl_xor steps on the 64-bit value (ds_bpermute / DPP, no LDS memory) and lane 0 adds the three numbers to LDS.  The hot
// level is given up when, in a batch of 16 voxel slots (4 in the slow paths), fewer than half of the wave's voxels had it: h := the level of
// lane 0's last voxel.  A peaked volume therefore costs a reduction per workgroup, a uniform one a reduction per 1,024 voxels.
// The class totals are per-lane register sums (all voxels, and those with target != 0: class 0 is the difference), reduced with the same
// butterfly once per wave, added to eight LDS words per workgroup, and from there to the output.  The workgroup adds its non-zero counters to
// the zeroed outputs with 64-bit global integer atomics.
#include "../../include/rcu.h"
#include "rcu_kernels.h"

#include <cmath>
#include <string>

namespace rcu {
namespace {

constexpr int CC_THREADS = 256, CC_THREADS_WIDE = 1024;
constexpr int CC_SMALL_LEVELS = 1365;       // as rcu_unc_hist.hip; 20 B + 4 <= 27 KB up to here: five workgroups per CU by LDS, four by registers
constexpr int CC_ROUNDS = 16;               // rounds of 4 consecutive voxels per thread and block: a block is THREADS * 64 voxels
constexpr int CC_BATCH = 4;                 // rounds whose loads are in flight together
// Blocks one workgroup takes at most.  A u32 LDS counter holds at most every voxel of its workgroup: CC_MAX_BLOCKS blocks of at most
// 1024 * 64 voxels = 2^22, plus at most 6 head / tail voxels -- below 2^23; a u64 sum of Q <= 2^32 each stays below 2^55.
constexpr unsigned CC_MAX_BLOCKS = 64;
constexpr unsigned CC_RULE_BLOCKS = 8;
constexpr int CC_MAX_VOLUMES = 65535;       // grid.y
constexpr float CC_P_FLOOR = 1.1920928955078125e-07f;      // 2^-23
constexpr float CC_L_MAX = 15.942385152878742f;            // 23 ln 2
constexpr float CC_N_SCALE = 1048576.f;                    // 2^20

int g_forced_blocks = 0;

// t_k: the smallest float32 >= k * ((1 + 1e-8) / B) -- rcu_ece_thresholds' arithmetic (IEEE float64 division and product: host and device agree)
__host__ __device__ inline float threshold_of(int k, int B)
{
    const double step = (1.0 + 1e-8) / (double)B;
    const double edge = (double)k * step;
    float t = (float)edge;
    if ((double)t < edge) {      // t > 0: the next float32 up is the next bit pattern
#if defined(__HIP_DEVICE_COMPILE__)
        t = __uint_as_float(__float_as_uint(t) + 1u);
#else
        t = std::nextafterf(t, INFINITY);
#endif
    }
    return t;
}

__global__ __launch_bounds__(CC_THREADS) void calib_curve_thresholds_kernel(float* __restrict__ thr, int B)
{
    const int k = blockIdx.x * CC_THREADS + threadIdx.x;
    if (k > B) return;
    thr[k] = (k == 0) ? -INFINITY : (k == B) ? INFINITY : threshold_of(k, B);
}

__device__ __forceinline__ float level_scale(int B) { return (float)((double)B / (1.0 + 1e-8)); }

// the level below the voxel's, or its level (see "Levels" above)
__device__ __forceinline__ unsigned level_guess(float p, float scale, int B)
{
    return (unsigned)(int)fminf(fmaxf(fmaf(p, scale, -0.5f), 0.f), (float)(B - 1));      // fmaxf(NaN, 0) = 0
}
__device__ __forceinline__ unsigned level_from(float p, unsigned c, float upper, int B)     // upper = thr[c + 1]
{
    return min(c + ((p >= upper) ? 1u : 0u), (unsigned)(B - 1));
}

// rint(x * 2^32) for x in [0, 1] as an integer (v_cvt_u32_f64 stops at 2^32 - 1: only x = 1 lies above)
__device__ __forceinline__ unsigned long long fixed32(double x)
{
    const double d = rint(x * 4294967296.0);
    return d >= 4294967296.0 ? 4294967296ull : (unsigned long long)(unsigned)d;
}
__device__ __forceinline__ double clamp01(float p) { return fmin(fmax((double)p, 0.0), 1.0); }      // fmax(NaN, 0) = 0
// l of a voxel: -log of the probability of its class, floored at 2^-23 (rcu_temperature_nll's convention), in [0, 23 ln 2]
__device__ __forceinline__ float nll_term(float p, bool y)
{
    const float py = y ? p : 1.0f - p;
    return fminf(fmaxf(-logf(fmaxf(py, CC_P_FLOOR)), 0.f), CC_L_MAX);
}
__device__ __forceinline__ unsigned nll_fixed(float l) { return (unsigned)rintf(l * CC_N_SCALE); }      // l * 2^20 < 2^24: exact, ties to even

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}
__device__ __forceinline__ void lds_add(unsigned* p, unsigned v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_add(unsigned long long* p, unsigned long long v)
{
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// what a wave carries between voxel slots: the hot level with its pending sums, and the class totals of its lanes -- everything but `hot` per lane
struct WaveState {
    unsigned hot;                      // wave-uniform
    unsigned hot_n, hot_n1;            // voxels of the hot level not yet in LDS: all, and those with target != 0
    unsigned seen_hot, seen;           // of the running batch
    unsigned long long hot_q;          // Q of the voxels of the hot level, not yet in LDS
    unsigned n_all, n_pos;
    unsigned long long q_all, q_pos, q2_all, q2_pos, nl_all, nl_pos;
};

struct Scan {
    unsigned long long* sumq;          // [B]
    unsigned* count;                   // [2][B]
    int B, lane;
    WaveState w;

    // one voxel slot of the wave (all 64 lanes together); `level` was made by level_from
    __device__ __forceinline__ void add(float p, unsigned level, bool y, bool active)
    {
        const double x = clamp01(p);
        const unsigned long long q = active ? fixed32(x) : 0ull, q2 = active ? fixed32(x * x) : 0ull;
        const unsigned long long nl = active ? (unsigned long long)nll_fixed(nll_term(p, y)) : 0ull;
        const bool pos = active & y;
        w.n_all += active ? 1u : 0u, w.n_pos += pos ? 1u : 0u;
        w.q_all += q, w.q_pos += pos ? q : 0ull;
        w.q2_all += q2, w.q2_pos += pos ? q2 : 0ull;
        w.nl_all += nl, w.nl_pos += pos ? nl : 0ull;
        const bool hot = active & (level == w.hot);
        w.hot_n += hot ? 1u : 0u, w.hot_n1 += (hot & y) ? 1u : 0u;
        w.hot_q += hot ? q : 0ull;
        w.seen += active ? 1u : 0u;
        if (active & !hot) {
            lds_add(count + (y ? (unsigned)B : 0u) + level, 1u);
            lds_add(sumq + level, q);
        }
    }
    // the pending sums of the hot level -> LDS (all 64 lanes together)
    __device__ __forceinline__ void flush()
    {
        if (__ballot(w.hot_n != 0u)) {      // wave-uniform
            const unsigned long long q = wave_sum(w.hot_q);
            const unsigned long long n = wave_sum(((unsigned long long)w.hot_n1 << 32) | w.hot_n);      // two sums below 2^32 in one butterfly
            if (lane == 0) {
                const unsigned n1 = (unsigned)(n >> 32), n0 = (unsigned)n - n1;
                if (n0) lds_add(count + w.hot, n0);
                if (n1) lds_add(count + B + w.hot, n1);
                if (q) lds_add(sumq + w.hot, q);
            }
        }
        w.hot_n = w.hot_n1 = 0u;
        w.hot_q = 0ull;
    }
    // end of a batch of slots: the hot level is given up when more than half of the lanes that had voxels in the batch found it at fewer
    // than half of theirs (one ballot pair per batch instead of counts per slot); `candidate`: a level of this lane
    __device__ __forceinline__ void end_batch(unsigned candidate)
    {
        const unsigned long long had = __ballot(w.seen != 0u), cold = __ballot(2u * (w.hot_n - w.seen_hot) < w.seen);
        if (2 * __popcll(cold) > __popcll(had)) {      // wave-uniform
            flush();
            w.hot = (unsigned)__builtin_amdgcn_readfirstlane((int)candidate);
        }
        w.seen_hot = w.hot_n;
        w.seen = 0u;
    }
};

template <int THREADS, bool MASK>
__global__ __launch_bounds__(THREADS, 4) void calib_curve_kernel(const float* __restrict__ p, const uint8_t* __restrict__ target,
                                                               const uint8_t* __restrict__ mask, size_t n, int B, const float* __restrict__ thr_dev,
                                                               unsigned long long* __restrict__ levels_out, unsigned long long* __restrict__ totals_out,
                                                               unsigned blocks_per_wg, unsigned nblocks, int vec)
{
    constexpr size_t BLOCK = (size_t)THREADS * 4 * CC_ROUNDS;
    extern __shared__ unsigned long long cc_lds[];           // [B] sums of Q, [8] class totals, then [2][B] u32 counts, then [B + 1] float thresholds
    unsigned long long* const sumq = cc_lds;
    unsigned long long* const tot = cc_lds + B;
    unsigned* const count = reinterpret_cast<unsigned*>(cc_lds + B + 8);
    float* const thr = reinterpret_cast<float*>(count + 2 * B);
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < B + 8; i += THREADS) cc_lds[i] = 0ull;
    for (int i = tid; i < 2 * B; i += THREADS) count[i] = 0u;
    for (int i = tid; i <= B; i += THREADS) thr[i] = thr_dev[i];
    __syncthreads();
    const size_t vol = blockIdx.y;
    const float* pv = p + vol * n;
    const uint8_t* tv = target + vol * n;
    const uint8_t* mv = MASK ? mask + vol * n : nullptr;
    size_t head = 0, body = n;
    if (vec) {
        head = (4 - ((vol * n) & 3)) & 3;
        head = head < n ? head : n;
        body = (n - head) & ~(size_t)3;
    }
    Scan s;
    s.sumq = sumq, s.count = count, s.B = B, s.lane = lane;
    const float scale = level_scale(B);
    s.w = WaveState{};
    auto nonzero_bytes = [](unsigned w) { return ((w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u; };
    // four voxels of a (target, mask) word pair: the four table reads first (in flight together), then the four adds; -> the last level
    auto add4 = [&](bool in, const float (&q)[4], unsigned t4, unsigned m4) {
        const unsigned Tg = nonzero_bytes(t4), A = in ? (MASK ? nonzero_bytes(m4) : 0x01010101u) : 0u;
        unsigned c[4];
        float up[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = level_guess(q[k], scale, B), up[k] = thr[c[k] + 1];
        unsigned level = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            level = level_from(q[k], c[k], up[k], B);
            s.add(q[k], level, ((Tg >> (8 * k)) & 1u) != 0u, ((A >> (8 * k)) & 1u) != 0u);
        }
        return level;
    };
    auto add1 = [&](bool in, size_t e) {      // element e of the volume, read on its own (in: e < n)
        float x = 0.f;
        bool act = in, tg = false;
        if (in) {
            x = pv[e];
            tg = tv[e] != 0;
            if (MASK) act = mv[e] != 0;
        }
        const unsigned c = level_guess(x, scale, B);
        const unsigned level = level_from(x, c, thr[c + 1], B);
        s.add(x, level, tg, act);
        return level;
    };
    // the head and the tail around the 16-byte part: at most 3 + 3 elements, taken by the first wave of the volume's first workgroup
    if (vec && blockIdx.x == 0 && tid < 64) {
        const size_t tail = n - head - body;
        s.end_batch(add1((size_t)tid < head + tail, (size_t)tid < head ? (size_t)tid : body + (size_t)tid));
    }
    const unsigned blk_end = min((blockIdx.x + 1) * blocks_per_wg, nblocks);
    for (unsigned blk = blockIdx.x * blocks_per_wg; blk < blk_end; ++blk) {
        const size_t base = (size_t)blk * BLOCK;             // relative to the 16-byte part
        if (vec && base + BLOCK <= body) {
            // A queue of CC_BATCH rounds in flight: each turn takes the oldest round, moves the others up (18 register moves) and issues the load
            // of round r + CC_BATCH behind them.  The loop is NOT unrolled: unrolled, the compiler does the LDS adds of all 64 voxel slots of a
            // block first and keeps every slot's Q, level and flags alive for the register sums behind them (256 registers and spills).
            float q[4], qn[CC_BATCH][4];
            unsigned t4, m4, t4n[CC_BATCH], m4n[CC_BATCH];
            auto load = [&](int r, int slot) {
                const size_t e = head + base + ((size_t)r * THREADS + tid) * 4;
                load4(pv + e, qn[slot]);
                t4n[slot] = stream_load(reinterpret_cast<const unsigned*>(tv + e));
                m4n[slot] = MASK ? stream_load(reinterpret_cast<const unsigned*>(mv + e)) : 0x01010101u;
            };
#pragma unroll
            for (int i = 0; i < CC_BATCH; ++i) load(i, i);
#pragma unroll 1
            for (int r = 0; r < CC_ROUNDS; ++r) {
#pragma unroll
                for (int k = 0; k < 4; ++k) q[k] = qn[0][k];
                t4 = t4n[0], m4 = m4n[0];
#pragma unroll
                for (int i = 0; i + 1 < CC_BATCH; ++i) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) qn[i][k] = qn[i + 1][k];
                    t4n[i] = t4n[i + 1], m4n[i] = m4n[i + 1];
                }
                if (r + CC_BATCH < CC_ROUNDS) load(r + CC_BATCH, CC_BATCH - 1);
                const unsigned level = add4(true, q, t4, m4);
                if ((r & 3) == 3) s.end_batch(level);
            }
        } else if (vec) {
#pragma unroll 1
            for (int r = 0; r < CC_ROUNDS; ++r) {            // the last, partial block of the 16-byte part (body % 4 == 0)
                const size_t rel = base + ((size_t)r * THREADS + tid) * 4;
                const bool in = rel < body;
                float q[4] = {0.f, 0.f, 0.f, 0.f};
                unsigned t4 = 0u, m4 = 0x01010101u;
                if (in) {
                    const size_t e = head + rel;
                    load4(pv + e, q);
                    t4 = *reinterpret_cast<const unsigned*>(tv + e);
                    if (MASK) m4 = *reinterpret_cast<const unsigned*>(mv + e);
                }
                s.end_batch(add4(in, q, t4, m4));
            }
        } else {
#pragma unroll 1
            for (int r = 0; r < 4 * CC_ROUNDS; ++r) {
                const size_t e = base + (size_t)r * THREADS + tid;
                const unsigned level = add1(e < n, e);
                if ((r & 3) == 3) s.end_batch(level);
            }
        }
    }
    s.flush();
    // class totals: per wave, then per workgroup through eight LDS words
    {
        const WaveState& w = s.w;
        const unsigned long long t8[8] = {wave_sum(w.n_all), wave_sum(w.q_all), wave_sum(w.q2_all), wave_sum(w.nl_all),
                                          wave_sum(w.n_pos), wave_sum(w.q_pos), wave_sum(w.q2_pos), wave_sum(w.nl_pos)};
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (t8[i]) lds_add(tot + i, t8[i]);
        }
    }
    __syncthreads();
    unsigned long long* const o = levels_out + vol * 3 * (size_t)B;
    for (int i = tid; i < 2 * B; i += THREADS) {
        const unsigned c = count[i];
        if (c != 0u) atomicAdd(o + i, (unsigned long long)c);      // integers: exact, whatever the order
    }
    for (int i = tid; i < B; i += THREADS) {
        const unsigned long long q = sumq[i];
        if (q != 0ull) atomicAdd(o + 2 * (size_t)B + i, q);
    }
    if (tid < 4) {      // [y][n, Q, Q2, N]: class 1 as summed, class 0 = all - class 1
        const unsigned long long all = tot[tid], pos = tot[4 + tid];
        unsigned long long* const t = totals_out + vol * 8;
        if (all - pos) atomicAdd(t + tid, all - pos);
        if (pos) atomicAdd(t + 4 + tid, pos);
    }
}

__global__ __launch_bounds__(CC_THREADS) void calib_curve_terms_kernel(const float* __restrict__ p, const uint8_t* __restrict__ target, size_t n,
                                                                        int B, int32_t* __restrict__ level, float* __restrict__ nll)
{
    const float scale = level_scale(B);
    for (size_t i = (size_t)blockIdx.x * CC_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * CC_THREADS) {
        const float x = p[i];
        const unsigned c = level_guess(x, scale, B);
        const float upper = (c + 1 == (unsigned)B) ? INFINITY : threshold_of((int)c + 1, B);      // what the scan reads from its table
        level[i] = (int32_t)level_from(x, c, upper, B);
        nll[i] = nll_term(x, target[i] != 0);
    }
}

inline size_t lds_bytes(int levels) { return (size_t)(levels + 8) * 8 + (size_t)2 * levels * 4 + (size_t)(levels + 1) * 4; }

// as rcu_unc_hist.hip's rule: a workgroup zeroes and scans its LDS once whatever it streams; at least four rounds of workgroups stay
unsigned blocks_for(size_t total_blocks, int levels)
{
    if (g_forced_blocks >= 1) return (unsigned)g_forced_blocks < CC_MAX_BLOCKS ? (unsigned)g_forced_blocks : CC_MAX_BLOCKS;
    const size_t resident = 256 * (levels <= CC_SMALL_LEVELS ? 4 : 1);
    const size_t k = total_blocks / (4 * resident);
    return (unsigned)(k < 1 ? 1 : k > CC_RULE_BLOCKS ? CC_RULE_BLOCKS : k);
}

template <int THREADS, bool MASK>
hipError_t launch_as(const float* p, const uint8_t* target, const uint8_t* mask, size_t n, int n_volumes, int B, const float* thr,
                     unsigned long long* levels_out, unsigned long long* totals_out, hipStream_t stream)
{
    const size_t lds = lds_bytes(B);
    if (lds > 48 * 1024) {
        const hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void*>(&calib_curve_kernel<THREADS, MASK>), (int)lds);
        if (e != hipSuccess) return e;
    }
    constexpr size_t BLOCK = (size_t)THREADS * 4 * CC_ROUNDS;
    const unsigned nblocks = (unsigned)((n + BLOCK - 1) / BLOCK);      // of the longest 16-byte part; a volume's own bounds are checked per round
    const unsigned bpw = blocks_for((size_t)nblocks * n_volumes, B);
    const unsigned gx = (nblocks + bpw - 1) / bpw;
    const int vec = (reinterpret_cast<uintptr_t>(p) % 16 == 0) && (reinterpret_cast<uintptr_t>(target) % 4 == 0) &&
                    (mask == nullptr || reinterpret_cast<uintptr_t>(mask) % 4 == 0);
    hipLaunchKernelGGL((calib_curve_kernel<THREADS, MASK>), dim3(gx, n_volumes), dim3(THREADS), lds, stream, p, target, mask, n, B, thr, levels_out,
                       totals_out, bpw, nblocks, vec);
    return hipGetLastError();
}

hipError_t launch(const float* p, const uint8_t* target, const uint8_t* mask, size_t n, int n_volumes, int B, unsigned long long* levels_out,
                  unsigned long long* totals_out, void* workspace, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(levels_out, 0, (size_t)n_volumes * 3 * B * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(totals_out, 0, (size_t)n_volumes * 8 * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    float* thr = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(calib_curve_thresholds_kernel, dim3((unsigned)((B + 1 + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, stream, thr, B);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (B <= CC_SMALL_LEVELS) {
        if (mask) return launch_as<CC_THREADS, true>(p, target, mask, n, n_volumes, B, thr, levels_out, totals_out, stream);
        return launch_as<CC_THREADS, false>(p, target, mask, n, n_volumes, B, thr, levels_out, totals_out, stream);
    }
    if (mask) return launch_as<CC_THREADS_WIDE, true>(p, target, mask, n, n_volumes, B, thr, levels_out, totals_out, stream);
    return launch_as<CC_THREADS_WIDE, false>(p, target, mask, n, n_volumes, B, thr, levels_out, totals_out, stream);
}

bool levels_ok(int levels) { return levels >= 2 && levels <= RCU_CALIB_CURVE_MAX_LEVELS; }
int bad_levels(const std::string& f, int levels)
{
    return report_error(RCU_ERR_INVALID, f + "levels must be in 2.." + std::to_string(RCU_CALIB_CURVE_MAX_LEVELS) + ", got " + std::to_string(levels));
}

}  // namespace
}  // namespace rcu

using namespace rcu;

extern "C" int rcu_calib_curve_thresholds(int levels, float* thr_host)
{
    if (!levels_ok(levels)) return bad_levels("rcu_calib_curve_thresholds: ", levels);
    if (!thr_host) return report_error(RCU_ERR_INVALID, "rcu_calib_curve_thresholds: null thr_host");
    for (int k = 1; k < levels; ++k) thr_host[k - 1] = threshold_of(k, levels);
    return RCU_OK;
}

extern "C" size_t rcu_calib_curve_workspace_bytes(size_t n_per_volume, int n_volumes, int levels)
{
    (void)n_per_volume;
    (void)n_volumes;
    if (!levels_ok(levels)) return 0;
    return round256((size_t)(levels + 1) * sizeof(float));      // the threshold table
}

extern "C" int rcu_calib_curve_set_blocks_per_workgroup(int blocks)
{
    if (blocks < 0) return report_error(RCU_ERR_INVALID, "rcu_calib_curve_set_blocks_per_workgroup: negative block count");
    g_forced_blocks = blocks;
    return RCU_OK;
}

extern "C" int rcu_calib_curve(const float* p_foreground_dev, const uint8_t* target_dev, const uint8_t* mask_dev, size_t n_per_volume, int n_volumes,
                               int levels, uint64_t* levels_dev, uint64_t* totals_dev, void* workspace_dev, void* stream)
{
    // every argument, before anything touches the GPU
    const std::string f = "rcu_calib_curve: ";
    if (!levels_ok(levels)) return bad_levels(f, levels);
    if (!p_foreground_dev) return report_error(RCU_ERR_INVALID, f + "null p_foreground_dev");
    if (!target_dev) return report_error(RCU_ERR_INVALID, f + "null target_dev");
    if (!levels_dev) return report_error(RCU_ERR_INVALID, f + "null levels_dev");
    if (!totals_dev) return report_error(RCU_ERR_INVALID, f + "null totals_dev");
    if (!workspace_dev) return report_error(RCU_ERR_INVALID, f + "null workspace_dev");
    if (n_per_volume == 0) return report_error(RCU_ERR_INVALID, f + "n_per_volume must be >= 1");
    if (int st = check_n_volumes(f, n_volumes, CC_MAX_VOLUMES)) return st;
    const hipError_t e = launch(p_foreground_dev, target_dev, mask_dev, n_per_volume, n_volumes, levels, reinterpret_cast<unsigned long long*>(levels_dev),
                                reinterpret_cast<unsigned long long*>(totals_dev), workspace_dev, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_calib_curve", e);
}

extern "C" int rcu_calib_curve_terms(const float* p_foreground_dev, const uint8_t* target_dev, size_t n, int levels, int32_t* level_dev, float* nll_dev,
                                     void* stream)
{
    const std::string f = "rcu_calib_curve_terms: ";
    if (!levels_ok(levels)) return bad_levels(f, levels);
    if (!p_foreground_dev) return report_error(RCU_ERR_INVALID, f + "null p_foreground_dev");
    if (!target_dev) return report_error(RCU_ERR_INVALID, f + "null target_dev");
    if (!level_dev) return report_error(RCU_ERR_INVALID, f + "null level_dev");
    if (!nll_dev) return report_error(RCU_ERR_INVALID, f + "null nll_dev");
    if (n == 0) return report_error(RCU_ERR_INVALID, f + "n must be >= 1");
    const size_t want = (n + CC_THREADS - 1) / CC_THREADS;
    hipLaunchKernelGGL(calib_curve_terms_kernel, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(CC_THREADS), 0, static_cast<hipStream_t>(stream),
                       p_foreground_dev, target_dev, n, levels, level_dev, nll_dev);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_calib_curve_terms", e);
}
