// Quantile rescale (include/rcu.h, "Quantile rescale"): one radix pass of an exact multi-quantile selection over float32 volumes
// (rcu_key_hist) and the rank transform of a map under a table of boundary keys (rcu_quantile_apply).
//   key(u)  = the order-preserving uint32 of the float32 value, -0.0 taken as +0.0; NaN has no key and is counted
//   pass    : hi = key >> (shift + bits), slot = index of hi in the sorted table of selected prefixes (no table: slot 0), voxels whose hi is
//             not listed are skipped, digit = (key >> shift) & (2^bits - 1), out[slot][digit] += 1  (int64, ADDED to what out holds)
//   apply   : l(u) = #{k in 1..Q-1 : key(u) > b_k}, out = (float)((l + 0.5) / Q) with the quotient in float64
// Everything rcu_key_hist adds is an integer: the table carries the same bits whatever the launch geometry, the batching, the alignment
// of the pointers or the order of the volumes.
//
// rcu_key_hist.  One workgroup = 4 waves over `blocks_per_wg` consecutive blocks of 16,384 voxels of one volume, as rcu_unc_hist.hip
// streams them: 16-byte non-temporal loads, 4 consecutive voxels per lane and round, the loads of 4 rounds (and their 4 mask words) in
// flight together; [head, head + body) is the part of a volume the 16-byte loads cover, the 0..3 elements before and behind it are read
// one by one by the volume's first wave; a map that is not 16-byte (a mask that is not 4-byte) aligned is read element by element.
// LDS: two u32 counters (NaN, population), the prefix table (at most 4095 entries: 16 KB, searched with a branch-free binary search)
// and, where there is no or one prefix, ONE histogram of the slot per workgroup: u32 counters flushed once for bits <= 12 (16 KB), u16
// counters packed two to a word and flushed after every block for wider digits (128 KB at 16 bits, 16 waves per workgroup; see Mode).
// (Measured first without the packed form: the 16-bit first pass of the default plan went through the global walk below and its atomics
// piled up on the few thousand counters a real map populates -- 21.3 ms on 8 native volumes of log-normal values, 8 x a sort of them.)
//
// Aggregation, per voxel slot of the wave (all 64 lanes together).  A wave keeps a RUN in scalar registers: a pair (slot, digit) and a
// count.  The lanes that hold the run's pair are found with one ballot and counted with one popcount -- no memory traffic at all.  A
// slot in which nobody holds it flushes the run (one add by lane 0) and adopts the pair of the first active lane.  The lanes left over
//   LDS forms   add 1 each to the workgroup's histogram (scattered pairs: few collide),
//   global form are walked as rcu_cc_pairs.hip walks its keys: the first remaining lane leads, the lanes with its pair are found with a
//               ballot, the leader ALONE adds the popcount with one 64-bit global atomic, the lanes are cleared.
// So the tie-heavy input (a BraTS map is 85 % one value) is the CHEAP case: a wave inside the ties issues no atomic until its run ends,
// and a wave that meets the tie value among others keeps it as its run.  Scattered input costs one atomic per distinct pair, wave and slot.
//
// rcu_quantile_apply.  The Q - 1 boundary keys and the Q output values sit in LDS (32 KB at Q = 4096), the values made once per workgroup
// with the float64 division of the definition.  A voxel's level is a branch-free binary search (12 steps at Q = 4096); its output is a
// function of its value and the table alone.  16 bytes per lane in and out (8 for the uint16 levels) where input and outputs share their
// misalignment, element by element otherwise.  NaN -> level 0.
#include "../../include/rcu.h"
#include "rcu_kernels.h"

#include <string>

namespace rcu {
namespace {

// Where a pair's count goes: straight to the global table, or into ONE histogram per workgroup in LDS when a whole slot fits it (no or one
// prefix) -- u32 counters up to 2^12 digits (16 KB), and for wider digits, up to 2^16, u16 counters packed two to a word (128 KB: one
// workgroup of 16 waves per CU).  A packed counter holds at most the voxels of ONE block of its workgroup (32,768 + 6 head / tail elements
// < 2^16): the workgroup flushes and zeroes its histogram after every block, so the low half of a word never carries into the high one.
enum Mode { MODE_GLOBAL = 0, MODE_LDS = 1, MODE_LDS_PACKED = 2 };
template <int MODE>
struct KhGeometry {
    static constexpr int THREADS = MODE == MODE_LDS_PACKED ? 1024 : 256;
    static constexpr int ROUNDS = MODE == MODE_LDS_PACKED ? 8 : 16;      // rounds of 4 consecutive voxels per thread and block
    static constexpr size_t BLOCK = (size_t)THREADS * 4 * ROUNDS;        // 16,384 voxels (packed: 32,768)
};
static_assert(KhGeometry<MODE_LDS_PACKED>::BLOCK + 6 < 65536, "a packed counter holds a block");
constexpr int KH_BATCH = 4;                 // rounds whose loads are in flight together: 64 bytes of map per lane
constexpr unsigned KH_RULE_BLOCKS = 8;      // blocks a workgroup takes at most: its u32 LDS counters and run counts stay below 2^19
constexpr int KH_LDS_BITS = 12;             // a slot of up to 2^12 digits lives in LDS as u32 counters
constexpr int KH_MAX_VOLUMES = 65535;       // grid.y
constexpr unsigned KH_NO_PAIR = 0xffffffffu;   // (a real pair is slot << bits | digit < 2^28)

constexpr int QA_THREADS = 256;
constexpr unsigned QA_MAX_GROUPS = 256 * 8;    // workgroups of a launch: the table is staged once per workgroup

// the order-preserving integer of a float32 bit pattern (-0.0 as +0.0); NaN: see is_nan_bits
__device__ __forceinline__ unsigned key_of_bits(unsigned b)
{
    b = (b == 0x80000000u) ? 0u : b;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ bool is_nan_bits(unsigned b) { return (b & 0x7fffffffu) > 0x7f800000u; }

__device__ __forceinline__ void lds_add(unsigned* p, unsigned v)
{
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// what a wave carries from slot to slot (wave-uniform)
struct Run {
    unsigned pair, count;
};

// `count` more voxels of `pair` (slot 0: the pair is the digit) in the workgroup's LDS histogram
template <int MODE>
__device__ __forceinline__ void lds_count(unsigned* hist, unsigned pair, unsigned count)
{
    if (MODE == MODE_LDS_PACKED) lds_add(hist + (pair >> 1), count << (16u * (pair & 1u)));
    else lds_add(hist + pair, count);
}

template <int MODE>
__device__ __forceinline__ void flush_run(const Run& run, unsigned* hist, unsigned long long* out, int lane)
{
    if (run.count != 0u && lane == 0) {
        if (MODE != MODE_GLOBAL) lds_count<MODE>(hist, run.pair, run.count);
        else atomicAdd(out + run.pair, (unsigned long long)run.count);
    }
}

// One voxel slot of the wave (see the aggregation rule above).  Called by all 64 lanes together.
template <int MODE>
__device__ __forceinline__ void wave_add(unsigned pair, bool active, Run& run, unsigned* hist, unsigned long long* out, int lane)
{
    unsigned long long remaining = __ballot(active);
    if (remaining == 0ull) return;      // (wave-uniform)
    unsigned long long hit = __ballot(active && pair == run.pair);
    if (hit == 0ull) {
        flush_run<MODE>(run, hist, out, lane);
        run.pair = (unsigned)__builtin_amdgcn_readlane((int)pair, __ffsll((long long)remaining) - 1);
        run.count = 0u;
        hit = __ballot(active && pair == run.pair);
    }
    run.count += (unsigned)__popcll(hit);
    remaining &= ~hit;
    if (MODE != MODE_GLOBAL) {
        if (active && pair != run.pair) lds_count<MODE>(hist, pair, 1u);
    } else {
        while (remaining != 0ull) {      // (wave-uniform: every other distinct pair of the slot once, at most 63 rounds)
            const int leader = __ffsll((long long)remaining) - 1;
            const unsigned p0 = (unsigned)__builtin_amdgcn_readlane((int)pair, leader);
            const unsigned long long same = __ballot(active && pair == p0);
            if (lane == leader) atomicAdd(out + p0, (unsigned long long)__popcll(same));
            remaining &= ~same;
        }
    }
}

// MODE: see Mode (the LDS forms: n_prefixes <= 1).  MASK = false: no mask array, every voxel is in the population.
template <int MODE, bool MASK>
__global__ __launch_bounds__(KhGeometry<MODE>::THREADS) void key_hist_kernel(const float* __restrict__ maps, const uint8_t* __restrict__ mask, size_t n,
                                                                             const unsigned* __restrict__ prefixes_dev, int n_prefixes, int search_top,
                                                                             int shift, int bits, unsigned long long* __restrict__ out,
                                                                             unsigned long long* __restrict__ counts, unsigned blocks_per_wg,
                                                                             unsigned nblocks, int vec)
{
    constexpr int KH_THREADS = KhGeometry<MODE>::THREADS, KH_ROUNDS = KhGeometry<MODE>::ROUNDS;
    constexpr size_t KH_BLOCK = KhGeometry<MODE>::BLOCK;
    extern __shared__ unsigned kh_lds[];                     // [2] NaN and population counts, [n_prefixes] the table, then the histogram
    unsigned* const wg_counts = kh_lds;
    unsigned* const table = kh_lds + 2;
    unsigned* const hist = table + n_prefixes;
    const int hist_words = MODE == MODE_LDS ? (1 << bits) : MODE == MODE_LDS_PACKED ? (1 << (bits - 1)) : 0;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 2) wg_counts[tid] = 0u;
    for (int i = tid; i < n_prefixes; i += KH_THREADS) table[i] = prefixes_dev[i];
    for (int i = tid; i < hist_words; i += KH_THREADS) hist[i] = 0u;
    __syncthreads();
    const size_t vol = blockIdx.y;
    const float* uv = maps + vol * n;
    const uint8_t* mv = MASK ? mask + vol * n : nullptr;
    size_t head = 0, body = n;
    if (vec) {
        head = (4 - ((vol * n) & 3)) & 3;
        head = head < n ? head : n;
        body = (n - head) & ~(size_t)3;
    }
    const unsigned digit_mask = (1u << bits) - 1u;
    const int hi_shift = shift + bits;      // 1..32: shifted as 64 bits
    Run run = {KH_NO_PAIR, 0u};
    unsigned nans = 0u, population = 0u;    // per lane
    // one voxel: its value's bit pattern and whether it belongs to the population
    auto add = [&](unsigned b, bool in) {
        const bool nan = is_nan_bits(b);
        population += in ? 1u : 0u;
        nans += (in && nan) ? 1u : 0u;
        const unsigned key = key_of_bits(b);
        const unsigned hi = (unsigned)((unsigned long long)key >> hi_shift);
        unsigned slot = 0u;
        bool listed = true;
        if (n_prefixes > 0) {      // the largest index whose prefix is <= hi (or 0), branch-free
            for (int step = search_top; step > 0; step >>= 1) {
                const unsigned probe = slot + (unsigned)step;
                const unsigned at = probe < (unsigned)n_prefixes ? probe : (unsigned)n_prefixes - 1u;
                slot = (probe < (unsigned)n_prefixes && table[at] <= hi) ? probe : slot;
            }
            listed = table[slot] == hi;
        }
        wave_add<MODE>((slot << bits) | ((key >> shift) & digit_mask), in && !nan && listed, run, hist, out, lane);
    };
    auto add4 = [&](bool in, const float (&q)[4], unsigned m4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) add(__float_as_uint(q[k]), in && ((m4 >> (8 * k)) & 0xffu) != 0u);
    };
    auto add1 = [&](bool in, size_t e) {      // element e of the volume, read on its own (in: e < n)
        unsigned b = 0u;
        bool act = in;
        if (in) {
            b = __float_as_uint(uv[e]);
            if (MASK) act = mv[e] != 0;
        }
        add(b, act);
    };
    // the head and the tail around the 16-byte part: at most 3 + 3 elements, taken by the first wave of the volume's first workgroup
    if (vec && blockIdx.x == 0 && tid < 64) {
        const size_t tail = n - head - body;
        add1((size_t)tid < head + tail, (size_t)tid < head ? (size_t)tid : body + (size_t)tid);
    }
    const unsigned blk_end = min((blockIdx.x + 1) * blocks_per_wg, nblocks);
    for (unsigned blk = blockIdx.x * blocks_per_wg; blk < blk_end; ++blk) {
        const size_t base = (size_t)blk * KH_BLOCK;          // relative to the 16-byte part
        if (vec && base + KH_BLOCK <= body) {
            for (int g = 0; g < KH_ROUNDS / KH_BATCH; ++g) {
                float q[KH_BATCH][4];
                unsigned m4[KH_BATCH];
#pragma unroll
                for (int i = 0; i < KH_BATCH; ++i) {
                    const size_t e = head + base + ((size_t)(g * KH_BATCH + i) * KH_THREADS + tid) * 4;
                    load4(uv + e, q[i]);
                    m4[i] = MASK ? stream_load(reinterpret_cast<const unsigned*>(mv + e)) : 0x01010101u;
                }
#pragma unroll
                for (int i = 0; i < KH_BATCH; ++i) add4(true, q[i], m4[i]);
            }
        } else if (vec) {
            for (int r = 0; r < KH_ROUNDS; ++r) {            // the last, partial block of the 16-byte part (body % 4 == 0)
                const size_t rel = base + ((size_t)r * KH_THREADS + tid) * 4;
                const bool in = rel < body;
                float q[4] = {0.f, 0.f, 0.f, 0.f};
                unsigned m4 = 0x01010101u;
                if (in) {
                    const size_t e = head + rel;
                    load4(uv + e, q);
                    if (MASK) m4 = *reinterpret_cast<const unsigned*>(mv + e);
                }
                add4(in, q, m4);
            }
        } else {
            for (int r = 0; r < 4 * KH_ROUNDS; ++r) {
                const size_t e = base + (size_t)r * KH_THREADS + tid;
                add1(e < n, e);
            }
        }
        if (MODE == MODE_LDS_PACKED) {      // the packed counters hold one block: every wave's run in, then flush and zero (slot 0: pair = digit)
            flush_run<MODE>(run, hist, out, lane);
            run.count = 0u;
            __syncthreads();
            for (int w = tid; w < hist_words; w += KH_THREADS) {
                const unsigned c = hist[w];
                if (c != 0u) {
                    hist[w] = 0u;
                    if ((c & 0xffffu) != 0u) atomicAdd(out + 2 * w, (unsigned long long)(c & 0xffffu));
                    if ((c >> 16) != 0u) atomicAdd(out + 2 * w + 1, (unsigned long long)(c >> 16));
                }
            }
            __syncthreads();
        }
    }
    flush_run<MODE>(run, hist, out, lane);      // (packed: nothing left, the last block flushed it)
    if (nans != 0u) lds_add(wg_counts + 0, nans);
    if (population != 0u) lds_add(wg_counts + 1, population);
    __syncthreads();
    if (tid < 2 && wg_counts[tid] != 0u) atomicAdd(counts + tid, (unsigned long long)wg_counts[tid]);
    if (MODE == MODE_LDS)
        for (int i = tid; i < hist_words; i += KH_THREADS) {
            const unsigned c = hist[i];
            if (c != 0u) atomicAdd(out + i, (unsigned long long)c);      // (slot 0) integers: exact, whatever the order
        }
}

// Blocks per workgroup: a large launch lets a workgroup keep its runs (and its LDS histogram) over several blocks, a small one keeps the
// chip full -- at least four rounds of 4 workgroups per CU stay (rcu_unc_hist.hip, blocks_for).
int g_forced_blocks = 0;      // rcu_key_hist_set_blocks_per_workgroup (tests: several blocks per workgroup from small inputs)

unsigned blocks_for(size_t total_blocks, int workgroups_per_cu)
{
    if (g_forced_blocks >= 1) return (unsigned)g_forced_blocks < KH_RULE_BLOCKS ? (unsigned)g_forced_blocks : KH_RULE_BLOCKS;
    const size_t k = total_blocks / (4 * 256 * (size_t)workgroups_per_cu);
    return (unsigned)(k < 1 ? 1 : k > KH_RULE_BLOCKS ? KH_RULE_BLOCKS : k);
}

template <int MODE, bool MASK>
hipError_t launch_key_hist(const float* maps, const uint8_t* mask, size_t n, int n_volumes, const unsigned* prefixes_dev, int n_prefixes, int shift,
                           int bits, unsigned long long* out, unsigned long long* counts, hipStream_t stream)
{
    constexpr int KH_THREADS = KhGeometry<MODE>::THREADS;
    constexpr size_t KH_BLOCK = KhGeometry<MODE>::BLOCK;
    const size_t hist_words = MODE == MODE_LDS ? ((size_t)1 << bits) : MODE == MODE_LDS_PACKED ? ((size_t)1 << (bits - 1)) : 0;
    const size_t lds = sizeof(unsigned) * (2 + (size_t)n_prefixes + hist_words);
    if (lds > 48 * 1024) {      // (the packed form alone; the attribute is set once per kernel and device: to the most the form ever asks for)
        const hipError_t e = set_max_dynamic_lds(reinterpret_cast<const void*>(&key_hist_kernel<MODE, MASK>), (int)(sizeof(unsigned) * (3 + ((size_t)1 << 15))));
        if (e != hipSuccess) return e;
    }
    const unsigned nblocks = (unsigned)((n + KH_BLOCK - 1) / KH_BLOCK);
    const unsigned bpw = blocks_for((size_t)nblocks * n_volumes, MODE == MODE_LDS_PACKED ? 1 : 4);
    const unsigned gx = (nblocks + bpw - 1) / bpw;
    const int vec = (reinterpret_cast<uintptr_t>(maps) % 16 == 0) && (mask == nullptr || reinterpret_cast<uintptr_t>(mask) % 4 == 0);
    int search_top = 0;      // the largest power of two below n_prefixes: the first step of the search
    while (n_prefixes > 1 && (search_top == 0 ? 1 : search_top * 2) < n_prefixes) search_top = search_top == 0 ? 1 : search_top * 2;
    hipLaunchKernelGGL((key_hist_kernel<MODE, MASK>), dim3(gx, n_volumes), dim3(KH_THREADS), lds, stream, maps, mask, n, prefixes_dev, n_prefixes,
                       search_top, shift, bits, out, counts, bpw, nblocks, vec);
    return hipGetLastError();
}

// level = #{k : key > bound[k]} over the m = Q - 1 non-decreasing boundaries, branch-free; top = the largest power of two <= m
__device__ __forceinline__ unsigned level_of_key(unsigned key, const unsigned* bound, unsigned m, unsigned top)
{
    unsigned level = 0u;
    for (unsigned step = top; step > 0u; step >>= 1) {
        const unsigned probe = level + step;      // would `probe` boundaries lie below the key?
        const unsigned at = probe <= m ? probe - 1u : m - 1u;
        level = (probe <= m && bound[at] < key) ? probe : level;
    }
    return level;
}

__global__ __launch_bounds__(QA_THREADS) void quantile_apply_kernel(const float* __restrict__ in, size_t n, const unsigned* __restrict__ bounds_dev, int Q,
                                                                    unsigned top, float* __restrict__ out, uint16_t* __restrict__ levels, size_t head,
                                                                    int vec)
{
    extern __shared__ unsigned qa_lds[];                     // [Q - 1] boundary keys, [Q] output values
    unsigned* const bound = qa_lds;
    float* const value = reinterpret_cast<float*>(qa_lds + (Q - 1));
    const int tid = threadIdx.x;
    const unsigned m = (unsigned)(Q - 1);
    for (int i = tid; i < Q - 1; i += QA_THREADS) bound[i] = bounds_dev[i];
    for (int i = tid; i < Q; i += QA_THREADS) value[i] = (float)(((double)i + 0.5) / (double)Q);      // IEEE: one division, one rounding to float32
    __syncthreads();
    auto level_of = [&](float x) {
        const unsigned b = __float_as_uint(x);
        return is_nan_bits(b) ? 0u : level_of_key(key_of_bits(b), bound, m, top);
    };
    auto one = [&](size_t e) {
        const unsigned l = level_of(in[e]);
        out[e] = value[l];
        if (levels) levels[e] = (uint16_t)l;
    };
    const size_t stride = (size_t)gridDim.x * QA_THREADS, first = (size_t)blockIdx.x * QA_THREADS + tid;
    if (!vec) {
        for (size_t e = first; e < n; e += stride) one(e);
        return;
    }
    // [head, head + body): 16-byte loads and stores; the 0..3 elements in front and behind go one by one
    const size_t body = (n - head) & ~(size_t)3, tail = n - head - body;
    if (blockIdx.x == 0 && (size_t)tid < head + tail) one((size_t)tid < head ? (size_t)tid : body + (size_t)tid);
    for (size_t i = first; i < body / 4; i += stride) {
        const size_t e = head + i * 4;
        float q[4];
        load4(in + e, q);
        unsigned l[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) l[k] = level_of(q[k]);
        *reinterpret_cast<float4*>(out + e) = float4{value[l[0]], value[l[1]], value[l[2]], value[l[3]]};
        if (levels) *reinterpret_cast<ushort4*>(levels + e) = ushort4{(unsigned short)l[0], (unsigned short)l[1], (unsigned short)l[2], (unsigned short)l[3]};
    }
}

}  // namespace
}  // namespace rcu

using namespace rcu;

extern "C" size_t rcu_key_hist_workspace_bytes(int n_prefixes)
{
    if (n_prefixes < 0 || n_prefixes > RCU_KEY_HIST_MAX_PREFIXES) return 0;
    return round256(sizeof(uint32_t) * (size_t)(n_prefixes > 0 ? n_prefixes : 1));
}

extern "C" int rcu_key_hist_set_blocks_per_workgroup(int blocks)
{
    if (blocks < 0) return report_error(RCU_ERR_INVALID, "rcu_key_hist_set_blocks_per_workgroup: negative block count");
    g_forced_blocks = blocks;
    return RCU_OK;
}

extern "C" int rcu_key_hist(const float* maps_dev, const uint8_t* mask_dev, size_t n_per_volume, int n_volumes, const uint32_t* prefixes_host,
                            int n_prefixes, int shift, int bits, int64_t* hist_dev, uint64_t* counts_dev, void* workspace_dev, void* stream)
{
    const std::string f = "rcu_key_hist: ";
    if (bits < 1 || bits > 16) return report_error(RCU_ERR_INVALID, f + "bits must be in 1..16, got " + std::to_string(bits));
    if (shift < 0 || shift + bits > 32)
        return report_error(RCU_ERR_INVALID, f + "shift must be >= 0 and shift + bits <= 32, got shift " + std::to_string(shift) + ", bits " + std::to_string(bits));
    if (n_prefixes < 0 || n_prefixes > RCU_KEY_HIST_MAX_PREFIXES)
        return report_error(RCU_ERR_INVALID, f + "n_prefixes must be in 0.." + std::to_string(RCU_KEY_HIST_MAX_PREFIXES) + ", got " + std::to_string(n_prefixes));
    if (n_prefixes > 0 && !prefixes_host) return report_error(RCU_ERR_INVALID, f + "null prefixes_host");
    for (int i = 1; i < n_prefixes; ++i)
        if (prefixes_host[i - 1] >= prefixes_host[i]) return report_error(RCU_ERR_INVALID, f + "prefixes_host must be strictly increasing (entry " + std::to_string(i) + ")");
    if (n_prefixes > 0 && shift + bits < 32 && (prefixes_host[n_prefixes - 1] >> (32 - shift - bits)) != 0u)
        return report_error(RCU_ERR_INVALID, f + "a prefix has more than 32 - shift - bits bits");
    if (n_prefixes > 0 && shift + bits == 32 && (n_prefixes > 1 || prefixes_host[0] != 0u))
        return report_error(RCU_ERR_INVALID, f + "with shift + bits = 32 the only prefix is 0");
    if (!maps_dev) return report_error(RCU_ERR_INVALID, f + "null maps_dev");
    if (!hist_dev) return report_error(RCU_ERR_INVALID, f + "null hist_dev");
    if (!counts_dev) return report_error(RCU_ERR_INVALID, f + "null counts_dev");
    if (!workspace_dev) return report_error(RCU_ERR_INVALID, f + "null workspace_dev");
    if (!batch_n_ok(n_per_volume)) return report_error(RCU_ERR_INVALID, f + "n_per_volume must be in 1..2^31-2, got " + std::to_string(n_per_volume));
    if (int st = check_n_volumes(f, n_volumes, KH_MAX_VOLUMES)) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned* prefixes_dev = reinterpret_cast<unsigned*>(workspace_dev);
    if (n_prefixes > 0) {
        const hipError_t e = hipMemcpyAsync(prefixes_dev, prefixes_host, sizeof(uint32_t) * (size_t)n_prefixes, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return hip_failed("rcu_key_hist", e);
    }
    unsigned long long* out = reinterpret_cast<unsigned long long*>(hist_dev);
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_dev);
    hipError_t e;
    if (n_prefixes <= 1 && bits <= KH_LDS_BITS) {
        e = mask_dev ? launch_key_hist<MODE_LDS, true>(maps_dev, mask_dev, n_per_volume, n_volumes, prefixes_dev, n_prefixes, shift, bits, out, counts, s)
                     : launch_key_hist<MODE_LDS, false>(maps_dev, mask_dev, n_per_volume, n_volumes, prefixes_dev, n_prefixes, shift, bits, out, counts, s);
    } else if (n_prefixes <= 1) {
        e = mask_dev ? launch_key_hist<MODE_LDS_PACKED, true>(maps_dev, mask_dev, n_per_volume, n_volumes, prefixes_dev, n_prefixes, shift, bits, out, counts, s)
                     : launch_key_hist<MODE_LDS_PACKED, false>(maps_dev, mask_dev, n_per_volume, n_volumes, prefixes_dev, n_prefixes, shift, bits, out, counts, s);
    } else {
        e = mask_dev ? launch_key_hist<MODE_GLOBAL, true>(maps_dev, mask_dev, n_per_volume, n_volumes, prefixes_dev, n_prefixes, shift, bits, out, counts, s)
                     : launch_key_hist<MODE_GLOBAL, false>(maps_dev, mask_dev, n_per_volume, n_volumes, prefixes_dev, n_prefixes, shift, bits, out, counts, s);
    }
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_key_hist", e);
}

extern "C" size_t rcu_quantile_apply_workspace_bytes(int quantiles)
{
    if (quantiles < 2 || quantiles > RCU_UNC_HIST_MAX_LEVELS) return 0;
    return round256(sizeof(uint32_t) * (size_t)(quantiles - 1));
}

extern "C" int rcu_quantile_apply(const float* map_dev, size_t n, const uint32_t* bounds_host, int quantiles, float* out_dev, uint16_t* levels_dev,
                                  void* workspace_dev, void* stream)
{
    const std::string f = "rcu_quantile_apply: ";
    if (quantiles < 2 || quantiles > RCU_UNC_HIST_MAX_LEVELS)
        return report_error(RCU_ERR_INVALID, f + "quantiles must be in 2.." + std::to_string(RCU_UNC_HIST_MAX_LEVELS) + ", got " + std::to_string(quantiles));
    if (!bounds_host) return report_error(RCU_ERR_INVALID, f + "null bounds_host");
    for (int i = 1; i < quantiles - 1; ++i)
        if (bounds_host[i - 1] > bounds_host[i]) return report_error(RCU_ERR_INVALID, f + "bounds_host must be non-decreasing (entry " + std::to_string(i) + ")");
    if (!map_dev) return report_error(RCU_ERR_INVALID, f + "null map_dev");
    if (!out_dev) return report_error(RCU_ERR_INVALID, f + "null out_dev");
    if (!workspace_dev) return report_error(RCU_ERR_INVALID, f + "null workspace_dev");
    if (n == 0) return report_error(RCU_ERR_INVALID, f + "n must be >= 1");
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned* bounds_dev = reinterpret_cast<unsigned*>(workspace_dev);
    hipError_t e = hipMemcpyAsync(bounds_dev, bounds_host, sizeof(uint32_t) * (size_t)(quantiles - 1), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_failed("rcu_quantile_apply", e);
    // 16-byte path: head = the 0..3 elements up to the input's first 16-byte boundary; the outputs must reach theirs (8 bytes: levels) there too
    const uintptr_t in_a = reinterpret_cast<uintptr_t>(map_dev), out_a = reinterpret_cast<uintptr_t>(out_dev), lv_a = reinterpret_cast<uintptr_t>(levels_dev);
    int vec = in_a % 4 == 0 && out_a % 4 == 0 && lv_a % 2 == 0;
    size_t head = 0;
    if (vec) {
        head = (4 - ((in_a / 4) & 3)) & 3;
        vec = (out_a + 4 * head) % 16 == 0 && (levels_dev == nullptr || (lv_a + 2 * head) % 8 == 0);
        head = head < n ? head : n;
    }
    if (!vec) head = 0;
    unsigned top = 1;      // the largest power of two <= Q - 1
    while (top * 2 <= (unsigned)(quantiles - 1)) top *= 2;
    const size_t items = vec ? (n + 3) / 4 : n;
    size_t groups = (items + QA_THREADS - 1) / QA_THREADS;
    groups = groups < 1 ? 1 : groups > QA_MAX_GROUPS ? QA_MAX_GROUPS : groups;
    const size_t lds = sizeof(unsigned) * (size_t)(quantiles - 1) + sizeof(float) * (size_t)quantiles;
    hipLaunchKernelGGL(quantile_apply_kernel, dim3((unsigned)groups), dim3(QA_THREADS), lds, s, map_dev, n, bounds_dev, quantiles, top, out_dev,
                       levels_dev, head, vec);
    e = hipGetLastError();
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_quantile_apply", e);
}
