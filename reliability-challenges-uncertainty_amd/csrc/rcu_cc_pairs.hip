// The sparse joint table of two labellings (include/rcu.h, "Component pairs"): per volume, for every pair (a, b) of a label of map A and a
// label of map B that share a voxel, the number of shared voxels and the number of those where a third map is not 0.
//   table = per volume an open-addressing hash table of `capacity` slots of one rcu_cc_pair each, then per volume two u32 counters
//           (used = slots claimed, dropped = voxels whose pair found no slot)
// Integer adds: the set of non-empty slots is a function of the inputs alone whenever dropped == 0 -- whatever the launch geometry, the
// batching or the hash; only the ORDER of the slots is the race's.
//
// Four voxels per lane: a wave owns four rows of 64 consecutive voxels, whole waves stay together (the ballots need every lane).  A wave
// without a lane where a > 0 && b > 0 -- almost every wave of a real mask -- returns after its eight loads.  Otherwise the wave walks its
// distinct keys: the first remaining lane leads, the lanes of all four rows that hold the leader's key are found with ballots and counted
// with popcounts, the leader ALONE inserts the key and adds the two counts, the lanes are cleared; at most 256 rounds.  A wave inside one
// pair costs one insert per 256 voxels, a wave with k pairs k inserts.  (One voxel per lane, measured first, left one 256-byte request
// per array in flight per wave and took 2.05 x the time of rcu_cc_table's pass on the same labels; tools/lesions_bench.py.)
// Insert: hash -> start slot, claim an empty slot with a 64-bit compare-and-swap on the slot's key word, probe linearly; after `capacity`
// probes the voxels are counted as dropped.  Nobody waits for anybody: no spin, no lock, no flag -- a lane that loses a claim reads what
// the winner left and either shares the slot (the same key) or moves on.  A key word only ever goes from 0 to its key, so a stale read of
// 0 costs a failed compare-and-swap, never a wrong slot.  Agent-scope atomics throughout, as in rcu_cc.hip: the XCDs' L2s are not
// coherent for plain accesses.
#include "../../include/rcu.h"
#include "rcu_kernels.h"

#include <string>

namespace rcu {
namespace {

constexpr int PAIRS_THREADS = 256;
constexpr int PAIRS_ROWS = 4;               // rows of 64 voxels per wave
constexpr size_t PAIRS_BLOCK = (size_t)PAIRS_THREADS * PAIRS_ROWS;      // voxels of a workgroup
constexpr int PAIRS_MAX_VOLUMES = 65535;       // grid.y
constexpr size_t PAIRS_MIN_CAPACITY = 64, PAIRS_MAX_CAPACITY = (size_t)1 << 26;

int g_hash_shift = 0;       // rcu_cc_pairs_set_hash_shift: the hash loses its low bits (tests: long probe chains from small inputs)

struct Slot {               // rcu_cc_pair; `key` overlays a (low half) and b (high half)
    unsigned long long key;
    unsigned voxels, inside_voxels;
};
static_assert(sizeof(Slot) == sizeof(rcu_cc_pair) && sizeof(Slot) == 16, "rcu_cc_pair is 16 bytes");

__device__ __forceinline__ unsigned long long mix64(unsigned long long x)       // MurmurHash3's finaliser
{
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// the slot of (a, b), claimed if the pair is new, gets count and inside_count; counters = {used, dropped} of the volume
__device__ __forceinline__ void insert_and_add(Slot* table, size_t capacity, unsigned a, unsigned b, unsigned count, unsigned inside_count,
                                               unsigned* counters, int hash_shift)
{
    const unsigned long long word = (unsigned long long)a | ((unsigned long long)b << 32);        // the slot's first 8 bytes: a, then b
    const size_t mask = capacity - 1;
    size_t slot = (size_t)(mix64(((unsigned long long)a << 32) | b) >> hash_shift) & mask;
    for (size_t probe = 0; probe < capacity; ++probe, slot = (slot + 1) & mask) {
        Slot* s = table + slot;
        unsigned long long seen = __hip_atomic_load(&s->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == 0ull) {
            seen = atomicCAS(&s->key, 0ull, word);
            if (seen == 0ull) {
                atomicAdd(counters, 1u);
                seen = word;
            }
        }
        if (seen == word) {
            atomicAdd(&s->voxels, count);
            if (inside_count) atomicAdd(&s->inside_voxels, inside_count);
            return;
        }
    }
    atomicAdd(counters + 1, count);
}

__global__ __launch_bounds__(PAIRS_THREADS) void cc_pairs_kernel(const int* __restrict__ a_labels, const int* __restrict__ b_labels,
                                                                 const uint8_t* __restrict__ inside, size_t n, Slot* table, size_t capacity,
                                                                 unsigned* counters, int hash_shift)
{
    // a wave owns PAIRS_ROWS rows of 64 consecutive voxels: every load is one coalesced row, 2 x PAIRS_ROWS of them in flight per lane
    const int lane = (int)(threadIdx.x & 63);
    const size_t first = ((size_t)blockIdx.x * (PAIRS_THREADS / 64) + (threadIdx.x >> 6)) * (64 * PAIRS_ROWS) + lane;
    const size_t off = (size_t)blockIdx.y * n;
    int la[PAIRS_ROWS], lb[PAIRS_ROWS];
#pragma unroll
    for (int r = 0; r < PAIRS_ROWS; ++r) {      // (no lane leaves before the ballots)
        const size_t i = first + (size_t)r * 64;
        la[r] = i < n ? a_labels[off + i] : 0;
        lb[r] = i < n ? b_labels[off + i] : 0;
    }
    bool active[PAIRS_ROWS], ins[PAIRS_ROWS];
    unsigned long long remaining[PAIRS_ROWS], any = 0ull;
#pragma unroll
    for (int r = 0; r < PAIRS_ROWS; ++r) {
        active[r] = la[r] > 0 && lb[r] > 0;
        remaining[r] = __ballot(active[r]);
        any |= remaining[r];
    }
    if (any == 0ull) return;
#pragma unroll
    for (int r = 0; r < PAIRS_ROWS; ++r) ins[r] = active[r] && inside != nullptr && inside[off + first + (size_t)r * 64] != 0;
    for (;;) {      // (wave-uniform: every distinct key of the wave's rows once, at most 64 x PAIRS_ROWS rounds)
        int leader = -1, a0 = 0, b0 = 0;
#pragma unroll
        for (int r = 0; r < PAIRS_ROWS; ++r)
            if (leader < 0 && remaining[r] != 0ull) {
                leader = __ffsll((long long)remaining[r]) - 1;
                a0 = __shfl(la[r], leader);
                b0 = __shfl(lb[r], leader);
            }
        if (leader < 0) break;
        unsigned count = 0, inside_count = 0;
#pragma unroll
        for (int r = 0; r < PAIRS_ROWS; ++r) {
            const bool same = active[r] && la[r] == a0 && lb[r] == b0;
            const unsigned long long lanes = __ballot(same);
            count += (unsigned)__popcll(lanes);
            inside_count += (unsigned)__popcll(__ballot(same && ins[r]));
            remaining[r] &= ~lanes;
        }
        if (lane == leader)
            insert_and_add(table + (size_t)blockIdx.y * capacity, capacity, (unsigned)a0, (unsigned)b0, count, inside_count,
                           counters + 2 * (size_t)blockIdx.y, hash_shift);
    }
}

bool capacity_ok(size_t capacity) { return capacity >= PAIRS_MIN_CAPACITY && capacity <= PAIRS_MAX_CAPACITY && (capacity & (capacity - 1)) == 0; }
size_t slots_bytes(size_t capacity, int n_volumes) { return round256((size_t)n_volumes * capacity * sizeof(Slot)); }

}  // namespace
}  // namespace rcu

using namespace rcu;

extern "C" int rcu_cc_pairs_set_hash_shift(int shift)
{
    if (shift < 0 || shift > 63) return report_error(RCU_ERR_INVALID, "rcu_cc_pairs_set_hash_shift: shift must be in 0..63, got " + std::to_string(shift));
    g_hash_shift = shift;
    return RCU_OK;
}

extern "C" size_t rcu_cc_pairs_bytes(size_t capacity, int n_volumes)
{
    if (!capacity_ok(capacity) || n_volumes < 1 || n_volumes > PAIRS_MAX_VOLUMES) return 0;
    return slots_bytes(capacity, n_volumes) + round256((size_t)n_volumes * 2 * sizeof(unsigned));
}

extern "C" int rcu_cc_pairs(const int32_t* a_dev, const int32_t* b_dev, const uint8_t* inside_dev, size_t n_per_volume, int n_volumes, size_t capacity,
                            void* table_dev, void* stream)
{
    const std::string f = "rcu_cc_pairs: ";
    if (int st = check_batch(f, n_per_volume, n_volumes, PAIRS_MAX_VOLUMES)) return st;
    if (!capacity_ok(capacity)) return report_error(RCU_ERR_INVALID, f + "capacity must be a power of two in 64..2^26, got " + std::to_string(capacity));
    if (!a_dev) return report_error(RCU_ERR_INVALID, f + "null a_dev");
    if (!b_dev) return report_error(RCU_ERR_INVALID, f + "null b_dev");
    if (!table_dev) return report_error(RCU_ERR_INVALID, f + "null table_dev");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(table_dev, 0, rcu_cc_pairs_bytes(capacity, n_volumes), s);
    if (e != hipSuccess) return hip_failed("rcu_cc_pairs", e);
    Slot* slots = reinterpret_cast<Slot*>(table_dev);
    unsigned* counters = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(table_dev) + slots_bytes(capacity, n_volumes));
    const dim3 grid((unsigned)((n_per_volume + PAIRS_BLOCK - 1) / PAIRS_BLOCK), n_volumes);
    hipLaunchKernelGGL(cc_pairs_kernel, grid, dim3(PAIRS_THREADS), 0, s, a_dev, b_dev, inside_dev, n_per_volume, slots, capacity, counters, g_hash_shift);
    e = hipGetLastError();
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_cc_pairs", e);
}
