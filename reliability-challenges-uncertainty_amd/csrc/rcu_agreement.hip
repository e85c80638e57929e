// Sample agreement of the MC passes as whole segmentations (include/rcu.h "Sample agreement"): the vote plane of a batch -- one bit per
// (voxel, pass), set where the pass's arg-max is not background -- turned into, per volume,
//   hist[c]      voxels with exactly c of the T bits set                     (c = 0..T)
//   pairs[i][j]  |A_i & A_j| for i <= j, row-major upper triangle with the diagonal: the diagonal holds the sample volumes |A_i|
// All integers: the tables are a function of the plane alone, whatever the grid, the order of the atomics and the slicing of a subject.
//
// A wave works on 64 voxels at a time.  __ballot of bit i over the wave IS the transposed view: a 64-bit mask M_i of the voxels pass i
// voted for, uniform over the wave.  The T masks go to the wave's LDS row, and lane l then owns the pairs l, l + 64, ...: one
// popcount(M_i & M_j) per pair and 64 voxels, added to a register counter -- no loop over pairs per voxel, no atomic per voxel.  The
// histogram goes the same way: the seven ballots of the bits of popcount(word) give lane c the mask of the voxels with exactly c votes.
// A set of 64 voxels without any vote -- most of a medical volume -- costs two ballots and one add.
// Totals leave the workgroup once: its waves add their counters in LDS, then one 64-bit atomicAdd per non-zero counter.
// T <= 33 (up to 9 pairs per lane) runs 1024 threads per workgroup; beyond that the 17 or 33 counters and their pair indices do not fit the 128
// registers such a workgroup leaves a lane, so those instantiations run 512 threads (256 registers) and keep everything in registers.
#include "rcu_kernels.h"

namespace rcu {

static constexpr int AG_THREADS = 1024;            // 16 waves: four per SIMD, one workgroup per CU (NPL <= 9)
static constexpr int AG_THREADS_WIDE = 512;        // NPL 17 and 33: two workgroups per CU, twice the registers per lane
static constexpr int AG_GROUP = 256;               // voxels a wave loads at once: four per lane (one 16-byte load where the plane allows)
static constexpr int AG_MAX_VOLUMES = 65535;

// the 64-bit vote words (bits at or above T cleared; 0 beyond the volume's end) of the lane's four voxels of group g, and whether they exist.
// vec: voxels g * 256 + 4 * lane + s (one 16-byte load per plane); else voxels g * 256 + 64 * s + lane (four coalesced 4-byte loads).
// Which 64 voxels meet in a ballot does not matter: every count is a sum over voxels.
struct AgGroup {
    uint32_t lo[4], hi[4];
    bool valid[4];
};
__device__ __forceinline__ void ag_load(const uint32_t* __restrict__ w0, const uint32_t* __restrict__ w1, uint32_t g, int lane, uint32_t n, int vec,
                                        uint32_t mask_lo, uint32_t mask_hi, AgGroup& q)
{
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const uint32_t base = g * (uint32_t)AG_GROUP;
    if (vec) {
        const uint32_t i = base + 4u * (uint32_t)lane;      // n % 4 == 0: the four exist together
        const bool ok = i < n;
        u4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
        if (ok) {
            a = __builtin_nontemporal_load(reinterpret_cast<const u4*>(w0 + i));
            if (w1 != nullptr) b = __builtin_nontemporal_load(reinterpret_cast<const u4*>(w1 + i));
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            q.lo[s] = a[s] & mask_lo;
            q.hi[s] = b[s] & mask_hi;
            q.valid[s] = ok;
        }
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint32_t i = base + 64u * (uint32_t)s + (uint32_t)lane;
            const bool ok = i < n;
            q.lo[s] = ok ? (__builtin_nontemporal_load(w0 + i) & mask_lo) : 0u;
            q.hi[s] = (ok && w1 != nullptr) ? (__builtin_nontemporal_load(w1 + i) & mask_hi) : 0u;
            q.valid[s] = ok;
        }
    }
}

// NPL: pairs per lane, >= ceil(T (T + 1) / 2 / 64); THREADS: of the workgroup
template <int NPL, int THREADS>
__global__ __launch_bounds__(THREADS) void agreement_kernel(const uint32_t* __restrict__ votes, size_t plane, int n_words, uint32_t n, int T, int vec,
                                                                unsigned long long* __restrict__ hist, unsigned long long* __restrict__ pairs)
{
    constexpr int AG_WAVES = THREADS / 64;
    __shared__ unsigned long long rows[AG_WAVES][64];      // the wave's masks M_0 .. M_{T-1}
    __shared__ uint32_t total[NPL * 64 + 65];              // the workgroup's pair counters, then its histogram (a volume has < 2^31 voxels)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t vol = blockIdx.y;
    const int P = T * (T + 1) / 2;
    const uint32_t* w0 = votes + vol * n;
    const uint32_t* w1 = n_words > 1 ? w0 + plane : nullptr;
    const uint32_t mask_lo = T >= 32 ? 0xFFFFFFFFu : ((1u << T) - 1u);
    const uint32_t mask_hi = T <= 32 ? 0u : (T >= 64 ? 0xFFFFFFFFu : ((1u << (T - 32)) - 1u));
    const int t_lo = T < 32 ? T : 32, t_hi = T - t_lo;

    for (int i = threadIdx.x; i < NPL * 64 + 65; i += THREADS) total[i] = 0u;
    __syncthreads();

    // the lane's pairs: pair p = lane + 64 k is (i, j) with p = i T - i (i - 1) / 2 + (j - i); pairs at or beyond P count (0, 0) and are dropped
    int pi[NPL], pj[NPL];
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        int p = lane + 64 * k, i = 0;
        if (p >= P) p = 0;
        while (p >= T - i) {
            p -= T - i;
            ++i;
        }
        pi[k] = i;
        pj[k] = i + p;
    }
    uint32_t cnt[NPL];
#pragma unroll
    for (int k = 0; k < NPL; ++k) cnt[k] = 0u;
    uint32_t h = 0u, h64 = 0u;      // lane c: voxels with exactly c votes (c < 64); lane 0 also: with 64

    const uint32_t groups = (n + (uint32_t)AG_GROUP - 1u) / (uint32_t)AG_GROUP;
    const uint32_t step = gridDim.x * (uint32_t)AG_WAVES;
    uint32_t g = blockIdx.x * (uint32_t)AG_WAVES + (uint32_t)wave;
    if (g < groups) {
        AgGroup cur, nxt;
        ag_load(w0, w1, g, lane, n, vec, mask_lo, mask_hi, cur);
        for (;;) {
            const uint32_t gn = g + step;      // (groups <= 2^23: no wrap)
            if (gn < groups) ag_load(w0, w1, gn, lane, n, vec, mask_lo, mask_hi, nxt);      // in flight while this group is counted
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint32_t lo = cur.lo[s], hi = cur.hi[s];
                const unsigned long long here = __ballot(cur.valid[s]);
                if (__ballot((lo | hi) != 0u) == 0ull) {      // nobody voted for any of the 64: they all have 0 votes
                    if (lane == 0) h += (uint32_t)__popcll(here);
                    continue;
                }
                const uint32_t c = (uint32_t)__popc(lo) + (uint32_t)__popc(hi);
                unsigned long long sel = here;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const unsigned long long b = __ballot(((c >> k) & 1u) != 0u);
                    sel &= ((lane >> k) & 1) ? b : ~b;
                }
                const unsigned long long b6 = __ballot(c >= 64u);
                h += (uint32_t)__popcll(sel & ~b6);
                if (lane == 0) h64 += (uint32_t)__popcll(b6);
                unsigned long long m = 0ull;
                for (int i = 0; i < t_lo; ++i) {
                    const unsigned long long b = __ballot(((lo >> i) & 1u) != 0u);
                    m = lane == i ? b : m;
                }
                for (int i = 0; i < t_hi; ++i) {
                    const unsigned long long b = __ballot(((hi >> i) & 1u) != 0u);
                    m = lane == 32 + i ? b : m;
                }
                // the row is the wave's own: LDS operations of a wave execute in order, the fences keep the compiler from moving them
                rows[wave][lane] = m;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int k = 0; k < NPL; ++k) cnt[k] += (uint32_t)__popcll(rows[wave][pi[k]] & rows[wave][pj[k]]);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            if (gn >= groups) break;
            cur = nxt;
            g = gn;
        }
    }

#pragma unroll
    for (int k = 0; k < NPL; ++k)
        if (lane + 64 * k < P && cnt[k] != 0u) atomicAdd(&total[lane + 64 * k], cnt[k]);
    if (h != 0u) atomicAdd(&total[NPL * 64 + lane], h);
    if (h64 != 0u) atomicAdd(&total[NPL * 64 + 64], h64);
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += THREADS)
        if (total[p] != 0u) atomicAdd(pairs + vol * (size_t)P + p, (unsigned long long)total[p]);
    for (int c = threadIdx.x; c <= T; c += THREADS)
        if (total[NPL * 64 + c] != 0u) atomicAdd(hist + vol * (size_t)(T + 1) + c, (unsigned long long)total[NPL * 64 + c]);
}

template <int NPL, int THREADS>
static hipError_t launch_agreement(const uint32_t* votes, size_t plane, int n_words, uint32_t n, int n_volumes, int T, int vec,
                                   unsigned long long* hist, unsigned long long* pairs, hipStream_t stream)
{
    // 16 waves per CU over the whole batch, never more workgroups than a volume has groups for, never less than one per volume
    constexpr uint32_t AG_WAVES = THREADS / 64;
    const uint32_t groups = (n + (uint32_t)AG_GROUP - 1u) / (uint32_t)AG_GROUP, want = (groups + AG_WAVES - 1) / AG_WAVES;
    uint32_t per_volume = (256u * 16u / AG_WAVES) / (uint32_t)n_volumes;
    per_volume = per_volume < 1u ? 1u : per_volume;
    per_volume = per_volume > want ? want : per_volume;
    hipLaunchKernelGGL((agreement_kernel<NPL, THREADS>), dim3(per_volume, (unsigned)n_volumes), dim3(THREADS), 0, stream, votes, plane, n_words, n, T, vec, hist,
                       pairs);
    return hipGetLastError();
}

}  // namespace rcu

using namespace rcu;

extern "C" int rcu_agreement_tables(const uint32_t* votes_dev, int n_words, size_t n_per_volume, int n_volumes, int passes, uint64_t* hist_dev,
                                    uint64_t* pairs_dev, void* stream)
{
    const std::string f = "rcu_agreement_tables: ";
    if (!votes_dev || !hist_dev || !pairs_dev) return report_error(RCU_ERR_INVALID, f + "null votes_dev / hist_dev / pairs_dev");
    if (n_words < 1 || n_words > RCU_VOTES_MAX_PASSES / 32)
        return report_error(RCU_ERR_INVALID, f + "n_words must be in 1..2, got " + std::to_string(n_words));
    if (passes < 1 || passes > 32 * n_words)
        return report_error(RCU_ERR_INVALID, f + "passes must be in 1.." + std::to_string(32 * n_words) + " (32 per word), got " + std::to_string(passes));
    if (int st = check_batch(f, n_per_volume, n_volumes, AG_MAX_VOLUMES)) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int T = passes, P = T * (T + 1) / 2, need = (P + 63) / 64;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit counters");
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(hist_dev);
    unsigned long long* pairs = reinterpret_cast<unsigned long long*>(pairs_dev);
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)n_volumes * (T + 1) * sizeof(uint64_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(pairs, 0, (size_t)n_volumes * P * sizeof(uint64_t), s);
    if (e != hipSuccess) return hip_failed("hipMemsetAsync", e);
    const size_t plane = n_per_volume * (size_t)n_volumes;
    const int vec = (n_per_volume % 4 == 0 && (reinterpret_cast<uintptr_t>(votes_dev) & 15u) == 0) ? 1 : 0;
    const uint32_t n = (uint32_t)n_per_volume;
    if (need <= 1) e = launch_agreement<1, AG_THREADS>(votes_dev, plane, n_words, n, n_volumes, T, vec, hist, pairs, s);              // T <= 10
    else if (need <= 4) e = launch_agreement<4, AG_THREADS>(votes_dev, plane, n_words, n, n_volumes, T, vec, hist, pairs, s);         // T <= 22
    else if (need <= 9) e = launch_agreement<9, AG_THREADS>(votes_dev, plane, n_words, n, n_volumes, T, vec, hist, pairs, s);         // T <= 33
    else if (need <= 17) e = launch_agreement<17, AG_THREADS_WIDE>(votes_dev, plane, n_words, n, n_volumes, T, vec, hist, pairs, s);       // T <= 46
    else e = launch_agreement<33, AG_THREADS_WIDE>(votes_dev, plane, n_words, n, n_volumes, T, vec, hist, pairs, s);                       // T <= 64
    if (e != hipSuccess) return hip_failed("agreement_kernel", e);
    return RCU_OK;
}
