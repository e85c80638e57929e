// Patch table and patch level histogram (include/rcu.h, "Patch-level uncertainty"): the volume cut into a grid of non-overlapping windows of
// pd x ph x pw voxels anchored at the origin (the far-edge patches are partial), per patch the integers {n, errors, foreground, sum_q} over its
// voxels inside the mask, and from those rows the histogram hist[volume][cell][level] += 1 of the patches by (accurate with foreground /
// inaccurate / accurate pure background) and by the level of their mean uncertainty.  Everything is integer arithmetic on q(u) of
// rcu_unc_source.h: the table is a function of the inputs alone.
//
// rcu_patch_table: ONE LANE PER PATCH, patches in raster order, so lane i of a volume owns patch i.  The lane walks the pd * ph rows of its
// patch, keeps the four sums in registers and stores its 32-byte row once: no LDS, no atomics, nothing shared -- the result cannot depend on
// the launch geometry or on the batch.  Neighbouring lanes own neighbouring patches of one row of patches, so what a wave asks for per patch
// row is one contiguous run of the volume row.
//   16-byte path (pw 4, 8 or 16, width % 4 == 0, 16-byte map base and 4-byte label bases, and a volume that starts on a multiple of 4
//   elements): a patch row is pw / 4 units of 4 voxels -- one 16-byte map load (two for float64), one 4-byte word per label array, the byte
//   logic of unc_hist_kernel::add4 done once per word.  The loads of 4 units (4 rows of a 4-wide patch) are issued together before any of
//   them is worked on.  width % 4 == 0 with pw % 4 == 0 makes every unit whole: the partial patch at the right edge ends on a unit boundary.
//   Element path (every other case; per volume, so volumes 1 and 2 of a batch of odd-sized volumes take it while volume 0 does not): the same
//   walk, one element at a time.
//
// rcu_patch_hist: one pass over the rows, 16 rows per thread and workgroup, the key cell * B + level added to ONE LDS histogram of 3 B u32
// per workgroup with the wave-aggregated add of the level histogram (rcu_unc_hist.hip, wave_add: nearly every patch of a real volume has the
// key [pure background][level 0], and 64 lanes adding to one LDS address would serialise), non-zero counters flushed with 64-bit global
// integer adds into the zeroed output.  The level of a patch's mean uncertainty sum_q / (n 2^24) is taken in integers:
//   level = #{k in 1..B-1 : sum_q B > k n 2^24} = min(B - 1, (sum_q B - 1) div (n 2^24)) for sum_q > 0, else 0
// -- the mean is never formed, so a mean that sits exactly on k / B is not above it, whatever B.
#include "../../include/rcu.h"
#include "rcu_kernels.h"
#include "rcu_unc_source.h"

#include <string>
#include <type_traits>

namespace rcu {
namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_UNITS = 4;                 // 4-voxel units whose loads are in flight together (16-byte path)
constexpr int PT_MAX_VOLUMES = 65535;       // grid.y
constexpr int PH_THREADS = 256;
constexpr int PH_ROUNDS = 16;               // table rows per thread: a workgroup takes 4096 rows, so its u32 LDS counters cannot overflow

template <int KIND>
using unc_type = typename std::conditional<KIND == RCU_CC_UNC_F64, double, float>::type;

// per byte 1 where the byte of w is not 0 (unc_hist_kernel's nonzero_bytes)
__device__ __forceinline__ unsigned nonzero_bytes(unsigned w) { return ((w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u; }

// The four sums of one patch.  add4: four voxels given as byte flags P (prediction != 0), T (target != 0), A (inside the mask and the volume)
struct PatchSums {
    unsigned n = 0u, errors = 0u, foreground = 0u;
    unsigned long long sum_q = 0ull;
    __device__ __forceinline__ void add4(unsigned P, unsigned T, unsigned A, const unsigned (&q)[4])
    {
        n += (unsigned)__popc(A);
        errors += (unsigned)__popc((P ^ T) & A);
        foreground += (unsigned)__popc((P | T) & A);
        unsigned s = 0u;      // four q <= 2^24 each: no overflow
#pragma unroll
        for (int k = 0; k < 4; ++k) s += ((A >> (8 * k)) & 1u) ? q[k] : 0u;
        sum_q += s;
    }
    __device__ __forceinline__ void add1(bool pr, bool tg, unsigned q)
    {
        n += 1u;
        errors += (pr != tg) ? 1u : 0u;
        foreground += (pr | tg) ? 1u : 0u;
        sum_q += q;
    }
};

// PW: the patch width of the 16-byte path (4, 8, 16), or 0 for a launch that reads element by element throughout.  vec_bases: the bases
// allow the 16-byte path; a volume takes it when it also starts on a multiple of 4 elements.
template <int KIND, int PW, bool MASK>
__global__ __launch_bounds__(PT_THREADS) void patch_table_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ target,
                                                                  const uint8_t* __restrict__ mask, const void* __restrict__ unc, int D, int H, int W,
                                                                  int pd, int ph, int pw, unsigned gy_n, unsigned gx_n, unsigned patches,
                                                                  unsigned long long* __restrict__ table, int vec_bases, int table16)
{
    using T = unc_type<KIND>;
    const unsigned patch = blockIdx.x * PT_THREADS + threadIdx.x;
    if (patch >= patches) return;
    const size_t vol = blockIdx.y, n = (size_t)D * H * W;
    const uint8_t* pv = pred + vol * n;
    const uint8_t* tv = target + vol * n;
    const uint8_t* mv = MASK ? mask + vol * n : nullptr;
    const T* uv = (KIND == RCU_CC_UNC_NONE) ? nullptr : reinterpret_cast<const T*>(unc) + vol * n;
    const unsigned gx = patch % gx_n, gyz = patch / gx_n, gy = gyz % gy_n, gz = gyz / gy_n;
    const int x0 = (int)gx * pw, y0 = (int)gy * ph, z0 = (int)gz * pd;
    PatchSums sums;
    if (PW != 0 && vec_bases && ((vol * n) & 3) == 0) {
        constexpr int CH = PW ? PW / 4 : 1;            // units per patch row
        constexpr int RB = PT_UNITS / CH;              // patch rows per batch of PT_UNITS units
        const int rows = pd * ph;
        for (int r0 = 0; r0 < rows; r0 += RB) {
            T u4[PT_UNITS][4];
            unsigned p4[PT_UNITS], t4[PT_UNITS], m4[PT_UNITS];
            bool in[PT_UNITS];
#pragma unroll
            for (int u = 0; u < PT_UNITS; ++u) {       // the loads of the batch, issued together
                const int r = r0 + u / CH, dz = r / ph, dy = r - dz * ph;
                const int z = z0 + dz, y = y0 + dy, x = x0 + 4 * (u % CH);
                in[u] = r < rows && z < D && y < H && x < W;      // (W % 4 == 0: the unit is whole or outside)
                p4[u] = t4[u] = 0u;
                m4[u] = 0x01010101u;
#pragma unroll
                for (int k = 0; k < 4; ++k) u4[u][k] = (T)0;
                if (in[u]) {
                    const size_t e = ((size_t)z * H + y) * W + x;
                    if constexpr (KIND != RCU_CC_UNC_NONE) load4(uv + e, u4[u]);
                    p4[u] = stream_load(reinterpret_cast<const unsigned*>(pv + e));
                    t4[u] = stream_load(reinterpret_cast<const unsigned*>(tv + e));
                    if (MASK) m4[u] = stream_load(reinterpret_cast<const unsigned*>(mv + e));
                }
            }
#pragma unroll
            for (int u = 0; u < PT_UNITS; ++u) {
                unsigned q[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) q[k] = quantised_unc<KIND>(&u4[u][k], 0);
                sums.add4(nonzero_bytes(p4[u]), nonzero_bytes(t4[u]), in[u] ? nonzero_bytes(m4[u]) : 0u, q);
            }
        }
    } else {
        const int z1 = min(z0 + pd, D), y1 = min(y0 + ph, H), x1 = min(x0 + pw, W);
        for (int z = z0; z < z1; ++z)
            for (int y = y0; y < y1; ++y) {
                const size_t row = ((size_t)z * H + y) * W;
#pragma unroll 4
                for (int x = x0; x < x1; ++x) {
                    const size_t e = row + x;
                    if (MASK && mv[e] == 0) continue;
                    sums.add1(pv[e] != 0, tv[e] != 0, quantised_unc<KIND>(uv, e));
                }
            }
    }
    unsigned long long* const o = table + (vol * patches + patch) * 4;
    if (table16) {
        typedef unsigned long long v2 __attribute__((ext_vector_type(2)));
        reinterpret_cast<v2*>(o)[0] = v2{(unsigned long long)sums.n, (unsigned long long)sums.errors};
        reinterpret_cast<v2*>(o)[1] = v2{(unsigned long long)sums.foreground, sums.sum_q};
    } else {
        o[0] = sums.n, o[1] = sums.errors, o[2] = sums.foreground, o[3] = sums.sum_q;
    }
}

struct PatchGrid {
    int D, H, W, pd, ph, pw;
    unsigned gz_n, gy_n, gx_n, patches;
};

template <int KIND, int PW, bool MASK>
hipError_t launch_table_as(const uint8_t* pred, const uint8_t* target, const uint8_t* mask, const void* unc, const PatchGrid& g, int n_volumes,
                           unsigned long long* table, int vec_bases, hipStream_t stream)
{
    const unsigned blocks = (g.patches + PT_THREADS - 1) / PT_THREADS;
    hipLaunchKernelGGL((patch_table_kernel<KIND, PW, MASK>), dim3(blocks, n_volumes), dim3(PT_THREADS), 0, stream, pred, target, mask, unc, g.D, g.H,
                       g.W, g.pd, g.ph, g.pw, g.gy_n, g.gx_n, g.patches, table, vec_bases, (int)(reinterpret_cast<uintptr_t>(table) % 16 == 0));
    return hipGetLastError();
}

template <int KIND, bool MASK>
hipError_t launch_table_kind(const uint8_t* pred, const uint8_t* target, const uint8_t* mask, const void* unc, const PatchGrid& g, int n_volumes,
                             unsigned long long* table, hipStream_t stream)
{
    auto aligned = [](const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; };
    const bool vec = g.W % 4 == 0 && aligned(unc, 16) && aligned(pred, 4) && aligned(target, 4) && aligned(mask, 4);      // (null pointers are aligned)
    if (vec && g.pw == 4) return launch_table_as<KIND, 4, MASK>(pred, target, mask, unc, g, n_volumes, table, 1, stream);
    if (vec && g.pw == 8) return launch_table_as<KIND, 8, MASK>(pred, target, mask, unc, g, n_volumes, table, 1, stream);
    if (vec && g.pw == 16) return launch_table_as<KIND, 16, MASK>(pred, target, mask, unc, g, n_volumes, table, 1, stream);
    return launch_table_as<KIND, 0, MASK>(pred, target, mask, unc, g, n_volumes, table, 0, stream);
}

// One table row per lane and round -> the workgroup's LDS histogram [cell][level] -> the output.  `aligned`: the table is 16-byte aligned.
__device__ __forceinline__ void lds_add(unsigned* p, unsigned v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// unc_hist_kernel's aggregation: lane 0's key is published, the lanes that share it are counted with one ballot and added by lane 0 in one
// LDS add; the other active lanes add 1 each.  Called by all 64 lanes together.
__device__ __forceinline__ void wave_add(unsigned* hist, unsigned key, bool active, int lane)
{
    const unsigned k0 = (unsigned)__builtin_amdgcn_readfirstlane((int)key);
    const bool same = active & (key == k0), other = active & !same;
    const unsigned count = (unsigned)__popcll(__ballot(same));
    const bool first = lane == 0;
    if (other | (first & (count != 0u))) lds_add(hist + key, first ? count : 1u);
}

__global__ __launch_bounds__(PH_THREADS) void patch_hist_kernel(const unsigned long long* __restrict__ table, size_t n_patches, int B,
                                                                 unsigned per_mille, unsigned long long* __restrict__ out, int table16)
{
    extern __shared__ unsigned ph_hist[];      // [3][B]
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < 3 * B; i += PH_THREADS) ph_hist[i] = 0u;
    __syncthreads();
    const size_t vol = blockIdx.y;
    const unsigned long long* const rows = table + vol * n_patches * 4;
    const size_t base = (size_t)blockIdx.x * PH_THREADS * PH_ROUNDS;
#pragma unroll 4
    for (int r = 0; r < PH_ROUNDS; ++r) {
        const size_t i = base + (size_t)r * PH_THREADS + tid;
        unsigned long long n = 0ull, errors = 0ull, fg = 0ull, sum_q = 0ull;
        if (i < n_patches) {
            if (table16) {
                typedef unsigned long long v2 __attribute__((ext_vector_type(2)));
                const v2 a = reinterpret_cast<const v2*>(rows + i * 4)[0], b = reinterpret_cast<const v2*>(rows + i * 4)[1];
                n = a.x, errors = a.y, fg = b.x, sum_q = b.y;
            } else {
                n = rows[i * 4], errors = rows[i * 4 + 1], fg = rows[i * 4 + 2], sum_q = rows[i * 4 + 3];
            }
        }
        const bool active = n != 0ull;
        const bool accurate = 1000ull * (n - errors) > (unsigned long long)per_mille * n;
        const unsigned cell = !accurate ? 1u : (fg != 0ull ? 0u : 2u);
        unsigned level = 0u;
        if (active && sum_q != 0ull) {
            // (sum_q B - 1) div (n 2^24) = ((sum_q B - 1) >> 24) div n; a table row has sum_q <= n 2^24 <= 2^36, so the product is below 2^49
            const unsigned long long t = ((sum_q * (unsigned long long)B - 1ull) >> 24) / n;
            level = t < (unsigned long long)(B - 1) ? (unsigned)t : (unsigned)(B - 1);
        }
        wave_add(ph_hist, cell * (unsigned)B + level, active, lane);      // key < 3 B whatever the row holds
    }
    __syncthreads();
    unsigned long long* const o = out + vol * 3 * (size_t)B;
    for (int i = tid; i < 3 * B; i += PH_THREADS) {
        const unsigned c = ph_hist[i];
        if (c != 0u) atomicAdd(o + i, (unsigned long long)c);      // integers: exact, whatever the order
    }
}

bool extents_ok(int depth, int height, int width, int pd, int ph, int pw)
{
    return depth >= 1 && height >= 1 && width >= 1 && pd >= 1 && pd <= RCU_PATCH_MAX_EXTENT && ph >= 1 && ph <= RCU_PATCH_MAX_EXTENT && pw >= 1 &&
           pw <= RCU_PATCH_MAX_EXTENT && batch_n_ok((size_t)depth * (size_t)height * (size_t)width);
}

PatchGrid grid_of(int depth, int height, int width, int pd, int ph, int pw)
{
    PatchGrid g{depth, height, width, pd, ph, pw, 0u, 0u, 0u, 0u};
    g.gz_n = (unsigned)((depth + pd - 1) / pd), g.gy_n = (unsigned)((height + ph - 1) / ph), g.gx_n = (unsigned)((width + pw - 1) / pw);
    g.patches = g.gz_n * g.gy_n * g.gx_n;      // <= depth * height * width < 2^31
    return g;
}

}  // namespace
}  // namespace rcu

using namespace rcu;

extern "C" size_t rcu_patch_count(int depth, int height, int width, int pd, int ph, int pw)
{
    if (!extents_ok(depth, height, width, pd, ph, pw)) return 0;
    return grid_of(depth, height, width, pd, ph, pw).patches;
}

extern "C" int rcu_patch_table(const uint8_t* prediction_dev, const uint8_t* target_dev, const uint8_t* mask_dev, const void* unc_dev, int unc_kind,
                               int depth, int height, int width, int n_volumes, int pd, int ph, int pw, uint64_t* table_dev, void* stream)
{
    const std::string f = "rcu_patch_table: ";
    if (pd < 1 || pd > RCU_PATCH_MAX_EXTENT || ph < 1 || ph > RCU_PATCH_MAX_EXTENT || pw < 1 || pw > RCU_PATCH_MAX_EXTENT)
        return report_error(RCU_ERR_INVALID, f + "patch extents must be in 1.." + std::to_string(RCU_PATCH_MAX_EXTENT) + ", got " + std::to_string(pd) +
                                                 " x " + std::to_string(ph) + " x " + std::to_string(pw));
    if (!extents_ok(depth, height, width, pd, ph, pw))
        return report_error(RCU_ERR_INVALID, f + "depth, height and width must be >= 1 and their product in 1..2^31-2");
    if (!prediction_dev) return report_error(RCU_ERR_INVALID, f + "null prediction_dev");
    if (!target_dev) return report_error(RCU_ERR_INVALID, f + "null target_dev");
    if (!table_dev) return report_error(RCU_ERR_INVALID, f + "null table_dev");
    if (int st = check_unc_source(f, unc_kind, unc_dev)) return st;
    if (int st = check_n_volumes(f, n_volumes, PT_MAX_VOLUMES)) return st;
    const PatchGrid g = grid_of(depth, height, width, pd, ph, pw);
    hipError_t e = hipSuccess;
    with_unc_kind(unc_kind, [&](auto kind) {
        constexpr int KIND = decltype(kind)::value;
        unsigned long long* const table = reinterpret_cast<unsigned long long*>(table_dev);
        hipStream_t s = static_cast<hipStream_t>(stream);
        e = mask_dev ? launch_table_kind<KIND, true>(prediction_dev, target_dev, mask_dev, unc_dev, g, n_volumes, table, s)
                     : launch_table_kind<KIND, false>(prediction_dev, target_dev, nullptr, unc_dev, g, n_volumes, table, s);
    });
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_patch_table", e);
}

extern "C" int rcu_patch_hist(const uint64_t* table_dev, size_t n_patches, int n_volumes, int levels, int accuracy_per_mille, uint64_t* hist_dev,
                              void* stream)
{
    const std::string f = "rcu_patch_hist: ";
    if (levels < 2 || levels > RCU_UNC_HIST_MAX_LEVELS)
        return report_error(RCU_ERR_INVALID, f + "levels must be in 2.." + std::to_string(RCU_UNC_HIST_MAX_LEVELS) + ", got " + std::to_string(levels));
    if (accuracy_per_mille < 0 || accuracy_per_mille > 999)
        return report_error(RCU_ERR_INVALID, f + "accuracy_per_mille must be in 0..999, got " + std::to_string(accuracy_per_mille));
    if (!table_dev) return report_error(RCU_ERR_INVALID, f + "null table_dev");
    if (!hist_dev) return report_error(RCU_ERR_INVALID, f + "null hist_dev");
    if (!batch_n_ok(n_patches)) return report_error(RCU_ERR_INVALID, f + "n_patches must be in 1..2^31-2, got " + std::to_string(n_patches));
    if (int st = check_n_volumes(f, n_volumes, PT_MAX_VOLUMES)) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(hist_dev, 0, (size_t)n_volumes * 3 * levels * sizeof(uint64_t), s);
    if (e != hipSuccess) return hip_failed("rcu_patch_hist", e);
    const size_t lds = (size_t)3 * levels * sizeof(unsigned);      // 48 KB at 4096 levels: what a kernel may ask for without raising its limit
    constexpr size_t PER_WG = (size_t)PH_THREADS * PH_ROUNDS;
    const unsigned blocks = (unsigned)((n_patches + PER_WG - 1) / PER_WG);
    hipLaunchKernelGGL(patch_hist_kernel, dim3(blocks, n_volumes), dim3(PH_THREADS), lds, s, reinterpret_cast<const unsigned long long*>(table_dev),
                       n_patches, levels, (unsigned)accuracy_per_mille, reinterpret_cast<unsigned long long*>(hist_dev),
                       (int)(reinterpret_cast<uintptr_t>(table_dev) % 16 == 0));
    e = hipGetLastError();
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_patch_hist", e);
}
