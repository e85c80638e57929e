// 3-D connected-component labelling and the per-component table (include/rcu.h, "Connected components"):
//   labels[v][i] = 0 for background, 1 + (the smallest linear index of the voxel's component) for foreground,
//   table       = per component, in increasing order of that label: root, voxels, other_voxels, unc_max, unc_sum
// Everything is integer arithmetic: labels and tables do not depend on tiles, workgroups, launch order or batching.
//
// Labelling = block-based union-find on the label array itself.  A label l > 0 of voxel i reads "the parent of i is voxel l - 1"; a voxel
// whose label is its own index + 1 is a root.  Parents only ever decrease (every link is an atomicMin towards the smaller index), so a
// tree's root is the smallest index of the tree, and once a component is one tree its root is the component's canonical label.
//   1. cc_local_kernel    one workgroup per tile (tz x ty x tx <= 1024 voxels, default 4 x 8 x 32, or 1 x 16 x 64 for depth 1): union-find of
//                         the tile in LDS over the "backward" half of the neighbourhood (the 13 / 3 neighbours that precede a voxel in raster
//                         order; every adjacent pair is seen from its later voxel), then every voxel writes its tile root's GLOBAL index + 1.
//                         The tile-local raster order is the global one restricted to the tile, so the tile root is the tile-wise minimum.
//   2. cc_seam_kernel     one thread per voxel: for every backward neighbour that lies in ANOTHER tile, union in global memory.
//   3. cc_flatten_kernel  one thread per voxel: label := root + 1.
// Passes 2 and 3 read parents that other workgroups are changing.  The XCDs' L2s are not coherent for plain accesses, so every access to
// a parent there is an agent-scope atomic (relaxed load, atomicMin, relaxed store).  The union is the lock-free form (Komura 2015; Playne
// & Hawick 2018): nobody ever waits for anybody -- a thread that loses a race re-reads and goes on from the value the winner left.  Any
// value a parent ever holds is an ancestor of the voxel in the final forest, so stale reads cost hops, not correctness, and every walk
// ends: each hop strictly decreases the index.  find() halves paths on the way (atomicMin of the grandparent: still an ancestor, still a
// decrease), which keeps the long chains of a serpentine short while thousands of threads walk them.  Whether a voxel is foreground
// never changes, so that test may use plain loads.
//
// Table: roots are ranked in raster order (cc_count / cc_scan / cc_rank: a three-kernel exclusive scan of the root flags of the WHOLE batch,
// so that rank = the row of the concatenated table; the rank of a root is kept in a voxel-sized map in the workspace), then one pass adds
// every voxel to the row of its root.  A tumour component has 1e5 and more voxels: per wave the key of the first foreground lane is
// published, the lanes that share it are combined with ballots and two wave reductions and ONE lane issues the row's atomics; only the
// foreground lanes with another key fall back to atomics of their own (mixed waves: component borders, noise islands).  Integer atomics
// (u32 add / max, u64 add): exact whatever the order.
#include "../../include/rcu.h"
#include "rcu_kernels.h"
#include "rcu_unc_source.h"

#include <string>
#include <type_traits>

namespace rcu {
namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_MAX_TILE = 1024;           // voxels of a tile = ints of LDS
constexpr int CC_MAX_VOLUMES = 65535;       // grid.y
constexpr int CC_SCAN_BLOCK = 4096;         // voxels whose roots one workgroup counts / ranks: 16 rounds of 256
constexpr int CC_SCAN_THREADS = 1024;

int g_tile[3] = {0, 0, 0};                  // forced tile (z, y, x); 0 = the launcher's choice

struct Dims {
    int d, h, w;         // the volume
    int tz, ty, tx;      // the tile
    int nty, ntx;        // tiles along y and x
};

__device__ __forceinline__ int aload(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int lload(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// is (dz, dy, dx) one of the neighbours that precede a voxel in raster order, under this connectivity
template <int CONN>
__device__ __forceinline__ constexpr bool backward(int dz, int dy, int dx)
{
    const bool before = dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0)));
    const int faces = (dz != 0) + (dy != 0) + (dx != 0);
    return before && (CONN == 26 || faces == 1);
}

// ---- the tile in LDS: parent[t] = local index of the parent, -1 = background (or outside the volume)
__device__ __forceinline__ int lds_find(const int* parent, int x)
{
    for (int p; (p = lload(parent + x)) != x;) x = p;
    return x;
}
__device__ __forceinline__ void lds_union(int* parent, int a, int b)
{
    for (;;) {
        a = lds_find(parent, a);
        b = lds_find(parent, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(parent + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);      // b -> a, a < b
        if (old == b) return;       // b was a root: linked
        b = old;                    // somebody linked b first: its tree and a's still have to meet
    }
}

template <int CONN>
__global__ __launch_bounds__(CC_THREADS) void cc_local_kernel(const uint8_t* __restrict__ mask, int* __restrict__ labels, Dims g)
{
    __shared__ int parent[CC_MAX_TILE];
    const int tile = g.tz * g.ty * g.tx, plane = g.ty * g.tx;
    const size_t n = (size_t)g.d * g.h * g.w;
    const uint8_t* mv = mask + (size_t)blockIdx.y * n;
    int* lv = labels + (size_t)blockIdx.y * n;
    const int bx = blockIdx.x % g.ntx, by = (blockIdx.x / g.ntx) % g.nty, bz = blockIdx.x / (g.ntx * g.nty);
    const int oz = bz * g.tz, oy = by * g.ty, ox = bx * g.tx;
    auto global_of = [&](int t) { return ((size_t)(oz + t / plane) * g.h + (oy + (t / g.tx) % g.ty)) * g.w + (ox + t % g.tx); };
    auto inside = [&](int t) { return oz + t / plane < g.d && oy + (t / g.tx) % g.ty < g.h && ox + t % g.tx < g.w; };
    int any = 0;
    for (int t = threadIdx.x; t < tile; t += CC_THREADS) {
        const bool fg = inside(t) && mv[global_of(t)] != 0;
        parent[t] = fg ? t : -1;
        any |= fg;
    }
    if (!__syncthreads_or(any)) {       // an empty tile: zeros
        for (int t = threadIdx.x; t < tile; t += CC_THREADS)
            if (inside(t)) lv[global_of(t)] = 0;
        return;
    }
    for (int t = threadIdx.x; t < tile; t += CC_THREADS) {
        if (parent[t] < 0) continue;      // (a foreground entry is never negative: the test is stable while others link)
        const int lz = t / plane, ly = (t / g.tx) % g.ty, lx = t % g.tx;
#pragma unroll
        for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!backward<CONN>(dz, dy, dx)) continue;
                    const int z = lz + dz, y = ly + dy, x = lx + dx;
                    if (z < 0 || y < 0 || y >= g.ty || x < 0 || x >= g.tx) continue;      // another tile's: the seam pass
                    const int u = (z * g.ty + y) * g.tx + x;
                    if (lload(parent + u) >= 0) lds_union(parent, t, u);
                }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < tile; t += CC_THREADS) {
        if (!inside(t)) continue;
        const int p = parent[t];
        lv[global_of(t)] = p < 0 ? 0 : (int)global_of(lds_find(parent, t)) + 1;
    }
}

// ---- the volume in global memory: L[i] = parent + 1, every access an agent-scope atomic
// root of x, linking the nodes it passes to their grandparents on the way (path halving); halve_start = false leaves the start node alone
// (the flatten pass stores that label itself)
__device__ __forceinline__ int global_find(int* L, int x, bool halve_start)
{
    bool halve = halve_start;
    for (;;) {
        const int p = aload(L + x) - 1;
        if (p == x) return x;
        const int gp = aload(L + p) - 1;
        if (gp == p) return p;
        if (halve) __hip_atomic_fetch_min(L + x, gp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        halve = true;
        x = gp;
    }
}
__device__ __forceinline__ void global_union(int* L, int a, int b)
{
    for (;;) {
        a = global_find(L, a, true);
        b = global_find(L, b, true);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(L + b, a + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;
        if (old == b) return;
        b = old;
    }
}

template <int CONN>
__global__ __launch_bounds__(CC_THREADS) void cc_seam_kernel(const uint8_t* __restrict__ mask, int* labels, Dims g)
{
    const size_t n = (size_t)g.d * g.h * g.w;
    const size_t i = (size_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned i32 = (unsigned)i, row = i32 / (unsigned)g.w;      // (n < 2^31: 32-bit divisions)
    const int x = (int)(i32 - row * (unsigned)g.w), y = (int)(row % (unsigned)g.h), z = (int)(row / (unsigned)g.h);
    const int rx = x % g.tx, ry = y % g.ty, rz = z % g.tz;
    // a backward neighbour lies in another tile only for voxels on the low z face, the low / high y faces or the low / high x faces
    if (rz != 0 && ry != 0 && ry != g.ty - 1 && rx != 0 && rx != g.tx - 1) return;
    const uint8_t* mv = mask + (size_t)blockIdx.y * n;
    if (mv[i] == 0) return;
    int* L = labels + (size_t)blockIdx.y * n;
#pragma unroll
    for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (!backward<CONN>(dz, dy, dx)) continue;
                const int nz = z + dz, ny = y + dy, nx = x + dx;
                if (nz < 0 || ny < 0 || ny >= g.h || nx < 0 || nx >= g.w) continue;
                const bool same_tile = (dz == 0 || rz != 0) && (dy == 0 || (dy < 0 ? ry != 0 : ry != g.ty - 1)) &&
                                       (dx == 0 || (dx < 0 ? rx != 0 : rx != g.tx - 1));
                if (same_tile) continue;
                const size_t u = ((size_t)nz * g.h + ny) * g.w + nx;
                if (mv[u] != 0) global_union(L, (int)i, (int)u);
            }
}

__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int* labels, size_t n)
{
    const size_t i = (size_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= n) return;
    int* L = labels + (size_t)blockIdx.y * n;
    const int l = aload(L + i);
    if (l == 0) return;
    const int r = global_find(L, (int)i, false) + 1;
    if (r != l) __hip_atomic_store(L + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- ranks of the roots.  Blocks of CC_SCAN_BLOCK voxels never straddle a volume: block b of volume v is entry v * nblocks + b.
__device__ __forceinline__ unsigned wave_rank(bool flag, unsigned& total)
{
    const unsigned long long m = __ballot(flag);
    total = (unsigned)__popcll(m);
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));      // flagged lanes below this one
}

__global__ __launch_bounds__(CC_THREADS) void cc_count_kernel(const int* __restrict__ labels, size_t n, unsigned nblocks, unsigned* __restrict__ block_sum)
{
    __shared__ unsigned wave_sum[CC_THREADS / 64];
    const int* L = labels + (size_t)blockIdx.y * n;
    const size_t base = (size_t)blockIdx.x * CC_SCAN_BLOCK;
    unsigned mine = 0;
    for (int r = 0; r < CC_SCAN_BLOCK / CC_THREADS; ++r) {
        const size_t i = base + (size_t)r * CC_THREADS + threadIdx.x;
        mine += (i < n && L[i] == (int)i + 1) ? 1u : 0u;
    }
    for (int s = 32; s > 0; s >>= 1) mine += __shfl_xor(mine, s);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
        for (int w = 0; w < CC_THREADS / 64; ++w) t += wave_sum[w];
        block_sum[(size_t)blockIdx.y * nblocks + blockIdx.x] = t;
    }
}

// One workgroup: block_sum[0 .. total) -> its exclusive prefix sums in place; vol_first[v] = roots in front of volume v (v = 0 .. n_volumes),
// counts[v] = roots of volume v.
__global__ __launch_bounds__(CC_SCAN_THREADS) void cc_scan_kernel(unsigned* __restrict__ block_sum, unsigned nblocks, int n_volumes,
                                                                  unsigned* vol_first, unsigned* __restrict__ counts)
{
    __shared__ unsigned wave_sum[CC_SCAN_THREADS / 64];
    __shared__ unsigned carry;
    const size_t total = (size_t)nblocks * n_volumes;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0u;
    __syncthreads();
    for (size_t first = 0; first < total; first += CC_SCAN_THREADS) {
        const size_t e = first + threadIdx.x;
        const unsigned v = e < total ? block_sum[e] : 0u;
        unsigned incl = v;
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned o = __shfl_up(incl, s);
            if (lane >= s) incl += o;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        unsigned before = carry;
        for (int w = 0; w < wave; ++w) before += wave_sum[w];
        const unsigned excl = before + incl - v;
        if (e < total) {
            block_sum[e] = excl;
            if (e % nblocks == 0) vol_first[e / nblocks] = excl;
        }
        __syncthreads();
        if (threadIdx.x == CC_SCAN_THREADS - 1) carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) vol_first[n_volumes] = carry;
    __syncthreads();
    for (int v = threadIdx.x; v < n_volumes; v += CC_SCAN_THREADS) counts[v] = vol_first[v + 1] - vol_first[v];
}

__global__ __launch_bounds__(CC_THREADS) void cc_rank_kernel(const int* __restrict__ labels, size_t n, unsigned nblocks,
                                                             const unsigned* __restrict__ block_first, unsigned* __restrict__ rank)
{
    __shared__ unsigned wave_sum[CC_THREADS / 64];
    const int* L = labels + (size_t)blockIdx.y * n;
    unsigned* R = rank + (size_t)blockIdx.y * n;
    const size_t base = (size_t)blockIdx.x * CC_SCAN_BLOCK;
    unsigned running = block_first[(size_t)blockIdx.y * nblocks + blockIdx.x];
    const int wave = threadIdx.x >> 6;
    for (int r = 0; r < CC_SCAN_BLOCK / CC_THREADS; ++r) {
        const size_t i = base + (size_t)r * CC_THREADS + threadIdx.x;
        const bool root = i < n && L[i] == (int)i + 1;
        unsigned in_wave;
        const unsigned below = wave_rank(root, in_wave);
        if ((threadIdx.x & 63) == 0) wave_sum[wave] = in_wave;
        __syncthreads();
        unsigned before = running, all = 0;
        for (int w = 0; w < CC_THREADS / 64; ++w) {
            if (w < wave) before += wave_sum[w];
            all += wave_sum[w];
        }
        if (root) R[i] = before + below;
        running += all;
        __syncthreads();
    }
}

// (dense may be labels itself: a thread reads its own label only)
__global__ __launch_bounds__(CC_THREADS) void cc_relabel_kernel(const int* labels, size_t n, const unsigned* __restrict__ rank,
                                                                const unsigned* __restrict__ vol_first, int* dense)
{
    const size_t i = (size_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= n) return;
    const size_t off = (size_t)blockIdx.y * n;
    const int l = labels[off + i];
    dense[off + i] = (l <= 0 || (size_t)l > n) ? 0 : (int)(rank[off + (size_t)(l - 1)] - vol_first[blockIdx.y]) + 1;
}

// ---- the table
struct Entry {            // rcu_cc_entry
    int root;
    unsigned voxels, other_voxels, unc_max;
    unsigned long long unc_sum;
};
static_assert(sizeof(Entry) == sizeof(rcu_cc_entry) && sizeof(Entry) == 24, "rcu_cc_entry is 24 bytes");

template <int KIND>
__global__ __launch_bounds__(CC_THREADS) void cc_table_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ other,
                                                              const void* __restrict__ unc, size_t n, const unsigned* __restrict__ rank,
                                                              Entry* __restrict__ table, size_t capacity)
{
    const size_t i = (size_t)blockIdx.x * CC_THREADS + threadIdx.x;      // (whole waves stay together: the ballots below need every lane)
    const size_t off = (size_t)blockIdx.y * n;
    const bool in = i < n;
    const int l = in ? labels[off + i] : 0;
    size_t row = 0;
    bool fg = l > 0 && (size_t)l <= n;      // (labels that are not rcu_cc_label's are not followed outside the volume)
    if (fg) {
        row = rank[off + (size_t)(l - 1)];
        fg = row < capacity;       // (a table smaller than the compaction said is refused on the host; never a write outside it)
    }
    if (!__any(fg)) return;
    unsigned q = 0;
    bool oth = false;
    if (fg) {
        oth = other != nullptr && other[off + i] != 0;
        q = quantised_unc<KIND>(unc, off + i);
        if (l == (int)i + 1) table[row].root = (int)i;
    }
    const unsigned long long fg_lanes = __ballot(fg);
    const int leader = __ffsll((long long)fg_lanes) - 1;
    const unsigned row0 = (unsigned)__shfl((unsigned)row, leader);
    const bool same = fg && (unsigned)row == row0;
    const unsigned count = (unsigned)__popcll(__ballot(same)), ocount = (unsigned)__popcll(__ballot(same && oth));
    unsigned sum = same ? q : 0u, mx = sum;      // 64 x 2^24 fits 32 bits
    if constexpr (KIND != RCU_CC_UNC_NONE) {
        for (int s = 32; s > 0; s >>= 1) {
            sum += __shfl_xor(sum, s);
            const unsigned o = __shfl_xor(mx, s);
            mx = o > mx ? o : mx;
        }
    }
    const bool lead = (int)(threadIdx.x & 63) == leader;
    if (lead || (fg && !same)) {
        Entry* e = table + row;
        atomicAdd(&e->voxels, lead ? count : 1u);
        const unsigned oc = lead ? ocount : (oth ? 1u : 0u);
        if (oc) atomicAdd(&e->other_voxels, oc);
        if constexpr (KIND != RCU_CC_UNC_NONE) {
            const unsigned s = lead ? sum : q, m = lead ? mx : q;
            if (s) atomicAdd(&e->unc_sum, (unsigned long long)s);
            if (m) atomicMax(&e->unc_max, m);
        }
    }
}

// ---- host side
Dims dims_for(int d, int h, int w)
{
    Dims g;
    g.d = d, g.h = h, g.w = w;
    if (g_tile[0] > 0) g.tz = g_tile[0], g.ty = g_tile[1], g.tx = g_tile[2];
    else if (d == 1) g.tz = 1, g.ty = 16, g.tx = 64;
    else g.tz = 4, g.ty = 8, g.tx = 32;
    g.nty = (h + g.ty - 1) / g.ty;
    g.ntx = (w + g.tx - 1) / g.tx;
    return g;
}

unsigned scan_blocks(size_t n) { return (unsigned)((n + CC_SCAN_BLOCK - 1) / CC_SCAN_BLOCK); }

// the workspace: [rank: n_volumes x n u32][block_first: n_volumes x scan_blocks u32][vol_first: n_volumes + 1 u32]
struct Workspace {
    unsigned *rank, *block_first, *vol_first;
};
Workspace carve(void* ws, size_t n, int n_volumes)
{
    char* p = reinterpret_cast<char*>(ws);
    Workspace w;
    w.rank = reinterpret_cast<unsigned*>(p);
    p += round256((size_t)n_volumes * n * sizeof(unsigned));
    w.block_first = reinterpret_cast<unsigned*>(p);
    p += round256((size_t)n_volumes * scan_blocks(n) * sizeof(unsigned));
    w.vol_first = reinterpret_cast<unsigned*>(p);
    return w;
}

}  // namespace
}  // namespace rcu

using namespace rcu;

extern "C" int rcu_cc_set_tile(int tile_depth, int tile_height, int tile_width)
{
    const bool unset = tile_depth == 0 && tile_height == 0 && tile_width == 0;
    if (!unset && (tile_depth < 1 || tile_height < 1 || tile_width < 1 || (long long)tile_depth * tile_height * tile_width > CC_MAX_TILE ||
                   tile_depth > CC_MAX_TILE || tile_height > CC_MAX_TILE || tile_width > CC_MAX_TILE))
        return report_error(RCU_ERR_INVALID, "rcu_cc_set_tile: every extent >= 1 and their product <= " + std::to_string(CC_MAX_TILE) + " (or 0, 0, 0)");
    g_tile[0] = tile_depth, g_tile[1] = tile_height, g_tile[2] = tile_width;
    return RCU_OK;
}

extern "C" int rcu_cc_label(const uint8_t* mask_dev, int depth, int height, int width, int n_volumes, int connectivity, int32_t* labels_dev,
                            void* stream)
{
    const std::string f = "rcu_cc_label: ";
    if (connectivity != 6 && connectivity != 26) return report_error(RCU_ERR_INVALID, f + "connectivity must be 6 or 26, got " + std::to_string(connectivity));
    if (depth < 1 || height < 1 || width < 1) return report_error(RCU_ERR_INVALID, f + "depth, height and width must be >= 1");
    const unsigned long long n64 = (unsigned long long)depth * (unsigned long long)height * (unsigned long long)width;
    if (n64 >= 0x7fffffffull) return report_error(RCU_ERR_INVALID, f + "a volume must have fewer than 2^31 - 1 voxels");
    if (int st = check_n_volumes(f, n_volumes, CC_MAX_VOLUMES)) return st;
    if (!mask_dev) return report_error(RCU_ERR_INVALID, f + "null mask_dev");
    if (!labels_dev) return report_error(RCU_ERR_INVALID, f + "null labels_dev");
    const size_t n = (size_t)n64;
    const Dims g = dims_for(depth, height, width);
    const unsigned long long tiles = (unsigned long long)((depth + g.tz - 1) / g.tz) * g.nty * g.ntx;
    if (tiles > 0x7fffffffull) return report_error(RCU_ERR_INVALID, f + "too many tiles for one launch (rcu_cc_set_tile)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 per_voxel((unsigned)((n + CC_THREADS - 1) / CC_THREADS), n_volumes), per_tile((unsigned)tiles, n_volumes);
    if (connectivity == 26) {
        hipLaunchKernelGGL(cc_local_kernel<26>, per_tile, dim3(CC_THREADS), 0, s, mask_dev, labels_dev, g);
        hipLaunchKernelGGL(cc_seam_kernel<26>, per_voxel, dim3(CC_THREADS), 0, s, mask_dev, labels_dev, g);
    } else {
        hipLaunchKernelGGL(cc_local_kernel<6>, per_tile, dim3(CC_THREADS), 0, s, mask_dev, labels_dev, g);
        hipLaunchKernelGGL(cc_seam_kernel<6>, per_voxel, dim3(CC_THREADS), 0, s, mask_dev, labels_dev, g);
    }
    hipLaunchKernelGGL(cc_flatten_kernel, per_voxel, dim3(CC_THREADS), 0, s, labels_dev, n);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_cc_label", e);
}

extern "C" size_t rcu_cc_workspace_bytes(size_t n_per_volume, int n_volumes)
{
    if (!batch_ok(n_per_volume, n_volumes, CC_MAX_VOLUMES)) return 0;
    return round256((size_t)n_volumes * n_per_volume * sizeof(unsigned)) + round256((size_t)n_volumes * scan_blocks(n_per_volume) * sizeof(unsigned)) +
           round256(((size_t)n_volumes + 1) * sizeof(unsigned));
}

extern "C" int rcu_cc_compact(const int32_t* labels_dev, size_t n_per_volume, int n_volumes, uint32_t* counts_dev, void* workspace_dev, void* stream)
{
    const std::string f = "rcu_cc_compact: ";
    if (int st = check_batch(f, n_per_volume, n_volumes, CC_MAX_VOLUMES)) return st;
    if (!labels_dev) return report_error(RCU_ERR_INVALID, f + "null labels_dev");
    if (!counts_dev) return report_error(RCU_ERR_INVALID, f + "null counts_dev");
    if (!workspace_dev) return report_error(RCU_ERR_INVALID, f + "null workspace_dev");
    const Workspace w = carve(workspace_dev, n_per_volume, n_volumes);
    const unsigned nblocks = scan_blocks(n_per_volume);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cc_count_kernel, dim3(nblocks, n_volumes), dim3(CC_THREADS), 0, s, labels_dev, n_per_volume, nblocks, w.block_first);
    hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(CC_SCAN_THREADS), 0, s, w.block_first, nblocks, n_volumes, w.vol_first, counts_dev);
    hipLaunchKernelGGL(cc_rank_kernel, dim3(nblocks, n_volumes), dim3(CC_THREADS), 0, s, labels_dev, n_per_volume, nblocks, w.block_first, w.rank);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_cc_compact", e);
}

extern "C" int rcu_cc_relabel(const int32_t* labels_dev, size_t n_per_volume, int n_volumes, const void* workspace_dev, int32_t* dense_dev, void* stream)
{
    const std::string f = "rcu_cc_relabel: ";
    if (int st = check_batch(f, n_per_volume, n_volumes, CC_MAX_VOLUMES)) return st;
    if (!labels_dev) return report_error(RCU_ERR_INVALID, f + "null labels_dev");
    if (!workspace_dev) return report_error(RCU_ERR_INVALID, f + "null workspace_dev");
    if (!dense_dev) return report_error(RCU_ERR_INVALID, f + "null dense_dev");
    const Workspace w = carve(const_cast<void*>(workspace_dev), n_per_volume, n_volumes);
    hipLaunchKernelGGL(cc_relabel_kernel, dim3((unsigned)((n_per_volume + CC_THREADS - 1) / CC_THREADS), n_volumes), dim3(CC_THREADS), 0,
                       static_cast<hipStream_t>(stream), labels_dev, n_per_volume, w.rank, w.vol_first, dense_dev);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_cc_relabel", e);
}

extern "C" int rcu_cc_table(const int32_t* labels_dev, const uint8_t* other_dev, const void* unc_dev, int unc_kind, size_t n_per_volume, int n_volumes,
                            const void* workspace_dev, rcu_cc_entry* table_dev, size_t table_entries, void* stream)
{
    const std::string f = "rcu_cc_table: ";
    if (int st = check_batch(f, n_per_volume, n_volumes, CC_MAX_VOLUMES)) return st;
    if (int st = check_unc_source(f, unc_kind, unc_dev)) return st;
    if (!labels_dev) return report_error(RCU_ERR_INVALID, f + "null labels_dev");
    if (!workspace_dev) return report_error(RCU_ERR_INVALID, f + "null workspace_dev");
    if (table_entries == 0) return RCU_OK;      // no component in the batch: nothing to fill
    if (!table_dev) return report_error(RCU_ERR_INVALID, f + "null table_dev");
    if (table_entries > 0xffffffffull) return report_error(RCU_ERR_INVALID, f + "table_entries must be below 2^32");
    const Workspace w = carve(const_cast<void*>(workspace_dev), n_per_volume, n_volumes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(table_dev, 0, table_entries * sizeof(rcu_cc_entry), s);
    if (e != hipSuccess) return hip_failed("rcu_cc_table", e);
    const dim3 grid((unsigned)((n_per_volume + CC_THREADS - 1) / CC_THREADS), n_volumes);
    Entry* t = reinterpret_cast<Entry*>(table_dev);
    with_unc_kind(unc_kind, [&](auto kind) {
        hipLaunchKernelGGL(cc_table_kernel<decltype(kind)::value>, grid, dim3(CC_THREADS), 0, s, labels_dev, other_dev, unc_dev, n_per_volume, w.rank, t, table_entries);
    });
    e = hipGetLastError();
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_cc_table", e);
}
