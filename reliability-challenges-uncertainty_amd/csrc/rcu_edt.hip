// Exact squared Euclidean distance transform and what the 'boundary' evaluation action needs from it (include/rcu.h, "Distance transform"):
//   rcu_edt_sq                 out[v] = min over the feature voxels w of the same volume of |v - w|^2 (uint32, exact; RCU_EDT_NONE without a feature)
//   rcu_border_mask            the reference's border shell (and float64 distance map) from the two transforms of a label map
//   rcu_boundary_table         voxels / errors / uncertainty sums per (side of the boundary, distance band)
//   rcu_surface_distance_hist  the two directed surface-distance multisets of two label maps, as histograms over d^2
//
// The transform is separable (Saito & Toriwaki 1994): three passes, in place in the output.
//   1. edt_rows_kernel   one wave per row (the width is contiguous).  A chunk of 64 voxels is one ballot: the nearest feature on the left of a
//                        lane is the highest set bit at or below it, the nearest on the right the lowest set bit at or above it; a forward sweep
//                        over the chunks carries the last feature seen and writes the left distance, a backward sweep carries the next one and
//                        writes min(left, right)^2, or NONE.
//   2. 3. edt_lines_kernel   out(i) = min_j f(j) + (i - j)^2 along the height, then the depth.  A workgroup stages a slab [line length][a run
//                        of xw adjacent x] in LDS -- global traffic stays coalesced along x, and the pass is in place because a workgroup reads
//                        and writes its own lines only --, then one thread per output walks j outward from i and stops as soon as (i - j)^2 is
//                        no smaller than the best so far.  Exact in integers, no lower-envelope stack.  xw shrinks with the line length so that
//                        the whole line always fits the slab (16384 entries: a line of the largest extent allowed gets xw = 1).
// NONE never enters a sum: a candidate f(j) + k^2 is taken iff f(j) < best - k^2, which NONE (the largest uint32) never is, and a real f(j)
// is at most 2 * 16383^2, so the sum stays below 2^32.  No float arithmetic anywhere in the transform: the result is a function of the mask
// alone, whatever the slab width or the batching.
#include "../../include/rcu.h"
#include "rcu_kernels.h"
#include "rcu_unc_source.h"

#include <string>

namespace rcu {
namespace {

constexpr int EDT_THREADS = 256;
constexpr int EDT_WAVE = 64;
constexpr int EDT_MAX_EXTENT = 16384;
constexpr int EDT_SLAB_ENTRIES = 16384;       // uint32 entries of LDS per workgroup (64 KB)
constexpr int EDT_MAX_SLAB_WIDTH = 64;
constexpr int EDT_DEFAULT_SLAB_WIDTH = 32;    // 128 bytes per global row segment; 30 KB of LDS for a line of 240
constexpr int EDT_MAX_VOLUMES = 65535;        // grid.y
constexpr unsigned NONE = RCU_EDT_NONE;
constexpr int BT_ROUNDS = 16;                 // rounds of 256 voxels per workgroup of the boundary table
constexpr int BT_MAX_BANDS = 64;

int g_slab_width = 0;                         // forced slab width; 0 = the launcher's choice

// ---- pass 1: rows
__global__ __launch_bounds__(EDT_THREADS) void edt_rows_kernel(const uint8_t* __restrict__ mask, unsigned* __restrict__ out, size_t rows, int w,
                                                               int zero_is_feature)
{
    const size_t row = (size_t)blockIdx.x * (EDT_THREADS / EDT_WAVE) + (threadIdx.x / EDT_WAVE);      // (a wave has one row: its ballots are whole)
    if (row >= rows) return;
    const int lane = threadIdx.x & (EDT_WAVE - 1);
    const uint8_t* m = mask + row * (size_t)w;
    unsigned* o = out + row * (size_t)w;
    const int chunks = (w + EDT_WAVE - 1) / EDT_WAVE;
    int carry = -1;       // x of the last feature in front of the chunk
    for (int c = 0; c < chunks; ++c) {
        const int x = c * EDT_WAVE + lane;
        const bool feat = x < w && ((m[x] == 0) == (zero_is_feature != 0));
        const unsigned long long b = __ballot(feat);
        const unsigned long long below = b & (~0ull >> (63 - lane));      // bits 0..lane
        const int left = below ? c * EDT_WAVE + 63 - __clzll((long long)below) : carry;
        if (x < w) o[x] = left < 0 ? NONE : (unsigned)(x - left);
        if (b) carry = c * EDT_WAVE + 63 - __clzll((long long)b);
    }
    carry = -1;           // x of the next feature behind the chunk
    for (int c = chunks - 1; c >= 0; --c) {
        const int x = c * EDT_WAVE + lane;
        const bool feat = x < w && ((m[x] == 0) == (zero_is_feature != 0));
        const unsigned long long b = __ballot(feat);
        const unsigned long long above = b & (~0ull << lane);             // bits lane..63
        const int right = above ? c * EDT_WAVE + __ffsll((long long)above) - 1 : carry;
        if (x < w) {
            const unsigned dl = o[x], dr = right < 0 ? NONE : (unsigned)(right - x);
            const unsigned d = dl < dr ? dl : dr;
            o[x] = d == NONE ? NONE : d * d;
        }
        if (b) carry = c * EDT_WAVE + __ffsll((long long)b) - 1;
    }
}

// ---- passes 2 and 3: lines of `len` entries, `line_stride` apart, for every x and every one of `n_outer` outer positions (`outer_stride` apart)
struct Lines {
    int len, w, xw, n_runs, n_outer;
    size_t line_stride, outer_stride, n;       // n = voxels per volume
};

__global__ __launch_bounds__(EDT_THREADS) void edt_lines_kernel(unsigned* __restrict__ out, Lines g)
{
    extern __shared__ unsigned slab[];          // [len][xw]
    const unsigned run = blockIdx.x % (unsigned)g.n_runs, outer = blockIdx.x / (unsigned)g.n_runs;
    const int x0 = (int)run * g.xw;
    unsigned* base = out + (size_t)blockIdx.y * g.n + (size_t)outer * g.outer_stride + x0;
    const int entries = g.len * g.xw;
    for (int e = threadIdx.x; e < entries; e += EDT_THREADS) {
        const int j = e / g.xw, xl = e - j * g.xw;
        if (x0 + xl < g.w) slab[e] = base[(size_t)j * g.line_stride + xl];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < entries; e += EDT_THREADS) {
        const int i = e / g.xw, xl = e - i * g.xw;
        if (x0 + xl >= g.w) continue;
        unsigned best = slab[e];
        for (int k = 1; k < g.len; ++k) {
            const unsigned k2 = (unsigned)k * (unsigned)k;
            if (k2 >= best) break;
            const bool lo = i - k >= 0, hi = i + k < g.len;
            if (!lo && !hi) break;
            if (lo) {
                const unsigned f = slab[e - k * g.xw];
                if (f < best - k2) best = f + k2;
            }
            if (hi) {
                const unsigned f = slab[e + k * g.xw];
                if (f < best - k2) best = f + k2;
            }
        }
        base[(size_t)i * g.line_stride + xl] = best;
    }
}

// ---- the border shell of the reference (common/utils/labelhelper.py:12-20), compared in integers
__global__ __launch_bounds__(EDT_THREADS) void border_mask_kernel(const unsigned* __restrict__ d_in, const unsigned* __restrict__ d_out, size_t n,
                                                                  unsigned in2, unsigned out2, uint8_t* __restrict__ mask,
                                                                  double* __restrict__ distance)
{
    const size_t i = (size_t)blockIdx.x * EDT_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned a = d_in[i], b = d_out[i];
    if (mask) mask[i] = (a != NONE && b != NONE && a <= in2 && b <= out2) ? 1 : 0;
    if (distance) distance[i] = (a == NONE || b == NONE) ? __longlong_as_double(0x7ff0000000000000ll) : __dsqrt_rn((double)((unsigned long long)a + b));
}

// ---- the boundary table
// band of the squared distance d: #{k in 1..bands : k^2 < d} = min(bands, floor(sqrt(d - 1))), in integers
__device__ __forceinline__ int band_of(unsigned d, int bands)
{
    if (d > (unsigned)(bands * bands)) return bands;
    if (d == 0) return 0;
    const unsigned t = d - 1;       // < 4096
    unsigned r = 0;
#pragma unroll
    for (unsigned b = 32; b > 0; b >>= 1)
        if ((r + b) * (r + b) <= t) r += b;
    return (int)r;
}

struct Cell {            // rcu_boundary_cell
    unsigned long long voxels, errors, unc_sum, unc_err_sum;
};
static_assert(sizeof(Cell) == sizeof(rcu_boundary_cell) && sizeof(Cell) == 32, "rcu_boundary_cell is 32 bytes");

template <int KIND>
__global__ __launch_bounds__(EDT_THREADS) void boundary_table_kernel(const uint8_t* __restrict__ prediction, const uint8_t* __restrict__ target,
                                                                     const unsigned* __restrict__ d_in, const unsigned* __restrict__ d_out,
                                                                     const void* __restrict__ unc, size_t n, int bands, Cell* __restrict__ table)
{
    __shared__ unsigned long long cell[2 * (BT_MAX_BANDS + 1) * 4];
    const int cells = 2 * (bands + 1);
    for (int c = threadIdx.x; c < cells * 4; c += EDT_THREADS) cell[c] = 0ull;
    __syncthreads();
    const size_t off = (size_t)blockIdx.y * n;
    const size_t first = (size_t)blockIdx.x * (BT_ROUNDS * EDT_THREADS);
    const int lane = threadIdx.x & (EDT_WAVE - 1);
    for (int r = 0; r < BT_ROUNDS; ++r) {
        const size_t i = first + (size_t)r * EDT_THREADS + threadIdx.x;      // (whole waves stay together: the ballots below need every lane)
        const bool in = i < n;
        int key = -1;
        bool err = false;
        unsigned q = 0;
        if (in) {
            const bool tg = target[off + i] != 0;
            err = (prediction[off + i] != 0) != tg;
            const unsigned a = d_in[off + i], b = d_out[off + i];
            const int band = (a == NONE || b == NONE || a > NONE - b) ? bands : band_of(a + b, bands);
            key = (tg ? bands + 1 : 0) + band;
            q = quantised_unc<KIND>(unc, off + i);
        }
        // one group per distinct key of the wave: the lanes that share the first remaining lane's key are combined, one lane adds them in LDS
        unsigned long long remaining = __ballot(in);
        while (remaining) {
            const int leader = __ffsll((long long)remaining) - 1;
            const int key0 = __shfl(key, leader);
            const bool same = in && key == key0;
            const unsigned long long same_lanes = __ballot(same);
            const unsigned count = (unsigned)__popcll(same_lanes), ecount = (unsigned)__popcll(__ballot(same && err));
            unsigned sum = same ? q : 0u, esum = (same && err) ? q : 0u;      // 64 x 2^24 fits 32 bits
            if constexpr (KIND != RCU_CC_UNC_NONE) {
                for (int s = 32; s > 0; s >>= 1) {
                    sum += __shfl_xor(sum, s);
                    esum += __shfl_xor(esum, s);
                }
            }
            if (lane == leader) {
                unsigned long long* c = cell + key0 * 4;
                atomicAdd(c + 0, (unsigned long long)count);
                if (ecount) atomicAdd(c + 1, (unsigned long long)ecount);
                if (sum) atomicAdd(c + 2, (unsigned long long)sum);
                if (esum) atomicAdd(c + 3, (unsigned long long)esum);
            }
            remaining &= ~same_lanes;
        }
    }
    __syncthreads();
    unsigned long long* t = reinterpret_cast<unsigned long long*>(table + (size_t)blockIdx.y * cells);
    for (int c = threadIdx.x; c < cells * 4; c += EDT_THREADS)
        if (cell[c]) atomicAdd(t + c, cell[c]);
}

// ---- surfaces and their distance histograms
// S(A) = the voxels of A with a face neighbour outside A inside the volume (= the voxels of A whose squared distance to the background is 1)
__global__ __launch_bounds__(EDT_THREADS) void surface_kernel(const uint8_t* __restrict__ a, uint8_t* __restrict__ surface, int d, int h, int w)
{
    const size_t n = (size_t)d * h * w;
    const size_t i = (size_t)blockIdx.x * EDT_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint8_t* av = a + (size_t)blockIdx.y * n;
    const unsigned i32 = (unsigned)i, row = i32 / (unsigned)w;      // (n < 2^31: 32-bit divisions)
    const int x = (int)(i32 - row * (unsigned)w), y = (int)(row % (unsigned)h), z = (int)(row / (unsigned)h);
    bool s = false;
    if (av[i] != 0) {
        const size_t plane = (size_t)h * w;
        s = (x > 0 && av[i - 1] == 0) || (x + 1 < w && av[i + 1] == 0) || (y > 0 && av[i - w] == 0) || (y + 1 < h && av[i + w] == 0) ||
            (z > 0 && av[i - plane] == 0) || (z + 1 < d && av[i + plane] == 0);
    }
    surface[(size_t)blockIdx.y * n + i] = s ? 1 : 0;
}

// hist[volume][bins]: bin d^2 for the surface voxels of this map, the last bin for those whose other surface is empty (NONE)
__global__ __launch_bounds__(EDT_THREADS) void surface_hist_kernel(const uint8_t* __restrict__ surface, const unsigned* __restrict__ dist, size_t n,
                                                                   unsigned* __restrict__ hist, size_t bins, size_t volume_stride)
{
    const size_t i = (size_t)blockIdx.x * EDT_THREADS + threadIdx.x;      // (whole waves stay together)
    const size_t off = (size_t)blockIdx.y * n;
    const bool on = i < n && surface[off + i] != 0;
    if (!__any(on)) return;
    size_t bin = 0;
    bool ok = false;
    if (on) {
        const unsigned d = dist[off + i];
        bin = d == NONE ? bins - 1 : (size_t)d;
        ok = bin < bins;       // (never a write outside the histogram)
    }
    // neighbours on a surface often share their distance: the lanes with the first lane's bin go in one add
    const unsigned long long lanes = __ballot(ok);
    if (!lanes) return;
    const int leader = __ffsll((long long)lanes) - 1;
    const unsigned long long bin0 = __shfl((unsigned long long)bin, leader);
    const bool same = ok && (unsigned long long)bin == bin0;
    const unsigned count = (unsigned)__popcll(__ballot(same));
    unsigned* hv = hist + (size_t)blockIdx.y * volume_stride;
    if ((int)(threadIdx.x & (EDT_WAVE - 1)) == leader) atomicAdd(hv + bin, count);
    else if (ok && !same) atomicAdd(hv + bin, 1u);
}

// ---- host side
int check_volume(const std::string& f, int depth, int height, int width, int n_volumes)
{
    const int extent[3] = {depth, height, width};
    const char* name[3] = {"depth", "height", "width"};
    for (int a = 0; a < 3; ++a)
        if (extent[a] < 1 || extent[a] > EDT_MAX_EXTENT)
            return report_error(RCU_ERR_INVALID, f + name[a] + " must be in 1.." + std::to_string(EDT_MAX_EXTENT) + ", got " + std::to_string(extent[a]));
    const unsigned long long n = (unsigned long long)depth * (unsigned long long)height * (unsigned long long)width;
    if (n >= 0x7fffffffull) return report_error(RCU_ERR_INVALID, f + "a volume (depth * height * width) must have fewer than 2^31 - 1 voxels");
    if (int st = check_n_volumes(f, n_volumes, EDT_MAX_VOLUMES)) return st;
    if (!batch_total_ok((size_t)n, n_volumes)) return report_error(RCU_ERR_INVALID, f + "n_per_volume * n_volumes must be below 2^32");
    return RCU_OK;
}

// the slab width of a pass over lines of `len` entries: the forced or the default one, halved until the whole line fits the slab
int slab_width_for(int len)
{
    int xw = g_slab_width > 0 ? g_slab_width : EDT_DEFAULT_SLAB_WIDTH;
    while (xw > 1 && (long long)xw * len > EDT_SLAB_ENTRIES) xw >>= 1;
    return xw;
}

void launch_lines(unsigned* out, int len, size_t line_stride, int n_outer, size_t outer_stride, int w, size_t n, int n_volumes, hipStream_t s)
{
    if (len < 2) return;       // a line of one entry is its own transform
    Lines g;
    g.len = len, g.w = w, g.xw = slab_width_for(len);
    g.n_runs = (w + g.xw - 1) / g.xw, g.n_outer = n_outer;
    g.line_stride = line_stride, g.outer_stride = outer_stride, g.n = n;
    hipLaunchKernelGGL(edt_lines_kernel, dim3((unsigned)g.n_runs * (unsigned)n_outer, n_volumes), dim3(EDT_THREADS),
                       (size_t)len * g.xw * sizeof(unsigned), s, out, g);
}

// (arguments checked by the callers)
void launch_edt(const uint8_t* mask, int d, int h, int w, int n_volumes, int zero_is_feature, unsigned* out, hipStream_t s)
{
    const size_t n = (size_t)d * h * w, rows = (size_t)n_volumes * d * h;
    const int waves = EDT_THREADS / EDT_WAVE;
    hipLaunchKernelGGL(edt_rows_kernel, dim3((unsigned)((rows + waves - 1) / waves)), dim3(EDT_THREADS), 0, s, mask, out, rows, w, zero_is_feature);
    launch_lines(out, h, (size_t)w, d, (size_t)h * w, w, n, n_volumes, s);      // along the height: one slice per outer position
    launch_lines(out, d, (size_t)h * w, h, (size_t)w, w, n, n_volumes, s);      // along the depth: one row of the slice per outer position
}

}  // namespace
}  // namespace rcu

using namespace rcu;

extern "C" int rcu_edt_set_slab_width(int slab_width)
{
    if (slab_width != 0 && (slab_width < 1 || slab_width > EDT_MAX_SLAB_WIDTH || (slab_width & (slab_width - 1)) != 0))
        return report_error(RCU_ERR_INVALID, "rcu_edt_set_slab_width: slab_width must be a power of two in 1.." + std::to_string(EDT_MAX_SLAB_WIDTH) +
                                                 " (or 0), got " + std::to_string(slab_width));
    g_slab_width = slab_width;
    return RCU_OK;
}

extern "C" int rcu_edt_sq(const uint8_t* mask_dev, int depth, int height, int width, int n_volumes, int zero_is_feature, uint32_t* out_dev, void* stream)
{
    const std::string f = "rcu_edt_sq: ";
    if (int st = check_volume(f, depth, height, width, n_volumes)) return st;
    if (zero_is_feature != 0 && zero_is_feature != 1)
        return report_error(RCU_ERR_INVALID, f + "zero_is_feature must be 0 or 1, got " + std::to_string(zero_is_feature));
    if (!mask_dev) return report_error(RCU_ERR_INVALID, f + "null mask_dev");
    if (!out_dev) return report_error(RCU_ERR_INVALID, f + "null out_dev");
    launch_edt(mask_dev, depth, height, width, n_volumes, zero_is_feature, out_dev, static_cast<hipStream_t>(stream));
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_edt_sq", e);
}

extern "C" int rcu_border_mask(const uint32_t* d_in_dev, const uint32_t* d_out_dev, size_t n, int distance_in, int distance_out, uint8_t* mask_dev,
                               double* distance_dev, void* stream)
{
    const std::string f = "rcu_border_mask: ";
    if (n == 0 || n > 0xffffffffull) return report_error(RCU_ERR_INVALID, f + "n must be in 1..2^32-1, got " + std::to_string(n));
    if (distance_in < 0 || distance_in > 65535) return report_error(RCU_ERR_INVALID, f + "distance_in must be in 0..65535, got " + std::to_string(distance_in));
    if (distance_out < 0 || distance_out > 65535)
        return report_error(RCU_ERR_INVALID, f + "distance_out must be in 0..65535, got " + std::to_string(distance_out));
    if (!d_in_dev) return report_error(RCU_ERR_INVALID, f + "null d_in_dev");
    if (!d_out_dev) return report_error(RCU_ERR_INVALID, f + "null d_out_dev");
    if (!mask_dev && !distance_dev) return report_error(RCU_ERR_INVALID, f + "mask_dev and distance_dev are both null");
    hipLaunchKernelGGL(border_mask_kernel, dim3((unsigned)((n + EDT_THREADS - 1) / EDT_THREADS)), dim3(EDT_THREADS), 0, static_cast<hipStream_t>(stream),
                       d_in_dev, d_out_dev, n, (unsigned)distance_in * (unsigned)distance_in, (unsigned)distance_out * (unsigned)distance_out, mask_dev,
                       distance_dev);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_border_mask", e);
}

extern "C" int rcu_boundary_table(const uint8_t* prediction_dev, const uint8_t* target_dev, const uint32_t* d_in_dev, const uint32_t* d_out_dev,
                                  const void* unc_dev, int unc_kind, size_t n_per_volume, int n_volumes, int bands, rcu_boundary_cell* table_dev,
                                  void* stream)
{
    const std::string f = "rcu_boundary_table: ";
    if (int st = check_batch(f, n_per_volume, n_volumes, EDT_MAX_VOLUMES)) return st;
    if (bands < 1 || bands > BT_MAX_BANDS) return report_error(RCU_ERR_INVALID, f + "bands must be in 1.." + std::to_string(BT_MAX_BANDS) + ", got " + std::to_string(bands));
    if (int st = check_unc_source(f, unc_kind, unc_dev)) return st;
    if (!prediction_dev) return report_error(RCU_ERR_INVALID, f + "null prediction_dev");
    if (!target_dev) return report_error(RCU_ERR_INVALID, f + "null target_dev");
    if (!d_in_dev) return report_error(RCU_ERR_INVALID, f + "null d_in_dev");
    if (!d_out_dev) return report_error(RCU_ERR_INVALID, f + "null d_out_dev");
    if (!table_dev) return report_error(RCU_ERR_INVALID, f + "null table_dev");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(table_dev, 0, (size_t)n_volumes * 2 * (bands + 1) * sizeof(rcu_boundary_cell), s);
    if (e != hipSuccess) return hip_failed("rcu_boundary_table", e);
    const size_t per_group = (size_t)BT_ROUNDS * EDT_THREADS;
    const dim3 grid((unsigned)((n_per_volume + per_group - 1) / per_group), n_volumes);
    Cell* t = reinterpret_cast<Cell*>(table_dev);
    with_unc_kind(unc_kind, [&](auto kind) {
        hipLaunchKernelGGL(boundary_table_kernel<decltype(kind)::value>, grid, dim3(EDT_THREADS), 0, s, prediction_dev, target_dev, d_in_dev, d_out_dev, unc_dev, n_per_volume, bands, t);
    });
    e = hipGetLastError();
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_boundary_table", e);
}

extern "C" size_t rcu_surface_distance_bins(int depth, int height, int width)
{
    if (depth < 1 || height < 1 || width < 1 || depth > EDT_MAX_EXTENT || height > EDT_MAX_EXTENT || width > EDT_MAX_EXTENT) return 0;
    const size_t d = depth - 1, h = height - 1, w = width - 1;
    return d * d + h * h + w * w + 2;
}

// the workspace: [surface of the prediction: n_volumes x n u8][surface of the target: the same][distances: n_volumes x n u32]
extern "C" size_t rcu_surface_distance_workspace_bytes(size_t n_per_volume, int n_volumes)
{
    if (!batch_ok(n_per_volume, n_volumes, EDT_MAX_VOLUMES)) return 0;
    const size_t all = n_per_volume * (size_t)n_volumes;
    return 2 * round256(all) + round256(all * sizeof(unsigned));
}

extern "C" int rcu_surface_distance_hist(const uint8_t* prediction_dev, const uint8_t* target_dev, int depth, int height, int width, int n_volumes,
                                         uint32_t* hist_dev, void* workspace_dev, void* stream)
{
    const std::string f = "rcu_surface_distance_hist: ";
    if (int st = check_volume(f, depth, height, width, n_volumes)) return st;
    if (!prediction_dev) return report_error(RCU_ERR_INVALID, f + "null prediction_dev");
    if (!target_dev) return report_error(RCU_ERR_INVALID, f + "null target_dev");
    if (!hist_dev) return report_error(RCU_ERR_INVALID, f + "null hist_dev");
    if (!workspace_dev) return report_error(RCU_ERR_INVALID, f + "null workspace_dev");
    const size_t n = (size_t)depth * height * width, all = n * (size_t)n_volumes, bins = rcu_surface_distance_bins(depth, height, width);
    char* p = reinterpret_cast<char*>(workspace_dev);
    uint8_t* sp = reinterpret_cast<uint8_t*>(p);
    uint8_t* st = reinterpret_cast<uint8_t*>(p + round256(all));
    unsigned* dist = reinterpret_cast<unsigned*>(p + 2 * round256(all));
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(hist_dev, 0, (size_t)n_volumes * 2 * bins * sizeof(uint32_t), s);
    if (e != hipSuccess) return hip_failed("rcu_surface_distance_hist", e);
    const dim3 per_voxel((unsigned)((n + EDT_THREADS - 1) / EDT_THREADS), n_volumes);
    hipLaunchKernelGGL(surface_kernel, per_voxel, dim3(EDT_THREADS), 0, s, prediction_dev, sp, depth, height, width);
    hipLaunchKernelGGL(surface_kernel, per_voxel, dim3(EDT_THREADS), 0, s, target_dev, st, depth, height, width);
    // direction 0: the prediction's surface voxels by their distance to the target's surface; direction 1: the other way round
    launch_edt(st, depth, height, width, n_volumes, 0, dist, s);
    hipLaunchKernelGGL(surface_hist_kernel, per_voxel, dim3(EDT_THREADS), 0, s, sp, dist, n, hist_dev, bins, 2 * bins);
    launch_edt(sp, depth, height, width, n_volumes, 0, dist, s);
    hipLaunchKernelGGL(surface_hist_kernel, per_voxel, dim3(EDT_THREADS), 0, s, st, dist, n, hist_dev + bins, bins, 2 * bins);
    e = hipGetLastError();
    return e == hipSuccess ? RCU_OK : hip_failed("rcu_surface_distance_hist", e);
}
