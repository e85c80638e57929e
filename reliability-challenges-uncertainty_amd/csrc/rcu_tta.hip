// Test-time augmentation (include/rcu.h, "Test-time augmentation"): the eight elements of the dihedral group D4 on the last two axes of
// NCHW float32 images (rcu_tta_transform) and the fold of a statistics blob accumulated over transformed images back into canonical
// orientation (rcu_mc_fold_transformed).  Both are one gather per H x W plane:
//     out[plane][i][j] (=|+=) in[plane][a][b]
// with (a, b) the source pixel of output pixel (i, j) under the element.  Memory-bound: nothing but the copy (and the add) per element.
//   codes 0-3 keep the axes:  a = i or H-1-i,  b = j or W-1-j -- a thread moves 16 bytes along the output row, read from the same row of the
//             source in the same or the reversed order (row-vector kernel; scalar where W is not a multiple of the vector)
//   codes 4-7 swap them (H == W = S): a = j or S-1-j,  b = i or S-1-i -- a source row becomes an output column, so 32 x 32 tiles go
//             through LDS: read along source rows, written along output rows (tile kernel)
#include "../../include/rcu.h"
#include "rcu_kernels.h"

#include <string>

namespace rcu {
namespace {

constexpr int TTA_THREADS = 256;
constexpr int TTA_TILE = 32;          // tile kernel: TTA_TILE x TTA_TILE pixels, TTA_TILE x (TTA_THREADS / TTA_TILE) threads
constexpr unsigned TTA_MAX_PLANE_BLOCKS = 4096;   // grid extent over planes; more planes are walked by a grid stride

// element -> its inverse (rot90 and rot270 are each other's; every other element is an involution)
constexpr int kInverse[8] = {0, 1, 2, 3, 4, 6, 5, 7};
inline bool swaps_axes(int e) { return e >= RCU_TTA_TRANSPOSE; }
// codes 0-3: flip of the row index (a = H-1-i) / of the column index (b = W-1-j)
inline int flips_rows(int e) { return e == RCU_TTA_FLIP_V || e == RCU_TTA_ROT180; }
inline int flips_cols(int e) { return e == RCU_TTA_FLIP_H || e == RCU_TTA_ROT180; }
// codes 4-7: a = S-1-j for rot270 / anti_transpose, b = S-1-i for rot90 / anti_transpose
inline int flips_a(int e) { return e == RCU_TTA_ROT270 || e == RCU_TTA_ANTI_TRANSPOSE; }
inline int flips_b(int e) { return e == RCU_TTA_ROT90 || e == RCU_TTA_ANTI_TRANSPOSE; }

template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) Vec {
    T v[VEC];
};

// Codes 0-3.  grid.x covers the H * W / VEC vectors of a plane, grid.y the planes (strided).
template <typename T, int VEC, bool ADD>
__global__ __launch_bounds__(TTA_THREADS) void tta_rows_kernel(const T* __restrict__ in, T* __restrict__ out, size_t planes, int H, int W,
                                                               int flip_rows, int flip_cols)
{
    using V = Vec<T, VEC>;
    const unsigned wv = (unsigned)(W / VEC);
    const unsigned t = blockIdx.x * TTA_THREADS + threadIdx.x;
    if (t >= (unsigned)H * wv) return;
    const unsigned i = t / wv, jv = t - i * wv;
    const unsigned si = flip_rows ? (unsigned)H - 1 - i : i;
    const unsigned sjv = flip_cols ? wv - 1 - jv : jv;
    const size_t plane_vecs = (size_t)H * wv;
    for (size_t p = blockIdx.y; p < planes; p += gridDim.y) {
        const V* src = reinterpret_cast<const V*>(in) + p * plane_vecs;
        V* dst = reinterpret_cast<V*>(out) + p * plane_vecs;
        V s = src[(size_t)si * wv + sjv];
        V r;
#pragma unroll
        for (int k = 0; k < VEC; ++k) r.v[k] = flip_cols ? s.v[VEC - 1 - k] : s.v[k];
        if (ADD) {
            const V d = dst[t];
#pragma unroll
            for (int k = 0; k < VEC; ++k) r.v[k] = d.v[k] + r.v[k];
        }
        dst[t] = r;
    }
}

// Codes 4-7 on S x S planes.  Block (bx, by) owns the output tile rows i0 .. i0+31, columns j0 .. j0+31; the source pixels it needs are
// rows a(j0 .. j0+31), columns b(i0 .. i0+31): read along those source rows into tile[r][c] = in[a(j0 + r)][b(i0 + c)], written along the
// output rows as out[i0 + r][j0 + c] = tile[c][r].
template <typename T, bool ADD>
__global__ __launch_bounds__(TTA_THREADS) void tta_tile_kernel(const T* __restrict__ in, T* __restrict__ out, size_t planes, int S, int flip_a,
                                                               int flip_b)
{
    __shared__ T tile[TTA_TILE][TTA_TILE + 1];
    constexpr int ROWS = TTA_THREADS / TTA_TILE;
    const int c = threadIdx.x % TTA_TILE, r0 = threadIdx.x / TTA_TILE;
    const int i0 = blockIdx.y * TTA_TILE, j0 = blockIdx.x * TTA_TILE;
    const size_t plane_elems = (size_t)S * S;
    for (size_t p = blockIdx.z; p < planes; p += gridDim.z) {
        const T* src = in + p * plane_elems;
        T* dst = out + p * plane_elems;
        for (int r = r0; r < TTA_TILE; r += ROWS) {
            const int j = j0 + r, i = i0 + c;
            if (j < S && i < S) {
                const int a = flip_a ? S - 1 - j : j, b = flip_b ? S - 1 - i : i;
                tile[r][c] = src[(size_t)a * S + b];
            }
        }
        __syncthreads();
        for (int r = r0; r < TTA_TILE; r += ROWS) {
            const int i = i0 + r, j = j0 + c;
            if (i < S && j < S) {
                const size_t o = (size_t)i * S + j;
                const T v = tile[c][r];
                dst[o] = ADD ? dst[o] + v : v;
            }
        }
        __syncthreads();      // the tile is refilled for the next plane
    }
}

inline unsigned plane_blocks(size_t planes) { return (unsigned)(planes < TTA_MAX_PLANE_BLOCKS ? planes : TTA_MAX_PLANE_BLOCKS); }

template <typename T, int VEC, bool ADD>
hipError_t launch_rows(const T* in, T* out, size_t planes, int H, int W, int e, hipStream_t stream)
{
    const unsigned vecs = (unsigned)H * (unsigned)(W / VEC);
    hipLaunchKernelGGL((tta_rows_kernel<T, VEC, ADD>), dim3((vecs + TTA_THREADS - 1) / TTA_THREADS, plane_blocks(planes)), dim3(TTA_THREADS), 0,
                       stream, in, out, planes, H, W, flips_rows(e), flips_cols(e));
    return hipGetLastError();
}

// out (=|+=) element e applied to every H x W plane of in
template <typename T, bool ADD>
hipError_t launch_apply(const T* in, T* out, size_t planes, int H, int W, int e, hipStream_t stream)
{
    if (swaps_axes(e)) {
        const unsigned tiles = (unsigned)((H + TTA_TILE - 1) / TTA_TILE);
        hipLaunchKernelGGL((tta_tile_kernel<T, ADD>), dim3(tiles, tiles, plane_blocks(planes)), dim3(TTA_THREADS), 0, stream, in, out, planes, H,
                           flips_a(e), flips_b(e));
        return hipGetLastError();
    }
    constexpr int VEC = 16 / sizeof(T);       // 16 bytes per thread where the rows are whole vectors and the planes start aligned
    const bool aligned = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % 16) == 0;
    if (W % VEC == 0 && aligned) return launch_rows<T, VEC, ADD>(in, out, planes, H, W, e, stream);
    return launch_rows<T, 1, ADD>(in, out, planes, H, W, e, stream);
}

int check_shape(const char* fn, size_t n, int height, int width, int element)
{
    if (element < RCU_TTA_IDENTITY || element > RCU_TTA_ANTI_TRANSPOSE)
        return report_error(RCU_ERR_INVALID, std::string(fn) + ": element code " + std::to_string(element) + " outside 0..7");
    if (n < 1 || height < 1 || width < 1) return report_error(RCU_ERR_INVALID, std::string(fn) + ": empty batch or plane (n, height, width >= 1)");
    if ((size_t)height * (size_t)width > (size_t)1 << 30) return report_error(RCU_ERR_INVALID, std::string(fn) + ": plane larger than 2^30 pixels");
    if (swaps_axes(element) && height != width)
        return report_error(RCU_ERR_INVALID, std::string(fn) + ": element " + std::to_string(element) + " swaps H and W and needs square planes, got " +
                                                 std::to_string(height) + " x " + std::to_string(width));
    return RCU_OK;
}

bool overlap(const void* a, const void* b, size_t bytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}

}  // namespace
}  // namespace rcu

using namespace rcu;

extern "C" int rcu_tta_transform(const float* x_dev, size_t n, int channels, int height, int width, int element, float* out_dev, void* stream)
{
    if (!x_dev || !out_dev) return report_error(RCU_ERR_INVALID, "rcu_tta_transform: null argument");
    if (int st = check_shape("rcu_tta_transform", n, height, width, element)) return st;
    if (channels < 1) return report_error(RCU_ERR_INVALID, "rcu_tta_transform: channels must be >= 1");
    const size_t planes = n * (size_t)channels;
    if (overlap(x_dev, out_dev, planes * (size_t)height * width * sizeof(float)))
        return report_error(RCU_ERR_INVALID, "rcu_tta_transform: out must not overlap x (out == x is not supported)");
    hipError_t e = launch_apply<float, false>(x_dev, out_dev, planes, height, width, element, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return report_error(RCU_ERR_HIP, std::string("rcu_tta_transform: ") + hipGetErrorString(e));
    return RCU_OK;
}

extern "C" int rcu_mc_fold_transformed(const void* src_stats_dev, void* dst_stats_dev, size_t n, int height, int width, int nb_classes, int flags,
                                       int element, void* stream)
{
    if (!src_stats_dev || !dst_stats_dev) return report_error(RCU_ERR_INVALID, "rcu_mc_fold_transformed: null argument");
    if (int st = check_shape("rcu_mc_fold_transformed", n, height, width, element)) return st;
    if (nb_classes < 1 || nb_classes > MAX_CLASSES) return report_error(RCU_ERR_INVALID, "rcu_mc_fold_transformed: nb_classes must be in 1..8");
    if (flags & ~(RCU_MC_MI | RCU_MC_VAR | RCU_MC_EXACT))
        return report_error(RCU_ERR_INVALID, "rcu_mc_fold_transformed: flags must be a combination of RCU_MC_MI, RCU_MC_VAR and RCU_MC_EXACT, got " +
                                                 std::to_string(flags));
    const size_t hw = (size_t)height * width;
    const size_t bytes = rcu_mc_stats_bytes(n, hw, nb_classes, flags);
    if (overlap(src_stats_dev, dst_stats_dev, bytes)) return report_error(RCU_ERR_INVALID, "rcu_mc_fold_transformed: src and dst must not overlap");
    const size_t planes = n * (size_t)(nb_classes + ((flags & RCU_MC_VAR) ? nb_classes : 0) + ((flags & RCU_MC_MI) ? 1 : 0));
    const int inv = kInverse[element];
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = (flags & (RCU_MC_VAR | RCU_MC_EXACT))
                       ? launch_apply<double, true>(static_cast<const double*>(src_stats_dev), static_cast<double*>(dst_stats_dev), planes, height,
                                                    width, inv, s)
                       : launch_apply<float, true>(static_cast<const float*>(src_stats_dev), static_cast<float*>(dst_stats_dev), planes, height,
                                                   width, inv, s);
    if (e != hipSuccess) return report_error(RCU_ERR_HIP, std::string("rcu_mc_fold_transformed: ") + hipGetErrorString(e));
    return RCU_OK;
}
