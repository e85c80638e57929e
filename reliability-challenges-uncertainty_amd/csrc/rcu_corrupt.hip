// Input corruptions (include/rcu.h, "Input corruptions"): eight seeded appearance corruptions of an NCHW float32 batch for dataset-shift runs of
// the test scripts.  The output of a slice is a function of (its pixels, kind, amount, key, its global index) alone: no kernel here lets the
// batch size, the position in the batch or the launch geometry into the arithmetic.
//   pointwise kinds (intensity_shift, bias_field, ghosting, channel_drop, the apply half of contrast): one thread per 16 bytes of an output row
//             (scalar where W is not a multiple of 4 or a pointer is not 16-byte aligned), grid.y strides over the planes -- rcu_tta.hip's shape
//   gaussian_noise: the same, but a thread owns its pixels in the FOUR channels of a normals block (logit_normals4 gives the normals of classes
//             4q .. 4q+3 at once): one Philox + Box-Muller per pixel and block instead of one per pixel and channel
//   gaussian_blur: a 32 x 64 output tile with its halo of r rows / columns (reflected at the borders) staged in LDS, the H pass written to a second
//             LDS image, the W pass read from it (eight fmaf chains per lane share each tap): every input element comes from HBM once per tile
//             that needs it
//   downsample: one thread per k x k block: the float32 sum in raster order, one division, k x k stores
//   contrast: one workgroup per plane sums it in float64 -- thread t takes the 4-element chunks t, t + 1024, ... in order, then a fixed LDS
//             tree -- and leaves the mean in the workspace; the apply half is a pointwise kernel
#include "../../include/rcu.h"
#include "rcu_head_common.h"
#include "rcu_kernels.h"

#include <cmath>
#include <string>

namespace rcu {
namespace {

constexpr int CR_THREADS = 256;
constexpr unsigned CR_MAX_PLANE_BLOCKS = 4096;    // grid extent over planes; more planes are walked by a grid stride
constexpr int BLUR_TH = 32, BLUR_TW = 64;         // output tile of the blur kernel: one column per lane, TH / 4 rows per wave
constexpr int BLUR_MAX_RADIUS = 32;               // int(4 * 8 + 0.5)
constexpr int MEAN_THREADS = 1024;
constexpr int AUX_CHUNK = 896;                    // floats of aux_host one fill launch carries as kernel arguments
constexpr int BIAS_TERMS = 8;                     // (u, v) in {0, 1, 2}^2 without (0, 0)

template <int VEC>
struct alignas(sizeof(float) * VEC) FVec {
    float v[VEC];
};

struct PointArgs {
    const float* x;
    float* out;
    size_t planes;
    int C, H, W;
    float a;
    unsigned mask;           // channel_drop
    const double* mean;      // contrast: [planes]
    const float* coef;       // bias_field: [C][8]
    const float* A;          //             [3][H]
    const float* B;          //             [3][W]
};

// kinds 3 (apply half), 4, 5, 6, 7.  grid.x covers the H * W / VEC vectors of a plane, grid.y the planes (strided).
template <int KIND, int VEC>
__global__ __launch_bounds__(CR_THREADS) void corrupt_point_kernel(PointArgs q)
{
    using V = FVec<VEC>;
    const unsigned wv = (unsigned)(q.W / VEC);
    const unsigned t = blockIdx.x * CR_THREADS + threadIdx.x;
    if (t >= (unsigned)q.H * wv) return;
    const unsigned i = t / wv, jv = t - i * wv;
    const size_t plane_vecs = (size_t)q.H * wv;
    float ab[BIAS_TERMS][VEC];      // bias_field: A_u[i] * B_v[j] of the thread's pixels, (u, v) in raster order without (0, 0)
    if (KIND == RCU_CORRUPT_BIAS_FIELD) {
#pragma unroll
        for (int e = 0; e < BIAS_TERMS; ++e) {
            const int u = (e + 1) / 3, v = (e + 1) % 3;
            const float au = q.A[(size_t)u * q.H + i];
#pragma unroll
            for (int k = 0; k < VEC; ++k) ab[e][k] = au * q.B[(size_t)v * q.W + jv * VEC + k];
        }
    }
    unsigned ti = t;                // ghosting: the vector of row (i + H / 2) mod H in the same columns
    if (KIND == RCU_CORRUPT_GHOSTING) ti = ((i + (unsigned)q.H / 2) % (unsigned)q.H) * wv + jv;
    for (size_t p = blockIdx.y; p < q.planes; p += gridDim.y) {
        const int c = (int)(p % (size_t)q.C);
        const V* src = reinterpret_cast<const V*>(q.x) + p * plane_vecs;
        V* dst = reinterpret_cast<V*>(q.out) + p * plane_vecs;
        V r;
        if (KIND == RCU_CORRUPT_CHANNEL_DROP && ((q.mask >> c) & 1u)) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) r.v[k] = 0.f;
            dst[t] = r;
            continue;
        }
        const V s = src[t];
        if (KIND == RCU_CORRUPT_CONTRAST) {
            const float m32 = (float)q.mean[p];
#pragma unroll
            for (int k = 0; k < VEC; ++k) r.v[k] = fmaf(q.a, s.v[k] - m32, m32);
        } else if (KIND == RCU_CORRUPT_INTENSITY_SHIFT) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) r.v[k] = s.v[k] + q.a;
        } else if (KIND == RCU_CORRUPT_BIAS_FIELD) {
            float f[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) f[k] = 0.f;
#pragma unroll
            for (int e = 0; e < BIAS_TERMS; ++e) {
                const float ce = q.coef[c * BIAS_TERMS + e];
#pragma unroll
                for (int k = 0; k < VEC; ++k) f[k] = fmaf(ce, ab[e][k], f[k]);
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) r.v[k] = s.v[k] * expf(q.a * f[k]);
        } else if (KIND == RCU_CORRUPT_GHOSTING) {
            const V g = src[ti];
#pragma unroll
            for (int k = 0; k < VEC; ++k) r.v[k] = fmaf(q.a, g.v[k], s.v[k]);
        } else {
            r = s;
        }
        dst[t] = r;
    }
}

// kind 0.  grid.y strides over (image, block q of four channels): the normals of channels 4q .. 4q+3 of a pixel are one logit_normals4.
template <int VEC>
__global__ __launch_bounds__(CR_THREADS) void corrupt_noise_kernel(const float* __restrict__ x, float* __restrict__ out, size_t n, int C, int H, int W,
                                                                   float a, unsigned long long key, unsigned long long first)
{
    using V = FVec<VEC>;
    const unsigned wv = (unsigned)(W / VEC);
    const unsigned t = blockIdx.x * CR_THREADS + threadIdx.x;
    if (t >= (unsigned)H * wv) return;
    const unsigned pix = t * VEC;                 // = i * W + j of the thread's first pixel (rows are whole vectors)
    const size_t plane_vecs = (size_t)H * wv;
    const unsigned qb = (unsigned)(C + 3) >> 2;
    for (size_t s = blockIdx.y; s < n * qb; s += gridDim.y) {
        const size_t img = s / qb;
        const unsigned qi = (unsigned)(s - img * qb);
        const int nc = C - 4 * (int)qi < 4 ? C - 4 * (int)qi : 4;
        float z[VEC][4];
#pragma unroll
        for (int k = 0; k < VEC; ++k) logit_normals4(key, first + img, pix + k, qi, z[k]);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            if (cc < nc) {
                const size_t p = img * (size_t)C + 4 * qi + cc;
                const V v = reinterpret_cast<const V*>(x)[p * plane_vecs + t];
                V r;
#pragma unroll
                for (int k = 0; k < VEC; ++k) r.v[k] = fmaf(a, z[k][cc], v.v[k]);
                reinterpret_cast<V*>(out)[p * plane_vecs + t] = r;
            }
        }
    }
}

struct BlurTaps {
    float w[2 * BLUR_MAX_RADIUS + 1];
};

// scipy's 'reflect' (d c b a | a b c d | d c b a); one reflection reaches every index a tile needs because r < n.  Tiles that hang over the far
// border also ask for rows / columns nobody reads: those are clamped into the plane.
__device__ __forceinline__ int reflect_index(int i, int n)
{
    if (i < 0) i = -i - 1;
    if (i >= n) i = 2 * n - 1 - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// kind 1.  Block (bx, by) owns output rows i0 .. i0+31, columns j0 .. j0+63 of a plane; LDS: tin[TH + 2r][TW + 2r], mid[TH][TW + 2r], the 2r + 1
// taps.  A wave owns 8 rows of the tile, a lane one column (conflict-free LDS rows, coalesced stores): 8 independent fmaf chains per lane share
// each tap, so a tap is read once per 8 products and the LDS latency of one chain hides behind the other seven.
__global__ __launch_bounds__(CR_THREADS) void corrupt_blur_kernel(const float* __restrict__ x, float* __restrict__ out, size_t planes, int H, int W, int r,
                                                                  BlurTaps taps)
{
    extern __shared__ float blur_lds[];
    constexpr int RB = BLUR_TH / (CR_THREADS / 64);      // rows per wave
    const int IW = BLUR_TW + 2 * r, IH = BLUR_TH + 2 * r, K = 2 * r + 1;
    float* tin = blur_lds;
    float* mid = tin + IH * IW;
    float* wl = mid + BLUR_TH * IW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = blockIdx.y * BLUR_TH, j0 = blockIdx.x * BLUR_TW;
    const int rbase = wave * RB;
    const size_t plane_elems = (size_t)H * W;
    for (int kk = 0; kk < K; ++kk)
        if (threadIdx.x == 0) wl[kk] = taps.w[kk];
    for (size_t p = blockIdx.z; p < planes; p += gridDim.z) {
        const float* src = x + p * plane_elems;
        float* dst = out + p * plane_elems;
        for (int rr = wave; rr < IH; rr += CR_THREADS / 64) {
            const size_t row = (size_t)reflect_index(i0 - r + rr, H) * W;
            for (int cc = lane; cc < IW; cc += 64) tin[rr * IW + cc] = src[row + reflect_index(j0 - r + cc, W)];
        }
        __syncthreads();
        // H axis: mid[ri][cc] = sum_k w[k] * x[i0 + ri + k][column cc], k = -r .. r, one fmaf chain from 0 per output
        for (int cc = lane; cc < IW; cc += 64) {
            float acc[RB];
#pragma unroll
            for (int o = 0; o < RB; ++o) acc[o] = 0.f;
            for (int kk = 0; kk < K; ++kk) {
                const float wk = wl[kk];
#pragma unroll
                for (int o = 0; o < RB; ++o) acc[o] = fmaf(wk, tin[(rbase + o + kk) * IW + cc], acc[o]);
            }
#pragma unroll
            for (int o = 0; o < RB; ++o) mid[(rbase + o) * IW + cc] = acc[o];
        }
        __syncthreads();
        // W axis, from the float32 result of the H pass
        {
            float acc[RB];
#pragma unroll
            for (int o = 0; o < RB; ++o) acc[o] = 0.f;
            for (int kk = 0; kk < K; ++kk) {
                const float wk = wl[kk];
#pragma unroll
                for (int o = 0; o < RB; ++o) acc[o] = fmaf(wk, mid[(rbase + o) * IW + lane + kk], acc[o]);
            }
#pragma unroll
            for (int o = 0; o < RB; ++o)
                if (i0 + rbase + o < H && j0 + lane < W) dst[(size_t)(i0 + rbase + o) * W + j0 + lane] = acc[o];
        }
        __syncthreads();      // both images are refilled for the next plane
    }
}

// kind 2.  One thread per k x k block (the blocks at the far edges are partial); grid.y strides over the planes.
__global__ __launch_bounds__(CR_THREADS) void corrupt_downsample_kernel(const float* __restrict__ x, float* __restrict__ out, size_t planes, int H, int W, int k)
{
    const unsigned bw = (unsigned)(W + k - 1) / (unsigned)k, bh = (unsigned)(H + k - 1) / (unsigned)k;
    const unsigned t = blockIdx.x * CR_THREADS + threadIdx.x;
    if (t >= bh * bw) return;
    const int bi = (int)(t / bw), bj = (int)(t - (unsigned)bi * bw);
    const int i0 = bi * k, j0 = bj * k;
    const int i1 = i0 + k < H ? i0 + k : H, j1 = j0 + k < W ? j0 + k : W;
    const float count = (float)((i1 - i0) * (j1 - j0));
    const size_t plane_elems = (size_t)H * W;
    for (size_t p = blockIdx.y; p < planes; p += gridDim.y) {
        const float* src = x + p * plane_elems;
        float* dst = out + p * plane_elems;
        float sum = 0.f;
        for (int i = i0; i < i1; ++i)
            for (int j = j0; j < j1; ++j) sum += src[(size_t)i * W + j];
        const float m = sum / count;
        for (int i = i0; i < i1; ++i)
            for (int j = j0; j < j1; ++j) dst[(size_t)i * W + j] = m;
    }
}

// kind 3, first half: mean[p] = (float64 sum of plane p) / (H W).  The partition is by element index alone -- thread t owns the 4-element chunks
// t, t + 1024, ... and adds their elements in order -- so the vector and the scalar load forms give the same bits.
__global__ __launch_bounds__(MEAN_THREADS) void corrupt_mean_kernel(const float* __restrict__ x, size_t planes, unsigned hw, int vec_ok, double* __restrict__ mean)
{
    __shared__ double part[MEAN_THREADS];
    const unsigned chunks = (hw + 3) / 4;
    for (size_t p = blockIdx.x; p < planes; p += gridDim.x) {
        const float* src = x + p * (size_t)hw;
        double s = 0.0;
        for (unsigned ch = threadIdx.x; ch < chunks; ch += MEAN_THREADS) {
            const unsigned e = ch * 4;
            if (vec_ok && e + 4 <= hw) {
                const FVec<4> v = *reinterpret_cast<const FVec<4>*>(src + e);
                s += (double)v.v[0];
                s += (double)v.v[1];
                s += (double)v.v[2];
                s += (double)v.v[3];
            } else {
                for (unsigned k = e; k < e + 4 && k < hw; ++k) s += (double)src[k];
            }
        }
        part[threadIdx.x] = s;
        __syncthreads();
        for (int half = MEAN_THREADS / 2; half > 0; half >>= 1) {
            if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
            __syncthreads();
        }
        if (threadIdx.x == 0) mean[p] = part[0] / (double)hw;
        __syncthreads();      // part is refilled for the next plane
    }
}

struct AuxChunk {
    float v[AUX_CHUNK];
};

// host values -> the workspace, carried as kernel arguments: stream-ordered, no staging copy, no synchronisation
__global__ __launch_bounds__(CR_THREADS) void corrupt_aux_fill_kernel(AuxChunk c, float* __restrict__ dst, int count)
{
    for (int k = threadIdx.x; k < count; k += CR_THREADS) dst[k] = c.v[k];
}

inline unsigned plane_blocks(size_t planes) { return (unsigned)(planes < CR_MAX_PLANE_BLOCKS ? planes : CR_MAX_PLANE_BLOCKS); }

template <int KIND>
hipError_t launch_point(const PointArgs& q, hipStream_t stream)
{
    const bool aligned = ((reinterpret_cast<uintptr_t>(q.x) | reinterpret_cast<uintptr_t>(q.out)) % 16) == 0;
    if (q.W % 4 == 0 && aligned) {
        const unsigned vecs = (unsigned)q.H * (unsigned)(q.W / 4);
        hipLaunchKernelGGL((corrupt_point_kernel<KIND, 4>), dim3((vecs + CR_THREADS - 1) / CR_THREADS, plane_blocks(q.planes)), dim3(CR_THREADS), 0,
                           stream, q);
    } else {
        const unsigned vecs = (unsigned)q.H * (unsigned)q.W;
        hipLaunchKernelGGL((corrupt_point_kernel<KIND, 1>), dim3((vecs + CR_THREADS - 1) / CR_THREADS, plane_blocks(q.planes)), dim3(CR_THREADS), 0,
                           stream, q);
    }
    return hipGetLastError();
}

hipError_t launch_noise(const float* x, float* out, size_t n, int C, int H, int W, float a, unsigned long long key, unsigned long long first,
                        hipStream_t stream)
{
    const bool aligned = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) % 16) == 0;
    const unsigned gy = plane_blocks(n * (size_t)((C + 3) / 4));
    if (W % 4 == 0 && aligned) {
        const unsigned vecs = (unsigned)H * (unsigned)(W / 4);
        hipLaunchKernelGGL((corrupt_noise_kernel<4>), dim3((vecs + CR_THREADS - 1) / CR_THREADS, gy), dim3(CR_THREADS), 0, stream, x, out, n, C, H, W, a,
                           key, first);
    } else {
        const unsigned vecs = (unsigned)H * (unsigned)W;
        hipLaunchKernelGGL((corrupt_noise_kernel<1>), dim3((vecs + CR_THREADS - 1) / CR_THREADS, gy), dim3(CR_THREADS), 0, stream, x, out, n, C, H, W, a,
                           key, first);
    }
    return hipGetLastError();
}

inline size_t blur_lds_bytes(int r) { return ((size_t)((BLUR_TH + 2 * r) + BLUR_TH) * (size_t)(BLUR_TW + 2 * r) + (size_t)(2 * r + 1)) * sizeof(float); }

// workspace of bias_field: aux_host as it is -- coef [C][8], A [3][H], B [3][W] back to back
inline size_t bias_aux_floats(int C, int H, int W) { return (size_t)BIAS_TERMS * C + 3 * (size_t)H + 3 * (size_t)W; }

hipError_t fill_aux(const float* host, size_t count, float* dst, hipStream_t stream)
{
    for (size_t done = 0; done < count; done += AUX_CHUNK) {
        AuxChunk c;
        const int part = (int)(count - done < (size_t)AUX_CHUNK ? count - done : (size_t)AUX_CHUNK);
        for (int k = 0; k < part; ++k) c.v[k] = host[done + k];
        for (int k = part; k < AUX_CHUNK; ++k) c.v[k] = 0.f;
        hipLaunchKernelGGL(corrupt_aux_fill_kernel, dim3(1), dim3(CR_THREADS), 0, stream, c, dst + done, part);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

bool overlap(const void* a, const void* b, size_t bytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}

int invalid(const std::string& msg) { return report_error(RCU_ERR_INVALID, "rcu_corrupt: " + msg); }

// r = int(4 sigma + 0.5), scipy.ndimage.gaussian_filter's radius at truncate = 4
inline int blur_radius(double sigma) { return (int)(4.0 * sigma + 0.5); }

}  // namespace
}  // namespace rcu

using namespace rcu;

extern "C" size_t rcu_corrupt_workspace_bytes(size_t n, int channels, int height, int width, int kind)
{
    if (n < 1 || channels < 1 || height < 1 || width < 1) return 0;
    if (kind == RCU_CORRUPT_CONTRAST) return round256(n * (size_t)channels * sizeof(double));
    if (kind == RCU_CORRUPT_BIAS_FIELD)
        return round256(bias_aux_floats(channels, height, width) * sizeof(float));
    return 0;
}

extern "C" int rcu_corrupt(const float* x_dev, size_t n, int channels, int height, int width, int kind, double amount, uint64_t key,
                           uint64_t first_sample, const float* aux_host, int n_aux, float* out_dev, void* workspace_dev, void* stream)
{
    if (!x_dev || !out_dev) return invalid("null argument (x_dev, out_dev)");
    if (kind < RCU_CORRUPT_GAUSSIAN_NOISE || kind > RCU_CORRUPT_CHANNEL_DROP) return invalid("kind code " + std::to_string(kind) + " outside 0..7");
    if (n < 1 || channels < 1 || height < 1 || width < 1) return invalid("empty batch or plane (n, channels, height, width >= 1)");
    if ((size_t)height * (size_t)width > (size_t)1 << 30) return invalid("plane larger than 2^30 pixels");
    if (channels > 4096 || n > (size_t)1 << 40) return invalid("channels must be <= 4096 and n <= 2^40");
    if (!std::isfinite(amount)) return invalid("amount must be finite");
    const std::string got = ", got " + std::to_string(amount);
    int r = 0, k = 0;
    unsigned mask = 0;
    size_t want_aux = 0;
    switch (kind) {
    case RCU_CORRUPT_GAUSSIAN_NOISE:
        if (amount < 0.0) return invalid("gaussian_noise: amount must be >= 0" + got);
        if (channels > MAX_CLASSES) return invalid("gaussian_noise: channels must be <= 8 (the normals are those of the logit sampling), got " + std::to_string(channels));
        break;
    case RCU_CORRUPT_GAUSSIAN_BLUR:
        if (!(amount > 0.0 && amount <= 8.0)) return invalid("gaussian_blur: amount (sigma) must be in (0, 8]" + got);
        r = blur_radius(amount);
        if (r >= (height < width ? height : width))
            return invalid("gaussian_blur: the radius int(4 sigma + 0.5) = " + std::to_string(r) + " must be below min(height, width)");
        want_aux = (size_t)(2 * r + 1);
        break;
    case RCU_CORRUPT_DOWNSAMPLE:
        if (!(amount >= 2.0 && amount < 17.0)) return invalid("downsample: the factor (int)amount must be in 2..16" + got);
        k = (int)amount;
        break;
    case RCU_CORRUPT_CONTRAST:
        if (!(amount >= 0.0 && amount <= 4.0)) return invalid("contrast: amount must be in [0, 4]" + got);
        break;
    case RCU_CORRUPT_INTENSITY_SHIFT:
        break;
    case RCU_CORRUPT_BIAS_FIELD:
        if (!(amount >= 0.0 && amount <= 2.0)) return invalid("bias_field: amount must be in [0, 2]" + got);
        want_aux = bias_aux_floats(channels, height, width);
        break;
    case RCU_CORRUPT_GHOSTING:
        if (!(amount >= 0.0 && amount <= 1.0)) return invalid("ghosting: amount must be in [0, 1]" + got);
        break;
    default:   // RCU_CORRUPT_CHANNEL_DROP
        if (channels < 2 || channels > 30) return invalid("channel_drop: channels must be in 2..30, got " + std::to_string(channels));
        if (amount != std::floor(amount) || amount < 1.0 || amount > (double)((1u << channels) - 2u))
            return invalid("channel_drop: amount is the channel mask, an integer in 1..2^channels - 2 (some channel dropped, some kept)" + got);
        mask = (unsigned)amount;
        break;
    }
    if (want_aux) {
        if (!aux_host || n_aux < 0 || (size_t)n_aux != want_aux)
            return invalid("aux_host must hold " + std::to_string(want_aux) + " floats for this kind and shape, got " +
                           (aux_host ? std::to_string(n_aux) : std::string("null")));
        for (size_t e = 0; e < want_aux; ++e)
            if (!std::isfinite(aux_host[e])) return invalid("aux_host[" + std::to_string(e) + "] is not finite");
    } else if (n_aux != 0) {
        return invalid("n_aux must be 0 for this kind (it takes no aux_host), got " + std::to_string(n_aux));
    }
    const size_t planes = n * (size_t)channels;
    if (overlap(x_dev, out_dev, planes * (size_t)height * width * sizeof(float))) return invalid("out must not overlap x (out == x is not supported)");
    if (rcu_corrupt_workspace_bytes(n, channels, height, width, kind) && !workspace_dev) return invalid("null workspace_dev (rcu_corrupt_workspace_bytes)");

    const hipStream_t s = static_cast<hipStream_t>(stream);
    PointArgs q{};
    q.x = x_dev, q.out = out_dev, q.planes = planes, q.C = channels, q.H = height, q.W = width, q.a = (float)amount, q.mask = mask;
    hipError_t e = hipSuccess;
    switch (kind) {
    case RCU_CORRUPT_GAUSSIAN_NOISE:
        e = launch_noise(x_dev, out_dev, n, channels, height, width, (float)amount, key, first_sample, s);
        break;
    case RCU_CORRUPT_GAUSSIAN_BLUR: {
        BlurTaps taps{};
        for (int t = 0; t < 2 * r + 1; ++t) taps.w[t] = aux_host[t];
        const dim3 grid((unsigned)((width + BLUR_TW - 1) / BLUR_TW), (unsigned)((height + BLUR_TH - 1) / BLUR_TH), plane_blocks(planes));
        e = set_max_dynamic_lds(reinterpret_cast<const void*>(corrupt_blur_kernel), (int)blur_lds_bytes(BLUR_MAX_RADIUS));      // 64 KB + the taps at r = 32
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(corrupt_blur_kernel, grid, dim3(CR_THREADS), blur_lds_bytes(r), s, x_dev, out_dev, planes, height, width, r, taps);
        e = hipGetLastError();
        break;
    }
    case RCU_CORRUPT_DOWNSAMPLE: {
        const unsigned blocks = (unsigned)((height + k - 1) / k) * (unsigned)((width + k - 1) / k);
        hipLaunchKernelGGL(corrupt_downsample_kernel, dim3((blocks + CR_THREADS - 1) / CR_THREADS, plane_blocks(planes)), dim3(CR_THREADS), 0, s, x_dev,
                           out_dev, planes, height, width, k);
        e = hipGetLastError();
        break;
    }
    case RCU_CORRUPT_CONTRAST: {
        const unsigned hw = (unsigned)height * (unsigned)width;
        const int vec_ok = hw % 4 == 0 && reinterpret_cast<uintptr_t>(x_dev) % 16 == 0;
        hipLaunchKernelGGL(corrupt_mean_kernel, dim3(plane_blocks(planes)), dim3(MEAN_THREADS), 0, s, x_dev, planes, hw, vec_ok,
                           static_cast<double*>(workspace_dev));
        e = hipGetLastError();
        if (e != hipSuccess) break;
        q.mean = static_cast<const double*>(workspace_dev);
        e = launch_point<RCU_CORRUPT_CONTRAST>(q, s);
        break;
    }
    case RCU_CORRUPT_INTENSITY_SHIFT:
        e = launch_point<RCU_CORRUPT_INTENSITY_SHIFT>(q, s);
        break;
    case RCU_CORRUPT_BIAS_FIELD: {
        float* coef = static_cast<float*>(workspace_dev);
        if ((e = fill_aux(aux_host, want_aux, coef, s)) != hipSuccess) break;
        q.coef = coef, q.A = coef + (size_t)BIAS_TERMS * channels, q.B = q.A + 3 * (size_t)height;
        e = launch_point<RCU_CORRUPT_BIAS_FIELD>(q, s);
        break;
    }
    case RCU_CORRUPT_GHOSTING:
        e = launch_point<RCU_CORRUPT_GHOSTING>(q, s);
        break;
    default:
        e = launch_point<RCU_CORRUPT_CHANNEL_DROP>(q, s);
        break;
    }
    if (e != hipSuccess) return report_error(RCU_ERR_HIP, std::string("rcu_corrupt: ") + hipGetErrorString(e));
    return RCU_OK;
}
