// UpConv's "nearest x2 -> conv3x3 (+bias)" (common/model/unet.py:105) in Winograd F(4x4, 3x3) form on the UP-SAMPLED grid, without the
// interpolation point the up-sampling makes vanish: 25 multiplications per 16 output pixels and (cin, cout) pair, against 36 in the
// sub-pixel F(2x2,2x2) form (rcu_wino_up.hip) and in a plain F(4x4,3x3).
//
// Put the 4x4 output tiles at multiples of 4 of the up-sampled image.  A tile's 6x6 input patch covers up-sampled rows -1 .. 4 = low-resolution
// rows -1, 0, 0, 1, 1, 2: in each direction the patch is (a, b, b, c, c, d).  Lavin & Gray's B^T (points 0, +-1, +-2, inf: rcu_wino4.hip) maps it to
//     row 0:  4a - 5b + c      row 1: -8b + 2c      row 2: 0      row 3: -3 (b - c)      row 4: b - c      row 5: 4b - 5c + d
// (row 2 -- the point -1 -- vanishes identically: up2(z)(t) = z(t^2)(1 + t)).  5 x 5 = 25 positions remain; rows 3 and 4 carry the same data up
// to the factor -3, which the host folds into the packed weights, so 4 x 4 = 16 transformed values per (tile, channel) -- made from the RAW 4x4
// low-resolution patch -- feed the 25 positions.  Weights: G g G^T without row and column 2 (rcu_wpack.h); output transform: A^T M A without
// column 2.  Zero padding of the up-sampled image is zero padding of the low-resolution image under this row map: the buffer resource's
// out-of-range zeros do all of it.
//
// Everything else is rcu_wino4.hip's design: one wave per SIMD (a wave owns 16 tiles x 32 couts x 25 positions = 200 accumulator registers, kept
// in the accumulator file by inline assembly), a workgroup of 4 waves per CU, persistent grid in XCD-aware order, staging by LDS-DMA only with
// the swizzle on the source side, a double-buffered Cin-chunk pipeline running across the tiles of a workgroup, 16-byte stores (paired tensors: without the lane trade).  What differs:
//   * the LDS input image is the LOW-resolution tile + a 1-pixel halo (18x18 positions for a 32x32 output tile), [slice][halo row][position]
//     [8 channels], position = x ^ (((x >> 3) ^ slice) & 1): tiles are 2 positions = 16 dwords apart, so the 16 tiles x 2 channel pairs a
//     ds_read_b64 serves per cycle fall two by two on the 32 two-dword slots of the 64 banks, as in rcu_wino4.hip;
//   * a lane reads 16 ds_read_b64 per chunk (36 there) and the transform is 56 packed operations (144 there);
//   * the epilogue adds the bias and stores: an UpConv has no dropout, BatchNorm, ReLU or pool; K is single-source.
// The tile grid walks the low-resolution level (ConvArgs::H x W), the geometry names are those of the OUTPUT tile.
#include "rcu_wino_common.h"
#include "rcu_wino4_geom.h"

namespace rcu {

// The workgroup tiles (Up4Tile), the LDS image and the slot / fragment geometry of both source layouts: rcu_wino4_geom.h.

// 200 accumulator registers per lane: 50 tuples of 4 in the accumulator file a[0:199], owned by the inline assembly below as in rcu_wino4.hip (see
// there for the why, the s_nop 1 that opens every MFMA and the audit: tests/test_upconv4_cpu.py).
#define UP4_ALL_AGPRS \
    "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", \
    "a16", "a17", "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", \
    "a32", "a33", "a34", "a35", "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", \
    "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", \
    "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73", "a74", "a75", "a76", "a77", "a78", "a79", \
    "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", "a91", "a92", "a93", "a94", "a95", \
    "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106", "a107", "a108", "a109", "a110", "a111", \
    "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124", "a125", "a126", "a127", \
    "a128", "a129", "a130", "a131", "a132", "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140", "a141", "a142", "a143", \
    "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156", "a157", "a158", "a159", \
    "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175", \
    "a176", "a177", "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191", \
    "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199"
// first AGPR of the accumulator tuple of (cout block b, packed position p)
__host__ __device__ constexpr int up4_areg(int b, int p) { return 4 * (25 * b + p); }

template <int B, int P, bool ZERO>
__device__ __forceinline__ void up4_mfma(float av, float wv)
{
    constexpr int R = up4_areg(B, P);
    if constexpr (ZERO)
        asm volatile("s_nop 1\n\tv_mfma_f32_16x16x4_f32 a[%c2:%c3], %0, %1, 0" ::"v"(av), "v"(wv), "i"(R), "i"(R + 3) : UP4_ALL_AGPRS);
    else
        asm volatile("s_nop 1\n\tv_mfma_f32_16x16x4_f32 a[%c2:%c3], %0, %1, a[%c2:%c3]" ::"v"(av), "v"(wv), "i"(R), "i"(R + 3) : UP4_ALL_AGPRS);
}

// element r of the accumulator tuple of (b, p)
template <int B, int P, int R>
__device__ __forceinline__ float up4_acc()
{
    float v;
    asm volatile("v_accvgpr_read_b32 %0, a%c1" : "=v"(v) : "i"(up4_areg(B, P) + R));
    return v;
}

// The 5 surviving positions of a direction, k = 0..4, are the F(4x4,3x3) rows 0, 1, 3, 4, 5; they read the transformed value 0, 1, 2, 2, 3 (rows 3 and
// 4 share one).  Packed position p = 5 ki + kj.  Position rows are multiplied in the order 0, 5, 1, 3, 4 (k = 0, 4, 1, 2, 3), so that only the values
// of row 0 precede the first MFMA.
__host__ __device__ constexpr int up4_val_of(int k) { return k < 3 ? k : k - 1; }
__host__ __device__ constexpr int up4_krow_of(int o) { return o == 0 ? 0 : o == 1 ? 4 : o - 1; }
__host__ __device__ constexpr int up4_pos_of(int q) { return 5 * up4_krow_of(q / 5) + q % 5; }          // packed position multiplied in slot q
__host__ __device__ constexpr int up4_v_of(int q) { return 4 * up4_val_of(up4_krow_of(q / 5)) + up4_val_of(q % 5); }   // its transformed value

// Output transform A^T M A without the dead row and column + bias of tile R of the lane's four: y[row][col], components = the lane's two couts.
template <int R>
__device__ __forceinline__ void up4_output_tile(const f32x2 bias, f32x2 (&y)[4][4])
{
    f32x2 nn[5][4];   // N[k][q] = sum_j M[k][j] A[j][q]
    wino_static_for<0, 5>([&](auto k_c) {
        constexpr int k = decltype(k_c)::value;
        auto m = [&](auto j_c) {
            constexpr int j = decltype(j_c)::value;
            return f32x2{up4_acc<0, 5 * k + j, R>(), up4_acc<1, 5 * k + j, R>()};
        };
        const f32x2 m0 = m(std::integral_constant<int, 0>{}), m1 = m(std::integral_constant<int, 1>{}), m3 = m(std::integral_constant<int, 2>{}),
                    m4 = m(std::integral_constant<int, 3>{}), m5 = m(std::integral_constant<int, 4>{});
        const f32x2 s3 = m3 + m4, s4 = m3 - m4;
        nn[k][0] = (m0 + m1) + s3;
        nn[k][1] = m1 + 2.f * s4;
        nn[k][2] = m1 + 4.f * s3;
        nn[k][3] = (m1 + 8.f * s4) + m5;
    });
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x2 s3 = nn[2][q] + nn[3][q], s4 = nn[2][q] - nn[3][q];
        y[0][q] = ((nn[0][q] + nn[1][q]) + s3) + bias;
        y[1][q] = (nn[1][q] + 2.f * s4) + bias;
        y[2][q] = (nn[1][q] + 4.f * s3) + bias;
        y[3][q] = ((nn[1][q] + 8.f * s4) + nn[4][q]) + bias;
    }
}

// Output transform + bias + stores of one finished tile; (y0, x0): the work item's origin on the OUTPUT grid.  `plan`: the lane's part of the store
// offset (slice, pixel and cout pair of its first tile relative to the workgroup tile's origin and cout tile), made once per kernel.
// PAIRED: `out` is a paired tensor (rcu_wino4_geom.h) -- a lane stores two adjacent pixels x its two couts as they are, no lane trade.
template <class T, bool PAIRED>
__device__ __forceinline__ void up4_epilogue(const ConvArgs& a, const f32x2 bias, int ntile, int n0, int y0, int x0, int lane, uint32_t plan)
{
    // every MFMA has long retired: the last chunk's barrier lies between them and this point; the nops cover the asm-to-asm case
    // (an MFMA's D read by v_accvgpr_read) the compiler cannot see
    asm volatile("s_nop 15\n\ts_nop 7");
    [[maybe_unused]] const int odd = lane & 1;
    const int oH = 2 * a.H, oW = 2 * a.W, CoutP = a.CoutP, N = a.N;   // one batch of scalar loads
    const uint32_t px_bytes = a.out_pix_bytes, chunk_bytes = a.out_chunk_bytes;
    float* const out = a.out;
    const uint32_t row_bytes = (uint32_t)oW * px_bytes;
    // lanes of slices beyond the batch need no flag: their offsets lie behind the tensor, where the buffer resource drops the write
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(out, 0, (uint32_t)(N * oH * oW) * (uint32_t)CoutP * 4u, 0x00020000);
    const uint32_t vo = plan + wino_out_offset(n0, oH * oW, CoutP, (uint32_t)(y0 * oW + x0), ntile * T::BN, px_bytes, chunk_bytes);
    wino_static_for<0, 4>([&](auto r_c) {
        constexpr int r = decltype(r_c)::value;   // tile r of the lane's four sits r tile columns right of its first
        f32x2 y[4][4];                            // [row][col], components = the two couts
        up4_output_tile<r>(bias, y);
        // Neighbouring lanes (couts 2n, 2n+1 | 2n+2, 2n+3 of the same pixels) trade pixel columns: the even lane ends up with four
        // couts of columns 0 and 2 of the tile, the odd lane with four couts of columns 1 and 3 -> 16-byte stores.
#pragma unroll
        for (int aa = 0; aa < 4; ++aa) {
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                if constexpr (PAIRED) {
                    const f32x4 o = {y[aa][2 * h2].x, y[aa][2 * h2].y, y[aa][2 * h2 + 1].x, y[aa][2 * h2 + 1].y};
                    wino_store16(o, ro, vo, (uint32_t)(4 * r + 2 * h2) * px_bytes + (uint32_t)aa * row_bytes);
                    continue;
                }
                const f32x2 keep = odd ? y[aa][2 * h2 + 1] : y[aa][2 * h2];
                const f32x2 send = odd ? y[aa][2 * h2] : y[aa][2 * h2 + 1];
                f32x2 recv;
                recv.x = wino_swap_adjacent(send.x);
                recv.y = wino_swap_adjacent(send.y);
                const f32x4 o = odd ? f32x4{recv.x, recv.y, keep.x, keep.y} : f32x4{keep.x, keep.y, recv.x, recv.y};
                wino_store16(o, ro, vo, (uint32_t)(4 * r + 2 * h2) * px_bytes + (uint32_t)aa * row_bytes);
            }
        }
    });
}

// PAIRED: the output tensor is paired (up4_epilogue); whether the source is paired is a run-time flag (ConvArgs::in_paired), as in rcu_wino4.hip.
// The kernels: up_wino4_stream<T> writes a blocked / channels-last tensor, up_wino4_pairs<T> a paired one (one body).
template <class T, bool PAIRED>
__device__ __forceinline__ void up_wino4_body(const ConvArgs& a, const int total_items)
{
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(1024))) float smem[];
    constexpr int KC = T::KC;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m16 = lane & 15, kq = lane >> 4;
    const int nchunks = a.C1 / KC;   // even, >= 4 (checked by the launcher); single source
    const uint32_t wchunk_bytes = (uint32_t)a.NT * T::W_DW * 4u;
    const uint32_t in_chunk_bytes = a.in_chunk_bytes;

    const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.src1), 0, a.src1_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wpack), 0, a.wpack_bytes, 0x00020000);

    // fragment addresses (dword offsets inside a buffer) of the lane's patch columns j = 0..3 in patch row 0; the row is an immediate offset.
    // Output tile (row oy, column ox) reads low-resolution rows oy / 2 - 1 .. oy / 2 + 2 = halo rows oy / 2 .. oy / 2 + 3, and columns alike.
    const bool in_paired = a.in_paired != 0;
    int aCol[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) aCol[j] = up4_patch_col<T>(in_paired, wave, m16, kq, j);
    const int b_addr = T::A_DW + (kq * T::BN + 2 * m16) * 2;
    const uint32_t w_voff = (uint32_t)(lane * 16);

    int item = wino_xcd_virtual_block(a.NT < 4 ? 4 : a.NT);
    bool has_next = item + (int)gridDim.x < total_items;
    WinoTileId tile = wino_tile_id<T>(a, item), ntile = tile;
    uint32_t dp[T::NA], geo[T::NA];
    int dp_wtile = tile.wtile;
#pragma unroll
    for (int j = 0; j < T::NA; ++j) {
        // the slot's plan: tile-independent offset | border flags
        geo[j] = in_paired ? wino4_slot_plan_paired<T>(a.H, a.W, a.C1, wino4_slot_geometry_paired<T>(j, wave, lane))
                           : wino_slot_plan<T>(a, up4_slot_geometry<T>(j, wave, lane));
        asm volatile("" : "+v"(geo[j]));
        dp[j] = wino_slot_offset(geo[j], wino_tile_offset<T>(a, tile));
    }

    // the lane's part of the store offsets: slice, output pixel and cout pair of its first tile relative to the workgroup tile's origin and cout tile
    uint32_t store_plan;
    {
        int bs, by, sb, tr, tc;
        T::block_origin(wave, bs, by);
        T::tile_of(4 * (lane >> 4), sb, tr, tc);
        // the even lane stores four couts of one pixel column, the odd lane of the next; PAIRED: every lane its own cout pair kq = n & 3 of pixel pairs
        // (unit kq of the pair's 64 bytes: 16 kq bytes into it where wino_out_offset counts 8 kq)
        const int n16 = lane & 15, odd = PAIRED ? 0 : n16 & 1, c = 2 * n16 - 2 * odd;
        const int oH = 2 * a.H, oW = 2 * a.W;
        store_plan = wino_out_offset(bs + sb, oH * oW, a.CoutP, (uint32_t)((by + 4 * tr) * oW + 4 * tc + odd), c, a.out_pix_bytes, a.out_chunk_bytes);
        if constexpr (PAIRED) store_plan += (uint32_t)(n16 & 3) * 8u;
        asm volatile("" : "+v"(store_plan));
    }

    // LDS-DMA of Cin chunk kc of a tile into LDS buffer `buf`: the wave's NA input pieces and NW weight pieces of 1 KB.  No branch per piece: a job
    // without work (behind the workgroup's last chunk) points out of range, where the buffer load writes zeros into a buffer nobody reads.
    struct DmaJob {
        uint32_t cb, wso, lb;
    };
    auto dma_job = [&](int wtile, int kc, int buf, bool active) {
        DmaJob j;
        j.cb = active ? wino_chunk_offset(in_chunk_bytes, kc * KC) : WINO_OOB;
        j.wso = active ? (uint32_t)kc * wchunk_bytes + (uint32_t)wtile * (T::W_DW * 4u) : WINO_OOB;
        j.lb = (uint32_t)buf * (T::BUF_DW * 4u);
        return j;
    };
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lds_ptr_t)smem;
    auto dma_piece = [&](const DmaJob& job, auto i_c) {
        constexpr int I = decltype(i_c)::value;
        // the input pieces first: they come from HBM (or another XCD's writes), the weight pieces are L2 hits shared by every workgroup of the cout tile
        if constexpr (I < T::NA) {
            constexpr int j = I;
            if ((j + 1) * T::WAVES <= T::A_PIECES || j * T::WAVES + wave < T::A_PIECES)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, (lds_ptr_t)(uintptr_t)(lds_base + job.lb + (j * T::WAVES + wave) * 1024), 16, dp[j], job.cb, 0, 0);
        } else if constexpr (I < T::NW + T::NA) {
            constexpr int k = I - T::NA;
            if ((k + 1) * T::WAVES <= T::W_PIECES || k * T::WAVES + wave < T::W_PIECES)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr_t)(uintptr_t)(lds_base + job.lb + T::A_DW * 4 + (k * T::WAVES + wave) * 1024), 16,
                                                         w_voff, job.wso + (uint32_t)(k * T::WAVES + wave) * 1024u, 0, 0);
        }
    };

    {
        const DmaJob job = dma_job(dp_wtile, 0, 0, true);
        wino_static_for<0, T::NW + T::NA>([&](auto i_c) { dma_piece(job, i_c); });
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    __syncthreads();

    f32x2 bias = {0.f, 0.f};

    // Pipeline of one Cin chunk out of LDS buffer BUF, 25 positions x 2 channel steps x 2 cout blocks = 100 MFMAs (rcu_wino4.hip's rules):
    //   groups 0..8 of 8 MFMAs (two positions), the weight reads of the positions AHEAD slots on and the next chunk's LDS-DMA pieces between the
    //     MFMAs, the transform of the coming position rows as one packed clump per group;
    //   s_waitcnt vmcnt(0) + barrier: the next chunk (of this tile or of the workgroup's next tile) has landed in the other buffer;
    //   groups 9..12 (the last one a single position) -- their weights were read before the barrier -- with the RAW patch of the next chunk and
    //     its first weights read between their MFMAs.
    constexpr int AHEAD = 4, NPRE = 9, NGROUPS = 13;
    static_assert(T::NA + T::NW <= 2 * NPRE, "one LDS-DMA piece per half group before the barrier");
    auto load_patch_row = [&](f32x2 (&d)[16], const float* Ab, int i) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            // volatile: keeps hipcc from fusing pairs of these reads into ds_read2_b64
            d[4 * i + j] = *(const volatile __attribute__((address_space(3))) f32x2*)(Ab + aCol[j] + i * (T::PITCH * 8));
    };
    auto load_weights = [&](f32x4 (&bv)[25], const float* Ab, int p) { bv[p] = *reinterpret_cast<const f32x4*>(Ab + b_addr + p * (8 * T::BN)); };
    // The reduced one-dimensional transform of (a, b, c, d), value v = 0..3, on channel pairs (packed operations)
    auto value = [](int v, const f32x2 xa, const f32x2 xb, const f32x2 xc, const f32x2 xd) -> f32x2 {
        if (v == 0) return 4.f * xa + (xc - 5.f * xb);
        if (v == 1) return 2.f * xc - 8.f * xb;
        if (v == 2) return xb - xc;
        return 4.f * xb + (xd - 5.f * xc);
    };
    // V[4 v + 0..3] := value v over the patch rows, then the four values over its columns
    auto transform_rows = [&](const f32x2 (&d)[16], f32x2 (&V)[16], int v) {
        f32x2 t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = value(v, d[j], d[4 + j], d[8 + j], d[12 + j]);
#pragma unroll
        for (int w = 0; w < 4; ++w) V[4 * v + w] = value(w, t[0], t[1], t[2], t[3]);
    };

    auto chunk = [&](auto buf_c, auto first_c, int kc, f32x2 (&d)[16], f32x2 (&dn)[16], f32x4 (&bv)[25], f32x4 (&bvn)[25]) {
        constexpr int BUF = decltype(buf_c)::value;
        constexpr bool FIRST = decltype(first_c)::value;
        const float* const Ab = smem + BUF * T::BUF_DW;
        const float* const An = smem + (BUF ^ 1) * T::BUF_DW;
        const bool more = kc + 1 < nchunks;
        if (!more && has_next) {   // last chunk of the tile: from here on the DMA works on the workgroup's next tile
            const WinoTileConsts ca = wino_tile_consts(wino_cold_args());   // one batch of scalar loads, one wait
            ntile = wino_tile_id<T>(ca, item + (int)gridDim.x);
            dp_wtile = ntile.wtile;
            const WinoTileOffset nto = wino_tile_offset<T>(ca, ntile);
#pragma unroll
            for (int j = 0; j < T::NA; ++j) dp[j] = wino_slot_offset(geo[j], nto);
        }
        // the bias: loaded a chunk early, so that the epilogue does not wait for memory
        if (kc == nchunks - 2) {
            const ConvArgs& ca = wino_cold_args();
            const int co = tile.wtile * T::BN + 2 * (lane & 15);   // < NT * BN, the length of betab / beta
            bias = *reinterpret_cast<const f32x2*>(ca.betab + co) + *reinterpret_cast<const f32x2*>(ca.beta + co);
        }
        const DmaJob job = dma_job(dp_wtile, more ? kc + 1 : 0, BUF ^ 1, more || has_next);
        f32x2 V[16];
        transform_rows(d, V, 0);
        wino_static_for<0, NGROUPS>([&](auto g_c) {
            constexpr int G = decltype(g_c)::value;
            constexpr bool PAIR = 2 * G + 1 < T::NPOS;
            constexpr int p0 = up4_pos_of(2 * G), p1 = up4_pos_of(PAIR ? 2 * G + 1 : 2 * G);
            constexpr int v0 = up4_v_of(2 * G), v1 = up4_v_of(PAIR ? 2 * G + 1 : 2 * G);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (G == NPRE) {
                // vmcnt(0): this wave's pieces of the next chunk (the next tile's first chunk behind a tile's last) have landed.  __syncthreads()
                // lowers to s_waitcnt vmcnt(0) lgkmcnt(0); s_barrier: every LDS read any wave has issued from buffer BUF's weights is complete, and
                // nobody reads the other buffer before the barrier -- the next chunk's DMA may overwrite BUF from its first group on.
                __builtin_amdgcn_s_waitcnt(0x0F70);
                __syncthreads();
                __builtin_amdgcn_sched_barrier(0);
            }
            // what goes between the MFMAs of the group: unit u follows MFMA u
            auto filler = [&](auto u_c) {
                constexpr int U = decltype(u_c)::value;
                if constexpr (G < NPRE) {
                    // weights of the positions AHEAD slots on; in the last groups before the barrier also those of groups 9..12
                    if constexpr (U == 0 || U == 4) {
                        constexpr int q = 2 * G + AHEAD + (U == 4 ? 1 : 0);
                        if constexpr (q < 2 * NPRE) load_weights(bv, Ab, up4_pos_of(q));
                    }
                    if constexpr (G >= NPRE - 4 && (U == 2 || U == 6)) {
                        constexpr int q = 2 * NPRE + 2 * (G - (NPRE - 4)) + (U == 6 ? 1 : 0);
                        if constexpr (q < T::NPOS) load_weights(bv, Ab, up4_pos_of(q));
                    }
                    if constexpr (U == 1 || U == 5) dma_piece(job, std::integral_constant<int, 2 * G + (U == 5 ? 1 : 0)>{});
                } else {
                    // behind the barrier: the raw patch of the next chunk and its first weights.  Unconditional (a conditional load would keep
                    // the old contents of dn alive through the whole chunk); in a tile's last chunk the values are dropped and the next tile's first
                    // chunk is read again behind the epilogue (load_first)
                    constexpr int slot = 8 * (G - NPRE) + U;   // 0..27
                    if constexpr (slot % 4 == 0 && slot < 16) load_patch_row(dn, An, slot / 4);
                    if constexpr (slot == 16)
                        wino_static_for<0, AHEAD>([&](auto q_c) { load_weights(bvn, An, up4_pos_of(decltype(q_c)::value)); });
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            up4_mfma<0, p0, FIRST>(V[v0].x, bv[p0].x);
            filler(std::integral_constant<int, 0>{});
            up4_mfma<1, p0, FIRST>(V[v0].x, bv[p0].z);
            filler(std::integral_constant<int, 1>{});
            if constexpr (PAIR) {
                up4_mfma<0, p1, FIRST>(V[v1].x, bv[p1].x);
                filler(std::integral_constant<int, 2>{});
                up4_mfma<1, p1, FIRST>(V[v1].x, bv[p1].z);
                filler(std::integral_constant<int, 3>{});
            }
            up4_mfma<0, p0, false>(V[v0].y, bv[p0].y);
            filler(std::integral_constant<int, 4>{});
            up4_mfma<1, p0, false>(V[v0].y, bv[p0].w);
            filler(std::integral_constant<int, 5>{});
            if constexpr (PAIR) {
                up4_mfma<0, p1, false>(V[v1].y, bv[p1].y);
                filler(std::integral_constant<int, 6>{});
                up4_mfma<1, p1, false>(V[v1].y, bv[p1].w);
                filler(std::integral_constant<int, 7>{});
            }
            // transform work for the coming position rows (multiplied in the order 0, 5, 1, 3 | 4: values 0, 3, 1, 2), one clump per group: value 3
            // is multiplied from slot 5 (group 2) on, value 1 from slot 10 (group 5), value 2 from slot 15 (group 7)
            if constexpr (G == 0) transform_rows(d, V, 3);
            if constexpr (G == 2) transform_rows(d, V, 1);
            if constexpr (G == 4) transform_rows(d, V, 2);
        });
    };

    f32x2 dA[16], dB[16];
    f32x4 bvA[25], bvB[25];
    // a tile's first chunk: nothing to hide the LDS round trip behind
    auto load_first = [&]() {
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) load_patch_row(dA, smem, ii);
        wino_static_for<0, AHEAD>([&](auto q_c) { load_weights(bvA, smem, up4_pos_of(decltype(q_c)::value)); });
    };
    load_first();

    for (;;) {
        chunk(std::integral_constant<int, 0>{}, std::true_type{}, 0, dA, dB, bvA, bvB);
        chunk(std::integral_constant<int, 1>{}, std::false_type{}, 1, dB, dA, bvB, bvA);
        for (int kc = 2; kc < nchunks; kc += 2) {
            chunk(std::integral_constant<int, 0>{}, std::false_type{}, kc, dA, dB, bvA, bvB);
            chunk(std::integral_constant<int, 1>{}, std::false_type{}, kc + 1, dB, dA, bvB, bvA);
        }
        up4_epilogue<T, PAIRED>(wino_cold_args(), bias, tile.wtile, tile.n0, 2 * tile.y0, 2 * tile.x0, lane, store_plan);
        if (!has_next) break;
        load_first();   // (no wait and no barrier here: the tile's last chunk waited for the next tile's first chunk at its barrier)
        item += (int)gridDim.x;
        tile = ntile;
        has_next = item + (int)gridDim.x < total_items;
    }
#endif
}

template <class T>
__global__ __launch_bounds__(256, 1) void up_wino4_stream(const ConvArgs a, const int total_items)
{
    up_wino4_body<T, false>(a, total_items);
}

template <class T>
__global__ __launch_bounds__(256, 1) void up_wino4_pairs(const ConvArgs a, const int total_items)
{
    up_wino4_body<T, true>(a, total_items);
}

using U4Cfg0 = Up4Tile<1, 2, 8, 1, 4>;   // 32x32 output pixels of one slice (16x16 low-resolution)
using U4Cfg1 = Up4Tile<1, 2, 8, 2, 2>;   // 16x32 output pixels of two consecutive slices (output heights not divisible by 32)
using U4Cfg2 = Up4Tile<2, 2, 4, 4, 1>;   // 8x16 output pixels of eight consecutive slices (the 24x16 level)

// TH x TW: the low-resolution tile, as the sub-pixel kernels report it (the tile grid walks the low-resolution level)
// id, winograd, reads_blocked, writes_blocked, part, weight_sets, mults: both layouts, but whole tiles of unpadded levels only (no ConvArgs::part
// form); 25 multiplications per 4x4 output tile = 2x2 low-resolution pixels
static constexpr ConvFamilyTraits kWino4Up = {ConvFamily::Wino4Up, true, true, true, false, 1, 6.25, true, true};

static const ConvConfigInfo kWino4UpInfo[3] = {
    {U4Cfg0::TS, U4Cfg0::TH, U4Cfg0::TW, U4Cfg0::BN, 8, 25, "upconv_winograd4<T32x32,N32,K8>", 8, 0, kWino4Up},
    {U4Cfg1::TS, U4Cfg1::TH, U4Cfg1::TW, U4Cfg1::BN, 8, 25, "upconv_winograd4<S2T16x32,N32,K8>", 8, 0, kWino4Up},
    {U4Cfg2::TS, U4Cfg2::TH, U4Cfg2::TW, U4Cfg2::BN, 8, 25, "upconv_winograd4<S8T8x16,N32,K8>", 8, 0, kWino4Up},
};

const ConvConfigInfo& wino4_up_config_info(int cfg) { return kWino4UpInfo[cfg - CONV_CFG_UPW4_T32x32_N32]; }

template <class T, bool PAIRED>
static hipError_t launch_wino4_up_kernel(const ConvArgs& a, hipStream_t stream)
{
    const void* kernel;
    if constexpr (PAIRED)
        kernel = reinterpret_cast<const void*>(&up_wino4_pairs<T>);
    else
        kernel = reinterpret_cast<const void*>(&up_wino4_stream<T>);
    hipError_t e = set_max_dynamic_lds(kernel, T::LDS_BYTES);
    if (e != hipSuccess) return e;
    const unsigned items = (unsigned)a.NT * a.tiles_x * a.tiles_y * a.slice_groups;
    const unsigned grid = wino_persistent_grid(items);
    if constexpr (PAIRED)
        hipLaunchKernelGGL((up_wino4_pairs<T>), dim3(grid), dim3(T::THREADS), T::LDS_BYTES, stream, a, (int)items);
    else
        hipLaunchKernelGGL((up_wino4_stream<T>), dim3(grid), dim3(T::THREADS), T::LDS_BYTES, stream, a, (int)items);
    return hipGetLastError();
}

template <class T>
static hipError_t launch_wino4_up_cfg(const ConvArgs& a, hipStream_t stream)
{
    const int nchunks = a.C1 / T::KC;
    // whole tiles of an unpadded level, bias only, one source; every byte offset a lane can form -- TS slices beyond the batch included -- stays
    // below 2^32, and the tensors below 2^31 (out-of-range markers)
    const size_t in_slice = (size_t)a.H * a.W * a.C1 * 4, out_slice = (size_t)a.H * a.W * a.CoutP * 16;
    if (nchunks < 4 || (nchunks & 1) != 0 || a.C1 % T::KC != 0 || a.C2 != 0 || a.src2 != nullptr || a.NTW_total != a.NT || a.CoutP != a.NT * T::BN ||
        a.src1_bytes == 0 || a.wpack_bytes == 0 || a.part || a.out_H != 0 || a.out_W != 0 || a.mask != nullptr || a.mask2 != nullptr || a.relu ||
        a.pooled != nullptr || a.accumulate || a.H % T::TH != 0 || a.W % T::TW != 0 || a.N < 1 || (size_t)a.N * in_slice >= ((size_t)1 << 31) ||
        (size_t)a.N * out_slice >= ((size_t)1 << 31) || (size_t)(a.N + T::TS) * in_slice >= ((size_t)1 << 32) ||
        (size_t)(a.N + T::TS) * out_slice >= ((size_t)1 << 32))
        return hipErrorInvalidValue;
    // paired tensors: even widths, the chunk stride of the blocked layout
    if (a.in_paired && ((a.W & 1) != 0 || a.in_pix_bytes != 32u || a.in_chunk_bytes != (uint32_t)(a.H * a.W) * 32u)) return hipErrorInvalidValue;
    if (a.out_paired && a.out_pix_bytes != 32u) return hipErrorInvalidValue;
    return a.out_paired ? launch_wino4_up_kernel<T, true>(a, stream) : launch_wino4_up_kernel<T, false>(a, stream);
}

hipError_t launch_upconv_wino4(int cfg, const ConvArgs& a, hipStream_t stream)
{
    switch (cfg) {
        case CONV_CFG_UPW4_T32x32_N32: return launch_wino4_up_cfg<U4Cfg0>(a, stream);
        case CONV_CFG_UPW4_S2T16x32_N32: return launch_wino4_up_cfg<U4Cfg1>(a, stream);
        case CONV_CFG_UPW4_S8T8x16_N32: return launch_wino4_up_cfg<U4Cfg2>(a, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rcu
