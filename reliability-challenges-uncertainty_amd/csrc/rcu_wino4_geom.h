// Tile geometry of the F(4x4,3x3) kernels (rcu_wino4.hip, rcu_wino4_up.hip): the workgroup tiles, the LDS image of a Cin chunk, which 16 bytes of
// the source tensor every LDS-DMA slot fetches and where a lane reads its patch -- for the channel-blocked layout and for the pixel-pair ("paired")
// layout of the same tensors.  Plain integer arithmetic, so that host code can include it: tests/test_paired_layout_cpu.py walks every tile type
// with it (every staged unit fetched once, the bank model of the patch reads, reads == what the slot plan put there).
//
// Paired layout [N][C/8][H][W/2][4 channel pairs][2 pixels][2 channels]: the channel-blocked layout with the 64 bytes of each aligned pixel pair
// (2 pixels x 8 channels) permuted --
//     byte offset inside a chunk plane = ((y W + x) >> 1) * 64 + kq * 16 + (x & 1) * 8 + (c & 1) * 4,   kq = (c & 7) >> 1
// -- so that the 16 bytes a lane of the Winograd epilogue holds after the output transform (two adjacent pixels x its two couts) are contiguous.
// LDS image of a paired source: [slice][halo row][pixel pair][kq][pixel parity][2 channels]; one 16-byte LDS-DMA unit is (pixel pair, kq).  Pairs are
// aligned to even image columns, so a row stages the columns x0 - 2 .. x0 + TW + 1 of the tile (TW + 4 <= PITCH for every tile with halo columns);
// a lane's ds_read_b64 still finds channels (2 kq, 2 kq + 1) of one pixel in 8 contiguous bytes.
// Swizzle: on the 8 units w = pairbit * 4 + kq of an aligned 128-byte group (two pairs), applied on the SOURCE side of the LDS-DMA as before.  The
// 8-byte slot (address / 8 mod 32) a lane (tile, kq) reads for patch column c is
//     row slots + 16 (G & 1) + 2 (w ^ swz) + (c & 1),   G = c >> 2,
// and the rows of the 16 tiles of a wave are whole multiples of 32 slots apart.  swz = 2 (((G >> 1) ^ slice) & 1) + 4 ((R >> 2) & 1) gives the tile
// columns G, G + 2 and the two tile rows / slices of a wave slots of their own: the 32 lanes of a half wave fall two by two on 16 slots (the other
// 16 belong to the other pixel parity) -- 2-way, what the blocked image has.  The folded 12x8 tile has 8 (slice, tile row) combinations per wave,
// consecutive values of q = 3 slice + tile row, and patch row i of tile row tr lies in halo row R = 4 tr + i: swz = 2 (((R >> 2) + 3 slice) & 3)
// = 2 ((q + (i >> 2)) mod 4) puts two of them on each of its four values.  (Lanes that read the SAME address -- the idle slots 60..63 of the folded
// tile repeat slot 59 -- are one broadcast access, not a conflict.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RCU_GEOM_FN __host__ __device__ __forceinline__
#else
#define RCU_GEOM_FN inline
#endif

namespace rcu {

// Workgroup tile: WS slice groups x WR block rows of MFMA row blocks; a block = SB slices x BR tile rows x BC tile columns = 16
// tiles of 4x4 pixels spanning the tile's full width.
// FULLW: the tile spans the image's width (checked by the launcher), so the halo columns are zero padding and are not staged at all:
// the LDS image holds TW positions per row and the lanes of the first / last tile column read their outer patch column from a region of zeros (ZERO_DW).
// What it buys is LDS: eight slices of 8x16 pixels (the 24x16 level) fit the 160 KB only without the two halo columns.
// FOLD: 12x8-pixel images (the BraTS bottom level).  A slice is 3 x 2 = 6 tiles of 4x4 pixels, and the workgroup's 64 tile slots -- slot k = wave
// k / 16, MFMA row k % 16 -- take the tiles of FOLD_TS = 10 consecutive slices one behind the other: slot k < 60 holds tile ((k % 6) / 2, k % 2) of
// slice k / 6, slots 60..63 are idle -- their MFMA rows read slice 9's last patch again and are never stored.  60 of 64 slots work: 2.25 x 64/60 =
// 2.4 multiplications per pixel against F(2x2,3x3)'s 4.  (Until the tile held ten slices a slice had the 8 slots of the S8 block geometry the tile
// descends from, two of them idle: 48 of 64.)  A slice's tiles do not line up with the waves or with a lane's four accumulator rows any more: wave 0
// holds slices 0, 1 and four tiles of slice 2, and the four slots 4j .. 4j+3 (j = 4 wave + g) of D-side lane (n, g) are tiles 0-3 of a slice
// (j % 3 = 0), tiles 2-5 (j % 3 = 2), or tiles 4, 5 of one slice and 0, 1 of the next (j % 3 = 1); j = 15 is idle.  So slice, Dropout2d factor and
// store offset are per tile in this geometry, derived in the epilogue (wino4_epilogue), not per lane.
template <int SB_, int BR_, int BC_, int WS_, int WR_, bool FULLW_ = false, bool FOLD_ = false>
struct Wino4Tile {
    static constexpr int SB = SB_, BR = BR_, BC = BC_, WS = WS_, WR = WR_;
    static constexpr bool FULLW = FULLW_, FOLD = FOLD_;
    static constexpr int FOLD_TS = 10;                                       // slices of a folded tile: 60 of the 64 slots
    static constexpr int TS = FOLD ? FOLD_TS : SB * WS, TH = FOLD ? 12 : 4 * BR * WR, TW = FOLD ? 8 : 4 * BC;
    static constexpr int TCOLS = FOLD ? 2 : BC;                              // tile columns of the workgroup tile
    static constexpr int BN = 32, KC = 8, THREADS = 256, WAVES = 4, NPOS = 36;
    static constexpr int XCOLS = FULLW ? TW : TW + 2;                        // staged pixel columns per row: x = -1 .. TW, or 0 .. TW - 1
    static constexpr int XCOLS_P = FULLW ? TW : TW + 4;                      // ... of a paired source: x = -2 .. TW + 1 (whole pixel pairs)
    static constexpr int XOFF_P = FULLW ? 0 : 2;                             // staged column of the tile's first pixel column, paired source
    static constexpr int PITCH = (XCOLS + 3) / 4 * 4;                        // positions per halo row, a multiple of 4
    static constexpr int SLICE_POS = ((TH + 2) * PITCH + 15) / 16 * 16;      // positions per slice image, a multiple of 16
    static constexpr int A_POS = 2 * TS * SLICE_POS;                         // 16-byte units: [slice][halo row][position][channel half]
    static constexpr int A_PIECES = (A_POS + 63) / 64;
    static constexpr int NA = (A_PIECES + WAVES - 1) / WAVES;
    static constexpr int A_DW = A_PIECES * 256;
    static constexpr int W_DW = NPOS * 4 * BN * 2;                           // [p][channel pair][cout][2]
    static constexpr int W_PIECES = W_DW / 256;
    static constexpr int NW = (W_PIECES + WAVES - 1) / WAVES;
    // FULLW: row slots at the row pitch behind the image and the weights of EACH chunk buffer that hold zeros for the whole kernel (cleared once,
    // never a target of the LDS-DMA: the pieces end at A_DW + W_DW).  The lanes of the first / last tile column read their outer patch column there.
    // One region per buffer, at the same offset from the buffer's base, because a lane's column addresses are offsets from that base; whole 1 KB
    // pieces, so the second buffer keeps the alignment of the first.  Four row slots serve the six patch rows: rows 0..3 and rows 4..5 have an
    // address register each (aCol), and the second one points four rows lower (the 8x32 tile of four slices fills the 160 KB exactly with them).
    static constexpr int ZERO_ROWS = 4;
    static constexpr int ZERO_DW = FULLW ? (ZERO_ROWS * PITCH * 8 + 255) / 256 * 256 : 0;
    static constexpr int ZERO_OFF = A_DW + W_DW;                             // dword offset of the region inside a buffer
    static constexpr int BUF_DW = A_DW + W_DW + ZERO_DW;
    static constexpr int LDS_BYTES = 2 * BUF_DW * 4;
    static_assert(SB * BR * BC == 16 && WS * WR == WAVES && BC % 4 == 0, "block geometry");
    static_assert(!FOLD || (SB == 2 && BR == 2 && BC == 4 && WS == 4 && WR == 1 && FULLW), "the folded 12x8 geometry descends from the S8 block");
    static_assert(!FOLD || 6 * TS <= 16 * WAVES, "a folded slice is 6 tiles");
    static_assert(W_DW % 256 == 0 && LDS_BYTES <= 160 * 1024, "LDS");
    static_assert(XCOLS_P <= PITCH && TW % 2 == 0, "the pixel pairs of a paired source fit the row pitch");
    // wave -> (first slice of its block inside the tile, top pixel row of its block inside the slice tile)
    static RCU_GEOM_FN void block_origin(int wave, int& s, int& y)
    {
        s = (wave / WR) * SB;
        y = (wave % WR) * (4 * BR);
    }
    // tile m of a block -> (slice inside the block, tile row, tile column)
    static RCU_GEOM_FN void tile_of(int m, int& sb, int& tr, int& tc)
    {
        sb = m / (BR * BC);
        tr = (m / BC) % BR;
        tc = m % BC;
    }
    // MFMA row m of wave `wave` -> (slice inside the workgroup tile, top pixel row of the 4x4 tile inside the slice tile, tile column)
    static RCU_GEOM_FN void row_tile(int wave, int m, int& s, int& y, int& tc)
    {
        if constexpr (FOLD) {
            const int k0 = 16 * wave + m, k = k0 < 6 * TS - 1 ? k0 : 6 * TS - 1;   // the idle slots read the last tile's patch
            s = k / 6;
            const int t = k - 6 * s;
            y = 4 * (t >> 1);
            tc = t & 1;
        } else {
            int bs, by, sb, tr;
            block_origin(wave, bs, by);
            tile_of(m, sb, tr, tc);
            s = bs + sb;
            y = by + 4 * tr;
        }
    }
    // FOLD: does MFMA row m of wave `wave` hold a tile?
    static RCU_GEOM_FN bool row_works(int wave, int m) { return !FOLD || 16 * wave + m < 6 * TS; }
    static RCU_GEOM_FN int swizzle(int x, int s, int R) { return (((x >> 3) ^ s) & 1) | (((R >> 2) & 1) << 1); }
    // paired source: XORed on the unit index pairbit * 4 + kq inside the aligned 128-byte group G of halo row R (see the header)
    static RCU_GEOM_FN int swizzle_paired(int G, int s, int R)
    {
        if constexpr (FOLD) return 2 * (((R >> 2) + 3 * s) & 3);
        return 2 * (((G >> 1) ^ s) & 1) + 4 * ((R >> 2) & 1);
    }
};

// Blocked source.  16-byte unit f of the LDS image -> what it holds, packed: x | halo row << 8 | slice << 16 | channel half << 24.
template <class T>
RCU_GEOM_FN uint32_t wino4_slot_geometry(int j, int wave, int lane)
{
    const int f = (j * T::WAVES + wave) * 64 + lane;       // 16-byte unit of the LDS image: adjacent lanes fetch the two halves of a pixel's 32 bytes
    const int hh = f & 1, rem = f >> 1;
    const int s = rem / T::SLICE_POS, r2 = rem % T::SLICE_POS;
    const int yy = r2 / T::PITCH, pos = r2 % T::PITCH;
    const int x = pos ^ T::swizzle(pos, s, yy);             // the swizzle only moves a position inside its aligned group of four
    const bool real = f < T::A_POS && yy < T::TH + 2 && x < T::XCOLS;
    // the x field is the column in halo coordinates (image column + 1), whichever layout the image has
    return real ? (uint32_t)((x + (T::FULLW ? 1 : 0)) | (yy << 8) | (s << 16) | (hh << 24)) : 0xFFFFFFFFu;
}

// Paired source.  The unit holds (pixel pair, kq): staged column of the pair's even pixel | halo row << 8 | slice << 16 | kq << 24.
template <class T>
RCU_GEOM_FN uint32_t wino4_slot_geometry_paired(int j, int wave, int lane)
{
    const int f = (j * T::WAVES + wave) * 64 + lane;
    const int rem = f >> 1;
    const int s = rem / T::SLICE_POS, r2 = rem % T::SLICE_POS;
    const int yy = r2 / T::PITCH, pos = r2 % T::PITCH;
    const int G = pos >> 2, w = (((pos & 3) << 1) | (f & 1)) ^ T::swizzle_paired(G, s, yy);
    const int c = 4 * G + 2 * (w >> 2);
    const bool real = f < T::A_POS && yy < T::TH + 2 && c < T::XCOLS_P;
    return real ? (uint32_t)(c | (yy << 8) | (s << 16) | ((w & 3) << 24)) : 0xFFFFFFFFu;
}

// The tile-independent part of a paired slot's byte offset with the border flags of wino_slot_plan (rcu_wino_common.h) in its low four bits: a pair
// wholly left or right of the tile lies outside the image exactly when the tile touches that border (tiles and images have even widths).
// H, W, C1: the source tensor's extent; the source address is pair * 64 + kq * 16 inside the chunk plane.
template <class T>
RCU_GEOM_FN uint32_t wino4_slot_plan_paired(int H, int W, int C1, uint32_t geo)
{
    const int c = geo & 0xFF, yy = (geo >> 8) & 0xFF, s = (geo >> 16) & 0xFF, kq = (geo >> 24) & 3;
    const uint32_t off = (uint32_t)s * ((uint32_t)(H * W) * (uint32_t)C1 * 4u) + (uint32_t)((yy - 1) * W + (c - T::XOFF_P)) * 32u + (uint32_t)kq * 16u;
    const uint32_t flags = (yy == 0 ? 1u : 0u) | (yy == T::TH + 1 ? 2u : 0u) | (T::XOFF_P != 0 && c == 0 ? 4u : 0u) |
                           (T::XOFF_P != 0 && c == T::TW + 2 ? 8u : 0u);
    return geo != 0xFFFFFFFFu ? (off | flags) : 0x80000000u;
}

// dword offset, inside a halo row of a paired image, of (staged column c, channel pair kq)
template <class T>
RCU_GEOM_FN int wino4_col_paired(int c, int kq, int s, int R)
{
    const int G = c >> 2, w = (((c >> 1) & 1) << 2) | kq;
    return 32 * G + 4 * (w ^ T::swizzle_paired(G, s, R)) + 2 * (c & 1);
}

// Fragment address (dword offset inside a chunk buffer) of patch column j of the lane (MFMA row m16, channel pair kq) for patch rows 0..3 (ip = 0)
// and 4..5 (ip = 1: the swizzle's row bit flips); the row itself is an immediate offset i * PITCH * 8.
template <class T>
RCU_GEOM_FN int wino4_patch_col(bool paired, int wave, int m16, int kq, int ip, int j)
{
    int s, R0, tc;
    T::row_tile(wave, m16, s, R0, tc);
    int row0 = (s * T::SLICE_POS + R0 * T::PITCH) * 8;
    int x = 4 * tc + j - (T::FULLW ? 1 : 0);   // staged column of patch column j (blocked image)
    if (T::FULLW) {
        // zero padding left and right of the image: the column outside is read from the buffer's zero region -- at the position its
        // clamped neighbour has in a row (the row bases are multiples of 64 dwords: the same banks as the neighbour), rows 4..5 four
        // rows lower, so that the immediate row offsets i * PITCH * 8 stay inside the region's ZERO_ROWS slots
        if (x < 0 || x >= T::TW) row0 = T::ZERO_OFF - 4 * ip * T::PITCH * 8;
        x = x < 0 ? 0 : x > T::TW - 1 ? T::TW - 1 : x;
    }
    if (paired) return row0 + wino4_col_paired<T>(x + (T::FULLW ? 0 : 1), kq, s, R0 + 4 * ip);
    return row0 + 2 * kq + 8 * (x ^ T::swizzle(x, s, R0 + 4 * ip));
}

// Workgroup tile of the up-convolution on the output grid: WS slice groups x WR block rows of MFMA row blocks; a block = SB slices x BR tile rows x
// BC tile columns = 16 tiles of 4x4 output pixels spanning the tile's full width (Wino4Tile).  TH x TW is the LOW-resolution tile the staging
// helpers of rcu_wino_common.h see.
template <int SB_, int BR_, int BC_, int WS_, int WR_>
struct Up4Tile {
    static constexpr int SB = SB_, BR = BR_, BC = BC_, WS = WS_, WR = WR_;
    static constexpr int TS = SB * WS, OTH = 4 * BR * WR, OTW = 4 * BC;      // output pixels
    static constexpr int TH = OTH / 2, TW = OTW / 2;                         // low-resolution pixels
    static constexpr int BN = 32, KC = 8, THREADS = 256, WAVES = 4, NPOS = 25;
    static constexpr int XCOLS = TW + 2;                                     // staged pixel columns per row: x = -1 .. TW
    static constexpr int XCOLS_P = TW + 4, XOFF_P = 2;                       // paired source: x = -2 .. TW + 1 (whole pixel pairs)
    static constexpr int PITCH = (XCOLS + 3) / 4 * 4;                        // positions per halo row
    static constexpr int SLICE_POS = ((TH + 2) * PITCH + 15) / 16 * 16;      // positions per slice image, a multiple of 16
    static constexpr int A_POS = 2 * TS * SLICE_POS;                         // 16-byte units: [slice][halo row][position][channel half]
    static constexpr int A_PIECES = (A_POS + 63) / 64;
    static constexpr int NA = (A_PIECES + WAVES - 1) / WAVES;
    static constexpr int A_DW = A_PIECES * 256;
    static constexpr int W_DW = NPOS * 4 * BN * 2;                           // [p][channel pair][cout][2]
    static constexpr int W_PIECES = W_DW / 256;
    static constexpr int NW = (W_PIECES + WAVES - 1) / WAVES;
    static constexpr int BUF_DW = A_DW + W_DW;
    static constexpr int LDS_BYTES = 2 * BUF_DW * 4;
    static_assert(SB * BR * BC == 16 && WS * WR == WAVES && BC % 4 == 0, "block geometry");
    static_assert(W_DW % 256 == 0 && LDS_BYTES <= 160 * 1024, "LDS");
    static_assert(XCOLS_P <= PITCH && TW % 2 == 0, "the pixel pairs of a paired source fit the row pitch");
    // wave -> (first slice of its block inside the tile, top OUTPUT pixel row of its block inside the slice tile)
    static RCU_GEOM_FN void block_origin(int wave, int& s, int& y)
    {
        s = (wave / WR) * SB;
        y = (wave % WR) * (4 * BR);
    }
    // tile m of a block -> (slice inside the block, tile row, tile column)
    static RCU_GEOM_FN void tile_of(int m, int& sb, int& tr, int& tc)
    {
        sb = m / (BR * BC);
        tr = (m / BC) % BR;
        tc = m % BC;
    }
    static RCU_GEOM_FN int swizzle(int x, int s) { return ((x >> 3) ^ s) & 1; }
    // paired source: as Wino4Tile::swizzle_paired without the row term (a wave's tile rows are whole multiples of 32 slots apart and the tile
    // columns, 2 positions apart, already use the pair bit)
    static RCU_GEOM_FN int swizzle_paired(int G, int s, int) { return 2 * (((G >> 1) ^ s) & 1); }
};

template <class T>
RCU_GEOM_FN uint32_t up4_slot_geometry(int j, int wave, int lane)
{
    const int f = (j * T::WAVES + wave) * 64 + lane;       // 16-byte unit of the LDS image: adjacent lanes fetch the two halves of a pixel's 32 bytes
    const int hh = f & 1, rem = f >> 1;
    const int s = rem / T::SLICE_POS, r2 = rem % T::SLICE_POS;
    const int yy = r2 / T::PITCH, pos = r2 % T::PITCH;
    const int x = pos ^ T::swizzle(pos, s);                 // the swizzle swaps the two positions of an aligned pair
    const bool real = f < T::A_POS && yy < T::TH + 2 && x < T::XCOLS;
    return real ? (uint32_t)(x | (yy << 8) | (s << 16) | (hh << 24)) : 0xFFFFFFFFu;   // (x, yy): halo coordinates, pixel + 1
}

// Fragment address (dword offset inside a chunk buffer) of patch column j = 0..3 of the lane in patch row 0; the row is an immediate offset.
// Output tile (row oy, column ox) reads low-resolution rows oy / 2 - 1 .. oy / 2 + 2 = halo rows oy / 2 .. oy / 2 + 3, and columns alike.
template <class T>
RCU_GEOM_FN int up4_patch_col(bool paired, int wave, int m16, int kq, int j)
{
    int bs, by, sb, tr, tc;
    T::block_origin(wave, bs, by);
    T::tile_of(m16, sb, tr, tc);
    const int s = bs + sb, R0 = (by + 4 * tr) >> 1;
    const int row0 = (s * T::SLICE_POS + R0 * T::PITCH) * 8;
    const int x = 2 * tc + j;
    if (paired) return row0 + wino4_col_paired<T>(x + 1, kq, s, R0);
    return row0 + 2 * kq + 8 * (x ^ T::swizzle(x, s));
}

}  // namespace rcu
