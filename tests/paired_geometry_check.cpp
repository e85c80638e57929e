// Host model of the paired LDS image of the F(4x4,3x3) kernels (csrc/rcu_wino4_geom.h), built and run by tests/test_paired_layout_cpu.py.
// For every tile type -- the five Wino4Tiles and the three Up4Tiles -- on a 2 x 2 grid of tiles (one column of two for the full-width tiles):
//   1. every staged (slice, halo row, pixel pair, kq) unit is fetched by exactly one LDS-DMA slot, and every slot lies inside the image region of
//      the chunk buffer (below the weights and the zero region);
//   2. bank model of ds_read_b64: for every patch read (i, j) and each half of a wave, no 8-byte LDS slot (address / 8 mod 32) is hit by more than
//      two DIFFERENT addresses (lanes that read the same address -- the idle slots of the folded tile -- are one broadcast access);
//   3. every lane reads, for every (i, j), exactly the 8 bytes of the source tensor that hold its pixel's channel pair: the LDS is filled from the
//      slot plans with the source byte offset of every unit as its tag, and the lane's address must carry the tag of
//      (slice, y, x, kq) = sample * H W 32 + ((y W + x) >> 1) * 64 + kq * 16 + (x & 1) * 8 -- or zeros (out of range, or the zero region) exactly
//      when the pixel lies outside the image.
#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "rcu_wino4_geom.h"

using namespace rcu;

static int failures = 0;
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            if (failures < 20) {             \
                printf("FAIL %s: ", name);   \
                printf(__VA_ARGS__);         \
                printf("\n");                \
            }                                \
            ++failures;                      \
        }                                    \
    } while (0)

constexpr uint32_t OOB = 0x80000000u;

// the LDS image of tile (ty, tx): source byte offset of every 16-byte unit (OOB: zeros)
template <class T>
static std::vector<uint32_t> stage(const char* name, int H, int W, int y0, int x0, uint32_t tensor_bytes)
{
    std::vector<uint32_t> lds((size_t)T::A_PIECES * 64, 0xFFFFFFFFu);
    const uint32_t t_off = (uint32_t)(y0 * W + x0) * 32u;
    const uint32_t border = (y0 == 0 ? 1u : 0u) | (y0 + T::TH == H ? 2u : 0u) | (x0 == 0 ? 4u : 0u) | (x0 + T::TW == W ? 8u : 0u);
    std::set<uint32_t> seen;
    int real = 0;
    for (int j = 0; j < T::NA; ++j)
        for (int wave = 0; wave < T::WAVES; ++wave)
            for (int lane = 0; lane < 64; ++lane) {
                if (j * T::WAVES + wave >= T::A_PIECES) continue;
                const int f = (j * T::WAVES + wave) * 64 + lane;
                const uint32_t geo = wino4_slot_geometry_paired<T>(j, wave, lane);
                if (geo != 0xFFFFFFFFu) {
                    ++real;
                    CHECK(seen.insert(geo).second, "unit %08x fetched twice", geo);
                    CHECK(f < T::A_POS && f * 4 < T::A_DW, "slot %d outside the image region", f);
                }
                const uint32_t plan = wino4_slot_plan_paired<T>(H, W, 8, geo);
                uint32_t off = (plan & border) != 0u ? OOB : ((plan + t_off) & ~15u);
                if (off >= tensor_bytes) off = OOB;
                lds[f] = off;
            }
    CHECK(real == T::TS * (T::TH + 2) * (T::XCOLS_P / 2) * 4, "%d staged units, expected %d", real, T::TS * (T::TH + 2) * (T::XCOLS_P / 2) * 4);
    return lds;
}

// one patch read of one lane: dword address -> check 3; returns the address for the bank model
template <class T>
static void check_read(const char* name, const std::vector<uint32_t>& lds, int addr, int zero_lo, int zero_hi, int H, int W, int s, int y, int x, int kq)
{
    const bool inside = y >= 0 && y < H && x >= 0 && x < W;
    CHECK(addr >= 0 && addr % 2 == 0, "address %d", addr);
    if (addr >= T::A_DW) {
        CHECK(addr >= zero_lo && addr + 2 <= zero_hi, "address %d in the weight region", addr);
        CHECK(!inside, "pixel (%d, %d) read from the zero region", y, x);
        return;
    }
    const uint32_t unit = lds[addr / 4];
    CHECK(unit != 0xFFFFFFFFu, "address %d was never staged", addr);
    if (!inside) {
        CHECK(unit == OOB, "pixel (%d, %d) outside the image reads data", y, x);
        return;
    }
    const uint32_t want = (uint32_t)s * (uint32_t)(H * W) * 32u + (uint32_t)((y * W + x) >> 1) * 64u + (uint32_t)kq * 16u + (uint32_t)(x & 1) * 8u;
    CHECK(unit != OOB && unit + (uint32_t)(addr % 4) * 4u == want, "slice %d pixel (%d, %d) kq %d: read %u, want %u", s, y, x, kq, unit + (addr % 4) * 4u, want);
}

static void bank_check(const char* name, const int (&addr)[64], int i, int j)
{
    for (int half = 0; half < 2; ++half) {
        std::map<int, std::set<int>> slots;
        for (int l = 0; l < 32; ++l) slots[(addr[32 * half + l] / 2) % 32].insert(addr[32 * half + l]);
        for (const auto& kv : slots) CHECK(kv.second.size() <= 2, "read (%d, %d) half %d: %d-way conflict on slot %d", i, j, half, (int)kv.second.size(), kv.first);
    }
}

template <class T>
static void conv_tile(const char* name)
{
    const int H = 2 * T::TH, W = T::FULLW ? T::TW : 2 * T::TW;
    const uint32_t bytes = (uint32_t)T::TS * H * W * 32u;
    for (int y0 = 0; y0 < H; y0 += T::TH)
        for (int x0 = 0; x0 < W; x0 += T::TW) {
            const std::vector<uint32_t> lds = stage<T>(name, H, W, y0, x0, bytes);
            for (int wave = 0; wave < T::WAVES; ++wave)
                for (int i = 0; i < 6; ++i)
                    for (int j = 0; j < 6; ++j) {
                        int addr[64];
                        for (int lane = 0; lane < 64; ++lane) {
                            const int m16 = lane & 15, kq = lane >> 4;
                            int s, R0, tc;
                            T::row_tile(wave, m16, s, R0, tc);
                            addr[lane] = wino4_patch_col<T>(true, wave, m16, kq, i >> 2, j) + i * T::PITCH * 8;
                            check_read<T>(name, lds, addr[lane], T::ZERO_OFF, T::ZERO_OFF + T::ZERO_DW, H, W, s, y0 + R0 + i - 1, x0 + 4 * tc + j - 1, kq);
                        }
                        if (y0 == 0 && x0 == 0) bank_check(name, addr, i, j);
                    }
        }
}

template <class T>
static void up_tile(const char* name)
{
    const int H = 2 * T::TH, W = 2 * T::TW;   // the low-resolution level
    const uint32_t bytes = (uint32_t)T::TS * H * W * 32u;
    for (int y0 = 0; y0 < H; y0 += T::TH)
        for (int x0 = 0; x0 < W; x0 += T::TW) {
            const std::vector<uint32_t> lds = stage<T>(name, H, W, y0, x0, bytes);
            for (int wave = 0; wave < T::WAVES; ++wave)
                for (int i = 0; i < 4; ++i)
                    for (int j = 0; j < 4; ++j) {
                        int addr[64];
                        for (int lane = 0; lane < 64; ++lane) {
                            const int m16 = lane & 15, kq = lane >> 4;
                            int bs, by, sb, tr, tc;
                            T::block_origin(wave, bs, by);
                            T::tile_of(m16, sb, tr, tc);
                            addr[lane] = up4_patch_col<T>(true, wave, m16, kq, j) + i * T::PITCH * 8;
                            check_read<T>(name, lds, addr[lane], 0, 0, H, W, bs + sb, y0 + ((by + 4 * tr) >> 1) + i - 1, x0 + 2 * tc + j - 1, kq);
                        }
                        if (y0 == 0 && x0 == 0) bank_check(name, addr, i, j);
                    }
        }
}

int main()
{
    conv_tile<Wino4Tile<1, 2, 8, 1, 4>>("T32x32");
    conv_tile<Wino4Tile<1, 2, 8, 2, 2>>("S2T16x32");
    conv_tile<Wino4Tile<2, 2, 4, 4, 1, true>>("S8T8x16");
    conv_tile<Wino4Tile<2, 2, 4, 4, 1, true, true>>("S8T12x8");
    conv_tile<Wino4Tile<1, 2, 8, 4, 1, true>>("S4T8x32");
    up_tile<Up4Tile<1, 2, 8, 1, 4>>("up T32x32");
    up_tile<Up4Tile<1, 2, 8, 2, 2>>("up S2T16x32");
    up_tile<Up4Tile<2, 2, 4, 4, 1>>("up S8T8x16");
    printf("%d failures\n", failures);
    return failures != 0;
}
