// Host-side packing of conv weights into the tiles the conv kernels stage (plain C++: no HIP, no device; tests/wpack_digest.cpp runs it alone).
#pragma once
#include <stddef.h>

namespace rcu {

// what the packer reads of a kernel's ConvConfigInfo (rcu_kernels.h) ...
struct WpackKernel {
    bool winograd;   // ConvFamilyTraits::winograd; the transform follows from TAPS, the number of positions
    int TAPS, BN, KC, KCP, SWZ, weight_sets;
};
template <class Info>   // (a template only because this header does not see rcu_kernels.h)
inline WpackKernel wpack_kernel(const Info& ci) { return {ci.family.winograd, ci.TAPS, ci.BN, ci.KC, ci.KCP, ci.SWZ, ci.family.weight_sets}; }
// ... and of a layer
struct WpackLayer {
    int cin1, c1p, cin2;   // real channels of the two sources, padded channels of the first: the second source's K range starts at c1p
    int cout, NT;          // real output channels of the conv (of one twin), cout tiles of the layer
    int upsample;
};

// floats of one packed weight tile
inline size_t wpack_tile_floats(const WpackKernel& k)
{
    if (k.winograd) return (size_t)k.TAPS * k.BN * k.KCP;   // the LDS image, piece by piece (LDS-DMA)
    const size_t units = (size_t)k.TAPS * k.BN * k.KCP / 4;   // [TAPS][BN][KC+4], rounded up to 256 threads x float4
    return (units + 255) / 256 * 256 * 4;
}
// floats of a layer's packed weights: [Cin chunk][weight set][cout tile] tiles
inline size_t wpack_floats(const WpackKernel& k, int cin_padded, int NT) { return (size_t)(cin_padded / k.KC) * k.weight_sets * NT * wpack_tile_floats(k); }

// Sub-pixel up-conv: output parity a (rows) folds the 3 kernel rows onto 2 low-res rows,
//   a = 0: low-res row y-1 <- {dy 0},   row y   <- {dy 1, 2}
//   a = 1: low-res row y   <- {dy 0, 1}, row y+1 <- {dy 2}            (same for columns with b)
inline bool fold_set(int parity, int t, int d) { return parity == 0 ? (t == 0 ? d == 0 : d >= 1) : (t == 0 ? d <= 1 : d == 2); }

// The square Winograd weight transforms U = G' g G'^T of a 3x3 kernel g: G' = the kept rows of G, and a factor per kept row (U[i][j] carries
// scale[i] * scale[j]).  Position p = n i + j.
struct WinoTransform {
    int n;                  // kept rows: n x n positions
    const double (*G)[3];
    int row[6];
    double scale[6];
};
// F(2x2,3x3), points 0, +-1, inf
static const double kG2[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
// F(4x4,3x3): the Lavin-Gray G for the points 0, +-1, +-2, inf
static const double kG4[6][3] = {{1.0 / 4, 0, 0},           {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                 {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6},  {0, 0, 1}};
static const WinoTransform kWinoTransforms[3] = {
    {4, kG2, {0, 1, 2, 3}, {1, 1, 1, 1}},               // rcu_wino.hip
    {6, kG4, {0, 1, 2, 3, 4, 5}, {1, 1, 1, 1, 1, 1}},   // rcu_wino4.hip
    // F(4x4,3x3) of the up-sampled image (rcu_wino4_up.hip): without row and column 2 (the point -1, where the up-sampled input vanishes); rows and
    // columns 3 (the point +2) carry the factor -3 by which the kernel's shared transformed value b - c differs from B^T's row 3 -- both
    // directions for the corner entry: 9
    {5, kG4, {0, 1, 3, 4, 5}, {1, 1, -3, 1, 1}},
};

// Packs the conv weights w [cout][cin1 + cin2][3][3] into wpack (wpack_floats, zero where nothing is written) at output-channel offset co0.
//   direct kernels: per Cin chunk, parity class (sub-pixel form) and cout tile a tile [tap][cout][KCP], taps as they are or folded per class
//   Winograd kernels: per Cin chunk, weight set and cout tile a tile [position p][channel pair][cout][2]; every value computed in double from the
//                     float taps and rounded once
inline void pack_conv_weights(const WpackKernel& k, const WpackLayer& l, const float* w, int co0, float* wpack)
{
    const int cin = l.cin1 + l.cin2;
    const size_t tile_floats = wpack_tile_floats(k);
    const WinoTransform* square = nullptr;   // TAPS = n x n names the transform; 18 = two classes of 3x3: F(2x2,2x2) below
    for (const WinoTransform& t : kWinoTransforms)
        if (k.winograd && t.n * t.n == k.TAPS) square = &t;
    for (int co = 0; co < l.cout; ++co) {
        const int cop = co0 + co;
        const int ntile = cop / k.BN, nn = cop % k.BN;
        for (int ci_ = 0; ci_ < cin; ++ci_) {
            const int kp = ci_ < l.cin1 ? ci_ : l.c1p + (ci_ - l.cin1);   // position in the padded K range
            const int chunk = kp / k.KC, kq = kp % k.KC;
            const float* w9 = w + ((size_t)co * cin + ci_) * 9;
            auto tile0 = [&](int set) { return (((size_t)chunk * k.weight_sets + set) * l.NT + ntile) * tile_floats; };
            auto position = [&](int set, int p) -> float& { return wpack[tile0(set) + (((size_t)p * 4 + (kq >> 1)) * k.BN + nn) * 2 + (kq & 1)]; };
            if (square) {
                const WinoTransform& t = *square;
                for (int i = 0; i < t.n; ++i)
                    for (int j = 0; j < t.n; ++j) {
                        double u = 0.0;
                        for (int r = 0; r < 3; ++r)
                            for (int c = 0; c < 3; ++c) u += t.G[t.row[i]][r] * (double)w9[r * 3 + c] * t.G[t.row[j]][c];
                        u *= t.scale[i] * t.scale[j];   // on the finished sum: (1.0 / 24) * -3 is not -1.0 / 8
                        position(0, t.n * i + j) = (float)u;
                    }
            } else if (k.winograd) {
                // F(2x2,2x2) per parity class (a, b): U^{ab} = G w^{ab} G^T, G = [[1,0],[1,1],[0,1]], w^{ab} the 2x2 folded taps.  Weight set a holds
                // p = 6 i + 3 b + j; column j = 0 of class b = 1 is negated because the kernel feeds P.2 - P.1 where F(2,2) wants P.1 - P.2
                // (rcu_wino_up.hip).
                static const double G2[3][2] = {{1, 0}, {1, 1}, {0, 1}};
                for (int pa = 0; pa < 2; ++pa)
                    for (int pb = 0; pb < 2; ++pb) {
                        double wc[2][2];
                        for (int ty = 0; ty < 2; ++ty)
                            for (int tx = 0; tx < 2; ++tx) {
                                double v = 0.0;
                                for (int dy = 0; dy < 3; ++dy)
                                    for (int dx = 0; dx < 3; ++dx)
                                        if (fold_set(pa, ty, dy) && fold_set(pb, tx, dx)) v += (double)w9[dy * 3 + dx];
                                wc[ty][tx] = v;
                            }
                        for (int i = 0; i < 3; ++i)
                            for (int j = 0; j < 3; ++j) {
                                double u = 0.0;
                                for (int ty = 0; ty < 2; ++ty)
                                    for (int tx = 0; tx < 2; ++tx) u += G2[i][ty] * wc[ty][tx] * G2[j][tx];
                                if (pb == 1 && j == 0) u = -u;
                                position(pa, 6 * i + 3 * pb + j) = (float)u;
                            }
                    }
            } else {
                for (int cls = 0; cls < k.weight_sets; ++cls)
                    for (int tap = 0; tap < k.TAPS; ++tap) {
                        float v;
                        if (!l.upsample) {
                            v = w9[tap];
                        } else {
                            const int a = cls >> 1, b = cls & 1, ty = tap >> 1, tx = tap & 1;
                            v = 0.f;
                            for (int dy = 0; dy < 3; ++dy)
                                for (int dx = 0; dx < 3; ++dx)
                                    if (fold_set(a, ty, dy) && fold_set(b, tx, dx)) v += w9[dy * 3 + dx];
                        }
                        // swizzled layout: the two 16-byte units of a row swap places for channels 16..31 (mod 32)
                        const int kdst = k.SWZ ? ((((kq >> 2) ^ ((nn >> 4) & 1)) << 2) | (kq & 3)) : kq;
                        wpack[tile0(cls) + ((size_t)tap * k.BN + nn) * k.KCP + kdst] = v;
                    }
            }
        }
    }
}

}  // namespace rcu
