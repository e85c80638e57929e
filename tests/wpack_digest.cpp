// Digests of the packed conv weights of every ConvConfig (csrc/rcu_wpack.h), without a GPU: for each cfg in [0, CONV_CFG_END) the layer shapes
// the family accepts are packed from seeded weights and one FNV-1a digest of the wpack bytes is printed per case.  tests/test_wpack_cpu.py
// compiles this program, links it with librcu_hip.so for rcu::conv_config_info and compares its output with tests/golden/g30_wpack_digest.json.
//   single  one source, cin = 13 (5 for the kernels of the first layer: K is one chunk of 8), cout = 37: neither a multiple of 8 nor of BN
//   dual    where the family takes two sources: cin1 = 13 padded to c1p = 32, cin2 = 21, cout = 19, and a twin packed at co0 = csplit = 32
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rcu_kernels.h"
#include "rcu_wpack.h"

using namespace rcu;

static std::vector<float> seeded_weights(size_t count, uint64_t seed)
{
    std::vector<float> w(count);
    uint64_t s = seed;
    for (float& v : w) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        v = (float)((int64_t)(s >> 40) - (1 << 23)) / (float)(1 << 21);   // 24 bits: exact, in [-4, 4)
    }
    return w;
}

static uint64_t fnv1a(const std::vector<float>& v)
{
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    uint64_t h = 14695981039346656037ull;
    for (size_t i = 0; i < v.size() * sizeof(float); ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

int main()
{
    for (int cfg = 0; cfg < CONV_CFG_END; ++cfg) {
        const ConvConfigInfo& ci = conv_config_info(cfg);
        const WpackKernel k = wpack_kernel(ci);
        const ConvFamily f = ci.family.id;
        const bool first_layer = f == ConvFamily::First || cfg == CONV_CFG_T8x16_N32_FIRST;
        const int upsample = (f == ConvFamily::DirectUp || f == ConvFamily::Wino2Up || f == ConvFamily::Wino4Up) ? 1 : 0;
        {
            const int cin = first_layer ? 5 : 13, c1p = first_layer ? 8 : 32, cout = 37;
            const int NT = (round_up(cout, 32) + ci.BN - 1) / ci.BN;
            std::vector<float> wpack(wpack_floats(k, c1p, NT), 0.f);
            const std::vector<float> w = seeded_weights((size_t)cout * cin * 9, 1000 + cfg);
            pack_conv_weights(k, WpackLayer{cin, c1p, 0, cout, NT, upsample}, w.data(), 0, wpack.data());
            std::printf("%d %s single %zu %016llx\n", cfg, ci.kernel_name, wpack.size(), (unsigned long long)fnv1a(wpack));
        }
        if ((f == ConvFamily::Direct || f == ConvFamily::Wino2 || f == ConvFamily::Wino4) && !first_layer) {
            const int cin1 = 13, c1p = 32, cin2 = 21, c2p = 32, cout = 19, csplit = 32;
            const int NT = (2 * csplit + ci.BN - 1) / ci.BN;
            std::vector<float> wpack(wpack_floats(k, c1p + c2p, NT), 0.f);
            const WpackLayer layer{cin1, c1p, cin2, cout, NT, 0};
            for (int twin = 0; twin < 2; ++twin) {
                const std::vector<float> w = seeded_weights((size_t)cout * (cin1 + cin2) * 9, 2000 + 2 * cfg + twin);
                pack_conv_weights(k, layer, w.data(), twin * csplit, wpack.data());
            }
            std::printf("%d %s dual %zu %016llx\n", cfg, ci.kernel_name, wpack.size(), (unsigned long long)fnv1a(wpack));
        }
    }
    return 0;
}
