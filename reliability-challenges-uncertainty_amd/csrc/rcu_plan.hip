// The U-Net kernel planner (rcu_plan.h): a function from (description, options) to a Plan value.  Host only: no HIP runtime call, no device memory.
#include "rcu_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace rcu {

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// a tensor of level `level` (allocated with the level's extent), or -- level < 0 -- one that is exactly Hr x Wr
static int new_tensor(Plan& p, int level, int Hr, int Wr, int cp)
{
    PlanTensor t;
    t.Hr = Hr; t.Wr = Wr; t.cp = cp;
    t.H = level >= 0 ? p.level_ext[level].first : Hr;
    t.W = level >= 0 ? p.level_ext[level].second : Wr;
    t.floats_per_slice = (size_t)t.H * t.W * cp;
    p.tensors.push_back(t);
    return (int)p.tensors.size() - 1;
}

static bool unit_has_dropout(const rcu_unet_desc& d, int level, bool is_down, int i)
{
    // common/model/unet.py:63-82
    if (!d.has_dropout) return false;
    if (d.dropout_center < 0) return true;                 // 'all'
    if (level == d.depth) return false;                    // 'no'
    if (level + d.dropout_center >= d.depth) return is_down ? (i == 1) : (i == 0);   // 'last' / 'first'
    return false;
}

static bool is_head_unit(const PlanLayer& L) { return L.name.rfind("conv_cls.0", 0) == 0; }

// The default rule of rcu_unet_options.upconv_winograd4 = 1, per layer: the 25-product up-convolution (rcu_wino4_up.hip) where its work items -- one
// per (slice group, low-resolution tile, 32-cout tile), one workgroup per CU -- fill the chip as far as the kernel has been measured against the
// sub-pixel one.  Measured per layer in one process, old - new - old (tools/upconv4_gate.py, profiles/upconv4_layer_gate.txt), on the four
// up-convolutions of the BraTS shape at 640 / 480 / 320 / 160 samples per launch: 22-28 % faster in all sixteen cases, the spread between the
// two legs of the old kernel below 1.5 %.  The smallest fill among them is 480 items (1.9 rounds of 256 workgroups: 512 -> 256 channels into
// 24x16 at 160 samples, 0.309-0.313 against 0.232 ms); below it nothing is measured, and a plan of a few slices keeps the sub-pixel kernels.
// The second condition is the plan size: only plans sized for the pass-group launches of the predict steps -- 480 samples of 192x128 and up, the
// sizes at which the 12x8 rule of pick_config changes kernels too -- take the kernel.  A 160-sample plan keeps the bits of an 8-sample one
// (tests/test_gpu_fullsize.py compares them), although the kernel is faster there as well: upconv_winograd4 = 2 takes it.
constexpr long kUpconv4MinItems = 480;
constexpr long long kUpconv4MinPlanPixels = 480LL * 192 * 128;   // samples x pixels of the network's input level
static bool upconv4_wins(int cfg, const PlanLayer& L, int n_slices)
{
    const ConvConfigInfo& ci = conv_config_info(cfg);
    const long items = (long)((n_slices + ci.TS - 1) / ci.TS) * (L.gh / ci.TH) * (L.gw / ci.TW) * (L.coutp / ci.BN);
    const int l = L.level - 1;   // the level of the output (L.level: the low-resolution level the tiles walk)
    const long long plan_pixels = (long long)n_slices * ((long long)L.H << l) * ((long long)L.W << l);
    return items >= kUpconv4MinItems && plan_pixels >= kUpconv4MinPlanPixels;
}

// Which kernel runs a layer.  (gh, gw) = L.gh x L.gw is the grid the tiles walk: the ALLOCATED extent of the layer's level (an up-convolution's
// low-resolution level), which is the real extent unless the level is padded (plan_unet); oh x ow the allocated extent of its output tensor.
static int pick_config(const PlanLayer& L, int n_slices, const rcu_unet_options& opt, int oh, int ow)
{
    // Winograd kernels (rcu_wino.hip, rcu_wino_up.hip): 16/36 (conv units) and 9/36 (up-convolutions) of the
    // multiplications.  They address activations through 32-bit byte offsets of a buffer resource (tensors < 2 GB)
    // and take whole tiles only.  Tiles that span two or eight slices are taken whatever the batch the plan is sized for (a last
    // group of slices that is not full reads zeros and stores nothing): the kernel of a layer -- and with it the bits of a slice's
    // result -- does not depend on the batch size, as long as every tensor stays below 2 GB.
    // rcu_unet_options.conv_winograd = 0 keeps every layer on the direct kernels of rcu_conv.hip (A/B tests)
    // a unit that adds to its output tensor (ConvResidualBlock's second unit) runs on the direct kernels, whose epilogue can
    const bool wino_on = opt.conv_winograd != 0 && !L.accumulate;
    const int gh = L.gh, gw = L.gw;
    // (an up-convolution reads the LOW-resolution grid: L.H x L.W is its output grid)
    const size_t in_px = (size_t)gh * gw;
    const size_t max_bytes = (size_t)n_slices * std::max(in_px * (size_t)std::max(L.c1p, L.c2p), (size_t)oh * ow * (size_t)L.coutp) * 4;
    const bool center_pad = L.upsample && (2 * (L.H / 2) != L.H || 2 * (L.W / 2) != L.W);   // unet.py:110-116: direct kernel only
    if (L.upsample && !center_pad && wino_on && L.c1p % 32 == 0 && L.c2p == 0 && max_bytes < ((size_t)1 << 31)) {
        const int lh = gh, lw = gw;
        // F(4x4,3x3) on the up-sampled grid without its vanishing point (rcu_wino4_up.hip): 25 instead of 36 multiplications per 16 output pixels.
        // Whole tiles of unpadded levels only -- the kernel has no ConvArgs::part form, so a padded level on either side keeps the sub-pixel
        // kernels below under every option value -- and every byte offset its lanes form, a tile's slices beyond the batch included, below 2^32.
        // rcu_unet_options.upconv_winograd4: 0 never, 2 wherever the geometry fits (parity tests on small batches), 1 (default) where the
        // plan's work items fill the chip and tools/upconv4_gate.py measured the kernel faster than the sub-pixel one at that plan size:
        // see upconv4_wins.
        const int u4_mode = opt.upconv_winograd4;
        const bool u4_fits = u4_mode != 0 && 2 * lh == L.H && 2 * lw == L.W && oh == L.H && ow == L.W &&
                             (size_t)(n_slices + 8) * std::max(in_px * (size_t)L.c1p, (size_t)oh * ow * (size_t)L.coutp) * 4 < ((size_t)1 << 32);
        if (u4_fits) {
            const int cfg4 = (lh % 16 == 0 && lw % 16 == 0) ? CONV_CFG_UPW4_T32x32_N32
                             : (lh % 8 == 0 && lw % 16 == 0) ? CONV_CFG_UPW4_S2T16x32_N32
                             : (lh % 4 == 0 && lw == 8)      ? CONV_CFG_UPW4_S8T8x16_N32
                                                             : -1;
            if (cfg4 >= 0 && (u4_mode == 2 || upconv4_wins(cfg4, L, n_slices))) return cfg4;
        }
        if (L.coutp == 32 && lh % 16 == 0 && lw % 32 == 0) return CONV_CFG_UPW_T16x32_N32;
        if (L.coutp > 32 && lh % 16 == 0 && lw % 16 == 0) return CONV_CFG_UPW_T16x16_N64;
        if (L.coutp > 32 && lh % 8 == 0 && lw % 16 == 0) return CONV_CFG_UPW_S2T8x16_N64;
        if (L.coutp > 32 && lh % 4 == 0 && lw == 8) return CONV_CFG_UPW_S8T4x8_N64;
    }
    if (L.upsample) {   // sub-pixel form; tiles run over the low-res input grid
        if (L.coutp <= 32) return (gh % 16 == 0 && gw % 16 == 0) ? CONV_CFG_UP_T16x16_N32 : CONV_CFG_UP_T8x16_N32;
        if (gh == 12 && gw == 8) return CONV_CFG_UP_S2T12x8_N64;
        return CONV_CFG_UP_T8x16_N64;
    }
    if (L.c1p + L.c2p == 8) {
        // the network's first conv unit: unpadded K = 9 x 4 (8) on whole 8x32 tiles (rcu_first.hip); rcu_unet_options.conv_first = 0
        // keeps the tiled kernel (A/B tests)
        const bool first_on = opt.conv_first != 0;
        if (first_on && L.c2p == 0 && gh % 8 == 0 && gw % 32 == 0 && (L.coutp == 32 || L.coutp == 64) && L.t_pool < 0 &&
            L.name2.empty() && !L.accumulate)
            return CONV_CFG_FIRST_T8x32;
        return CONV_CFG_T8x16_N32_FIRST;
    }
    if (wino_on && (L.c1p + L.c2p) % 32 == 0 && (L.c2p == 0 || L.c2p == L.c1p) && max_bytes < ((size_t)1 << 31)) {
        // F(4x4,3x3) (rcu_wino4.hip) where its 32-pixel-wide tiles fit: 2.25 instead of 4 multiplications per output pixel.  Measured
        // per layer on the BraTS volume (tools/wino4_check.py, tools/layer_report.py): 1.1x at 32 -> 64 channels to 1.4x at 128 -> 128 and
        // 256 -> 128 over F(2x2,3x3).  The 32-channel full-resolution layers -- four Cin chunks per tile, so a tile switch (cold fetch +
        // epilogue) per four chunks -- lost to F(2x2,3x3) while the activations were channels-last (0.39-0.69 against 0.36-0.64 ms); with
        // the channel-blocked layout, whose chunks are cold one at a time, they win too (round 3: 0.31 / 0.47 / 0.28 against
        // 0.35 / 0.60 / 0.33 ms).  rcu_unet_options.conv_winograd4 = 0 keeps F(2x2,3x3) everywhere, 3 takes F(4x4,3x3) for the layers with
        // >= 64 output channels only (the round-2 choice; A/B tests).
        const int w4_mode = opt.conv_winograd4;
        // The head unit (conv_cls.0 alone: one 32-cout tile, no sigma twin) has its classifier fused into the epilogue of either family
        // (forward_impl); the F(4x4,3x3) form exists for the 32x32 tile only, elsewhere -- and under head_winograd4 = 0, the plan of
        // rounds 1-4 -- it stays on F(2x2,3x3).  The 64-cout cls + sigma twin unit has no fused form and takes F(4x4,3x3) like any layer.
        const bool lone_head = is_head_unit(L) && L.name2.empty();
        const bool w4_ok = w4_mode != 0 && (L.coutp >= 64 || w4_mode != 3) &&
                           !(lone_head && (opt.head_winograd4 == 0 || L.coutp != 32 || gh % 32 != 0 || gw % 32 != 0));
        if (w4_ok && gw % 32 == 0) {
            if (gh % 32 == 0) return CONV_CFG_WINO4_T32x32_N32;
            if (gh % 16 == 0) return CONV_CFG_WINO4_S2T16x32_N32;
        }
        // images exactly 32 wide whose height is a multiple of 8 but not of 16 (24x32: the fourth level of the reference's ISIC size 192x256): the
        // full-width tile of four slices takes them as they are (round 6; padded to 32x32 the level would compute a third more)
        if (w4_ok && gw == 32 && gh % 8 == 0) return CONV_CFG_WINO4_S4T8x32_N32;
        if (w4_ok && gw == 16 && gh % 8 == 0) return CONV_CFG_WINO4_S8T8x16_N32;
        // the 12x8 level (bottom_convs): F(4x4,3x3) with the 60 tiles of ten slices in the 64 tile slots of a workgroup -- 2.4 multiplications per
        // output pixel executed (2.25 x 64/60) against F(2x2,3x3)'s 4 (round 5; ten slices instead of eight -- 48 of 64 slots -- since
        // profiles/fold10_gate.txt; no pooled output in this geometry)
        if (w4_ok && gw == 8 && gh % 12 == 0 && L.t_pool < 0) {
            // ... where its few, long work items fill the chip's rounds: one item = 10 slices x 32 couts against F(2x2,3x3)'s 8 slices x a 4x8 strip x
            // 64 couts.  Measured per round of 256 workgroups (bottom_convs, tools/layer_report.py) while an item was 8 slices: 0.282 against
            // 0.210 ms, so the folded form wins when rounds_4 * 1.35 < rounds_2 -- 640 samples: 4 against 8 rounds, 480: 3 against 6.  A round
            // of ten slices measured 0.295 ms against the eight-slice tile's 0.284 on the same box (profiles/fold10_gate.txt): 1.18 against
            // 1.42 ms at 640 samples, 0.89 against 1.14 at 480.
            // Plans below the pass-group sizes of the predict steps (480 samples of 192x128, as upconv4_wins) keep the decisions of the 8-slice
            // tile, i.e. the same rule with rounds_4 counted in groups of eight: 160 samples (an ensemble member's launch) 2 against 2, 320: 3
            // against 4 -- F(2x2,3x3) stays.  Ten slices would take both (1 against 2, 2 against 4 rounds) and the kernel would win there too, but
            // a 160-sample plan keeps the bits of an 8-sample one (tests/test_gpu_fullsize.py compares them); conv_winograd4 = 2 takes it.
            const long long plan_pixels = (long long)n_slices * ((long long)L.H << L.level) * ((long long)L.W << L.level);
            const long groups2 = (n_slices + 7) / 8;
            const long groups4 = plan_pixels >= kUpconv4MinPlanPixels ? (n_slices + 9) / 10 : groups2;
            const long rounds4 = (groups4 * (gh / 12) * (L.coutp / 32) + 255) / 256;
            const long rounds2 = (groups2 * (gh / 4) * ((L.coutp + 63) / 64) + 255) / 256;
            if (w4_mode == 2 || L.coutp <= 32 || (double)rounds4 * 1.35 < (double)rounds2) return CONV_CFG_WINO4_S8T12x8_N32;   // (2: whatever the fill -- parity tests on small batches)
        }
        if (L.coutp == 32 && gh % 16 == 0 && gw % 32 == 0) return CONV_CFG_WINO_T16x32_N32;
        if (L.coutp > 32 && gh % 16 == 0 && gw % 16 == 0) return CONV_CFG_WINO_T16x16_N64;
        if (L.coutp > 32 && gh % 8 == 0 && gw % 16 == 0) return CONV_CFG_WINO_S2T8x16_N64;
        if (L.coutp > 32 && gh % 4 == 0 && gw == 8) return CONV_CFG_WINO_S8T4x8_N64;
    }
    if (L.coutp > 32) {
        if (gh == 12 && gw == 8) return CONV_CFG_S2T12x8_N64;
        // 128-pixel tiles run 3 workgroups per CU (768 slots), 256-pixel tiles 2 (512 slots) with half the staging,
        // barriers and fragment reads per MFMA.  Measured on the BraTS levels (tools/layer_report.py): the big tile
        // wins where every work item stages its own input tile (one channel tile) and where the small tile's last
        // round of work items is badly filled (24x16: 2.5 rounds); it loses 3 % at 48x32 (5 full rounds).
        const int nt = (L.coutp + 63) / 64;
        const long items = (long)((gh + 7) / 8) * ((gw + 15) / 16) * n_slices * nt;
        const double fill = (double)items / (double)((items + 767) / 768 * 768);
        if (nt == 1 || fill < 0.9) {
            if (gh % 16 == 0 && gw % 16 == 0) return CONV_CFG_T16x16_N64;
            if (gh % 8 == 0 && gw % 16 == 0 && n_slices % 2 == 0) return CONV_CFG_S2T8x16_N64;
        }
        return CONV_CFG_T8x16_N64;
    }
    return (gh % 16 == 0 && gw % 16 == 0) ? CONV_CFG_T16x16_N32 : CONV_CFG_T8x16_N32;
}

static void add_unit(Plan& p, const rcu_unet_desc& d, const std::string& prefix, int cin1, int c1p, int cin2, int c2p, int cout, int level, int H, int W,
                     bool dropout, int t_src1, int t_src2, int t_out, int t_pool, bool residual_tail = false)
{
    PlanLayer L;
    L.name = prefix + ".conv2d_batch_relu.conv";
    if (d.bn) L.bn = prefix + ".conv2d_batch_relu.bn";
    L.cin1 = cin1; L.c1p = c1p; L.cin2 = cin2; L.c2p = c2p;
    L.cout = cout; L.coutp = round_up(cout, 32); L.csplit = L.coutp;
    L.H = H; L.W = W; L.relu = residual_tail ? 0 : 1;
    L.level = level; L.gh = p.level_ext[level].first; L.gw = p.level_ext[level].second;
    L.accumulate = residual_tail ? 1 : 0;
    if (dropout) {
        L.site = (int)p.sites.size();
        p.sites.push_back({prefix + ".conv2d_batch_relu.dropout", cout});
    }
    L.t_src1 = t_src1; L.t_src2 = t_src2; L.t_out = t_out; L.t_pool = t_pool;
    p.layers.push_back(L);
}

// ConvResidualBlock (common/model/unet.py:42-60): conv1x1(block input) + bias into the block's output tensor; the block's second
// unit (no ReLU) then adds its result to it.  `prefix`: the block's module path ("down_convs.0.block", "bottom_convs", ...).
static void add_residual_conv(Plan& p, const std::string& prefix, int cin1, int c1p, int cin2, int c2p, int cout, int level, int H, int W,
                              int t_src1, int t_src2, int t_out)
{
    PlanLayer L;
    L.name = prefix + ".residual";
    L.is_1x1 = 1;
    L.cin1 = cin1; L.c1p = c1p; L.cin2 = cin2; L.c2p = c2p;
    L.cout = cout; L.coutp = round_up(cout, 32); L.csplit = L.coutp;
    L.H = H; L.W = W; L.relu = 0;
    L.level = level; L.gh = p.level_ext[level].first; L.gw = p.level_ext[level].second;
    L.t_src1 = t_src1; L.t_src2 = t_src2; L.t_out = t_out;
    p.layers.push_back(L);
}

// the kernels whose store side honours ConvArgs::part (a padded level): the Winograd families but rcu_wino4_up.hip (never chosen on a padded level,
// pick_config), and rcu_first.hip
bool cfg_handles_padding(int cfg) { return conv_config_info(cfg).family.part; }

// Which activation tensors take the channel-blocked layout [N][C/8][H][W][8] (rcu_kernels.h, ConvArgs): every tensor all of whose
// producers and consumers are Winograd kernels (rcu_first.hip as a producer), except the network input, the head unit's output
// (head_kernel reads channels-last) and -- when the caller wants rcu_unet_features -- the feature tensor.  The two sources of a
// cat-free decoder unit share one layout.  rcu_unet_options.act_layout = 1 keeps everything channels-last (A/B tests).
// One level further, the paired layout (rcu_kernels.h): a blocked tensor of even width all of whose producers and consumers are F(4x4,3x3) kernels
// not in the ConvArgs::part form (conv units with or without the fused head, up-convolutions; rcu_first.hip as a producer).  The two sources of a
// cat-free unit share it, and so do a unit's output and pooled output.  act_layout = 2 stops at blocked.
bool layer_runs_part(const Plan& p, const PlanLayer& L)
{
    if (!cfg_handles_padding(L.cfg)) return false;
    const PlanTensor &tsrc = p.tensors[L.t_src1], &tout = p.tensors[L.t_out];
    const int os = L.upsample ? 2 : 1;
    const bool pool_differs = L.t_pool >= 0 && (p.tensors[L.t_pool].H != L.gh / 2 || p.tensors[L.t_pool].W != L.gw / 2);
    return tsrc.padded() || tout.H != os * L.gh || tout.W != os * L.gw || pool_differs;
}

static void assign_paired(Plan& p, const rcu_unet_options& opt)
{
    for (PlanTensor& t : p.tensors) t.paired = opt.act_layout == 0 && t.blocked && !t.padded() && t.W % 2 == 0;
    for (bool changed = true; changed;) {
        changed = false;
        auto clear = [&](int t) {
            if (t >= 0 && p.tensors[t].paired) {
                p.tensors[t].paired = false;
                changed = true;
            }
        };
        for (const PlanLayer& L : p.layers) {
            const ConvFamilyTraits& family = conv_config_info(L.cfg).family;
            const bool part = layer_runs_part(p, L);
            if (!family.reads_paired || part) {
                clear(L.t_src1);
                clear(L.t_src2);
            }
            if (!family.writes_paired || part) {
                clear(L.t_out);
                clear(L.t_pool);
            }
            if (L.t_src2 >= 0 && p.tensors[L.t_src1].paired != p.tensors[L.t_src2].paired) {
                clear(L.t_src1);
                clear(L.t_src2);
            }
            if (L.t_pool >= 0 && p.tensors[L.t_out].paired != p.tensors[L.t_pool].paired) {
                clear(L.t_out);
                clear(L.t_pool);
            }
        }
    }
}

static void assign_layouts(Plan& p, const rcu_unet_desc& d, const rcu_unet_options& opt)
{
    const bool on = opt.act_layout != 1;
    for (PlanTensor& t : p.tensors) t.blocked = on && t.cp % 8 == 0 && !t.zero_fill;
    p.tensors[p.t_input].blocked = false;
    p.tensors[p.t_head].blocked = false;
    if (d.provide_features) p.tensors[p.layers.back().t_src1].blocked = false;
    for (bool changed = true; changed;) {
        changed = false;
        auto clear = [&](int t) {
            if (t >= 0 && p.tensors[t].blocked) {
                p.tensors[t].blocked = false;
                changed = true;
            }
        };
        for (const PlanLayer& L : p.layers) {
            const ConvFamilyTraits& family = conv_config_info(L.cfg).family;
            if (!family.reads_blocked) {
                clear(L.t_src1);
                clear(L.t_src2);
            }
            if (!family.writes_blocked) {
                clear(L.t_out);
                clear(L.t_pool);
            }
            if (L.t_src2 >= 0 && p.tensors[L.t_src1].blocked != p.tensors[L.t_src2].blocked) {
                clear(L.t_src1);
                clear(L.t_src2);
            }
        }
    }
    assign_paired(p, opt);
}

// Builds layers and tensors of `p` for the level extents `level_ext` (plan_unet: the real extents first, then padded ones).
// *valid = false when a layer that touches a padded tensor got a kernel that cannot: such a plan must not run.
static int build_plan_for(const rcu_unet_desc& d, const rcu_unet_options& opt, const std::vector<std::pair<int, int>>& level_ext, Plan& p, bool* valid)
{
    const int depth = d.depth;
    p.level_ext = level_ext;
    p.layers.clear();
    p.tensors.clear();
    p.sites.clear();
    p.in_cp = round_up(d.in_channels, 8);
    p.t_input = new_tensor(p, 0, d.height, d.width, p.in_cp);
    std::vector<int> skip(depth), skip_c(depth);
    int cur = p.t_input, cur_c = d.in_channels, cur_cp = p.in_cp;
    int c = d.start_filters;
    char buf[128];
    for (int l = 0; l < depth; ++l) {
        const int H = d.height >> l, W = d.width >> l, cp = round_up(c, 32);
        const int t_tmp = new_tensor(p, l, H, W, cp), t_skip = new_tensor(p, l, H, W, cp);
        const int t_pool = new_tensor(p, l + 1, H / 2, W / 2, cp);
        snprintf(buf, sizeof buf, "down_convs.%d.block.block.0", l);
        add_unit(p, d, buf, cur_c, cur_cp, 0, 0, c, l, H, W, unit_has_dropout(d, l, true, 0), cur, -1, t_tmp, -1);
        if (d.residual) {
            snprintf(buf, sizeof buf, "down_convs.%d.block", l);
            add_residual_conv(p, buf, cur_c, cur_cp, 0, 0, c, l, H, W, cur, -1, t_skip);
        }
        snprintf(buf, sizeof buf, "down_convs.%d.block.block.1", l);
        add_unit(p, d, buf, c, cp, 0, 0, c, l, H, W, unit_has_dropout(d, l, true, 1), t_tmp, -1, t_skip, t_pool, d.residual != 0);
        skip[l] = t_skip; skip_c[l] = c;
        cur = t_pool; cur_c = c; cur_cp = cp;
        c *= 2;
    }
    {
        const int H = d.height >> depth, W = d.width >> depth, cp = round_up(c, 32);
        const int t_tmp = new_tensor(p, depth, H, W, cp), t_out = new_tensor(p, depth, H, W, cp);
        add_unit(p, d, "bottom_convs.block.0", cur_c, cur_cp, 0, 0, c, depth, H, W, unit_has_dropout(d, depth, true, 0), cur, -1,
                 t_tmp, -1);
        if (d.residual) add_residual_conv(p, "bottom_convs", cur_c, cur_cp, 0, 0, c, depth, H, W, cur, -1, t_out);
        add_unit(p, d, "bottom_convs.block.1", c, cp, 0, 0, c, depth, H, W, unit_has_dropout(d, depth, true, 1), t_tmp, -1, t_out,
                 -1, d.residual != 0);
        cur = t_out; cur_c = c; cur_cp = cp;
    }
    for (int j = 0; j < depth; ++j) {
        const int l = depth - 1 - j;
        const int H = d.height >> l, W = d.width >> l;
        const int co = cur_c / 2, cop = round_up(co, 32);
        const int t_up = new_tensor(p, l, H, W, cop), t_tmp = new_tensor(p, l, H, W, cop), t_out = new_tensor(p, l, H, W, cop);
        PlanLayer U;   // nearest x2 + conv3x3 + bias, no BN / ReLU / dropout (unet.py:105)
        snprintf(buf, sizeof buf, "up_convs.%d.upconv.1", j);
        U.name = buf;
        U.cin1 = cur_c; U.c1p = cur_cp; U.cout = co; U.coutp = cop; U.csplit = cop;
        U.H = H; U.W = W; U.upsample = 1; U.relu = 0;
        U.level = l + 1; U.gh = p.level_ext[l + 1].first; U.gw = p.level_ext[l + 1].second;   // its tiles walk the low-resolution level
        U.t_src1 = cur; U.t_out = t_up;
        if (2 * (H / 2) != H || 2 * (W / 2) != W) p.tensors[t_up].zero_fill = true;   // centre pad (unet.py:110-116)
        p.layers.push_back(U);
        // cat((up, skip), 1) -> block: K split over the two tensors (unet.py:118-119)
        snprintf(buf, sizeof buf, "up_convs.%d.block.block.0", j);
        add_unit(p, d, buf, co, cop, skip_c[l], round_up(skip_c[l], 32), co, l, H, W, unit_has_dropout(d, l, false, 0), t_up,
                 skip[l], t_tmp, -1);
        if (d.residual) {
            snprintf(buf, sizeof buf, "up_convs.%d.block", j);
            add_residual_conv(p, buf, co, cop, skip_c[l], round_up(skip_c[l], 32), co, l, H, W, t_up, skip[l], t_out);
        }
        snprintf(buf, sizeof buf, "up_convs.%d.block.block.1", j);
        add_unit(p, d, buf, co, cop, 0, 0, co, l, H, W, unit_has_dropout(d, l, false, 1), t_tmp, -1, t_out, -1, d.residual != 0);
        cur = t_out; cur_c = co; cur_cp = cop;
    }
    {   // head unit(s): conv_cls.0 [+ conv_sigma.0 stacked on the output channels] (unet.py:161-164)
        const int cp = round_up(cur_c, 32);
        p.head_cph = cp;
        p.head_cp = d.sigma_out ? 2 * cp : cp;
        // the head unit's output is read by head_kernel as [voxel][channel]: exactly the real image, whatever level 0 is allocated with
        p.t_head = new_tensor(p, -1, d.height, d.width, p.head_cp);
        add_unit(p, d, "conv_cls.0", cur_c, cur_cp, 0, 0, cur_c, 0, d.height, d.width, d.has_dropout != 0, cur, -1, p.t_head,
                 -1);
        PlanLayer& L = p.layers.back();
        if (d.sigma_out) {
            L.name2 = "conv_sigma.0.conv2d_batch_relu.conv";
            if (d.bn) L.bn2 = "conv_sigma.0.conv2d_batch_relu.bn";
            L.csplit = cp;
            L.coutp = 2 * cp;
            if (d.has_dropout) {
                L.site2 = (int)p.sites.size();
                p.sites.push_back({"conv_sigma.0.conv2d_batch_relu.dropout", cur_c});
            }
        }
    }
    p.t_features = -1;
    if (d.provide_features && p.tensors[p.layers.back().t_src1].padded()) {
        // rcu_unet_features hands the input of conv_cls.0 out as [voxel][channel]: on a padded level 0 a compact copy is made behind the forward
        const PlanTensor f = p.tensors[p.layers.back().t_src1];
        p.t_features = new_tensor(p, -1, f.Hr, f.Wr, f.cp);
    }
    p.site_offset.assign(p.sites.size() + 1, 0);
    for (size_t s = 0; s < p.sites.size(); ++s) p.site_offset[s + 1] = p.site_offset[s] + p.sites[s].second;
    p.mask_floats = p.site_offset.back();
    if (valid) *valid = true;
    for (PlanLayer& L : p.layers) {
        const PlanTensor& to = p.tensors[L.t_out];
        L.cfg = pick_config(L, d.max_batch, opt, to.H, to.W);
        const ConvConfigInfo& ci = conv_config_info(L.cfg);
        if ((L.c1p % ci.KC) != 0 || (L.c2p % ci.KC) != 0)
            return report_error(RCU_ERR_INVALID, "internal: channel chunking does not divide for layer " + L.name);
        L.NT = (L.coutp + ci.BN - 1) / ci.BN;
        // a padded tensor may only be touched by a kernel that keeps its zeros: read as a tile grid and written by the Winograd families /
        // rcu_first.hip -- or written by a direct up-convolution, which places its image in a larger tensor anyway (the centre pad), or as
        // the pooled output of a direct conv unit (it writes the real pooled pixels at the tensor's own pitch)
        const bool src_padded = p.tensors[L.t_src1].padded() && L.t_src1 != p.t_input;
        const bool first_reads_caller = L.t_src1 == p.t_input && p.tensors[L.t_src1].padded();
        const bool out_padded = to.padded() && !(L.upsample && !cfg_handles_padding(L.cfg) && !p.tensors[L.t_src1].padded());
        if ((src_padded || first_reads_caller || out_padded) && !cfg_handles_padding(L.cfg) && valid) *valid = false;
    }
    assign_layouts(p, d, opt);
    return RCU_OK;
}

// pixels of the grid a layer's tiles walk, whole tiles counted (an up-convolution: the low-resolution grid)
static double walked_pixels(const PlanLayer& L, const ConvConfigInfo& ci)
{
    const double tiles = (double)((L.gh + ci.TH - 1) / ci.TH) * ((L.gw + ci.TW - 1) / ci.TW);
    return tiles * ci.TH * ci.TW;
}

// Rough time of a plan's conv stack per slice, arbitrary units: multiplications the layer's kernel executes on whole tiles of the grid it walks
// / the executed fraction of the matrix peak the kernel family has measured at (the direct kernels on the native BraTS
// volume: profiles/r06_layer_report_native_155_nopad.txt, 0.73-0.80).  It only has to rank "pad the level to whole Winograd tiles" against
// "keep the real extent on the direct kernels" and one padding against another.
static double plan_cost(const Plan& p)
{
    double total = 0.0;
    for (const PlanLayer& L : p.layers) {
        const ConvConfigInfo& ci = conv_config_info(L.cfg);
        const double px = walked_pixels(L, ci);
        const double kn = (double)(L.c1p + L.c2p) * (double)(L.NT * ci.BN);
        double eff = 0.0;
        switch (ci.family.id) {
            case ConvFamily::First: eff = 0.25; break;                                  // a write stream, not a matrix kernel
            case ConvFamily::Wino4: eff = (L.c1p + L.c2p) <= 32 ? 0.45 : 0.58; break;
            case ConvFamily::Wino2Up: eff = 0.72; break;
            case ConvFamily::Wino4Up: eff = 0.70; break;                                // measured 0.63-0.76
            case ConvFamily::Wino2: eff = 0.62; break;
            case ConvFamily::DirectUp: eff = 0.72; break;
            case ConvFamily::Direct: eff = 0.75; break;
        }
        total += px * kn * (ci.family.mults * ci.slot_factor) / eff;
    }
    return total;
}

bool head_fusable(const Plan& p, const rcu_unet_desc& d)
{
    const PlanLayer& last = p.layers.back();
    return conv_config_info(last.cfg).head_cfg >= 0 && d.nb_classes == 2 && last.name2.empty() && p.head_cph == 32;
}

void plan_layer_info(const Plan& p, const rcu_unet_desc& d, int layer, rcu_layer_info* out)
{
    const PlanLayer& L = p.layers[layer];
    std::memset(out, 0, sizeof *out);
    std::snprintf(out->name, sizeof out->name, "%s", L.name.c_str());
    std::snprintf(out->kernel, sizeof out->kernel, "%s", conv_config_info(L.cfg).kernel_name);
    out->cin = L.cin1 + L.cin2;
    out->cout = L.name2.empty() ? L.cout : 2 * L.cout;
    out->height = L.H; out->width = L.W;
    out->grid_height = L.gh; out->grid_width = L.gw;
    out->upsample = L.upsample; out->pooled = L.t_pool >= 0; out->dual_source = L.t_src2 >= 0;
    out->head_fusable = (layer + 1 == (int)p.layers.size() && head_fusable(p, d)) ? 1 : 0;
    // an up-convolution works on the up-sampled grid, which a centre pad leaves smaller than the skip tensor it is padded to
    out->flops_per_slice = 2.0 * out->cin * out->cout * (L.is_1x1 ? 1.0 : 9.0) * (L.upsample ? 4.0 * (L.H / 2) * (L.W / 2) : (double)L.H * L.W);
    // executed on the matrix pipe: padded K and N, full tiles of the grid the tiles walk (the allocated extent of the level: rcu_layer_info.grid_height /
    // grid_width), the family's multiplications per pixel of it (ConvFamilyTraits::mults: what plan_cost counts), every tile slot
    const ConvConfigInfo& ci = conv_config_info(L.cfg);
    const double ncols = (double)L.NT * ci.BN;
    // (rcu_first.hip: K = 4 channels per tap unless more than four are real)
    const int k = ci.family.id == ConvFamily::First ? (L.cin1 > 4 ? 8 : 4) : L.c1p + L.c2p;
    out->mfma_flops_per_slice = 2.0 * k * ncols * ci.family.mults * walked_pixels(L, ci) * ci.slot_factor;
}

// Allocated extent of every level.  A Winograd kernel takes whole tiles; where the real extent of a level (H >> l) x (W >> l) is not a
// whole number of them -- the reference's BraTS slices are 240 x 240 (levels 240, 120, 60, 30, 15: scripts/create_brats18_dataset.py:53-72 never
// crops), ISIC's 192 x 256 ends in a 12 x 16 level (scripts/prepare_isic_data.py:29-30) -- the level's tensors are ALLOCATED with a padded extent,
// the padding holds zeros that no kernel writes (ConvArgs::part), and the level runs on the Winograd kernels instead of the direct ones: 2.25 x
// (1 + padding) instead of 9 multiplications per pixel.  Every level chooses for itself: a pooled output and an up-convolution carry the extents
// of the tensors on both sides.  The choice minimises plan_cost over a small set of roundings per axis; a level keeps its real extent where
// nothing is gained (whole tiles fit: the benchmark's 192 x 128) or where a layer of the level has no kernel that keeps the zeros (residual
// blocks' adding units, feature taps).
// The search holds two plans: the best so far and the candidate being tried, which takes the best's place (a swap, no copy) when it is valid and cheaper.
int plan_unet(const rcu_unet_desc& d, const rcu_unet_options& opt, Plan* out)
{
    std::vector<std::pair<int, int>> ext(d.depth + 1);
    for (int l = 0; l <= d.depth; ++l) ext[l] = {d.height >> l, d.width >> l};
    Plan& best = *out;
    bool valid = true;
    int rc = build_plan_for(d, opt, ext, best, &valid);
    if (rc != RCU_OK || opt.pad_levels == 0 || opt.conv_winograd == 0) return rc;
    double best_cost = plan_cost(best);
    Plan cand;
    static const int kRound[] = {4, 8, 12, 16, 32};
    for (int sweep = 0; sweep < 2; ++sweep)
        for (int l = 0; l <= d.depth; ++l) {
            const int Hl = d.height >> l, Wl = d.width >> l;
            for (int rh : kRound)
                for (int rw : kRound) {
                    ext = best.level_ext;
                    ext[l] = {round_up(Hl, rh), round_up(Wl, rw)};
                    if (ext[l] == best.level_ext[l] || (rw == 12)) continue;
                    rc = build_plan_for(d, opt, ext, cand, &valid);
                    if (rc != RCU_OK) return rc;
                    const double cost = plan_cost(cand);
                    if (valid && cost < best_cost * 0.999) {
                        best_cost = cost;
                        std::swap(best, cand);
                    }
                }
        }
    return RCU_OK;
}

}  // namespace rcu
