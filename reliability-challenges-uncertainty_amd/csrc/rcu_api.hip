// C ABI of librcu_hip.so (see include/rcu.h): the U-Net handle -- a Plan (rcu_plan.h) plus its device state: BN folding, weight packing,
// workspace -- and its forwards.  The other entry points live next to their kernels.
#include "../../include/rcu.h"
#include "rcu_kernels.h"
#include "rcu_plan.h"
#include "rcu_wpack.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

using namespace rcu;

static thread_local std::string g_last_error;

static int fail(int code, const std::string& msg)
{
    g_last_error = msg;
    return code;
}
int rcu::report_error(int code, const std::string& msg) { return fail(code, msg); }
static int hip_fail(hipError_t e, const char* what)
{
    return fail(RCU_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define RCU_HIP(call)                                      \
    do {                                                   \
        hipError_t e_ = (call);                            \
        if (e_ != hipSuccess) return hip_fail(e_, #call);  \
    } while (0)

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
// what rcu_unet_finalize_weights uploads for the plan layer of the same index
struct LayerDevice {
    float *wpack = nullptr, *alpha = nullptr, *betab = nullptr, *beta = nullptr;
    size_t wpack_floats = 0;
};

// The activation tensors of a plan: owned by the handle that allocated them, shared (shared_ptr) with the handles created with
// that handle as their workspace donor (rcu_unet_create_with); freed with the last user.
struct Workspace {
    std::vector<float*> dev;      // one allocation per plan tensor
    std::vector<size_t> bytes;
    int max_batch = 0;
    ~Workspace()
    {
        for (float* p : dev)
            if (p) (void)hipFree(p);
    }
};

struct rcu_unet {
    rcu_unet_desc d{};
    rcu_unet_options opt{};
    Plan plan;
    std::vector<LayerDevice> dev;   // [plan.layers.size()]
    std::shared_ptr<Workspace> ws;
    bool ws_borrowed = false;
    std::map<std::string, std::vector<float>> host_weights;
    float *w_cls = nullptr, *b_cls = nullptr, *w_sig = nullptr, *b_sig = nullptr;
    double temperature = 1.0;  // rcu_unet_set_temperature: conv_cls.1 is packed divided by it
    bool finalized = false;
    bool plan_only = false;   // rcu_unet_plan: no workspace -- the handle can be inspected, never run
    bool head_input_kept = false;   // the last forward took the separate head kernel: act[plan.t_head] is conv_cls.0's output (rcu_unet_head_features)
    int64_t workspace_bytes = 0;
    std::vector<void*> allocs;
    // optional per-layer timing with HIP events on the caller's stream (rcu_unet_profile_*)
    std::vector<hipEvent_t> prof_events;   // [max_forwards][slots], slots = layers + 3
    int prof_capacity = 0, prof_used = 0;
};

static int prof_slots(const rcu_unet* h) { return (int)h->plan.layers.size() + 3; }

extern "C" const char* rcu_last_error(void) { return g_last_error.c_str(); }
extern "C" const char* rcu_version(void) { return "librcu_hip 0.1.0 gfx950"; }

extern "C" void rcu_unet_default_options(rcu_unet_options* opts)
{
    if (!opts) return;
    std::memset(opts, 0, sizeof *opts);
    opts->conv_winograd = 1;
    opts->conv_winograd4 = 1;
    opts->conv_first = 1;
    opts->act_layout = 0;
    opts->fuse_head = 1;
    opts->head_winograd4 = 1;
    opts->pad_levels = 1;
    opts->upconv_winograd4 = 1;
}

// desc / options checks + the plan (layers, tensors, level extents); no device memory
static int make_plan(const rcu_unet_desc* desc, const rcu_unet_options* opts, const rcu_unet* donor, rcu_unet** out)
{
    if (!desc || !out) return fail(RCU_ERR_INVALID, "rcu_unet_create: null argument");
    const rcu_unet_desc& d = *desc;
    if (d.nb_classes < 1 || d.nb_classes > MAX_CLASSES) return fail(RCU_ERR_INVALID, "nb_classes must be in 1..8");
    if (d.in_channels < 1 || d.depth < 1 || d.depth > 8 || d.start_filters < 1 || d.max_batch < 1)
        return fail(RCU_ERR_INVALID, "rcu_unet_create: bad in_channels / depth / start_filters / max_batch");
    if (d.in_channels > 8 && d.in_channels % 32 != 0)
        return fail(RCU_ERR_INVALID, "in_channels must be <= 8 or a multiple of 32");
    const int div = 1 << d.depth;
    if (d.height < div || d.width < div)
        return fail(RCU_ERR_INVALID, "height and width must be at least 2^depth (one pixel at the bottom level)");
    rcu_unet_options o;
    rcu_unet_default_options(&o);
    if (opts) {
        o = *opts;
        if ((o.conv_winograd | 1) != 1 || (o.conv_winograd4 < 0 || o.conv_winograd4 > 3) ||
            (o.conv_first | 1) != 1 || o.act_layout < 0 || o.act_layout > 2 || (o.fuse_head | 1) != 1 || (o.head_winograd4 | 1) != 1 || (o.pad_levels | 1) != 1 ||
            (o.upconv_winograd4 < 0 || o.upconv_winograd4 > 2))
            return fail(RCU_ERR_INVALID, "rcu_unet_create_with: bad rcu_unet_options value");
    }
    rcu_unet* h = new rcu_unet();
    h->d = d;
    h->opt = o;
    // A borrower is planned for the DONOR's batch: the planner's choices (kernel family per layer, tensor layouts) depend on max_batch, and
    // two plans that share one workspace must agree on every tensor -- identical by construction instead of by luck
    if (donor && donor->ws && donor->ws->max_batch >= d.max_batch) h->d.max_batch = donor->ws->max_batch;
    int rc = plan_unet(h->d, h->opt, &h->plan);
    if (rc != RCU_OK) {
        delete h;
        return rc;
    }
    h->dev.resize(h->plan.layers.size());
    *out = h;
    return RCU_OK;
}

extern "C" int rcu_unet_plan(const rcu_unet_desc* desc, const rcu_unet_options* opts, rcu_unet** out)
{
    int rc = make_plan(desc, opts, nullptr, out);
    if (rc == RCU_OK) (*out)->plan_only = true;
    return rc;
}

extern "C" int rcu_unet_create_with(const rcu_unet_desc* desc, const rcu_unet_options* opts, rcu_unet* donor, rcu_unet** out)
{
    rcu_unet* h = nullptr;
    int rc = make_plan(desc, opts, donor, &h);
    if (rc != RCU_OK) return rc;
    const rcu_unet_desc& d = *desc;
    // 32-bit element offsets inside the conv kernel
    for (const PlanTensor& t : h->plan.tensors)
        if (t.floats_per_slice * (size_t)h->d.max_batch >= (size_t)1 << 31) {
            delete h;
            return fail(RCU_ERR_INVALID, "max_batch too large: an activation tensor would exceed 2^31 elements");
        }
    if (donor) {
        // the donor's plan must hold the same tensors (same shapes, same layouts, same never-written borders) for at least this batch
        if (!(donor->ws && donor->plan == h->plan && donor->ws->max_batch >= d.max_batch)) {
            delete h;
            return fail(RCU_ERR_INVALID, "rcu_unet_create_with: the workspace donor's plan differs (shape, options) or is sized for a smaller batch");
        }
        h->ws = donor->ws;
        h->ws_borrowed = true;
        *out = h;
        return RCU_OK;
    }
    h->ws = std::make_shared<Workspace>();
    h->ws->max_batch = d.max_batch;
    bool zeroed = false;
    for (const PlanTensor& t : h->plan.tensors) {
        const size_t bytes = t.floats_per_slice * (size_t)d.max_batch * sizeof(float);
        float* dev = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev), bytes);
        if (e != hipSuccess) {
            rcu_unet_destroy(h);
            return hip_fail(e, "hipMalloc(activation workspace)");
        }
        h->ws->dev.push_back(dev);
        h->ws->bytes.push_back(bytes);
        h->workspace_bytes += (int64_t)bytes;
        if (t.zero_fill || t.padded()) {   // pixels no kernel ever writes and every reader takes for the conv's zero padding
            e = hipMemset(dev, 0, bytes);
            if (e != hipSuccess) {
                rcu_unet_destroy(h);
                return hip_fail(e, "hipMemset(centre-pad border / level padding)");
            }
            zeroed = true;
        }
    }
    if (zeroed) {
        // a memset of device memory may return before it has run, and the forwards come on the caller's (non-blocking) streams, which the null
        // stream does not order: the zeros are in place before the handle is handed out
        hipError_t e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) {
            rcu_unet_destroy(h);
            return hip_fail(e, "hipStreamSynchronize(level padding)");
        }
    }
    *out = h;
    return RCU_OK;
}

extern "C" int rcu_unet_create(const rcu_unet_desc* desc, rcu_unet** out) { return rcu_unet_create_with(desc, nullptr, nullptr, out); }

extern "C" int rcu_unet_set_fuse_head(rcu_unet* h, int on)
{
    if (!h) return fail(RCU_ERR_INVALID, "rcu_unet_set_fuse_head: null handle");
    h->opt.fuse_head = on ? 1 : 0;
    return RCU_OK;
}

extern "C" int rcu_unet_set_temperature(rcu_unet* h, double temperature)
{
    if (!h) return fail(RCU_ERR_INVALID, "rcu_unet_set_temperature: null handle");
    if (!std::isfinite(temperature) || !(temperature > 0.0))
        return fail(RCU_ERR_INVALID, "rcu_unet_set_temperature: the temperature must be finite and > 0");
    if (h->d.sigma_out)
        return fail(RCU_ERR_INVALID, "rcu_unet_set_temperature: a sigma_out model's sigma is in logit units; scaling the logits alone is not defined");
    if (h->finalized) return fail(RCU_ERR_STATE, "rcu_unet_set_temperature after rcu_unet_finalize_weights");
    h->temperature = temperature;
    return RCU_OK;
}

extern "C" int rcu_unet_destroy(rcu_unet* h)
{
    if (!h) return RCU_OK;
    for (void* p : h->allocs) (void)hipFree(p);     // packed weights, epilogue constants
    for (hipEvent_t e : h->prof_events) (void)hipEventDestroy(e);
    delete h;                                       // drops its reference to the activation workspace
    return RCU_OK;
}

extern "C" int64_t rcu_unet_workspace_bytes(const rcu_unet* h) { return h ? h->workspace_bytes : 0; }
extern "C" int rcu_unet_num_dropout_sites(const rcu_unet* h) { return h ? (int)h->plan.sites.size() : 0; }
extern "C" int rcu_unet_dropout_site_channels(const rcu_unet* h, int site)
{
    if (!h || site < 0 || site >= (int)h->plan.sites.size()) return fail(RCU_ERR_INVALID, "bad dropout site index");
    return h->plan.sites[site].second;
}
extern "C" const char* rcu_unet_dropout_site_name(const rcu_unet* h, int site)
{
    if (!h || site < 0 || site >= (int)h->plan.sites.size()) return "";
    return h->plan.sites[site].first.c_str();
}
extern "C" int rcu_unet_mask_floats_per_sample(const rcu_unet* h) { return h ? h->plan.mask_floats : 0; }

extern "C" int rcu_unet_load_weight(rcu_unet* h, const char* name, const float* data, size_t count)
{
    if (!h || !name || (!data && count)) return fail(RCU_ERR_INVALID, "rcu_unet_load_weight: null argument");
    std::string key(name);
    if (key.rfind("module.", 0) == 0) key = key.substr(7);
    h->host_weights[key].assign(data, data + count);
    h->finalized = false;
    return RCU_OK;
}

static int get_weight(rcu_unet* h, const std::string& key, size_t count, const std::vector<float>** out)
{
    auto it = h->host_weights.find(key);
    if (it == h->host_weights.end()) return fail(RCU_ERR_WEIGHTS, "missing weight tensor '" + key + "'");
    if (it->second.size() != count)
        return fail(RCU_ERR_WEIGHTS, "weight tensor '" + key + "' has " + std::to_string(it->second.size()) +
                                         " elements, expected " + std::to_string(count));
    *out = &it->second;
    return RCU_OK;
}

template <typename T>
static int upload(rcu_unet* h, const std::vector<T>& host, T** dev)
{
    RCU_HIP(hipMalloc(reinterpret_cast<void**>(dev), host.size() * sizeof(T)));
    h->allocs.push_back(*dev);
    h->workspace_bytes += (int64_t)(host.size() * sizeof(T));
    RCU_HIP(hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return RCU_OK;
}

// Fold one conv (+ optional BN) into (packed weights, alpha, betab, beta) at output-channel offset co0.
static int fold_conv(rcu_unet* h, const PlanLayer& L, const std::string& conv, const std::string& bn, int co0,
                     std::vector<float>& wpack, std::vector<float>& alpha, std::vector<float>& betab,
                     std::vector<float>& beta)
{
    const int cin = L.cin1 + L.cin2;
    const std::vector<float>*w, *b;
    std::vector<float> w_centre;
    int rc;
    if (L.is_1x1) {   // [cout][cin][1][1] -> [cout][cin][3][3] with the centre tap set
        if ((rc = get_weight(h, conv + ".weight", (size_t)L.cout * cin, &w))) return rc;
        w_centre.assign((size_t)L.cout * cin * 9, 0.f);
        for (size_t i = 0; i < (size_t)L.cout * cin; ++i) w_centre[i * 9 + 4] = (*w)[i];
        w = &w_centre;
    } else {
        rc = get_weight(h, conv + ".weight", (size_t)L.cout * cin * 9, &w);
    }
    if (rc) return rc;
    rc = get_weight(h, conv + ".bias", (size_t)L.cout, &b);
    if (rc) return rc;
    const std::vector<float>*g = nullptr, *bt = nullptr, *mu = nullptr, *var = nullptr;
    if (!bn.empty()) {
        if ((rc = get_weight(h, bn + ".weight", L.cout, &g))) return rc;
        if ((rc = get_weight(h, bn + ".bias", L.cout, &bt))) return rc;
        if ((rc = get_weight(h, bn + ".running_mean", L.cout, &mu))) return rc;
        if ((rc = get_weight(h, bn + ".running_var", L.cout, &var))) return rc;
    }
    for (int co = 0; co < L.cout; ++co) {
        float A = 1.f, B = 0.f;
        if (g) {
            A = (*g)[co] / std::sqrt((*var)[co] + 1e-5f);
            B = (*bt)[co] - A * (*mu)[co];
        }
        alpha[co0 + co] = A;
        betab[co0 + co] = A * (*b)[co];
        beta[co0 + co] = B;
    }
    pack_conv_weights(wpack_kernel(conv_config_info(L.cfg)), WpackLayer{L.cin1, L.c1p, L.cin2, L.cout, L.NT, L.upsample}, w->data(), co0, wpack.data());
    return RCU_OK;
}

extern "C" int rcu_unet_finalize_weights(rcu_unet* h)
{
    if (!h) return fail(RCU_ERR_INVALID, "null handle");
    if (h->plan_only) return fail(RCU_ERR_STATE, "rcu_unet_finalize_weights: the handle is a plan without a workspace (rcu_unet_plan)");
    if (h->finalized) return RCU_OK;
    for (size_t li = 0; li < h->plan.layers.size(); ++li) {
        const PlanLayer& L = h->plan.layers[li];
        LayerDevice& D = h->dev[li];
        const ConvConfigInfo& ci = conv_config_info(L.cfg);
        D.wpack_floats = wpack_floats(wpack_kernel(ci), L.c1p + L.c2p, L.NT);
        std::vector<float> wpack(D.wpack_floats, 0.f);
        const int cpad = L.NT * ci.BN;
        std::vector<float> alpha(cpad, 0.f), betab(cpad, 0.f), beta(cpad, 0.f);
        int rc = fold_conv(h, L, L.name, L.bn, 0, wpack, alpha, betab, beta);
        if (rc) return rc;
        if (!L.name2.empty()) {
            rc = fold_conv(h, L, L.name2, L.bn2, L.csplit, wpack, alpha, betab, beta);
            if (rc) return rc;
        }
        if ((rc = upload(h, wpack, &D.wpack))) return rc;
        if ((rc = upload(h, alpha, &D.alpha))) return rc;
        if ((rc = upload(h, betab, &D.betab))) return rc;
        if ((rc = upload(h, beta, &D.beta))) return rc;
    }
    // 1x1 heads (unet.py:161, 164): [C][CPh] zero padded
    const int C = h->d.nb_classes, cph = h->plan.head_cph, creal = h->plan.layers.back().cout;
    // `temperature` (rcu_unet_set_temperature): the classifier divided by T, (float)((double)w / T) -- T = 1 leaves every value as it is
    auto head = [&](const std::string& key, float** w_dev, float** b_dev, double temperature) -> int {
        const std::vector<float>*w, *b;
        int rc = get_weight(h, key + ".weight", (size_t)C * creal, &w);
        if (rc) return rc;
        if ((rc = get_weight(h, key + ".bias", (size_t)C, &b))) return rc;
        auto scaled = [temperature](float v) { return temperature == 1.0 ? v : (float)((double)v / temperature); };
        std::vector<float> wp((size_t)C * cph, 0.f);
        for (int c = 0; c < C; ++c)
            for (int k = 0; k < creal; ++k) wp[(size_t)c * cph + k] = scaled((*w)[(size_t)c * creal + k]);
        if ((rc = upload(h, wp, w_dev))) return rc;
        std::vector<float> bp(b->size());
        for (size_t c = 0; c < b->size(); ++c) bp[c] = scaled((*b)[c]);
        return upload(h, bp, b_dev);
    };
    int rc = head("conv_cls.1", &h->w_cls, &h->b_cls, h->temperature);
    if (rc) return rc;
    if (h->d.sigma_out && (rc = head("conv_sigma.1", &h->w_sig, &h->b_sig, 1.0))) return rc;
    h->host_weights.clear();
    h->finalized = true;
    return RCU_OK;
}

// `head`: when set (conv_cls.0 on the 32-cout Winograd tile, two classes), the 1x1 classifier + softmax + statistics run in
// the layer's epilogue and its output tensor is not written (rcu_wino.hip, wino_epilogue_head).
struct FusedHead {
    float* logits;
    void* stats;
    int flags;
    int passes;   // pass group: the batch holds `passes` x (n / passes) samples, all adding into the statistics of n / passes images
};

static int run_layer(rcu_unet* h, int layer, int n, const float* masks, hipStream_t stream, const FusedHead* head = nullptr,
                     const float* x_nchw = nullptr, int n_images = 0)
{
    const Plan& p = h->plan;
    const PlanLayer& L = p.layers[layer];
    const LayerDevice& D = h->dev[layer];
    const std::vector<float*>& act = h->ws->dev;   // the activation tensors, by plan tensor index
    const ConvConfigInfo& ci = conv_config_info(L.cfg);
    ConvArgs a{};
    a.src1 = act[L.t_src1];
    a.src2 = L.t_src2 >= 0 ? act[L.t_src2] : nullptr;
    a.wpack = D.wpack; a.alpha = D.alpha; a.betab = D.betab; a.beta = D.beta;
    a.mask = (masks && L.site >= 0) ? masks + (size_t)n * p.site_offset[L.site] : nullptr;
    a.mask2 = (masks && L.site2 >= 0) ? masks + (size_t)n * p.site_offset[L.site2] : nullptr;
    a.out = act[L.t_out];
    a.pooled = L.t_pool >= 0 ? act[L.t_pool] : nullptr;
    const int gh = L.gh, gw = L.gw;   // tile grid = the (allocated) input grid
    a.N = n; a.H = gh; a.W = gw;
    const PlanTensor& tsrc = p.tensors[L.t_src1];
    const PlanTensor& tout = p.tensors[L.t_out];
    if (cfg_handles_padding(L.cfg)) {
        // padded level on either side (ConvArgs::part): the tiles walk the allocated grid, the stores keep to the real image, the output and
        // pooled tensors have the extents of their own levels (the head unit's output: exactly the real image)
        if (layer_runs_part(p, L)) {
            a.part = 1;
            a.Hr = L.upsample ? 2 * (L.H / 2) : L.H;
            a.Wr = L.upsample ? 2 * (L.W / 2) : L.W;
            a.out_H = tout.H; a.out_W = tout.W;
            if (L.t_pool >= 0) { a.pool_H = p.tensors[L.t_pool].H; a.pool_W = p.tensors[L.t_pool].W; }
        }
    } else if (L.t_pool >= 0 && p.tensors[L.t_pool].padded()) {
        a.pool_H = p.tensors[L.t_pool].H; a.pool_W = p.tensors[L.t_pool].W;   // a direct unit pooling into a padded level
    } else if (L.upsample && (2 * gh != tout.H || 2 * gw != tout.W)) {
        // the direct up-convolution places its 2 gh x 2 gw image in a larger tensor: the reference's centre pad
        // F.pad(up, (dw // 2, dw - dw // 2, dh // 2, dh - dh // 2)) (unet.py:110-116), and / or a padded level around it
        a.out_H = tout.H; a.out_W = tout.W;
        a.out_y0 = (L.H - 2 * gh) / 2; a.out_x0 = (L.W - 2 * gw) / 2;
    }
    a.C1 = L.c1p; a.C2 = L.c2p; a.CoutP = L.coutp;
    a.cin_real = L.cin1;
    a.x_nchw = ci.family.id == ConvFamily::First ? x_nchw : nullptr;
    a.n_images = n_images;
    a.Cmask = L.cout; a.Csplit = L.csplit; a.Cmask2 = L.cout;
    a.relu = L.relu;
    a.accumulate = L.accumulate;
    a.tiles_y = (gh + ci.TH - 1) / ci.TH;
    a.tiles_x = (gw + ci.TW - 1) / ci.TW;
    a.slice_groups = (n + ci.TS - 1) / ci.TS;
    a.NT = L.NT;
    a.NTW_total = L.NT * ci.family.weight_sets;
    {
        const unsigned long long items = (unsigned long long)a.NTW_total * a.tiles_x * a.tiles_y * a.slice_groups;
        auto magic = [&](int d) -> uint32_t {
            return (d > 1 && items * (unsigned long long)d < (1ull << 32)) ? (uint32_t)(((1ull << 32) + d - 1) / d) : 0u;
        };
        a.magic_ntw = magic(a.NTW_total); a.magic_tx = magic(a.tiles_x); a.magic_ty = magic(a.tiles_y);
    }
    {
        auto strides = [](const PlanTensor& t, uint32_t& pix_bytes, uint32_t& chunk_bytes) {
            pix_bytes = t.blocked ? 32u : (uint32_t)t.cp * 4u;
            chunk_bytes = t.blocked ? (uint32_t)(t.H * t.W) * 32u : 32u;
        };
        strides(tsrc, a.in_pix_bytes, a.in_chunk_bytes);
        strides(tout, a.out_pix_bytes, a.out_chunk_bytes);
        if (L.t_pool >= 0) strides(p.tensors[L.t_pool], a.pool_pix_bytes, a.pool_chunk_bytes);
        // a paired tensor has the strides of the blocked one (assign_layouts: both sources alike, output and pooled output alike)
        a.in_paired = tsrc.paired ? 1 : 0;
        a.out_paired = tout.paired ? 1 : 0;
    }
    a.src1_bytes = (uint32_t)std::min<size_t>(tsrc.floats_per_slice * (size_t)n * 4, 0xFFFFFFFFu);
    a.src2_bytes = L.t_src2 >= 0 ? (uint32_t)std::min<size_t>(p.tensors[L.t_src2].floats_per_slice * (size_t)n * 4, 0xFFFFFFFFu) : 0u;
    a.wpack_bytes = (uint32_t)std::min<size_t>(D.wpack_floats * 4, 0xFFFFFFFFu);
    int cfg = L.cfg;
    if (head) {
        cfg = ci.head_cfg;   // (forward_impl: head_fusable)
        a.head_w = h->w_cls; a.head_b = h->b_cls;
        a.head_logits = head->logits; a.head_stats = head->stats; a.head_flags = head->flags;
        a.head_passes = head->passes;
        a.head_images = n / head->passes;
        a.head_V = (size_t)a.head_images * L.H * L.W;
    }
    RCU_HIP(launch_conv3x3(cfg, a, stream));
    return RCU_OK;
}

// `passes` > 1 (statistics only): the n images run as ONE batch of n * passes samples -- sample t * n + i is image i
// under the mask rows [site][t * n + i] -- and the head adds all passes into the n statistics entries.
// test-time logit sampling in the head (rcu_unet_forward_sample_sigma_passes): keys[t] of pass t, S samples per voxel
struct HeadSampling {
    const uint64_t* keys;
    uint64_t first_sample;
    int samples;
};

// sample votes in the head (rcu_unet_forward_accumulate_votes): bit bits[t] of the plane for pass t
struct HeadVotes {
    uint32_t* plane;
    int n_words;
    const int32_t* bits;
};

static int forward_impl(rcu_unet* h, const float* x, int n, const float* masks, float* logits, float* sigma, void* stats,
                        int flags, hipStream_t stream, int passes = 1, float* sigma_sum = nullptr, int sigma_log = 0,
                        const HeadSampling* sampling = nullptr, const HeadVotes* votes = nullptr)
{
    if (!h || !x) return fail(RCU_ERR_INVALID, "rcu_unet_forward: null argument");
    if (!h->finalized) return fail(RCU_ERR_STATE, "rcu_unet_forward before rcu_unet_finalize_weights");
    if (n < 1 || passes < 1 || (long)n * passes > h->d.max_batch)
        return fail(RCU_ERR_INVALID, "batch size (times passes) outside 1..max_batch");
    if (passes > 1 && (!stats || logits || sigma)) return fail(RCU_ERR_INVALID, "pass groups only feed the statistics");
    const int n_one = n;
    n *= passes;
    if ((sigma || sigma_sum) && !h->d.sigma_out) return fail(RCU_ERR_INVALID, "sigma output requested from a model without sigma_out");
    h->head_input_kept = false;
    const Plan& p = h->plan;
    const std::vector<float*>& act = h->ws->dev;
    hipEvent_t* ev = nullptr;
    if (h->prof_capacity > 0 && h->prof_used < h->prof_capacity)
        ev = h->prof_events.data() + (size_t)(h->prof_used++) * prof_slots(h);
    if (ev) RCU_HIP(hipEventRecord(*ev++, stream));
    // the first-layer kernel reads the caller's NCHW input itself; every other first layer wants the channels-last copy
    const bool direct_input = conv_config_info(p.layers.front().cfg).family.id == ConvFamily::First;
    if (!direct_input)
        RCU_HIP(launch_pack_input(x, act[p.t_input], n_one, h->d.in_channels, p.in_cp, h->d.height, h->d.width,
                                  p.tensors[p.t_input].H, p.tensors[p.t_input].W, passes, stream));
    if (ev) RCU_HIP(hipEventRecord(*ev++, stream));
    // conv_cls.0 and the classifier as one kernel where the shapes allow (the shipped configurations; rcu_unet_options.fuse_head = 0 /
    // rcu_unet_set_fuse_head keep them apart): two classes, no sigma twin, 32-cout Winograd tile; the passes of a pass group run back to back on the
    // workgroup that owns the tile, so their read-modify-writes of the statistics are ordered (pass 0 first, as head_kernel adds them)
    const int last = (int)p.layers.size() - 1;
    const bool fuse = head_fusable(p, h->d) && sigma == nullptr && (logits != nullptr || stats != nullptr) && h->opt.fuse_head != 0 && sampling == nullptr &&
                      votes == nullptr;      // (the voting head is the separate kernel: same statistics bits, fused == unfused)
    for (int layer = 0; layer <= last; ++layer) {
        const FusedHead fh{logits, stats, flags, passes};
        int rc = run_layer(h, layer, n, masks, stream, (fuse && layer == last) ? &fh : nullptr, direct_input ? x : nullptr, n_one);
        if (rc) return rc;
        if (ev) RCU_HIP(hipEventRecord(*ev++, stream));
    }
    if (p.t_features >= 0) {   // (provide_features plans never fuse the head away from this point: the copy runs behind the last conv unit either way)
        const int t_f = p.layers.back().t_src1;
        const PlanTensor& f = p.tensors[t_f];
        RCU_HIP(launch_crop_nhwc(act[t_f], act[p.t_features], n, f.Hr, f.Wr, f.H, f.W, f.cp, stream));
    }
    if (fuse) {
        if (ev) RCU_HIP(hipEventRecord(*ev++, stream));
        return RCU_OK;
    }
    HeadArgs a{};
    a.act = act[p.t_head];
    a.w_cls = h->w_cls; a.b_cls = h->b_cls; a.w_sig = h->w_sig; a.b_sig = h->b_sig;
    a.logits = logits; a.sigma = sigma; a.stats = stats;
    a.sigma_sum = sigma_sum; a.sigma_log = sigma_log;
    a.C = h->d.nb_classes; a.CP = p.head_cp; a.CPh = p.head_cph; a.stats_flags = flags;
    a.HW = (size_t)h->d.height * h->d.width;
    a.V = a.HW * n_one;
    a.passes = passes;
    if (sampling) {
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "pass keys");
        RCU_HIP(launch_head_sampled(a, reinterpret_cast<const unsigned long long*>(sampling->keys), sampling->first_sample, sampling->samples, stream));
    } else if (votes) {
        RCU_HIP(launch_head_votes(a, votes->plane, votes->n_words, votes->bits, stream));
    } else {
        RCU_HIP(launch_head(a, stream));
    }
    h->head_input_kept = true;
    if (ev) RCU_HIP(hipEventRecord(*ev++, stream));
    return RCU_OK;
}

extern "C" int rcu_unet_profile_begin(rcu_unet* h, int max_forwards)
{
    if (!h || max_forwards < 0) return fail(RCU_ERR_INVALID, "rcu_unet_profile_begin: bad argument");
    for (hipEvent_t e : h->prof_events) (void)hipEventDestroy(e);
    h->prof_events.clear();
    h->prof_capacity = h->prof_used = 0;
    const size_t total = (size_t)max_forwards * prof_slots(h);
    h->prof_events.resize(total);
    for (size_t i = 0; i < total; ++i) {
        hipError_t e = hipEventCreate(&h->prof_events[i]);
        if (e != hipSuccess) {
            h->prof_events.resize(i);
            return hip_fail(e, "hipEventCreate");
        }
    }
    h->prof_capacity = max_forwards;
    return RCU_OK;
}

extern "C" int rcu_unet_profile_collect(rcu_unet* h, double* ms_sum, int* forwards)
{
    if (!h || !ms_sum || !forwards) return fail(RCU_ERR_INVALID, "rcu_unet_profile_collect: null argument");
    const int slots = prof_slots(h);
    for (int i = 0; i < slots - 1; ++i) ms_sum[i] = 0.0;
    for (int f = 0; f < h->prof_used; ++f) {
        hipEvent_t* ev = h->prof_events.data() + (size_t)f * slots;
        RCU_HIP(hipEventSynchronize(ev[slots - 1]));
        for (int i = 0; i < slots - 1; ++i) {
            float ms = 0.f;
            RCU_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            ms_sum[i] += ms;
        }
    }
    *forwards = h->prof_used;
    h->prof_used = 0;
    return RCU_OK;
}

extern "C" int rcu_unet_forward(rcu_unet* h, const float* x_dev, int n, const float* masks_dev, float* logits_dev,
                                float* sigma_dev, void* stream)
{
    return forward_impl(h, x_dev, n, masks_dev, logits_dev, sigma_dev, nullptr, 0, static_cast<hipStream_t>(stream));
}

extern "C" int rcu_unet_forward_accumulate(rcu_unet* h, const float* x_dev, int n, const float* masks_dev, void* stats_dev,
                                           int flags, void* stream)
{
    if (!stats_dev) return fail(RCU_ERR_INVALID, "rcu_unet_forward_accumulate: null stats");
    return forward_impl(h, x_dev, n, masks_dev, nullptr, nullptr, stats_dev, flags & (RCU_MC_MI | RCU_MC_VAR | RCU_MC_EXACT),
                        static_cast<hipStream_t>(stream));
}

extern "C" int rcu_unet_forward_accumulate_sigma(rcu_unet* h, const float* x_dev, int n, const float* masks_dev, void* stats_dev,
                                                 int flags, float* sigma_sum_dev, int is_log_sigma, void* stream)
{
    if (!stats_dev || !sigma_sum_dev) return fail(RCU_ERR_INVALID, "rcu_unet_forward_accumulate_sigma: null stats / sigma sum");
    return forward_impl(h, x_dev, n, masks_dev, nullptr, nullptr, stats_dev, flags & (RCU_MC_MI | RCU_MC_VAR | RCU_MC_EXACT),
                        static_cast<hipStream_t>(stream), 1, sigma_sum_dev, is_log_sigma ? 1 : 0);
}

extern "C" int rcu_unet_forward_accumulate_sigma_passes(rcu_unet* h, const float* x_dev, int n, int passes, const float* masks_dev,
                                                        void* stats_dev, int flags, float* sigma_sum_dev, int is_log_sigma, void* stream)
{
    if (!stats_dev || !sigma_sum_dev) return fail(RCU_ERR_INVALID, "rcu_unet_forward_accumulate_sigma_passes: null stats / sigma sum");
    return forward_impl(h, x_dev, n, masks_dev, nullptr, nullptr, stats_dev, flags & (RCU_MC_MI | RCU_MC_VAR | RCU_MC_EXACT),
                        static_cast<hipStream_t>(stream), passes, sigma_sum_dev, is_log_sigma ? 1 : 0);
}

extern "C" int rcu_unet_forward_sample_sigma_passes(rcu_unet* h, const float* x_dev, int n, int passes, const float* masks_dev,
                                                    const uint64_t* keys_host, uint64_t first_sample, int samples, void* stats_dev, int flags,
                                                    float* sigma_sum_dev, int is_log_sigma, void* stream)
{
    const char* fn = "rcu_unet_forward_sample_sigma_passes";
    if (!h) return fail(RCU_ERR_INVALID, std::string(fn) + ": null handle");
    if (!x_dev || !keys_host || !stats_dev || !sigma_sum_dev)
        return fail(RCU_ERR_INVALID, std::string(fn) + ": null x_dev / keys_host / stats_dev / sigma_sum_dev");
    if (!h->d.sigma_out) return fail(RCU_ERR_INVALID, std::string(fn) + ": the handle has no sigma head (sigma_out = 0)");
    if (n < 1 || passes < 1 || (long)n * passes > h->d.max_batch)
        return fail(RCU_ERR_INVALID, std::string(fn) + ": batch size (times passes) outside 1..max_batch");
    if (int st = check_logit_sampling_shape(fn, (size_t)n, (size_t)h->d.height * h->d.width, h->d.nb_classes, samples)) return st;
    const HeadSampling sampling{keys_host, first_sample, samples};
    return forward_impl(h, x_dev, n, masks_dev, nullptr, nullptr, stats_dev, flags & (RCU_MC_MI | RCU_MC_VAR | RCU_MC_EXACT),
                        static_cast<hipStream_t>(stream), passes, sigma_sum_dev, is_log_sigma ? 1 : 0, &sampling);
}

extern "C" int rcu_unet_features(const rcu_unet* h, const float** features_dev, int* channels, int* channel_pitch)
{
    if (!h || !features_dev) return fail(RCU_ERR_INVALID, "rcu_unet_features: null argument");
    if (!h->finalized) return fail(RCU_ERR_STATE, "rcu_unet_features before rcu_unet_finalize_weights");
    const Plan& p = h->plan;
    for (const PlanLayer& L : p.layers)
        if (L.name == "conv_cls.0.conv2d_batch_relu.conv") {
            if (p.tensors[L.t_src1].blocked || (p.tensors[L.t_src1].padded() && p.t_features < 0))
                return fail(RCU_ERR_STATE, "rcu_unet_features: the handle was created without rcu_unet_desc.provide_features (the feature "
                                           "tensor is held channel-blocked / on a padded level)");
            *features_dev = h->ws->dev[p.t_features >= 0 ? p.t_features : L.t_src1];
            if (channels) *channels = L.cin1;
            if (channel_pitch) *channel_pitch = L.c1p;
            return RCU_OK;
        }
    return fail(RCU_ERR_STATE, "rcu_unet_features: no conv_cls layer in the plan");
}

extern "C" int rcu_unet_head_features(const rcu_unet* h, const float** features_dev, int* channels, int* channel_pitch)
{
    if (!h || !features_dev) return fail(RCU_ERR_INVALID, "rcu_unet_head_features: null argument");
    if (!h->finalized) return fail(RCU_ERR_STATE, "rcu_unet_head_features before rcu_unet_finalize_weights");
    if (h->d.sigma_out)
        return fail(RCU_ERR_STATE, "rcu_unet_head_features: a sigma_out handle's head tensor interleaves the sigma twin's channels");
    if (h->plan.t_head < 0) return fail(RCU_ERR_STATE, "rcu_unet_head_features: no conv_cls layer in the plan");
    if (!h->head_input_kept)
        return fail(RCU_ERR_STATE, "rcu_unet_head_features: the last forward on this handle fused the classifier into conv_cls.0 (or there was "
                                   "none): run it with rcu_unet_set_fuse_head(h, 0)");
    *features_dev = h->ws->dev[h->plan.t_head];
    if (channels) *channels = h->d.start_filters;
    if (channel_pitch) *channel_pitch = h->plan.head_cp;
    return RCU_OK;
}

extern "C" int rcu_unet_forward_accumulate_passes(rcu_unet* h, const float* x_dev, int n, int passes, const float* masks_dev,
                                                  void* stats_dev, int flags, void* stream)
{
    if (!stats_dev) return fail(RCU_ERR_INVALID, "rcu_unet_forward_accumulate_passes: null stats");
    return forward_impl(h, x_dev, n, masks_dev, nullptr, nullptr, stats_dev, flags & (RCU_MC_MI | RCU_MC_VAR | RCU_MC_EXACT),
                        static_cast<hipStream_t>(stream), passes);
}

extern "C" int rcu_unet_forward_accumulate_votes(rcu_unet* h, const float* x_dev, int n, int passes, const float* masks_dev, void* stats_dev,
                                                 int flags, uint32_t* votes_dev, int n_words, const int32_t* bits_host, void* stream)
{
    const std::string fn = "rcu_unet_forward_accumulate_votes";
    if (!h) return fail(RCU_ERR_INVALID, fn + ": null handle");
    if (!x_dev || !stats_dev || !votes_dev || !bits_host) return fail(RCU_ERR_INVALID, fn + ": null x_dev / stats_dev / votes_dev / bits_host");
    if (int st = check_vote_plane(fn, n_words)) return st;
    if (h->d.nb_classes < 1 || h->d.nb_classes > MAX_CLASSES) return fail(RCU_ERR_INVALID, fn + ": nb_classes must be in 1..8");
    if (n < 1 || passes < 1 || (long)n * passes > h->d.max_batch) return fail(RCU_ERR_INVALID, fn + ": batch size (times passes) outside 1..max_batch");
    for (int t = 0; t < passes; ++t)
        if (int st = check_vote_bit(fn, bits_host[t], n_words)) return st;
    const HeadVotes votes{votes_dev, n_words, bits_host};
    return forward_impl(h, x_dev, n, masks_dev, nullptr, nullptr, stats_dev, flags & (RCU_MC_MI | RCU_MC_VAR | RCU_MC_EXACT),
                        static_cast<hipStream_t>(stream), passes, nullptr, 0, nullptr, &votes);
}

extern "C" int rcu_unet_num_layers(const rcu_unet* h) { return h ? (int)h->plan.layers.size() : 0; }

extern "C" int rcu_unet_layer_info(const rcu_unet* h, int layer, rcu_layer_info* out)
{
    if (!h || !out || layer < 0 || layer >= (int)h->plan.layers.size()) return fail(RCU_ERR_INVALID, "bad layer index");
    plan_layer_info(h->plan, h->d, layer, out);
    return RCU_OK;
}

extern "C" int rcu_unet_layer_layouts(const rcu_unet* h, int layer, int32_t* src1, int32_t* src2, int32_t* out, int32_t* pooled)
{
    if (!h || layer < 0 || layer >= (int)h->plan.layers.size()) return fail(RCU_ERR_INVALID, "bad layer index");
    const PlanLayer& L = h->plan.layers[layer];
    auto layout = [&](int t) -> int32_t {
        if (t < 0) return -1;
        const PlanTensor& T = h->plan.tensors[t];
        return T.paired ? RCU_LAYOUT_PAIRED : T.blocked ? RCU_LAYOUT_BLOCKED : RCU_LAYOUT_NHWC;
    };
    if (src1) *src1 = layout(L.t_src1);
    if (src2) *src2 = layout(L.t_src2);
    if (out) *out = layout(L.t_out);
    if (pooled) *pooled = layout(L.t_pool);
    return RCU_OK;
}

extern "C" int rcu_unet_run_layer(rcu_unet* h, int layer, int n, const float* masks_dev, void* stream)
{
    if (!h || layer < 0 || layer >= (int)h->plan.layers.size()) return fail(RCU_ERR_INVALID, "bad layer index");
    if (!h->finalized) return fail(RCU_ERR_STATE, "rcu_unet_run_layer before rcu_unet_finalize_weights");
    if (n < 1 || n > h->d.max_batch) return fail(RCU_ERR_INVALID, "batch size outside 1..max_batch");
    return run_layer(h, layer, n, masks_dev, static_cast<hipStream_t>(stream));
}
