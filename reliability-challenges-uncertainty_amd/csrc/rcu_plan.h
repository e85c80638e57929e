// The U-Net kernel plan as a value (rcu_plan.hip): which kernel runs every conv layer, the activation tensors they read and write, the allocated
// extent of every level, the dropout sites.  Host only, no HIP runtime call; the handle (rcu_api.hip) holds one Plan plus the device state.
#pragma once
#include "rcu_kernels.h"

#include <string>
#include <utility>
#include <vector>

namespace rcu {

struct PlanLayer {
    std::string name;        // state_dict prefix of the conv ("....conv" for units, "...upconv.1" for up convs)
    std::string bn;          // prefix of the BatchNorm2d, empty when the conv has none
    std::string name2, bn2;  // fused twin (conv_sigma.0) stacked on the output channels, or empty
    int cin1 = 0, cin2 = 0;  // real channels per source
    int c1p = 0, c2p = 0;    // padded channels per source
    int cout = 0;            // real output channels (per twin)
    int coutp = 0;           // padded output channels (both twins)
    int csplit = 0;          // first channel of the twin
    int H = 0, W = 0;        // REAL extent of the unit's output grid (an up-convolution: of the up-sampled grid before the centre pad)
    int level = 0;           // level of the tile grid: the unit's own level, an up-convolution's LOW-resolution level
    int gh = 0, gw = 0;      // ALLOCATED extent of that level = the grid the tiles walk (== its real extent unless the level is padded)
    int upsample = 0, relu = 0;
    int is_1x1 = 0;          // ConvResidualBlock's residual conv: a 1x1 kernel, run as a 3x3 unit whose centre tap alone is non-zero
    int accumulate = 0;      // the unit's result is added to what its output tensor holds (the residual conv's output)
    int site = -1, site2 = -1;
    int cfg = 0, NT = 0;
    int t_src1 = -1, t_src2 = -1, t_out = -1, t_pool = -1;
};

struct PlanTensor {
    size_t floats_per_slice = 0;
    bool zero_fill = false;   // centre-padded up-conv output: the border is never written and must read as zero
    int H = 0, W = 0, cp = 0; // ALLOCATED extent (floats_per_slice = H W cp)
    int Hr = 0, Wr = 0;       // real extent; smaller on a padded level (plan_unet): the pixels beyond it hold zeros nobody writes
    bool padded() const { return H != Hr || W != Wr; }
    bool blocked = false;     // [N][C/8][H][W][8] instead of NHWC (rcu_kernels.h, ConvArgs): decided per tensor by assign_layouts
    bool paired = false;      // blocked, with the 64 bytes of each aligned pixel pair permuted (rcu_kernels.h): F(4x4,3x3) kernels on both sides only
    bool operator==(const PlanTensor& o) const
    {
        return floats_per_slice == o.floats_per_slice && H == o.H && W == o.W && Hr == o.Hr && Wr == o.Wr && cp == o.cp && blocked == o.blocked && paired == o.paired &&
               zero_fill == o.zero_fill;
    }
};

struct Plan {
    std::vector<PlanLayer> layers;
    std::vector<PlanTensor> tensors;
    std::vector<std::pair<int, int>> level_ext;       // allocated (H, W) of the activation tensors of level 0 .. depth (plan_unet)
    std::vector<std::pair<std::string, int>> sites;   // (name, channels)
    std::vector<int> site_offset;                     // prefix sums of channels
    int mask_floats = 0;
    int in_cp = 0, head_cp = 0, head_cph = 0;
    int t_input = -1, t_head = -1;
    int t_features = -1;      // provide_features on a padded level 0: the compact [voxel][channel] copy rcu_unet_features hands out
    // the same tensors (same shapes, same layouts, same never-written borders): what two handles that share one workspace must agree on
    bool operator==(const Plan& o) const { return tensors == o.tensors; }
};

// The plan of a (checked) description under the options: the level extents chosen, every layer's kernel, the tensor layouts.  RCU_OK, or the
// error of a plan that cannot be built (reported through report_error; *out is then unspecified).
int plan_unet(const rcu_unet_desc& d, const rcu_unet_options& opt, Plan* out);

// the kernels whose store side honours ConvArgs::part (a padded level)
bool cfg_handles_padding(int cfg);
// does layer L run in the ConvArgs::part form: a padded level on either side, or output / pooled tensors with extents of their own
bool layer_runs_part(const Plan& p, const PlanLayer& L);
// the plan's last unit can take the classifier into its epilogue: two classes, no sigma twin, one 32-cout Winograd tile of either family
bool head_fusable(const Plan& p, const rcu_unet_desc& d);
// the rcu_layer_info of layer `layer` (0 <= layer < p.layers.size())
void plan_layer_info(const Plan& p, const rcu_unet_desc& d, int layer, rcu_layer_info* out);

}  // namespace rcu
