// The uncertainty source of the per-component table (rcu_cc.hip) and the boundary table (rcu_edt.hip): an RCU_CC_UNC_* kind plus a device
// map, read per voxel as the integer q(u).  ONE definition of q, of the load per kind, of the argument check and of the kind -> template
// dispatch, so that the two tables quantise identically (include/rcu.h promises it, the host metrics divide by the same 2^24).
#pragma once
#include "../../include/rcu.h"
#include "rcu_entropy.h"
#include "rcu_kernels.h"

#include <string>
#include <type_traits>

namespace rcu {

#if defined(__HIPCC__)
// q(u) = rint(clamp(u, 0, 1) * 2^24) in float64, ties to even, NaN -> 0 (fmax(NaN, 0) = 0)
__device__ __forceinline__ unsigned quantise(double u) { return (unsigned)rint(fmin(fmax(u, 0.0), 1.0) * 16777216.0); }

// q of voxel idx of a map of this kind (float32 map, float64 map, float32 foreground probability whose entropy is taken); 0 without a map
template <int KIND>
__device__ __forceinline__ unsigned quantised_unc(const void* unc, size_t idx)
{
    if constexpr (KIND == RCU_CC_UNC_F32) return quantise((double)reinterpret_cast<const float*>(unc)[idx]);
    if constexpr (KIND == RCU_CC_UNC_F64) return quantise(reinterpret_cast<const double*>(unc)[idx]);
    if constexpr (KIND == RCU_CC_UNC_P) return quantise(normalised_entropy_of_p(reinterpret_cast<const float*>(unc)[idx]));
    return 0;
}
#endif

inline int check_unc_source(const std::string& f, int unc_kind, const void* unc_dev)
{
    if (unc_kind != RCU_CC_UNC_NONE && unc_kind != RCU_CC_UNC_F32 && unc_kind != RCU_CC_UNC_F64 && unc_kind != RCU_CC_UNC_P)
        return report_error(RCU_ERR_INVALID, f + "unc_kind must be one of RCU_CC_UNC_NONE, _F32, _F64, _P, got " + std::to_string(unc_kind));
    if ((unc_kind == RCU_CC_UNC_NONE) != (unc_dev == nullptr))
        return report_error(RCU_ERR_INVALID, f + "unc_dev must be null for RCU_CC_UNC_NONE and only then");
    return RCU_OK;
}

// launch(std::integral_constant<int, KIND>) for a kind that check_unc_source has passed
template <class Launch>
void with_unc_kind(int unc_kind, Launch launch)
{
    switch (unc_kind) {
    case RCU_CC_UNC_F32: launch(std::integral_constant<int, RCU_CC_UNC_F32>()); break;
    case RCU_CC_UNC_F64: launch(std::integral_constant<int, RCU_CC_UNC_F64>()); break;
    case RCU_CC_UNC_P: launch(std::integral_constant<int, RCU_CC_UNC_P>()); break;
    default: launch(std::integral_constant<int, RCU_CC_UNC_NONE>()); break;
    }
}

}  // namespace rcu
