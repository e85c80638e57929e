// ToEntropy of a foreground probability (rechun/eval/analysis.py:196-203 on [1 - p, p]; numpyfunctions.py:166-168): float32 products
// f * logf(f), float64 sum, divided by log 2.  ONE definition for every kernel that needs the value -- rcu_normalised_entropy writes it out
// (rcu_calib.hip), rcu_unc_hist_from_p bins it in registers (rcu_unc_hist.hip) -- so that the two agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace rcu {

#if defined(__HIPCC__)
constexpr double ENTROPY_LOG2 = 0.6931471805599453;

// the entropy in nats, before the division: -(b log b + f log f)
__device__ __forceinline__ double entropy_nats_of_p(float f)
{
    const float b = 1.0f - f;
    // (the product or 0 is selected as a 32-bit pattern, then widened: the same float64 value, one select less than selecting the float64)
    const double tf = (double)__uint_as_float((f > 0.f) ? __float_as_uint(f * logf(f)) : 0u);
    const double tb = (double)__uint_as_float((b > 0.f) ? __float_as_uint(b * logf(b)) : 0u);
    return -(tb + tf);
}
// nats -> the normalised entropy: ONE float64 division, monotone in s (what lets rcu_unc_hist_from_p compare in nats, rcu_unc_hist.hip)
__device__ __forceinline__ double normalised_entropy_of_nats(double s) { return s / ENTROPY_LOG2; }
__device__ __forceinline__ double normalised_entropy_of_p(float f) { return normalised_entropy_of_nats(entropy_nats_of_p(f)); }
#endif

}  // namespace rcu
