// kl_internal.h — one term of the Kullback-Leibler data fit KL(b, y) = sum_i y_i - b_i + b_i log(b_i / y_i), ONE definition for
// k_mlem_ratio (mlem.hip) and the KL dual of PDHG (pdhg_internal.h): fp64 from the fp32 values, nothing contracted.
#pragma once
#include "trk_internal.h"

namespace trk {

//   b > 0, y > 0 (both finite):  (y - b) + b * log(b / y)
//   b == 0, y >= 0:              y
//   otherwise:                   +inf — the point lies outside the domain of the Poisson likelihood (y <= 0 under a count, a negative
//                                or non-finite operand)
// No case produces a NaN: an infinite operand would give inf - inf in the first form and is sent to the third.
__device__ __forceinline__ double kl_term(float b, float y) {
#pragma clang fp contract(off)
  const float inf = __builtin_inff();
  if (b > 0.f && y > 0.f && b < inf && y < inf) {
    const double bd = (double)b, yd = (double)y;
    return (yd - bd) + bd * log(bd / yd);
  }
  if (b == 0.f && y >= 0.f) return (double)y;
  return __builtin_inf();
}

}  // namespace trk
