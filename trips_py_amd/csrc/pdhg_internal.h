// pdhg_internal.h — one entry of the three PDHG updates (include/trk.h: the iteration and the eight sums), ONE definition for the
// streaming kernels of pdhg.hip (float4 body and tail) and the fused first-difference kernels of tvops.hip: the same operations in
// the same order, so the fused and the generic path leave the same bits.  Every multiply-add is an explicit fmaf and nothing else
// may be contracted.
#pragma once
#include "trk_internal.h"

namespace trk {

// dual of the data term: e = w - b ; p' = fmaf(sig, e, p) * c with c = (float)(1 / (1 + sigma)) ; s0 += e^2, s2 += (p' - p)^2
__device__ __forceinline__ float pdhg_p_entry(float sig, float c, float w, float b, float p, double& s0, double& s2) {
#pragma clang fp contract(off)
  const float e = w - b;
  const float pn = fmaf(sig, e, p) * c;
  const double dp = (double)pn - (double)p;
  s0 += (double)e * (double)e;
  s2 += dp * dp;
  return pn;
}

// dual of the regulariser: q' = clip(fmaf(sig, u, q), -lam, lam) ; s1 += |u|, s3 += (q' - q)^2
__device__ __forceinline__ float pdhg_q_entry(float sig, float lam, float u, float q, double& s1, double& s3) {
#pragma clang fp contract(off)
  const float qn = fminf(fmaxf(fmaf(sig, u, q), -lam), lam);
  const double dq = (double)qn - (double)q;
  s1 += fabs((double)u);
  s3 += dq * dq;
  return qn;
}

// primal: g = z + v (formed by the caller) ; x' = clip(fmaf(-tau, g, x), lo, hi) ; xbar' = fmaf(2, x', -x) ; d = x' - x
// s4 += x'^2, s5 += d^2, s6 += (x' - x_true)^2, s7 += 1 where x' sits on a bound
template <bool HAS_XT>
__device__ __forceinline__ void pdhg_x_entry(float tau, float lo, float hi, float x, float g, float xt, float& xn, float& xb, double& s4,
                                             double& s5, double& s6, double& s7) {
#pragma clang fp contract(off)
  xn = fminf(fmaxf(fmaf(-tau, g, x), lo), hi);
  xb = fmaf(2.f, xn, -x);
  const float d = xn - x;
  s4 += (double)xn * (double)xn;
  s5 += (double)d * (double)d;
  if (HAS_XT) {
    const double e = (double)xn - (double)xt;
    s6 += e * e;
  }
  if (xn == lo || xn == hi) s7 += 1.0;
}

// tvops.hip: the blocks (= rows of 8 partials) of the fused forms on a 2-D first-difference handle, 0 for any other handle
int pdhg_tv_blocks(const trk_op* L);

}  // namespace trk
