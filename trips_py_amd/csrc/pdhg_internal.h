// pdhg_internal.h — one entry of the three PDHG updates (include/trk.h: the iteration and the eight sums), ONE definition for the
// streaming kernels of pdhg.hip (float4 body and tail) and the fused first-difference kernels of pdhg_tv.hip: the same operations in
// the same order, so the fused and the generic path leave the same bits.  Every multiply-add is an explicit fmaf and nothing else
// may be contracted.
#pragma once
#include "trk_internal.h"
#include "kl_internal.h"

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

// dual of the Kullback-Leibler data term KL(b, y + bg): the prox of sigma F* at z = p + sigma (w + bg), F*(p) = sum -b log(1 - p) - bg p,
//   p' = 1/2 (1 + z - sqrt((z - 1)^2 + 4 sigma b)), in a form that does not cancel for large z.  c2 = (float)(2 sigma), c4 = (float)(4 sigma):
//   y = w + bg ; z = fmaf(sig, y, p) ; d = z - 1 ; r = sqrtf(fmaf(d, d, c4 * b))
//   p' = (d <= 0) ? fmaf(0.5, d - r, 1) : 1 - (c2 * b) / (d + r)          (b = 0: p' = min(z, 1))
//   s0 += kl(b, y) (kl_internal.h: +inf where y leaves the domain, the update itself is unaffected), s2 += (p' - p)^2
__device__ __forceinline__ float pdhg_p_entry_kl(float sig, float c2, float c4, float w, float bg, float b, float p, double& s0,
                                                 double& s2) {
#pragma clang fp contract(off)
  const float y = w + bg;
  const float z = fmaf(sig, y, p);
  const float d = z - 1.f;
  const float r = sqrtf(fmaf(d, d, c4 * b));
  const float pn = (d <= 0.f) ? fmaf(0.5f, d - r, 1.f) : 1.f - (c2 * b) / (d + r);
  const double dp = (double)pn - (double)p;
  s0 += kl_term(b, y);
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

// dual of the regulariser, isotropic: the H and V entry of one pixel are projected together onto the 2-norm ball of radius lam.
//   th = fmaf(sig, uh, qh) ; tv = fmaf(sig, uv, qv) ; m = sqrtf(fmaf(th, th, tv * tv))
//   m <= lam: q' = t ; else s = lam / m, q' = t * s          (lam = 0: m = 0 keeps t = 0, m > 0 gives s = 0)
//   s1 += sqrt(uh^2 + uv^2) ; s3 += (qh' - qh)^2 + (qv' - qv)^2     (fp64 from the fp32 values)
// sqrtf and / are the correctly rounded ones (no fast-math): a host restatement with the same operations has the same bits.
__device__ __forceinline__ void pdhg_q_pair(float sig, float lam, float uh, float uv, float& qh, float& qv, double& s1, double& s3) {
#pragma clang fp contract(off)
  const float th = fmaf(sig, uh, qh), tv = fmaf(sig, uv, qv);
  const float m = sqrtf(fmaf(th, th, tv * tv));
  float nh = th, nv = tv;
  if (!(m <= lam)) {
    const float s = lam / m;
    nh = th * s;
    nv = tv * s;
  }
  const double dh = (double)nh - (double)qh, dv = (double)nv - (double)qv;
  s1 += sqrt((double)uh * (double)uh + (double)uv * (double)uv);
  s3 += dh * dh + dv * dv;
  qh = nh;
  qv = nv;
}

// dual of the regulariser, isotropic in space and time: the H, V and T entry of one voxel are projected together.
//   th = fmaf(sig, uh, qh) ; tv = fmaf(sig, uv, qv) ; tt = fmaf(sig, ut, qt) ; m = sqrtf(fmaf(th, th, fmaf(tv, tv, tt * tt)))
//   m <= lam: q' = t ; else s = lam / m, q' = t * s          (lam = 0: as the pair)
//   s1 += sqrt(uh^2 + uv^2 + ut^2) ; s3 += (qh' - qh)^2 + (qv' - qv)^2 + (qt' - qt)^2     (fp64 from the fp32 values)
__device__ __forceinline__ void pdhg_q_triple(float sig, float lam, float uh, float uv, float ut, float& qh, float& qv, float& qt,
                                              double& s1, double& s3) {
#pragma clang fp contract(off)
  const float th = fmaf(sig, uh, qh), tv = fmaf(sig, uv, qv), tt = fmaf(sig, ut, qt);
  const float m = sqrtf(fmaf(th, th, fmaf(tv, tv, tt * tt)));
  float nh = th, nv = tv, nt = tt;
  if (!(m <= lam)) {
    const float s = lam / m;
    nh = th * s;
    nv = tv * s;
    nt = tt * s;
  }
  const double dh = (double)nh - (double)qh, dv = (double)nv - (double)qv, dt = (double)nt - (double)qt;
  s1 += sqrt((double)uh * (double)uh + (double)uv * (double)uv + (double)ut * (double)ut);
  s3 += dh * dh + dv * dv + dt * dt;
  qh = nh;
  qv = nv;
  qt = nt;
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

// How the rows of L are grouped in the dual update of q: every row alone (the l1 term), the pairs (h, v) of a pixel, or the
// triples (h, v, t) of a voxel.  The one spelling of the mode for the loop of pdhg.hip and the kernels of pdhg_tv.hip.
enum class Groups { kRows, kPairs, kTriples };

// tvops.hip (tv_internal.h, which pdhg.hip cannot include beside vec_internal.h: both define NT): the kind and the geometry of a
// first-difference handle with every frame on this rank, 0 for any other handle.  The fused forms of kRows and kPairs take the 2-D
// handle (kind 3), those of kTriples the space-time handle (kind 4).
int tv_geometry_of(const trk_op* L, int* N, int* frames);
inline bool pdhg_fusable(const trk_op* L, Groups g, int* N, int* frames) {
  return tv_geometry_of(L, N, frames) == (g == Groups::kTriples ? 4 : 3);
}
inline const char* pdhg_fusable_wanted(Groups g) {          // what TRK_EUNSUPPORTED says after the entry's name
  return g == Groups::kTriples ? "the fused space-time forms take a handle from trk_spacetime_create with every frame on one rank"
                               : "the fused forms take a handle from trk_deriv2d_create only";
}

// pdhg_tv.hip: the blocks (= rows of 8 partials) of ONE launch of a column-thread kernel on the groups g of geometry (N, frames);
// the fused dual, the fused primal and the unfused grouped dual of a mode share the grid.
int pdhg_tv_blocks(Groups g, int N, int frames);
// pdhg_tv.hip: the unfused grouped dual (kPairs: `frames` blocks of [H ; V] rows; kTriples: the space-time rows) on u = L xbar and
// q in memory, slots 1 and 3 of rows 0 .. blocks - 1.  No checks: trk_pdhg_dual_q_iso and trk_pdhg_dual_q_iso3 make them.
void pdhg_grouped_dual_launch(Groups g, int N, int frames, float sig, float lam, const float* u, float* q, double* partials,
                              hipStream_t s);
// pdhg_tv.hip: the checked launches behind trk_pdhg_tv_dual, trk_pdhg_tv_dual_iso, trk_pdhg_st_dual_iso3 (g names the entry, and
// the entry's name opens the error text) and behind trk_pdhg_tv_primal, trk_pdhg_st_primal (kTriples: the space-time one).
int pdhg_fused_dual(Groups g, trk_op* L, double sigma, double lam, const float* xbar, float* q, double* partials, int capacity_blocks,
                    int* n_blocks, trk_stream st);
int pdhg_fused_primal(Groups g, trk_op* L, double tau, double lo, double hi, const float* x, const float* z, const float* q,
                      float* x_new, float* xbar, const float* x_true, double* partials, int capacity_blocks, int* n_blocks,
                      trk_stream st);

}  // namespace trk
