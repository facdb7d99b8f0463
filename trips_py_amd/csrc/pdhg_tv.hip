// pdhg_tv.hip — PDHG's fused forms on the first differences (pdhg.hip chains them; the entries of one row: pdhg_internal.h).  Nothing
// of the length of L xbar or L^T q touches memory:
//   k_pdhg_tv_dual<G, true>:   q' = the groups G of q + sig L xbar projected (kRows: every row clipped to [-lam, lam]; kPairs: the
//                              (h, v) of a pixel onto the 2-norm ball of radius lam; kTriples: the (h, v, t) of a voxel), the
//                              differences formed in registers as k_d2_fwd and k_time_fwd form them (xbar read: 4n, the next frame
//                              re-read with kTriples; q read and written: 8 rows); partials 1 and 3 of the block's row
//   k_pdhg_tv_dual<G, false>:  the same projection on a stored u = L xbar, u read where the fused kernel forms a difference
//   k_pdhg_tv_primal:          x' = clip(x - tau (z + L^T q), lo, hi), xbar' = 2 x' - x, L^T q gathered by AdjGather (tv_internal.h),
//                              as k_d2_adj gathers it (x, z read: 8n, q read: 4 rows; x', xbar' written: 8n); partials 4 to 7; it
//                              knows nothing of the grouping
// One thread per image column over batches of RB rows, blockIdx.z = frame, as the stencils of tvops.hip; every thread stays to the
// block sums.  The kernels of a mode share one grid — grid2(N, frames, true) on the 2-D layouts, grid3(N, frames) on the space-time
// layout — and write disjoint slots of row (z gridDim.y + y) gridDim.x + x.  The bodies stride over the row batches: the grid
// decides the order of the block partials and nothing else.
#include "tv_internal.h"
#include "pdhg_internal.h"

using namespace trk;

namespace {

// One pixel's or voxel's rows: the thread of column j of frame f holds every member of the group of (f, i, j).  kRows: every member
// alone, h before v.  Else three members: the triple; two: pdhg_q_pair with the members in row order (h before v before t); one
// (the last row's H, the last column's V, ...): the clip; the last voxel has no row.  Only kTriples has a temporal member.
template <Groups G>
__device__ __forceinline__ void pdhg_q_group(bool has_h, bool has_v, bool has_t, float sig, float lam, float uh, float uv, float ut,
                                             float ph, float pv, float pt, float* dh, float* dv, float* dt, double& s1, double& s3) {
  if (G == Groups::kRows) {
    if (has_h) *dh = pdhg_q_entry(sig, lam, uh, ph, s1, s3);
    if (has_v) *dv = pdhg_q_entry(sig, lam, uv, pv, s1, s3);
    return;
  }
  if (G != Groups::kTriples) has_t = false;
  if (has_h && has_v && has_t) {
    pdhg_q_triple(sig, lam, uh, uv, ut, ph, pv, pt, s1, s3);
    *dh = ph;
    *dv = pv;
    *dt = pt;
  } else if (has_h && has_v) {
    pdhg_q_pair(sig, lam, uh, uv, ph, pv, s1, s3);
    *dh = ph;
    *dv = pv;
  } else if (has_h && has_t) {
    pdhg_q_pair(sig, lam, uh, ut, ph, pt, s1, s3);
    *dh = ph;
    *dt = pt;
  } else if (has_v && has_t) {
    pdhg_q_pair(sig, lam, uv, ut, pv, pt, s1, s3);
    *dv = pv;
    *dt = pt;
  } else if (has_h) {
    *dh = pdhg_q_entry(sig, lam, uh, ph, s1, s3);
  } else if (has_v) {
    *dv = pdhg_q_entry(sig, lam, uv, pv, s1, s3);
  } else if (has_t) {
    *dt = pdhg_q_entry(sig, lam, ut, pt, s1, s3);
  }
}

// FUSED: src = xbar (frames of N^2), the differences in registers; else src = u = L xbar with q's layout: per frame [H ; V] and, with
// kTriples, T_f at nt 2 N (N - 1) + f N^2.  q in place (an entry is read and then written by the same thread): no __restrict__.
template <Groups G, bool FUSED>
__global__ __launch_bounds__(NT) void k_pdhg_tv_dual(const float* __restrict__ src, float* q, int N, int nt, float sig, float lam,
                                                     double* __restrict__ partials) {
  constexpr bool T3 = G == Groups::kTriples;
  __shared__ double red[NT / 64];
  const int f = blockIdx.z;
  const int64_t npix = (int64_t)N * N, ps = 2 * (int64_t)N * (N - 1);
  const bool ht = T3 && f < nt - 1;
  float* qh = q + f * ps;
  float* qv = qh + (int64_t)N * (N - 1);
  float* qt = T3 ? q + nt * ps + f * npix : q;                           // (read and written where ht only)
  const float* __restrict__ xf = FUSED ? src + f * npix : src;           // FUSED: this frame and the next
  const float* __restrict__ sh = FUSED ? src : src + f * ps;             // !FUSED: u laid out as q
  const float* __restrict__ sv = FUSED ? src : sh + (int64_t)N * (N - 1);
  const float* __restrict__ st = (FUSED || !T3) ? src : src + nt * ps + f * npix;
  const int j = blockIdx.x * NT + threadIdx.x;
  double s1 = 0.0, s3 = 0.0;
  if (j < N) {
    const bool hr = j < N - 1;
    for (int i0 = blockIdx.y * RB; i0 < N; i0 += gridDim.y * RB) {
      const int64_t o0 = (int64_t)i0 * N + j;
      const int64_t h0 = (int64_t)i0 * (N - 1) + j;
      float xc[RB + 1], ah[RB], at[RB], ph[RB], pv[RB], pt[RB];   // FUSED: ah = the right neighbour, at = the next frame
      if (FUSED) {
#pragma unroll
        for (int t = 0; t <= RB; ++t) xc[t] = (i0 + t < N) ? xf[o0 + (int64_t)t * N] : 0.f;
      } else {
#pragma unroll
        for (int t = 0; t < RB; ++t) xc[t] = (i0 + t < N - 1) ? sv[o0 + (int64_t)t * N] : 0.f;     // xc[t] = u_v
      }
#pragma unroll
      for (int t = 0; t < RB; ++t) {
        const bool in = i0 + t < N;
        const int64_t o = o0 + (int64_t)t * N, hb = h0 + (int64_t)t * (N - 1);
        if (FUSED) {
          ah[t] = (hr && in) ? xf[o + 1] : 0.f;
          at[t] = (ht && in) ? xf[npix + o] : 0.f;
        } else {
          ah[t] = (hr && in) ? sh[hb] : 0.f;
          at[t] = (ht && in) ? st[o] : 0.f;
        }
        ph[t] = (hr && in) ? qh[hb] : 0.f;
        pv[t] = (i0 + t < N - 1) ? qv[o] : 0.f;
        pt[t] = (ht && in) ? qt[o] : 0.f;
      }
#pragma unroll
      for (int t = 0; t < RB; ++t) {
        const int i = i0 + t;
        if (i < N) {
          const int64_t o = o0 + (int64_t)t * N;
          const float uh = FUSED ? xc[t] - ah[t] : ah[t];
          const float uv = FUSED ? xc[t] - xc[t + 1] : xc[t];
          const float ut = FUSED ? xc[t] - at[t] : at[t];
          pdhg_q_group<G>(hr, i < N - 1, ht, sig, lam, uh, uv, ut, ph[t], pv[t], pt[t], qh + h0 + (int64_t)t * (N - 1), qv + o, qt + o,
                          s1, s3);
        }
      }
    }
  }
  s1 = block_sum<NT>(s1, red);
  s3 = block_sum<NT>(s3, red);
  if (threadIdx.x == 0) {
    const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partials[blk * 8 + 1] = s1;
    partials[blk * 8 + 3] = s3;
  }
}

// x_new may be x (a pixel is read and then written by the same thread): no __restrict__ on the two.  TEMPORAL: q has the space-time
// layout, T_f at q + nt 2 N (N - 1) + f N^2, and frame f gathers + T_f (f < nt - 1) - T_{f-1} (f > 0).
template <bool HAS_XT, bool TEMPORAL>
__global__ __launch_bounds__(NT) void k_pdhg_tv_primal(const float* x, const float* __restrict__ z, const float* __restrict__ q,
                                                       float* x_new, float* __restrict__ xbar, const float* __restrict__ x_true, int N,
                                                       int nt, float tau, float lo, float hi, double* __restrict__ partials) {
  __shared__ double red[NT / 64];
  const int f = blockIdx.z;
  const int64_t npix = (int64_t)N * N, ps = 2 * (int64_t)N * (N - 1);
  const float* __restrict__ qh = q + f * ps;
  const float* __restrict__ qv = qh + (int64_t)N * (N - 1);
  const float* __restrict__ tc = nullptr;
  const float* __restrict__ tp = nullptr;
  if (TEMPORAL) {
    const float* __restrict__ qt = q + nt * ps;
    if (f < nt - 1) tc = qt + f * npix;
    if (f > 0) tp = qt + (f - 1) * npix;
  }
  x += f * npix;
  z += f * npix;
  x_new += f * npix;
  xbar += f * npix;
  if (HAS_XT) x_true += f * npix;
  const int j = blockIdx.x * NT + threadIdx.x;
  double s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
  if (j < N) {
    for (int i0 = blockIdx.y * RB; i0 < N; i0 += gridDim.y * RB) {
      const int64_t o0 = (int64_t)i0 * N + j;
      AdjGather<TEMPORAL> g;
      float xv[RB], zv[RB], tv[RB];
      g.load(qh, qv, tc, tp, N, i0, j);
#pragma unroll
      for (int t = 0; t < RB; ++t) {
        const bool in = i0 + t < N;
        const int64_t o = o0 + (int64_t)t * N;
        xv[t] = in ? x[o] : 0.f;
        zv[t] = in ? z[o] : 0.f;
        tv[t] = (HAS_XT && in) ? x_true[o] : 0.f;
      }
#pragma unroll
      for (int t = 0; t < RB; ++t) {
        const int i = i0 + t;
        if (i < N) {
          float xn, xb;
          pdhg_x_entry<HAS_XT>(tau, lo, hi, xv[t], zv[t] + g.sum(t, i, N), tv[t], xn, xb, s4, s5, s6, s7);
          x_new[o0 + (int64_t)t * N] = xn;
          xbar[o0 + (int64_t)t * N] = xb;
        }
      }
    }
  }
  s4 = block_sum<NT>(s4, red);
  s5 = block_sum<NT>(s5, red);
  if (HAS_XT) s6 = block_sum<NT>(s6, red);
  s7 = block_sum<NT>(s7, red);
  if (threadIdx.x == 0) {
    const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partials[blk * 8 + 4] = s4;
    partials[blk * 8 + 5] = s5;
    partials[blk * 8 + 6] = HAS_XT ? s6 : 0.0;
    partials[blk * 8 + 7] = s7;
  }
}

inline dim3 mode_grid(Groups g, int N, int frames) { return g == Groups::kTriples ? grid3(N, frames) : grid2(N, frames, true).g; }

// the five instantiations: kRows has no unfused form here (every row alone is the streaming k_pdhg_dual_q of pdhg.hip)
void launch_dual(Groups g, bool fused, int N, int frames, float sig, float lam, const float* src, float* q, double* partials,
                 hipStream_t s) {
  const dim3 grid = mode_grid(g, N, frames);
#define DUAL(G, F) hipLaunchKernelGGL((k_pdhg_tv_dual<G, F>), grid, dim3(NT), 0, s, src, q, N, frames, sig, lam, partials)
  if (g == Groups::kTriples) { if (fused) DUAL(Groups::kTriples, true); else DUAL(Groups::kTriples, false); }
  else if (g == Groups::kPairs) { if (fused) DUAL(Groups::kPairs, true); else DUAL(Groups::kPairs, false); }
  else DUAL(Groups::kRows, true);
#undef DUAL
}

const char* const kDualEntry[] = {"trk_pdhg_tv_dual", "trk_pdhg_tv_dual_iso", "trk_pdhg_st_dual_iso3"};   // by Groups

}  // namespace

int trk::pdhg_tv_blocks(Groups g, int N, int frames) {
  const dim3 grid = mode_grid(g, N, frames);
  return (int)(grid.x * grid.y * grid.z);
}

void trk::pdhg_grouped_dual_launch(Groups g, int N, int frames, float sig, float lam, const float* u, float* q, double* partials,
                                   hipStream_t s) {
  launch_dual(g, false, N, frames, sig, lam, u, q, partials, s);
}

int trk::pdhg_fused_dual(Groups g, trk_op* L, double sigma, double lam, const float* xbar, float* q, double* partials,
                         int capacity_blocks, int* n_blocks, trk_stream st) {
  const char* who = kDualEntry[(int)g];
  TRK_REQUIRE(L && xbar && q && partials && n_blocks, "%s: NULL argument", who);
  int N = 0, nt = 0;
  if (!pdhg_fusable(L, g, &N, &nt)) return fail(TRK_EUNSUPPORTED, "%s: %s", who, pdhg_fusable_wanted(g));
  TRK_REQUIRE(nt <= 65535, "%s: at most 65535 frames", who);
  TRK_REQUIRE(sigma > 0.0 && sigma < __builtin_inf(), "%s: sigma must be finite and > 0", who);
  TRK_REQUIRE(lam >= 0.0 && lam < __builtin_inf(), "%s: lam must be finite and >= 0", who);
  TRK_REQUIRE(q != xbar, "%s: q must not alias xbar", who);
  const int nb = pdhg_tv_blocks(g, N, nt);
  TRK_REQUIRE(nb <= capacity_blocks, "%s: partial buffer too small (%d blocks needed)", who, nb);
  *n_blocks = nb;
  launch_dual(g, true, N, nt, (float)sigma, (float)lam, xbar, q, partials, (hipStream_t)st);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk::pdhg_fused_primal(Groups g, trk_op* L, double tau, double lo, double hi, const float* x, const float* z, const float* q,
                           float* x_new, float* xbar, const float* x_true, double* partials, int capacity_blocks, int* n_blocks,
                           trk_stream st) {
  const bool temporal = g == Groups::kTriples;
  const char* who = temporal ? "trk_pdhg_st_primal" : "trk_pdhg_tv_primal";
  TRK_REQUIRE(L && x && z && q && x_new && xbar && partials && n_blocks, "%s: NULL argument", who);
  int N = 0, nt = 0;
  if (!pdhg_fusable(L, g, &N, &nt)) return fail(TRK_EUNSUPPORTED, "%s: %s", who, pdhg_fusable_wanted(g));
  TRK_REQUIRE(nt <= 65535, "%s: at most 65535 frames", who);
  TRK_REQUIRE(tau > 0.0 && tau < __builtin_inf(), "%s: tau must be finite and > 0", who);
  TRK_REQUIRE(lo <= hi, "%s: need lo <= hi (either may be infinite)", who);
  TRK_REQUIRE(xbar != x && xbar != x_new && xbar != z && xbar != q && xbar != x_true, "%s: xbar must not alias another operand", who);
  TRK_REQUIRE(x_new != z && x_new != q && x_new != x_true, "%s: x_new may alias x only", who);
  const int nb = pdhg_tv_blocks(g, N, nt);
  TRK_REQUIRE(nb <= capacity_blocks, "%s: partial buffer too small (%d blocks needed)", who, nb);
  *n_blocks = nb;
  with_bools([&](auto HAS_XT, auto TEMPORAL) {
    hipLaunchKernelGGL((k_pdhg_tv_primal<HAS_XT, TEMPORAL>), mode_grid(g, N, nt), dim3(NT), 0, (hipStream_t)st, x, z, q, x_new, xbar,
                       x_true, N, nt, (float)tau, (float)lo, (float)hi, partials);
  }, x_true != nullptr, temporal);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

extern "C" {

int trk_pdhg_fused_caps(const trk_op* L, int* can) {
  TRK_REQUIRE(L && can, "trk_pdhg_fused_caps: NULL argument");
  *can = L->kind == 3 ? 1 : 0;
  return TRK_OK;
}

int trk_pdhg_tv_dual(trk_op* L, double sigma, double lam, const float* xbar, float* q, double* partials, int capacity_blocks,
                     int* n_blocks, trk_stream st) {
  return pdhg_fused_dual(Groups::kRows, L, sigma, lam, xbar, q, partials, capacity_blocks, n_blocks, st);
}

int trk_pdhg_tv_dual_iso(trk_op* L, double sigma, double lam, const float* xbar, float* q, double* partials, int capacity_blocks,
                         int* n_blocks, trk_stream st) {
  return pdhg_fused_dual(Groups::kPairs, L, sigma, lam, xbar, q, partials, capacity_blocks, n_blocks, st);
}

int trk_pdhg_st_dual_iso3(trk_op* L, double sigma, double lam, const float* xbar, float* q, double* partials, int capacity_blocks,
                          int* n_blocks, trk_stream st) {
  return pdhg_fused_dual(Groups::kTriples, L, sigma, lam, xbar, q, partials, capacity_blocks, n_blocks, st);
}

// (the 2-D primal knows nothing of the grouping: kRows stands for both modes of the 2-D handle)
int trk_pdhg_tv_primal(trk_op* L, double tau, double lo, double hi, const float* x, const float* z, const float* q, float* x_new,
                       float* xbar, const float* x_true, double* partials, int capacity_blocks, int* n_blocks, trk_stream st) {
  return pdhg_fused_primal(Groups::kRows, L, tau, lo, hi, x, z, q, x_new, xbar, x_true, partials, capacity_blocks, n_blocks, st);
}

int trk_pdhg_st_primal(trk_op* L, double tau, double lo, double hi, const float* x, const float* z, const float* q, float* x_new,
                       float* xbar, const float* x_true, double* partials, int capacity_blocks, int* n_blocks, trk_stream st) {
  return pdhg_fused_primal(Groups::kTriples, L, tau, lo, hi, x, z, q, x_new, xbar, x_true, partials, capacity_blocks, n_blocks, st);
}

}  // extern "C"
