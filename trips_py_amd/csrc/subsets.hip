// subsets.hip — row-action iterations over an operator cut into S row subsets A_1 .. A_S (handles of their own, the data held
// subset-major): OSEM, the ordered-subsets form of MLEM (mlem.hip), and SIRT / OS-SIRT / SART, its additive least-squares twin
//   x <- P_box(x + omega C_s A_s^T R_s (b_s - A_s x)),  R_s = 1 / (A_s 1),  C_s = 1 / (A_s^T 1).
// A pass visits the subsets in a fixed order; a sub-step is w = A_s x, ONE streaming kernel over the subset's data (OSEM: mlem.hip's
// ratio; SIRT: the weighted residual), t = A_s^T rho and ONE streaming kernel over the unknowns.  No device scalar steers the loops:
// trk_osem_iterate / trk_sirt_iterate enqueue whole solves.  Vectors fp32, sums fp64 block partials in PDHG's rows of 8, no atomics.
// An unknown the CURRENT subset does not see (its reciprocal is 0) keeps its value in OSEM: a multiplicative iteration never moves a
// 0 again.  docs/kernels/ordered_subsets.md: the operations, the keep rule, the byte count.
#include "vec_internal.h"

using namespace trk;

namespace {

// ------------------------------------------------------------------ one entry of each update, ONE definition for the float4 body and the tail
// x' = (sinv > 0) ? fmaxf((x * t) * sinv, 0) : x ; d = x' - xr in fp32 (xr: the reference entry, x itself without x_ref)
template <bool HAS_XT>
__device__ __forceinline__ float osem_x_entry(float x, float t, float sinv, float xr, float xt, double& s4, double& s5, double& s6,
                                              double& s7) {
#pragma clang fp contract(off)
  const float xn = (sinv > 0.f) ? fmaxf((x * t) * sinv, 0.f) : x;
  const float d = xn - xr;
  s4 += (double)xn * (double)xn;
  s5 += (double)d * (double)d;
  if (HAS_XT) {
    const double e = (double)xn - (double)xt;
    s6 += e * e;
  }
  if (xn == 0.f) s7 += 1.0;
  return xn;
}

// d = b - w ; rho = d * rinv (d without rinv) ; s0 += d^2, s1 += rho d in fp64 from the fp32 values
template <bool HAS_R>
__device__ __forceinline__ float sirt_r_entry(float w, float b, float rinv, double& s0, double& s1) {
#pragma clang fp contract(off)
  const float d = b - w;
  const float rho = HAS_R ? d * rinv : d;
  s0 += (double)d * (double)d;
  s1 += (double)rho * (double)d;
  return rho;
}

// u = t * cinv (t without cinv) ; x' = fminf(fmaxf(fmaf(om, u, x), lo), hi) ; d = x' - xr ; s7 counts x' on a FINITE bound
template <bool HAS_C, bool HAS_XT>
__device__ __forceinline__ float sirt_x_entry(float om, float lo, float hi, float x, float t, float cinv, float xr, float xt, double& s4,
                                              double& s5, double& s6, double& s7) {
#pragma clang fp contract(off)
  const float u = HAS_C ? t * cinv : t;
  const float xn = fminf(fmaxf(fmaf(om, u, x), lo), hi);
  const float d = xn - xr;
  s4 += (double)xn * (double)xn;
  s5 += (double)d * (double)d;
  if (HAS_XT) {
    const double e = (double)xn - (double)xt;
    s6 += e * e;
  }
  if ((xn == lo && lo > -__builtin_inff()) || (xn == hi && hi < __builtin_inff())) s7 += 1.0;
  return xn;
}

// ------------------------------------------------------------------ the kernels
// A kernel writes ITS slots of ITS blocks' rows of 8 partials and leaves the rest as it finds them: the caller zeroes.
__device__ __forceinline__ void store_x_sums(double s4, double s5, double s6, double s7, bool has_xt, double* lds, double* partials) {
  s4 = block_sum<NT>(s4, lds);
  s5 = block_sum<NT>(s5, lds);
  if (has_xt) s6 = block_sum<NT>(s6, lds);
  s7 = block_sum<NT>(s7, lds);
  if (threadIdx.x == 0) {
    partials[blockIdx.x * 8 + 4] = s4;
    partials[blockIdx.x * 8 + 5] = s5;
    partials[blockIdx.x * 8 + 6] = has_xt ? s6 : 0.0;
    partials[blockIdx.x * 8 + 7] = s7;
  }
}

// x_new may be x (read, then written by the same thread): no __restrict__ on the two.
template <bool HAS_REF, bool HAS_XT, bool VEC>
__global__ __launch_bounds__(NT) void k_osem_update(int64_t n, const float* x, const float* __restrict__ t,
                                                    const float* __restrict__ sinv, const float* __restrict__ x_ref,
                                                    const float* __restrict__ x_true, float* x_new, double* __restrict__ partials) {
  __shared__ double lds[NT / 64];
  double s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      const float4 xv = ld4(x, i), tv = ld4(t, i), sv = ld4(sinv, i);
      const float4 rv = HAS_REF ? ld4(x_ref, i) : xv;
      const float4 ev = HAS_XT ? ld4(x_true, i) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 xn;
      xn.x = osem_x_entry<HAS_XT>(xv.x, tv.x, sv.x, rv.x, ev.x, s4, s5, s6, s7);
      xn.y = osem_x_entry<HAS_XT>(xv.y, tv.y, sv.y, rv.y, ev.y, s4, s5, s6, s7);
      xn.z = osem_x_entry<HAS_XT>(xv.z, tv.z, sv.z, rv.z, ev.z, s4, s5, s6, s7);
      xn.w = osem_x_entry<HAS_XT>(xv.w, tv.w, sv.w, rv.w, ev.w, s4, s5, s6, s7);
      st4(x_new, i, xn);
    }
  }
  for (int64_t i = tail + tid; i < n; i += nth) {
    const float xi = x[i];
    x_new[i] = osem_x_entry<HAS_XT>(xi, t[i], sinv[i], HAS_REF ? x_ref[i] : xi, HAS_XT ? x_true[i] : 0.f, s4, s5, s6, s7);
  }
  store_x_sums(s4, s5, s6, s7, HAS_XT, lds, partials);
}

// rho may be w (an entry is read and then written by the same thread): no __restrict__ on the two.
template <bool HAS_R, bool VEC>
__global__ __launch_bounds__(NT) void k_sirt_residual(int64_t m, const float* __restrict__ rinv, const float* w,
                                                      const float* __restrict__ b, float* rho, double* __restrict__ partials) {
  __shared__ double lds[NT / 64];
  double s0 = 0.0, s1 = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail = 0;
  if (VEC) {
    const int64_t m4 = m >> 2;
    tail = m4 << 2;
    for (int64_t i = tid; i < m4; i += nth) {
      const float4 wv = ld4(w, i), bv = ld4(b, i);
      const float4 iv = HAS_R ? ld4(rinv, i) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 rv;
      rv.x = sirt_r_entry<HAS_R>(wv.x, bv.x, iv.x, s0, s1);
      rv.y = sirt_r_entry<HAS_R>(wv.y, bv.y, iv.y, s0, s1);
      rv.z = sirt_r_entry<HAS_R>(wv.z, bv.z, iv.z, s0, s1);
      rv.w = sirt_r_entry<HAS_R>(wv.w, bv.w, iv.w, s0, s1);
      st4(rho, i, rv);
    }
  }
  for (int64_t i = tail + tid; i < m; i += nth) rho[i] = sirt_r_entry<HAS_R>(w[i], b[i], HAS_R ? rinv[i] : 0.f, s0, s1);
  s0 = block_sum<NT>(s0, lds);
  s1 = block_sum<NT>(s1, lds);
  if (threadIdx.x == 0) {
    partials[blockIdx.x * 8 + 0] = s0;
    partials[blockIdx.x * 8 + 1] = s1;
  }
}

// x_new may be x (read, then written by the same thread): no __restrict__ on the two.
template <bool HAS_C, bool HAS_REF, bool HAS_XT, bool VEC>
__global__ __launch_bounds__(NT) void k_sirt_update(int64_t n, float om, float lo, float hi, const float* x, const float* __restrict__ t,
                                                    const float* __restrict__ cinv, const float* __restrict__ x_ref,
                                                    const float* __restrict__ x_true, float* x_new, double* __restrict__ partials) {
  __shared__ double lds[NT / 64];
  double s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      const float4 xv = ld4(x, i), tv = ld4(t, i);
      const float4 cv = HAS_C ? ld4(cinv, i) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 rv = HAS_REF ? ld4(x_ref, i) : xv;
      const float4 ev = HAS_XT ? ld4(x_true, i) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 xn;
      xn.x = sirt_x_entry<HAS_C, HAS_XT>(om, lo, hi, xv.x, tv.x, cv.x, rv.x, ev.x, s4, s5, s6, s7);
      xn.y = sirt_x_entry<HAS_C, HAS_XT>(om, lo, hi, xv.y, tv.y, cv.y, rv.y, ev.y, s4, s5, s6, s7);
      xn.z = sirt_x_entry<HAS_C, HAS_XT>(om, lo, hi, xv.z, tv.z, cv.z, rv.z, ev.z, s4, s5, s6, s7);
      xn.w = sirt_x_entry<HAS_C, HAS_XT>(om, lo, hi, xv.w, tv.w, cv.w, rv.w, ev.w, s4, s5, s6, s7);
      st4(x_new, i, xn);
    }
  }
  for (int64_t i = tail + tid; i < n; i += nth) {
    const float xi = x[i];
    x_new[i] = sirt_x_entry<HAS_C, HAS_XT>(om, lo, hi, xi, t[i], HAS_C ? cinv[i] : 0.f, HAS_REF ? x_ref[i] : xi,
                                           HAS_XT ? x_true[i] : 0.f, s4, s5, s6, s7);
  }
  store_x_sums(s4, s5, s6, s7, HAS_XT, lds, partials);
}

inline bool finite_nonneg(double v) { return v >= 0.0 && v < __builtin_inf(); }

// What the two loops check of the subsets before the first launch; *need: the largest block count of a sub-step's kernels.
int check_subsets(const char* who, trk_op* const* ops, int S, const int* order, const int64_t* row_off, int64_t* n_out, int* need) {
  TRK_REQUIRE(S >= 1, "%s: need S >= 1", who);
  TRK_REQUIRE(ops && order && row_off, "%s: NULL argument", who);
  TRK_REQUIRE(row_off[0] == 0, "%s: row_off must start at 0", who);
  int64_t m_max = 0;
  for (int s = 0; s < S; ++s) {
    TRK_REQUIRE(ops[s], "%s: NULL operator (subset %d)", who, s);
    TRK_REQUIRE(row_off[s + 1] > row_off[s], "%s: row_off must be increasing (subset %d)", who, s);
    TRK_REQUIRE(ops[s]->rows == row_off[s + 1] - row_off[s], "%s: subset %d has %lld rows, row_off says %lld", who, s,
                (long long)ops[s]->rows, (long long)(row_off[s + 1] - row_off[s]));
    TRK_REQUIRE(ops[s]->cols == ops[0]->cols, "%s: the subsets must share their columns (subset %d)", who, s);
    if (ops[s]->rows > m_max) m_max = ops[s]->rows;
    TRK_REQUIRE(order[s] >= 0 && order[s] < S, "%s: order is not a permutation of 0 .. S-1", who);
    for (int j = 0; j < s; ++j) TRK_REQUIRE(order[j] != order[s], "%s: order is not a permutation of 0 .. S-1", who);
  }
  *n_out = ops[0]->cols;
  *need = stream_grid(m_max > *n_out ? m_max : *n_out);
  return TRK_OK;
}

// Where sub-step `pos` of pass k reads and writes: the first reads the pass's start iterate, the last writes the slot, measures its
// step from the start iterate and its error from x_true; everything in between lives in xw.
struct SubStep {
  const float* x_in;
  float* x_out;
  const float *x_ref, *x_true;
  double* part;
};
inline SubStep substep(int pos, int S, int k, const float* x_start, float* xw, float* x_slot, const float* x_true, double* NP, int cap) {
  const bool first = pos == 0, last = pos == S - 1;
  return {first ? x_start : xw, last ? x_slot : xw, (last && !first) ? x_start : nullptr, last ? x_true : nullptr,
          NP + 8 * (int64_t)cap * ((int64_t)(k - 1) * S + pos)};
}

}  // namespace

// ======================================================================================= C ABI
extern "C" {

int trk_subsets_blocks(int64_t m_max, int64_t n, int* blocks) {
  TRK_REQUIRE(blocks && m_max >= 1 && n >= 1, "trk_subsets_blocks: need m_max, n >= 1");
  *blocks = stream_grid(m_max > n ? m_max : n);
  return TRK_OK;
}

int trk_osem_update(int64_t n, const float* x, const float* t, const float* sinv, const float* x_ref, const float* x_true, float* x_new,
                    double* partials, int capacity_blocks, int* n_blocks, trk_stream st) {
  TRK_REQUIRE(x && t && sinv && x_new && partials && n_blocks, "trk_osem_update: NULL argument");
  TRK_REQUIRE(n >= 1, "trk_osem_update: need n >= 1");
  TRK_REQUIRE(x_new != t && x_new != sinv && x_new != x_true && x_new != x_ref, "trk_osem_update: x_new may alias x only");
  const int grid = stream_grid(n);
  TRK_REQUIRE(grid <= capacity_blocks, "trk_osem_update: partial buffer too small (%d blocks needed)", grid);
  *n_blocks = grid;
  const bool vec = aligned16(x) && aligned16(t) && aligned16(sinv) && aligned16(x_new) && (!x_ref || aligned16(x_ref)) &&
                   (!x_true || aligned16(x_true));
  with_bools([&](auto HAS_REF, auto HAS_XT, auto VEC) {
    hipLaunchKernelGGL((k_osem_update<HAS_REF, HAS_XT, VEC>), dim3(grid), dim3(NT), 0, (hipStream_t)st, n, x, t, sinv, x_ref, x_true, x_new,
                       partials);
  }, x_ref != nullptr, x_true != nullptr, vec);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_sirt_residual(int64_t m, const float* rinv, const float* w, const float* b, float* rho, double* partials, int capacity_blocks,
                      int* n_blocks, trk_stream st) {
  TRK_REQUIRE(w && b && rho && partials && n_blocks, "trk_sirt_residual: NULL argument");
  TRK_REQUIRE(m >= 1, "trk_sirt_residual: need m >= 1");
  TRK_REQUIRE(rho != b && rho != rinv, "trk_sirt_residual: rho may alias w only");
  const int grid = stream_grid(m);
  TRK_REQUIRE(grid <= capacity_blocks, "trk_sirt_residual: partial buffer too small (%d blocks needed)", grid);
  *n_blocks = grid;
  with_bools([&](auto HAS_R, auto VEC) {
    hipLaunchKernelGGL((k_sirt_residual<HAS_R, VEC>), dim3(grid), dim3(NT), 0, (hipStream_t)st, m, rinv, w, b, rho, partials);
  }, rinv != nullptr, aligned16(w) && aligned16(b) && aligned16(rho) && (!rinv || aligned16(rinv)));
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_sirt_update(int64_t n, double omega, double lo, double hi, const float* x, const float* t, const float* cinv, const float* x_ref,
                    const float* x_true, float* x_new, double* partials, int capacity_blocks, int* n_blocks, trk_stream st) {
  TRK_REQUIRE(x && t && x_new && partials && n_blocks, "trk_sirt_update: NULL argument");
  TRK_REQUIRE(n >= 1, "trk_sirt_update: need n >= 1");
  TRK_REQUIRE(omega > 0.0 && omega < __builtin_inf(), "trk_sirt_update: omega must be finite and > 0");
  TRK_REQUIRE(lo <= hi, "trk_sirt_update: need lo <= hi");                       // (a NaN bound fails this too)
  TRK_REQUIRE(x_new != t && x_new != cinv && x_new != x_true && x_new != x_ref, "trk_sirt_update: x_new may alias x only");
  const int grid = stream_grid(n);
  TRK_REQUIRE(grid <= capacity_blocks, "trk_sirt_update: partial buffer too small (%d blocks needed)", grid);
  *n_blocks = grid;
  const bool vec = aligned16(x) && aligned16(t) && aligned16(x_new) && (!cinv || aligned16(cinv)) && (!x_ref || aligned16(x_ref)) &&
                   (!x_true || aligned16(x_true));
  with_bools([&](auto HAS_C, auto HAS_REF, auto HAS_XT, auto VEC) {
    hipLaunchKernelGGL((k_sirt_update<HAS_C, HAS_REF, HAS_XT, VEC>), dim3(grid), dim3(NT), 0, (hipStream_t)st, n, (float)omega, (float)lo,
                       (float)hi, x, t, cinv, x_ref, x_true, x_new, partials);
  }, cinv != nullptr, x_ref != nullptr, x_true != nullptr, vec);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_osem_iterate(trk_op* const* ops, int S, const int* order, const int64_t* row_off, int k_first, int n_iters, double bg,
                     const float* bg_vec, const float* b, const float* SINV, int64_t sinv_ld, float* w, float* t, float* xw, float* X,
                     int64_t x_ld, int keep_history, const float* x_prev, const float* x_true, double* NP, int np_capacity_blocks,
                     trk_stream stream) {
  TRK_REQUIRE(b && SINV && w && t && X && x_prev && NP, "trk_osem_iterate: NULL argument");
  int64_t n = 0;
  int need = 0, rc;
  if ((rc = check_subsets("trk_osem_iterate", ops, S, order, row_off, &n, &need))) return rc;
  TRK_REQUIRE(S == 1 || (xw && xw != x_prev), "trk_osem_iterate: S > 1 needs a scratch iterate xw of its own");
  TRK_REQUIRE(k_first >= 1 && n_iters >= 0, "trk_osem_iterate: need k_first >= 1, n_iters >= 0");
  TRK_REQUIRE(bg_vec || finite_nonneg(bg), "trk_osem_iterate: the background must be finite and >= 0");
  TRK_REQUIRE(x_ld >= n && sinv_ld >= n, "trk_osem_iterate: need x_ld, sinv_ld >= the columns of the subsets");
  TRK_REQUIRE(need <= np_capacity_blocks, "trk_osem_iterate: partial buffer too small (%d blocks needed)", need);
  for (int k = k_first; k < k_first + n_iters; ++k) {
    float* x_new = X + (int64_t)(keep_history ? (k - 1) : ((k - 1) & 1)) * x_ld;
    for (int pos = 0; pos < S; ++pos) {
      const int s = order[pos];
      const int64_t off = row_off[s], ms = row_off[s + 1] - off;
      const SubStep ss = substep(pos, S, k, x_prev, xw, x_new, x_true, NP, np_capacity_blocks);
      int nb = 0;
      if ((rc = trk_op_apply(ops[s], 0, ss.x_in, 0, w, 0, 1, nullptr, stream))) return rc;                       // w = A_s x
      if ((rc = trk_mlem_ratio(ms, bg, bg_vec ? bg_vec + off : nullptr, w, b + off, w, ss.part, np_capacity_blocks, &nb, stream)))
        return rc;                                                                                             // rho over w
      if ((rc = trk_op_apply(ops[s], 1, w, 0, t, 0, 1, nullptr, stream))) return rc;                          // t = A_s^T rho
      if ((rc = trk_osem_update(n, ss.x_in, t, SINV + (int64_t)s * sinv_ld, ss.x_ref, ss.x_true, ss.x_out, ss.part,
                                np_capacity_blocks, &nb, stream)))
        return rc;
    }
    x_prev = x_new;
  }
  return TRK_OK;
}

int trk_sirt_iterate(trk_op* const* ops, int S, const int* order, const int64_t* row_off, int k_first, int n_iters, const float* b,
                     const float* RINV, const float* CINV, int64_t cinv_ld, double omega, double lo, double hi, float* w, float* t,
                     float* xw, float* X, int64_t x_ld, int keep_history, const float* x_prev, const float* x_true, double* NP,
                     int np_capacity_blocks, trk_stream stream) {
  TRK_REQUIRE(b && w && t && X && x_prev && NP, "trk_sirt_iterate: NULL argument");
  int64_t n = 0;
  int need = 0, rc;
  if ((rc = check_subsets("trk_sirt_iterate", ops, S, order, row_off, &n, &need))) return rc;
  TRK_REQUIRE(S == 1 || (xw && xw != x_prev), "trk_sirt_iterate: S > 1 needs a scratch iterate xw of its own");
  TRK_REQUIRE(k_first >= 1 && n_iters >= 0, "trk_sirt_iterate: need k_first >= 1, n_iters >= 0");
  TRK_REQUIRE(omega > 0.0 && omega < __builtin_inf(), "trk_sirt_iterate: omega must be finite and > 0");
  TRK_REQUIRE(lo <= hi, "trk_sirt_iterate: need lo <= hi");
  TRK_REQUIRE(x_ld >= n && (!CINV || cinv_ld >= n), "trk_sirt_iterate: need x_ld, cinv_ld >= the columns of the subsets");
  TRK_REQUIRE(need <= np_capacity_blocks, "trk_sirt_iterate: partial buffer too small (%d blocks needed)", need);
  for (int k = k_first; k < k_first + n_iters; ++k) {
    float* x_new = X + (int64_t)(keep_history ? (k - 1) : ((k - 1) & 1)) * x_ld;
    for (int pos = 0; pos < S; ++pos) {
      const int s = order[pos];
      const int64_t off = row_off[s], ms = row_off[s + 1] - off;
      const SubStep ss = substep(pos, S, k, x_prev, xw, x_new, x_true, NP, np_capacity_blocks);
      int nb = 0;
      if ((rc = trk_op_apply(ops[s], 0, ss.x_in, 0, w, 0, 1, nullptr, stream))) return rc;                       // w = A_s x
      if ((rc = trk_sirt_residual(ms, RINV ? RINV + off : nullptr, w, b + off, w, ss.part, np_capacity_blocks, &nb, stream)))
        return rc;                                                                                             // rho over w
      if ((rc = trk_op_apply(ops[s], 1, w, 0, t, 0, 1, nullptr, stream))) return rc;                          // t = A_s^T rho
      if ((rc = trk_sirt_update(n, omega, lo, hi, ss.x_in, t, CINV ? CINV + (int64_t)s * cinv_ld : nullptr, ss.x_ref,
                                ss.x_true, ss.x_out, ss.part, np_capacity_blocks, &nb, stream)))
        return rc;
    }
    x_prev = x_new;
  }
  return TRK_OK;
}

}  // extern "C"
