// mlem.hip — MLEM / Richardson-Lucy: maximise the Poisson likelihood of b ~ Poisson(A x + beta), i.e. min KL(b, A x + beta) over x >= 0,
//   x_k = x_{k-1} . A^T(b / (A x_{k-1} + beta)) / (A^T 1)
// with beta >= 0 a known background (a scalar or an m-vector) and A^T the operator's own transpose, also behind s = A^T 1.
// An iteration is w = A x, ONE streaming kernel over the data (rho = b / (w + beta), the KL value and the residual), t = A^T rho and ONE
// streaming kernel over the unknowns (x' = x t / s and its norms).  No device scalar steers the loop: trk_mlem_iterate enqueues a
// whole solve.  Vectors fp32, sums fp64 block partials in the rows of 8 of PDHG (include/trk.h), no atomics: every result is
// reproducible from run to run.  docs/kernels/mlem.md: the byte count, the out-of-domain rule, what s_i = 0 does.
#include "vec_internal.h"
#include "kl_internal.h"

using namespace trk;

namespace {

// ------------------------------------------------------------------ one entry of each update, ONE definition for the float4 body and the tail
// y = w + bg ; rho = (y > 0) ? b / y : 0 (the correctly rounded fp32 division) ; s0 += kl(b, y) ; s1 += (y - b)^2 in fp64
__device__ __forceinline__ float mlem_ratio_entry(float w, float bg, float b, double& s0, double& s1) {
#pragma clang fp contract(off)
  const float y = w + bg;
  const float rho = (y > 0.f) ? b / y : 0.f;
  const double e = (double)y - (double)b;
  s0 += kl_term(b, y);
  s1 += e * e;
  return rho;
}

// x' = fmaxf((x * t) * sinv, 0) ; d = x' - x in fp32 ; s4 += x'^2, s5 += d^2, s6 += (x' - x_true)^2, s7 += 1 where x' == 0
template <bool HAS_XT>
__device__ __forceinline__ float mlem_x_entry(float x, float t, float sinv, float xt, double& s4, double& s5, double& s6, double& s7) {
#pragma clang fp contract(off)
  const float xn = fmaxf((x * t) * sinv, 0.f);
  const float d = xn - x;
  s4 += (double)xn * (double)xn;
  s5 += (double)d * (double)d;
  if (HAS_XT) {
    const double e = (double)xn - (double)xt;
    s6 += e * e;
  }
  if (xn == 0.f) s7 += 1.0;
  return xn;
}

// ------------------------------------------------------------------ the kernels
// A kernel writes ITS slots of ITS blocks' rows of 8 partials and leaves the rest as it finds them: the caller zeroes.
// rho may be w (an entry is read and then written by the same thread): no __restrict__ on the two.
template <bool VEC, bool BG_VEC>
__global__ __launch_bounds__(NT) void k_mlem_ratio(int64_t m, float bg, const float* __restrict__ bgv, const float* w,
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
      const float4 gv = BG_VEC ? ld4(bgv, i) : make_float4(bg, bg, bg, bg);
      float4 rv;
      rv.x = mlem_ratio_entry(wv.x, gv.x, bv.x, s0, s1);
      rv.y = mlem_ratio_entry(wv.y, gv.y, bv.y, s0, s1);
      rv.z = mlem_ratio_entry(wv.z, gv.z, bv.z, s0, s1);
      rv.w = mlem_ratio_entry(wv.w, gv.w, bv.w, s0, s1);
      st4(rho, i, rv);
    }
  }
  for (int64_t i = tail + tid; i < m; i += nth) rho[i] = mlem_ratio_entry(w[i], BG_VEC ? bgv[i] : bg, b[i], s0, s1);
  s0 = block_sum<NT>(s0, lds);
  s1 = block_sum<NT>(s1, lds);
  if (threadIdx.x == 0) {
    partials[blockIdx.x * 8 + 0] = s0;
    partials[blockIdx.x * 8 + 1] = s1;
  }
}

// x_new may be x (read, then written by the same thread): no __restrict__ on the two.
template <bool HAS_XT, bool VEC>
__global__ __launch_bounds__(NT) void k_mlem_update(int64_t n, const float* x, const float* __restrict__ t,
                                                    const float* __restrict__ sinv, const float* __restrict__ x_true, float* x_new,
                                                    double* __restrict__ partials) {
  __shared__ double lds[NT / 64];
  double s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      const float4 xv = ld4(x, i), tv = ld4(t, i), sv = ld4(sinv, i);
      const float4 ev = HAS_XT ? ld4(x_true, i) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 xn;
      xn.x = mlem_x_entry<HAS_XT>(xv.x, tv.x, sv.x, ev.x, s4, s5, s6, s7);
      xn.y = mlem_x_entry<HAS_XT>(xv.y, tv.y, sv.y, ev.y, s4, s5, s6, s7);
      xn.z = mlem_x_entry<HAS_XT>(xv.z, tv.z, sv.z, ev.z, s4, s5, s6, s7);
      xn.w = mlem_x_entry<HAS_XT>(xv.w, tv.w, sv.w, ev.w, s4, s5, s6, s7);
      st4(x_new, i, xn);
    }
  }
  for (int64_t i = tail + tid; i < n; i += nth)
    x_new[i] = mlem_x_entry<HAS_XT>(x[i], t[i], sinv[i], HAS_XT ? x_true[i] : 0.f, s4, s5, s6, s7);
  s4 = block_sum<NT>(s4, lds);
  s5 = block_sum<NT>(s5, lds);
  if (HAS_XT) s6 = block_sum<NT>(s6, lds);
  s7 = block_sum<NT>(s7, lds);
  if (threadIdx.x == 0) {
    partials[blockIdx.x * 8 + 4] = s4;
    partials[blockIdx.x * 8 + 5] = s5;
    partials[blockIdx.x * 8 + 6] = HAS_XT ? s6 : 0.0;
    partials[blockIdx.x * 8 + 7] = s7;
  }
}

// sinv = (s > 0) ? 1 / s : 0 (the correctly rounded fp32 division); sinv may be s.
template <bool VEC>
__global__ __launch_bounds__(NT) void k_mlem_sinv(int64_t n, const float* s, float* sinv) {
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      float4 v = ld4(s, i);
      v.x = v.x > 0.f ? 1.f / v.x : 0.f;
      v.y = v.y > 0.f ? 1.f / v.y : 0.f;
      v.z = v.z > 0.f ? 1.f / v.z : 0.f;
      v.w = v.w > 0.f ? 1.f / v.w : 0.f;
      st4(sinv, i, v);
    }
  }
  for (int64_t i = tail + tid; i < n; i += nth) {
    const float v = s[i];
    sinv[i] = v > 0.f ? 1.f / v : 0.f;
  }
}

inline bool finite_nonneg(double v) { return v >= 0.0 && v < __builtin_inf(); }

}  // namespace

// ======================================================================================= C ABI
extern "C" {

int trk_mlem_blocks(int64_t m, int64_t n, int* blocks) {
  TRK_REQUIRE(blocks && m >= 1 && n >= 1, "trk_mlem_blocks: need m, n >= 1");
  *blocks = stream_grid(m > n ? m : n);
  return TRK_OK;
}

int trk_mlem_sinv(int64_t n, const float* s, float* sinv, trk_stream st) {
  TRK_REQUIRE(s && sinv, "trk_mlem_sinv: NULL argument");
  TRK_REQUIRE(n >= 1, "trk_mlem_sinv: need n >= 1");
  const int grid = stream_grid(n);
  with_bools([&](auto VEC) { hipLaunchKernelGGL((k_mlem_sinv<VEC>), dim3(grid), dim3(NT), 0, (hipStream_t)st, n, s, sinv); },
             aligned16(s) && aligned16(sinv));
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_mlem_ratio(int64_t m, double bg, const float* bg_vec, const float* w, const float* b, float* rho, double* partials,
                   int capacity_blocks, int* n_blocks, trk_stream st) {
  TRK_REQUIRE(w && b && rho && partials && n_blocks, "trk_mlem_ratio: NULL argument");
  TRK_REQUIRE(m >= 1, "trk_mlem_ratio: need m >= 1");
  TRK_REQUIRE(bg_vec || finite_nonneg(bg), "trk_mlem_ratio: the background must be finite and >= 0");
  TRK_REQUIRE(rho != b && rho != bg_vec, "trk_mlem_ratio: rho may alias w only");
  const int grid = stream_grid(m);
  TRK_REQUIRE(grid <= capacity_blocks, "trk_mlem_ratio: partial buffer too small (%d blocks needed)", grid);
  *n_blocks = grid;
  with_bools([&](auto VEC, auto BG_VEC) {
    hipLaunchKernelGGL((k_mlem_ratio<VEC, BG_VEC>), dim3(grid), dim3(NT), 0, (hipStream_t)st, m, (float)bg, bg_vec, w, b, rho, partials);
  }, aligned16(w) && aligned16(b) && aligned16(rho) && (!bg_vec || aligned16(bg_vec)), bg_vec != nullptr);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_mlem_update(int64_t n, const float* x, const float* t, const float* sinv, const float* x_true, float* x_new, double* partials,
                    int capacity_blocks, int* n_blocks, trk_stream st) {
  TRK_REQUIRE(x && t && sinv && x_new && partials && n_blocks, "trk_mlem_update: NULL argument");
  TRK_REQUIRE(n >= 1, "trk_mlem_update: need n >= 1");
  TRK_REQUIRE(x_new != t && x_new != sinv && x_new != x_true, "trk_mlem_update: x_new may alias x only");
  const int grid = stream_grid(n);
  TRK_REQUIRE(grid <= capacity_blocks, "trk_mlem_update: partial buffer too small (%d blocks needed)", grid);
  *n_blocks = grid;
  const bool vec = aligned16(x) && aligned16(t) && aligned16(sinv) && aligned16(x_new) && (!x_true || aligned16(x_true));
  with_bools([&](auto HAS_XT, auto VEC) {
    hipLaunchKernelGGL((k_mlem_update<HAS_XT, VEC>), dim3(grid), dim3(NT), 0, (hipStream_t)st, n, x, t, sinv, x_true, x_new, partials);
  }, x_true != nullptr, vec);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_mlem_iterate(trk_op* A, int k_first, int n_iters, double bg, const float* bg_vec, const float* b, const float* sinv, float* w,
                     float* t, float* X, int64_t x_ld, int keep_history, const float* x_prev, const float* x_true, double* NP,
                     int np_capacity_blocks, trk_stream stream) {
  TRK_REQUIRE(A && b && sinv && w && t && X && x_prev && NP, "trk_mlem_iterate: NULL argument");
  TRK_REQUIRE(k_first >= 1 && n_iters >= 0, "trk_mlem_iterate: need k_first >= 1, n_iters >= 0");
  TRK_REQUIRE(bg_vec || finite_nonneg(bg), "trk_mlem_iterate: the background must be finite and >= 0");
  const int64_t m = A->rows, n = A->cols;
  TRK_REQUIRE(x_ld >= n, "trk_mlem_iterate: need x_ld >= the columns of A");
  const int need = stream_grid(m > n ? m : n);
  TRK_REQUIRE(need <= np_capacity_blocks, "trk_mlem_iterate: partial buffer too small (%d blocks needed)", need);
  for (int k = k_first; k < k_first + n_iters; ++k) {
    double* part = NP + 8 * (int64_t)np_capacity_blocks * (k - 1);
    float* x_new = X + (int64_t)(keep_history ? (k - 1) : ((k - 1) & 1)) * x_ld;
    int nb = 0, rc;
    if ((rc = trk_op_apply(A, 0, x_prev, 0, w, 0, 1, nullptr, stream))) return rc;                     // w = A x
    if ((rc = trk_mlem_ratio(m, bg, bg_vec, w, b, w, part, np_capacity_blocks, &nb, stream))) return rc;   // rho over w
    if ((rc = trk_op_apply(A, 1, w, 0, t, 0, 1, nullptr, stream))) return rc;                          // t = A^T rho
    if ((rc = trk_mlem_update(n, x_prev, t, sinv, x_true, x_new, part, np_capacity_blocks, &nb, stream))) return rc;
    x_prev = x_new;
  }
  return TRK_OK;
}

}  // extern "C"
