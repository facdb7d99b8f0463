// mrnsd.hip — MRNSD, the modified residual norm steepest descent of Nagy and Strakos (IR Tools' IRmrnsd): min ||b - A x|| over x >= 0
// by steepest descent in the x-scaled metric, the step capped where an entry would cross zero.  An iteration is u = A s, z = A^T u and
// ONE streaming kernel in the style of cgls_update.hip that carries every scalar on the device; trk_mrnsd_iterate chains them.
//
//   start        r = b - A x0 ; g = -A^T r ; s = -(x . g) ; gamma = -sum g s ; bound = min_{s_i < 0} x_i / -s_i (+inf: none) ; rho = ||r||^2
//   iteration    theta = gamma / ||u||^2 ; alpha = min(theta, bound), 0 if ||u||^2 <= 0 or gamma <= 0 ; step = (float)alpha
//                x' = max(x + step s, 0) ; g' = g + step z ; s' = -(x' g') ; r' = r - step u ; gamma', bound' from x', g', s'
// Vectors fp32, scalars and reductions fp64; no atomics: every result is reproducible from run to run.
// docs/kernels/mrnsd.md: the byte count, why r is stored, why the clamp.
#include "vec_internal.h"

using namespace trk;

namespace {

// ------------------------------------------------------------------ one entry of the update, ONE definition for the float4 body and the tail
// x' = max(fma(step, s, x), 0): (float)alpha may have rounded up past the exact bound, the clamp keeps x' >= 0 exactly.
// d = step * s is the reported direction (as the CGLS kernels take step * p), also where the clamp cut the step short.
template <bool HAS_XT>
__device__ __forceinline__ void mrnsd_entry(float step, float x, float g, float s, float z, float xt, float& xn, float& gn, float& sn,
                                            double& gam, double& bnd, double& s0, double& s1, double& s2) {
  xn = fmaxf(fmaf(step, s, x), 0.f);
  gn = fmaf(step, z, g);
  sn = -(xn * gn);
  const float d = step * s;
  gam -= (double)gn * sn;
  if (sn < 0.f) bnd = min_nan(bnd, (double)xn / -(double)sn);
  s0 += (double)xn * xn;
  s1 += (double)d * d;
  if (HAS_XT) {
    const double e = (double)xn - xt;
    s2 += e * e;
  }
}

// ------------------------------------------------------------------ the fused MRNSD update
// gamma, bound, unorm: finished scalars (n = 1) or block partials of the producing kernels — one wave of every block reduces them
// (the same order in every block: the same alpha everywhere).  The gamma' / bound' partials go to gpart / bpart, which are NOT the
// buffers gamma / bound are read from: other blocks of this launch are still reading those (the caller ping-pongs).
// norm partials: [block][4] = ||x'||^2, ||step s||^2, ||x' - x_true||^2 (0 without), ||r'||^2.
// Block 0 publishes row[0] = ||u||^2, row[1] = alpha and, with pub_gb, pub_gb[0] = gamma, pub_gb[1] = bound as it consumed them.
// x_new may be x; g, s, r are updated in place (an entry is read and then written by the same thread): no __restrict__ on them.
template <bool HAS_XT, bool VEC>
__global__ __launch_bounds__(NT) void k_mrnsd_update(int64_t n, int64_t m, ScalarSrc gamma, ScalarSrc bound, ScalarSrc unorm, const float* x,
                                                     float* x_new, float* g, float* s, const float* __restrict__ z, float* r,
                                                     const float* __restrict__ u, const float* __restrict__ x_true,
                                                     double* __restrict__ gpart, double* __restrict__ bpart,
                                                     double* __restrict__ partials, double* row, double* pub_gb) {
  __shared__ double lds[NT / 64];
  __shared__ double bc;
  if (threadIdx.x < 64) {
    const double ga = scalar_from_wave(gamma, threadIdx.x), bd = scalar_min_from_wave(bound, threadIdx.x);
    const double uu = scalar_from_wave(unorm, threadIdx.x);
    if (threadIdx.x == 0) {
      const double theta = ga / uu;
      // a broken-down state (nothing left to descend along, or A s = 0) freezes instead of turning into NaN
      const double alpha = (uu <= 0.0 || ga <= 0.0) ? 0.0 : min_nan(theta, bd);
      bc = alpha;
      if (blockIdx.x == 0) {
        if (row != unorm.p) row[0] = uu;
        row[1] = alpha;
        if (pub_gb && pub_gb != gamma.p) {
          pub_gb[0] = ga;
          pub_gb[1] = bd;
        }
      }
    }
  }
  __syncthreads();
  const float step = (float)bc;
  double gam = 0.0, bnd = __builtin_inf(), s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t ntail = 0, mtail = 0;
  if (VEC) {
    const int64_t n4 = n >> 2, m4 = m >> 2;
    ntail = n4 << 2;
    mtail = m4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      const float4 xv = ld4(x, i), gv = ld4(g, i), sv = ld4(s, i), zv = ld4(z, i);
      const float4 tv = HAS_XT ? ld4(x_true, i) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 xn, gn, sn;
      mrnsd_entry<HAS_XT>(step, xv.x, gv.x, sv.x, zv.x, tv.x, xn.x, gn.x, sn.x, gam, bnd, s0, s1, s2);
      mrnsd_entry<HAS_XT>(step, xv.y, gv.y, sv.y, zv.y, tv.y, xn.y, gn.y, sn.y, gam, bnd, s0, s1, s2);
      mrnsd_entry<HAS_XT>(step, xv.z, gv.z, sv.z, zv.z, tv.z, xn.z, gn.z, sn.z, gam, bnd, s0, s1, s2);
      mrnsd_entry<HAS_XT>(step, xv.w, gv.w, sv.w, zv.w, tv.w, xn.w, gn.w, sn.w, gam, bnd, s0, s1, s2);
      st4(x_new, i, xn);
      st4(g, i, gn);
      st4(s, i, sn);
    }
    for (int64_t i = tid; i < m4; i += nth) {
      float4 rv = ld4(r, i);
      const float4 uv = ld4(u, i);
      rv.x = fmaf(-step, uv.x, rv.x);
      rv.y = fmaf(-step, uv.y, rv.y);
      rv.z = fmaf(-step, uv.z, rv.z);
      rv.w = fmaf(-step, uv.w, rv.w);
      st4(r, i, rv);
      s3 += (double)rv.x * rv.x + (double)rv.y * rv.y + (double)rv.z * rv.z + (double)rv.w * rv.w;
    }
  }
  for (int64_t i = ntail + tid; i < n; i += nth) {
    float xn, gn, sn;
    mrnsd_entry<HAS_XT>(step, x[i], g[i], s[i], z[i], HAS_XT ? x_true[i] : 0.f, xn, gn, sn, gam, bnd, s0, s1, s2);
    x_new[i] = xn;
    g[i] = gn;
    s[i] = sn;
  }
  for (int64_t i = mtail + tid; i < m; i += nth) {
    const float rv = fmaf(-step, u[i], r[i]);
    r[i] = rv;
    s3 += (double)rv * rv;
  }
  gam = block_sum<NT>(gam, lds);
  bnd = block_min<NT>(bnd, lds);
  s0 = block_sum<NT>(s0, lds);
  s1 = block_sum<NT>(s1, lds);
  if (HAS_XT) s2 = block_sum<NT>(s2, lds);
  s3 = block_sum<NT>(s3, lds);
  if (threadIdx.x == 0) {
    gpart[blockIdx.x] = gam;
    bpart[blockIdx.x] = bnd;
    partials[blockIdx.x * 4 + 0] = s0;
    partials[blockIdx.x * 4 + 1] = s1;
    partials[blockIdx.x * 4 + 2] = HAS_XT ? s2 : 0.0;
    partials[blockIdx.x * 4 + 3] = s3;
  }
}

// ------------------------------------------------------------------ the start, and the finishing kernel
// Vector form (fin_g.n == 0): s = -(x g) and the block partials of gamma = -sum g s, bound = min_{s < 0} x / -s and ||r||^2.
// Finishing form (fin_g.n > 0, ONE block, no vectors): out[0] = S(fin_g), out[1] = min(fin_b) and, with fin_r.n > 0, out[2] = S(fin_r)
// — the reductions of k_mrnsd_update's head, the same bits: what the last iteration's row and a per-iteration read-back need.
template <bool VEC>
__global__ __launch_bounds__(NT) void k_mrnsd_init(int64_t n, int64_t m, const float* __restrict__ x, const float* __restrict__ g,
                                                   const float* __restrict__ r, float* __restrict__ s, double* __restrict__ gpart,
                                                   double* __restrict__ bpart, double* __restrict__ rpart, ScalarSrc fin_g,
                                                   ScalarSrc fin_b, ScalarSrc fin_r, double* out) {
  __shared__ double lds[NT / 64];
  if (fin_g.n > 0) {                                   // grid-uniform
    if (threadIdx.x < 64) {
      const double ga = scalar_from_wave(fin_g, threadIdx.x), bd = scalar_min_from_wave(fin_b, threadIdx.x);
      const double rho = fin_r.n > 0 ? scalar_from_wave(fin_r, threadIdx.x) : 0.0;
      if (threadIdx.x == 0 && blockIdx.x == 0) {
        out[0] = ga;
        out[1] = bd;
        if (fin_r.n > 0) out[2] = rho;
      }
    }
    return;
  }
  double gam = 0.0, bnd = __builtin_inf(), rho = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t ntail = 0, mtail = 0;
  if (VEC) {
    const int64_t n4 = n >> 2, m4 = m >> 2;
    ntail = n4 << 2;
    mtail = m4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      const float4 xv = ld4(x, i), gv = ld4(g, i);
      const float4 sv = make_float4(-(xv.x * gv.x), -(xv.y * gv.y), -(xv.z * gv.z), -(xv.w * gv.w));
      st4(s, i, sv);
      gam -= (double)gv.x * sv.x + (double)gv.y * sv.y + (double)gv.z * sv.z + (double)gv.w * sv.w;
      if (sv.x < 0.f) bnd = min_nan(bnd, (double)xv.x / -(double)sv.x);
      if (sv.y < 0.f) bnd = min_nan(bnd, (double)xv.y / -(double)sv.y);
      if (sv.z < 0.f) bnd = min_nan(bnd, (double)xv.z / -(double)sv.z);
      if (sv.w < 0.f) bnd = min_nan(bnd, (double)xv.w / -(double)sv.w);
    }
    for (int64_t i = tid; i < m4; i += nth) {
      const float4 rv = ld4(r, i);
      rho += (double)rv.x * rv.x + (double)rv.y * rv.y + (double)rv.z * rv.z + (double)rv.w * rv.w;
    }
  }
  for (int64_t i = ntail + tid; i < n; i += nth) {
    const float xv = x[i], gv = g[i], sv = -(xv * gv);
    s[i] = sv;
    gam -= (double)gv * sv;
    if (sv < 0.f) bnd = min_nan(bnd, (double)xv / -(double)sv);
  }
  for (int64_t i = mtail + tid; i < m; i += nth) rho += (double)r[i] * r[i];
  gam = block_sum<NT>(gam, lds);
  bnd = block_min<NT>(bnd, lds);
  rho = block_sum<NT>(rho, lds);
  if (threadIdx.x == 0) {
    gpart[blockIdx.x] = gam;
    bpart[blockIdx.x] = bnd;
    rpart[blockIdx.x] = rho;
  }
}

// [p, p + n) and [q, q + k) share an element
inline bool overlap(const double* p, int64_t n, const double* q, int64_t k) { return p < q + k && q < p + n; }

int launch_finish(const double* gamma, int gamma_n, const double* bound, int bound_n, const double* rho, int rho_n, double* out,
                  hipStream_t s) {
  hipLaunchKernelGGL((k_mrnsd_init<false>), dim3(1), dim3(NT), 0, s, (int64_t)0, (int64_t)0, (const float*)nullptr, (const float*)nullptr,
                     (const float*)nullptr, (float*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr,
                     ScalarSrc{gamma, gamma_n}, ScalarSrc{bound, bound_n}, ScalarSrc{rho, rho_n}, out);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

}  // namespace

// ======================================================================================= C ABI
extern "C" {

int trk_mrnsd_init(int64_t n, int64_t m, const float* x0, const float* g, const float* r, float* s, double* gb_out, int gb_capacity,
                   double* S0, int* n_blocks, trk_stream st) {
  TRK_REQUIRE(x0 && g && r && s && gb_out && S0 && n_blocks, "trk_mrnsd_init: NULL argument");
  TRK_REQUIRE(n >= 1 && m >= 1, "trk_mrnsd_init: need n >= 1, m >= 1");
  TRK_REQUIRE(s != x0 && s != g, "trk_mrnsd_init: s must not alias x0 or g");
  hipStream_t hs = (hipStream_t)st;
  const int grid = stream_grid(n > m ? n : m);
  TRK_REQUIRE(grid <= gb_capacity, "trk_mrnsd_init: partial buffer too small (%d blocks needed)", grid);
  TRK_REQUIRE(!overlap(S0, 3, gb_out, 2 * (int64_t)gb_capacity), "trk_mrnsd_init: S0 lies inside gb_out");
  double* rpart = nullptr;
  if (int rc = scratch_doubles(hs, (size_t)grid, &rpart)) return rc;
  *n_blocks = grid;
  with_bools([&](auto VEC) {
    hipLaunchKernelGGL((k_mrnsd_init<VEC>), dim3(grid), dim3(NT), 0, hs, n, m, x0, g, r, s, gb_out, gb_out + gb_capacity, rpart,
                       ScalarSrc{nullptr, 0}, ScalarSrc{nullptr, 0}, ScalarSrc{nullptr, 0}, (double*)nullptr);
  }, aligned16(x0) && aligned16(g) && aligned16(r) && aligned16(s));
  TRK_LAUNCH_CHECK();
  return launch_finish(gb_out, grid, gb_out + gb_capacity, grid, rpart, grid, S0, hs);
}

int trk_mrnsd_finish(const double* gamma, int gamma_n, const double* bound, int bound_n, double* out, trk_stream st) {
  TRK_REQUIRE(gamma && bound && out && gamma_n >= 1 && bound_n >= 1, "trk_mrnsd_finish: bad argument");
  TRK_REQUIRE(!overlap(out, 2, gamma, gamma_n) && !overlap(out, 2, bound, bound_n), "trk_mrnsd_finish: out lies inside a source");
  return launch_finish(gamma, gamma_n, bound, bound_n, nullptr, 0, out, (hipStream_t)st);
}

int trk_mrnsd_update(int64_t n, int64_t m, const double* gamma, int gamma_n, const double* bound, int bound_n, const double* unorm,
                     int unorm_n, const float* x, float* x_new, float* g, float* s, const float* z, float* r, const float* u,
                     const float* x_true, double* gb_out, int gb_capacity, double* row, double* publish_gb, double* norm_partials,
                     int capacity_blocks, int* n_blocks, trk_stream st) {
  TRK_REQUIRE(gamma && bound && unorm && x && x_new && g && s && z && r && u && gb_out && row && norm_partials && n_blocks,
              "trk_mrnsd_update: NULL argument");
  TRK_REQUIRE(gamma_n >= 1 && bound_n >= 1 && unorm_n >= 1, "trk_mrnsd_update: a scalar source needs n >= 1");
  TRK_REQUIRE(n >= 1 && m >= 1, "trk_mrnsd_update: need n >= 1, m >= 1");
  const int grid = stream_grid(n > m ? n : m);
  TRK_REQUIRE(grid <= capacity_blocks && grid <= gb_capacity, "trk_mrnsd_update: partial buffer too small (%d blocks needed)", grid);
  // the other blocks of the launch are still reading gamma / bound / unorm when a block writes its partials
  TRK_REQUIRE(!overlap(gb_out, 2 * (int64_t)gb_capacity, gamma, gamma_n) && !overlap(gb_out, 2 * (int64_t)gb_capacity, bound, bound_n) &&
              !overlap(gb_out, 2 * (int64_t)gb_capacity, unorm, unorm_n),
              "trk_mrnsd_update: gb_out must be another buffer than the scalar sources (ping-pong)");
  // (a finished ||u||^2 may already sit in row[0], where the operator left it)
  TRK_REQUIRE(!overlap(row, 2, gamma, gamma_n) && !overlap(row, 2, bound, bound_n) && !overlap(row, 2, gb_out, 2 * (int64_t)gb_capacity) &&
              ((unorm_n == 1 && unorm == row) || !overlap(row, 2, unorm, unorm_n)),
              "trk_mrnsd_update: row lies inside a scalar source or gb_out");
  TRK_REQUIRE(!publish_gb || publish_gb == gamma ||
              (!overlap(publish_gb, 2, gamma, gamma_n) && !overlap(publish_gb, 2, bound, bound_n) && !overlap(publish_gb, 2, unorm, unorm_n)),
              "trk_mrnsd_update: publish_gb lies inside a scalar source");
  TRK_REQUIRE(publish_gb != gamma || (gamma_n == 1 && bound_n == 1 && bound == gamma + 1),
              "trk_mrnsd_update: publish_gb == gamma needs finished scalars with bound behind gamma");
  *n_blocks = grid;
  const bool vec = aligned16(x) && aligned16(x_new) && aligned16(g) && aligned16(s) && aligned16(z) && aligned16(r) && aligned16(u) &&
                   (!x_true || aligned16(x_true));
  const ScalarSrc ga{gamma, gamma_n}, bd{bound, bound_n}, uu{unorm, unorm_n};
  hipStream_t hs = (hipStream_t)st;
  with_bools([&](auto HAS_XT, auto VEC) {
    hipLaunchKernelGGL((k_mrnsd_update<HAS_XT, VEC>), dim3(grid), dim3(NT), 0, hs, n, m, ga, bd, uu, x, x_new, g, s, z, r, u, x_true, gb_out,
                       gb_out + gb_capacity, norm_partials, row, publish_gb);
  }, x_true != nullptr, vec);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_mrnsd_iterate(trk_op* A, int k_first, int n_iters, float* g, float* s, float* z, float* r, float* u, float* X, int64_t x_ld,
                      int keep_history, const float* x_prev, const float* x_true, double* S, double* GB, int gb_capacity, double* NP,
                      int np_capacity_blocks, int* n_np_inout, double* PU, int pcap, trk_stream stream) {
  TRK_REQUIRE(A && g && s && z && r && u && X && x_prev && S && GB && NP && n_np_inout, "trk_mrnsd_iterate: NULL argument");
  TRK_REQUIRE(k_first >= 1 && n_iters >= 0, "trk_mrnsd_iterate: need k_first >= 1, n_iters >= 0");
  TRK_REQUIRE(*n_np_inout >= 1 && *n_np_inout <= gb_capacity,
              "trk_mrnsd_iterate: *n_np_inout must be the block count trk_mrnsd_init returned");
  const int64_t m = A->rows, n = A->cols;
  int n_np = *n_np_inout;
  int caps = 0;
  if (int rc = trk_op_fused_caps(A, &caps)) return rc;
  const bool raw = PU && pcap > 0 && caps != 0;      // the operator leaves ||u||^2 as raw block partials: no finalize launch
  for (int k = k_first; k < k_first + n_iters; ++k) {
    double* row = S + 8 * (int64_t)k;                  // [||u||^2, alpha, gamma_k, bound_k, ||x||^2, ||dx||^2, ||x-xt||^2, ||r||^2]
    float* x_new = X + (int64_t)(keep_history ? (k - 1) : ((k - 1) & 1)) * x_ld;
    const double* src = GB + (int64_t)((k - 1) & 1) * 2 * gb_capacity;     // gamma_{k-1} | bound_{k-1} partials
    double* dst = GB + (int64_t)(k & 1) * 2 * gb_capacity;
    int n_u = 1, rc;
    if (raw) rc = trk_op_apply_fused(A, 0, s, nullptr, 0.0, nullptr, 0, nullptr, 0, nullptr, u, PU, pcap, &n_u, stream);
    else rc = trk_op_apply(A, 0, s, 0, u, 0, 1, row, stream);                                   // u = A s, ||u||^2
    if (rc) return rc;
    rc = trk_op_apply(A, 1, u, 0, z, 0, 1, nullptr, stream);                                    // z = A^T u
    if (rc) return rc;
    rc = trk_mrnsd_update(n, m, src, n_np, src + gb_capacity, n_np, raw ? PU : row, raw ? n_u : 1, x_prev, x_new, g, s, z, r, u, x_true,
                          dst, gb_capacity, row, k == 1 ? S : row - 6, NP + 4 * (int64_t)n_np * (k - 1), np_capacity_blocks, &n_np,
                          stream);
    if (rc) return rc;
    x_prev = x_new;
  }
  *n_np_inout = n_np;
  return TRK_OK;
}

}  // extern "C"
