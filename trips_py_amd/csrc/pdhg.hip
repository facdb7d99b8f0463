// pdhg.hip — the primal-dual hybrid gradient iteration (Chambolle and Pock 2011, algorithm 1, theta = 1) for
//   min_x  1/2 ||A x - b||^2 + lam ||L x||_1   subject to  lo <= x <= hi
// with K = [A; L], duals p (rows of A) and q (rows of L), and the extrapolated point xbar = 2 x_k - x_{k-1}:
//   w = A xbar ;  p' = (p + sig (w - b)) / (1 + sig)
//   u = L xbar ;  q' = clip(q + sig u, -lam, lam)
//   z = A^T p' ;  v = L^T q' ;  x' = clip(x - tau (z + v), lo, hi) ;  xbar' = 2 x' - x
// Isotropic TV (the *_iso entry points): lam sum_g ||(L x)_g||_2 with the groups of a geometry (N, frames) on the first-difference
// row layout (include/trk.h); q' = every group of q + sig u projected onto the 2-norm ball of radius lam, everything else unchanged.
// The grouped rows run on k_pdhg_tv_dual<kPairs, false> (pdhg_tv.hip: the column-thread layout), the tail rows on k_pdhg_dual_q below.
// Isotropic space-time TV (the *_iso3 entry points): the groups (h, v, t) of a voxel on the space-time row layout, one kernel
// (k_pdhg_tv_dual<kTriples, false>) or, on the space-time handle, the fused pair k_pdhg_tv_dual<kTriples, true> /
// k_pdhg_tv_primal<., true> of pdhg_tv.hip.
// sig, tau, lam, lo, hi are host constants: nothing is read back inside the loop and trk_pdhg_iterate enqueues a whole solve.
// The three streaming kernels are here; the fused forms for the first differences (no vector of the length of L xbar or L^T q
// in memory) are in pdhg_tv.hip and share one entry (pdhg_internal.h).  Vectors fp32, sums fp64 block partials, no atomics: every
// result is reproducible from run to run.  docs/kernels/pdhg.md: the byte count, why xbar is stored.
#include "vec_internal.h"
#include "pdhg_internal.h"

using namespace trk;

namespace {

// A kernel writes ITS slots of ITS blocks' rows of 8 partials (include/trk.h) and leaves the rest as it finds them: the caller zeroes.
// p in place (an entry is read and then written by the same thread): no __restrict__ on it.
template <bool VEC>
__global__ __launch_bounds__(NT) void k_pdhg_dual_p(int64_t m, float sig, float c, const float* __restrict__ w,
                                                    const float* __restrict__ b, float* p, double* __restrict__ partials) {
  __shared__ double lds[NT / 64];
  double s0 = 0.0, s2 = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail = 0;
  if (VEC) {
    const int64_t m4 = m >> 2;
    tail = m4 << 2;
    for (int64_t i = tid; i < m4; i += nth) {
      const float4 wv = ld4(w, i), bv = ld4(b, i);
      float4 pv = ld4(p, i);
      pv.x = pdhg_p_entry(sig, c, wv.x, bv.x, pv.x, s0, s2);
      pv.y = pdhg_p_entry(sig, c, wv.y, bv.y, pv.y, s0, s2);
      pv.z = pdhg_p_entry(sig, c, wv.z, bv.z, pv.z, s0, s2);
      pv.w = pdhg_p_entry(sig, c, wv.w, bv.w, pv.w, s0, s2);
      st4(p, i, pv);
    }
  }
  for (int64_t i = tail + tid; i < m; i += nth) p[i] = pdhg_p_entry(sig, c, w[i], b[i], p[i], s0, s2);
  s0 = block_sum<NT>(s0, lds);
  s2 = block_sum<NT>(s2, lds);
  if (threadIdx.x == 0) {
    partials[blockIdx.x * 8 + 0] = s0;
    partials[blockIdx.x * 8 + 2] = s2;
  }
}

// The dual of the Kullback-Leibler data term (pdhg_p_entry_kl): k_pdhg_dual_p's loads and stores, and bg or the vector bgv.
template <bool VEC, bool BG_VEC>
__global__ __launch_bounds__(NT) void k_pdhg_dual_p_kl(int64_t m, float sig, float c2, float c4, float bg, const float* __restrict__ bgv,
                                                       const float* __restrict__ w, const float* __restrict__ b, float* p,
                                                       double* __restrict__ partials) {
  __shared__ double lds[NT / 64];
  double s0 = 0.0, s2 = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail = 0;
  if (VEC) {
    const int64_t m4 = m >> 2;
    tail = m4 << 2;
    for (int64_t i = tid; i < m4; i += nth) {
      const float4 wv = ld4(w, i), bv = ld4(b, i);
      const float4 gv = BG_VEC ? ld4(bgv, i) : make_float4(bg, bg, bg, bg);
      float4 pv = ld4(p, i);
      pv.x = pdhg_p_entry_kl(sig, c2, c4, wv.x, gv.x, bv.x, pv.x, s0, s2);
      pv.y = pdhg_p_entry_kl(sig, c2, c4, wv.y, gv.y, bv.y, pv.y, s0, s2);
      pv.z = pdhg_p_entry_kl(sig, c2, c4, wv.z, gv.z, bv.z, pv.z, s0, s2);
      pv.w = pdhg_p_entry_kl(sig, c2, c4, wv.w, gv.w, bv.w, pv.w, s0, s2);
      st4(p, i, pv);
    }
  }
  for (int64_t i = tail + tid; i < m; i += nth) p[i] = pdhg_p_entry_kl(sig, c2, c4, w[i], BG_VEC ? bgv[i] : bg, b[i], p[i], s0, s2);
  s0 = block_sum<NT>(s0, lds);
  s2 = block_sum<NT>(s2, lds);
  if (threadIdx.x == 0) {
    partials[blockIdx.x * 8 + 0] = s0;
    partials[blockIdx.x * 8 + 2] = s2;
  }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void k_pdhg_dual_q(int64_t rows, float sig, float lam, const float* __restrict__ u, float* q,
                                                    double* __restrict__ partials) {
  __shared__ double lds[NT / 64];
  double s1 = 0.0, s3 = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail = 0;
  if (VEC) {
    const int64_t r4 = rows >> 2;
    tail = r4 << 2;
    for (int64_t i = tid; i < r4; i += nth) {
      const float4 uv = ld4(u, i);
      float4 qv = ld4(q, i);
      qv.x = pdhg_q_entry(sig, lam, uv.x, qv.x, s1, s3);
      qv.y = pdhg_q_entry(sig, lam, uv.y, qv.y, s1, s3);
      qv.z = pdhg_q_entry(sig, lam, uv.z, qv.z, s1, s3);
      qv.w = pdhg_q_entry(sig, lam, uv.w, qv.w, s1, s3);
      st4(q, i, qv);
    }
  }
  for (int64_t i = tail + tid; i < rows; i += nth) q[i] = pdhg_q_entry(sig, lam, u[i], q[i], s1, s3);
  s1 = block_sum<NT>(s1, lds);
  s3 = block_sum<NT>(s3, lds);
  if (threadIdx.x == 0) {
    partials[blockIdx.x * 8 + 1] = s1;
    partials[blockIdx.x * 8 + 3] = s3;
  }
}

// x_new may be x (read, then written by the same thread): no __restrict__ on the two.  HAS_V = false: no regulariser term, g = z.
template <bool HAS_V, bool HAS_XT, bool VEC>
__global__ __launch_bounds__(NT) void k_pdhg_primal(int64_t n, float tau, float lo, float hi, const float* x, const float* __restrict__ z,
                                                    const float* __restrict__ v, float* x_new, float* __restrict__ xbar,
                                                    const float* __restrict__ x_true, double* __restrict__ partials) {
  __shared__ double lds[NT / 64];
  double s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nth = (int64_t)gridDim.x * NT;
  int64_t tail = 0;
  if (VEC) {
    const int64_t n4 = n >> 2;
    tail = n4 << 2;
    for (int64_t i = tid; i < n4; i += nth) {
      const float4 xv = ld4(x, i), zv = ld4(z, i);
      const float4 vv = HAS_V ? ld4(v, i) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 tv = HAS_XT ? ld4(x_true, i) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 xn, xb;
      pdhg_x_entry<HAS_XT>(tau, lo, hi, xv.x, HAS_V ? zv.x + vv.x : zv.x, tv.x, xn.x, xb.x, s4, s5, s6, s7);
      pdhg_x_entry<HAS_XT>(tau, lo, hi, xv.y, HAS_V ? zv.y + vv.y : zv.y, tv.y, xn.y, xb.y, s4, s5, s6, s7);
      pdhg_x_entry<HAS_XT>(tau, lo, hi, xv.z, HAS_V ? zv.z + vv.z : zv.z, tv.z, xn.z, xb.z, s4, s5, s6, s7);
      pdhg_x_entry<HAS_XT>(tau, lo, hi, xv.w, HAS_V ? zv.w + vv.w : zv.w, tv.w, xn.w, xb.w, s4, s5, s6, s7);
      st4(x_new, i, xn);
      st4(xbar, i, xb);
    }
  }
  for (int64_t i = tail + tid; i < n; i += nth) {
    float xn, xb;
    pdhg_x_entry<HAS_XT>(tau, lo, hi, x[i], HAS_V ? z[i] + v[i] : z[i], HAS_XT ? x_true[i] : 0.f, xn, xb, s4, s5, s6, s7);
    x_new[i] = xn;
    xbar[i] = xb;
  }
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

inline bool finite_pos(double v) { return v > 0.0 && v < __builtin_inf(); }

// the C entries of a mode, by Groups (pdhg_internal.h): their names open the error texts
const char* const kBlocksEntry[] = {"trk_pdhg_blocks", "trk_pdhg_blocks_iso", "trk_pdhg_blocks_iso3"};
const char* const kDualQEntry[] = {"trk_pdhg_dual_q", "trk_pdhg_dual_q_iso", "trk_pdhg_dual_q_iso3"};

// the rows of L that the groups g of geometry (N, frames) cover: the rows [H ; V] of `frames` N x N images (kPairs: a tail of groups
// of one may follow) and, with kTriples, the (frames - 1) N^2 temporal rows of the space-time operator
inline int64_t grouped_rows(Groups g, int N, int frames) {
  return (int64_t)frames * 2 * N * (N - 1) + (g == Groups::kTriples ? (int64_t)(frames - 1) * N * N : 0);
}

// what the block counts and the unfused grouped duals ask of a geometry and of the rows of L
int check_geometry(const char* who, Groups g, int N, int frames, int64_t rows) {
  TRK_REQUIRE(N >= 2 && frames >= 1 && frames <= 65535, "%s: need N >= 2, 1 <= frames <= 65535", who);
  const int64_t want = grouped_rows(g, N, frames);
  if (g == Groups::kTriples)
    TRK_REQUIRE(rows == want, "%s: %lld rows are not the %lld of the space-time differences of %d images of %d x %d", who,
                (long long)rows, (long long)want, frames, N, N);
  else
    TRK_REQUIRE(rows >= want, "%s: %lld rows are fewer than the %lld of %d images of %d x %d", who, (long long)rows, (long long)want,
                frames, N, N);
  return TRK_OK;
}

// The largest block count of an iteration's kernels, behind trk_pdhg_blocks, trk_pdhg_blocks_iso and trk_pdhg_blocks_iso3.
int pdhg_blocks(Groups g, int64_t m, int64_t n, int64_t rows, int N, int frames, const trk_op* L_fused, int* blocks) {
  const char* who = kBlocksEntry[(int)g];
  TRK_REQUIRE(blocks && m >= 1 && n >= 1 && rows >= 1, "%s: need m, n, rows >= 1", who);
  int64_t longest = m > n ? m : n;                       // of the vectors the streaming kernels sweep
  if (g == Groups::kRows) longest = rows > longest ? rows : longest;
  else if (int rc = check_geometry(who, g, N, frames, rows)) return rc;
  int t = 0;                                             // the column-thread kernels' blocks
  if (L_fused) {
    int hN = 0, hf = 0;
    if (!pdhg_fusable(L_fused, g, &hN, &hf)) return fail(TRK_EUNSUPPORTED, "%s: %s", who, pdhg_fusable_wanted(g));
    if (g == Groups::kTriples)
      TRK_REQUIRE(hN == N && hf == frames, "%s: the fused forms take the geometry of their handle, (%d, %d)", who, hN, hf);
    t = pdhg_tv_blocks(g, hN, hf);
  } else if (g != Groups::kRows) {                       // grouped rows, then the tail's
    const int64_t off = grouped_rows(g, N, frames);
    t = pdhg_tv_blocks(g, N, frames) + (rows > off ? stream_grid(rows - off) : 0);
  }
  const int sg = stream_grid(longest);
  *blocks = t > sg ? t : sg;
  return TRK_OK;
}

// The unfused grouped duals behind trk_pdhg_dual_q_iso and trk_pdhg_dual_q_iso3: the column-thread kernel on the grouped rows, then
// (kPairs) the streaming kernel on a tail of groups of one.
int grouped_dual_q(Groups g, int N, int frames, int64_t rows, double sigma, double lam, const float* u, float* q, double* partials,
                   int capacity_blocks, int* n_blocks, trk_stream st) {
  const char* who = kDualQEntry[(int)g];
  TRK_REQUIRE(u && q && partials && n_blocks, "%s: NULL argument", who);
  if (int rc = check_geometry(who, g, N, frames, rows)) return rc;
  TRK_REQUIRE(finite_pos(sigma), "%s: sigma must be finite and > 0", who);
  TRK_REQUIRE(lam >= 0.0 && lam < __builtin_inf(), "%s: lam must be finite and >= 0", who);
  TRK_REQUIRE(q != u, "%s: q must not alias u", who);
  const int64_t off = grouped_rows(g, N, frames);
  const int grouped = pdhg_tv_blocks(g, N, frames), tail = rows > off ? stream_grid(rows - off) : 0;
  TRK_REQUIRE(grouped + tail <= capacity_blocks, "%s: partial buffer too small (%d blocks needed)", who, grouped + tail);
  *n_blocks = grouped + tail;
  pdhg_grouped_dual_launch(g, N, frames, (float)sigma, (float)lam, u, q, partials, (hipStream_t)st);
  TRK_LAUNCH_CHECK();
  if (tail) {   // groups of one: the streaming kernel on the slices, its blocks' rows of partials behind the grouped kernel's
    int nt = 0;
    return trk_pdhg_dual_q(rows - off, sigma, lam, u + off, q + off, partials + 8 * (int64_t)grouped, capacity_blocks - grouped, &nt, st);
  }
  return TRK_OK;
}

// The loop of trk_pdhg_iterate, trk_pdhg_iterate_iso and trk_pdhg_iterate_iso3 (the groups of geometry (N, frames)).  Only the
// dual update of q differs, and with `fused` the handle the two fused kernels belong to.  data: kDataL2 (the least-squares dual of p)
// or kDataKL (trk_pdhg_dual_p_kl with the background bg / bg_vec, which kDataL2 ignores).
enum { kDataL2 = 0, kDataKL = 1 };
int pdhg_iterate(const char* who, trk_op* A, trk_op* L, Groups groups, int N, int frames, int data, double bg, const float* bg_vec,
                 int k_first, int n_iters, double sigma,
                 double tau, double lam, double lo, double hi, int fused, const float* b, float* p, float* q, float* w, float* u, float* z,
                 float* v, float* X, int64_t x_ld, int keep_history, const float* x_prev, float* xbar, const float* x_true, double* NP,
                 int np_capacity_blocks, trk_stream stream) {
  TRK_REQUIRE(A && L && b && p && q && w && z && X && x_prev && xbar && NP, "%s: NULL argument", who);
  TRK_REQUIRE(fused || (u && v), "%s: the generic path needs u and v", who);
  TRK_REQUIRE(k_first >= 1 && n_iters >= 0, "%s: need k_first >= 1, n_iters >= 0", who);
  TRK_REQUIRE(L->cols == A->cols, "%s: A and L must have the same number of columns", who);
  const int64_t m = A->rows, n = A->cols, rows = L->rows;
  int need = 0, hN = 0, hf = 0;
  if (groups == Groups::kTriples)
    TRK_REQUIRE(rows == grouped_rows(groups, N, frames) && n == (int64_t)frames * N * N,
                "%s: L is %lld x %lld, not the space-time first differences of %d images of %d x %d", who, (long long)rows, (long long)n,
                frames, N, N);
  else if (groups == Groups::kPairs)
    TRK_REQUIRE(rows >= grouped_rows(groups, N, frames) && n == (int64_t)frames * N * N,
                "%s: L is %lld x %lld, not the first differences of %d images of %d x %d (and a tail)", who, (long long)rows,
                (long long)n, frames, N, N);
  if (int rc = pdhg_blocks(groups, m, n, rows, N, frames, fused ? L : nullptr, &need)) return rc;      // TRK_EUNSUPPORTED: no fused form
  if (groups == Groups::kPairs && fused)
    TRK_REQUIRE(pdhg_fusable(L, groups, &hN, &hf) && hN == N && frames == 1, "%s: the fused form takes the geometry of its handle, (%d, 1)",
                who, hN);
  TRK_REQUIRE(need <= np_capacity_blocks, "%s: partial buffer too small (%d blocks needed)", who, need);
  for (int k = k_first; k < k_first + n_iters; ++k) {
    double* part = NP + 8 * (int64_t)np_capacity_blocks * (k - 1);
    float* x_new = X + (int64_t)(keep_history ? (k - 1) : ((k - 1) & 1)) * x_ld;
    int nb = 0, rc;
    if ((rc = trk_op_apply(A, 0, xbar, 0, w, 0, 1, nullptr, stream))) return rc;                       // w = A xbar
    rc = data == kDataKL ? trk_pdhg_dual_p_kl(m, sigma, bg, bg_vec, w, b, p, part, np_capacity_blocks, &nb, stream)
                         : trk_pdhg_dual_p(m, sigma, w, b, p, part, np_capacity_blocks, &nb, stream);
    if (rc) return rc;
    if (fused) {
      rc = pdhg_fused_dual(groups, L, sigma, lam, xbar, q, part, np_capacity_blocks, &nb, stream);
    } else {
      if ((rc = trk_op_apply(L, 0, xbar, 0, u, 0, 1, nullptr, stream))) return rc;                     // u = L xbar
      rc = groups == Groups::kRows ? trk_pdhg_dual_q(rows, sigma, lam, u, q, part, np_capacity_blocks, &nb, stream)
                                   : grouped_dual_q(groups, N, frames, rows, sigma, lam, u, q, part, np_capacity_blocks, &nb, stream);
    }
    if (rc) return rc;
    if ((rc = trk_op_apply(A, 1, p, 0, z, 0, 1, nullptr, stream))) return rc;                          // z = A^T p'
    if (fused) {
      rc = pdhg_fused_primal(groups, L, tau, lo, hi, x_prev, z, q, x_new, xbar, x_true, part, np_capacity_blocks, &nb, stream);
    } else {
      if ((rc = trk_op_apply(L, 1, q, 0, v, 0, 1, nullptr, stream))) return rc;                        // v = L^T q'
      rc = trk_pdhg_primal(n, tau, lo, hi, x_prev, z, v, x_new, xbar, x_true, part, np_capacity_blocks, &nb, stream);
    }
    if (rc) return rc;
    x_prev = x_new;
  }
  return TRK_OK;
}

}  // namespace

// ======================================================================================= C ABI
extern "C" {

int trk_pdhg_blocks(int64_t m, int64_t n, int64_t rows, const trk_op* L_fused, int* blocks) {
  return pdhg_blocks(Groups::kRows, m, n, rows, 0, 0, L_fused, blocks);
}

int trk_pdhg_dual_p(int64_t m, double sigma, const float* w, const float* b, float* p, double* partials, int capacity_blocks,
                    int* n_blocks, trk_stream st) {
  TRK_REQUIRE(w && b && p && partials && n_blocks, "trk_pdhg_dual_p: NULL argument");
  TRK_REQUIRE(m >= 1, "trk_pdhg_dual_p: need m >= 1");
  TRK_REQUIRE(finite_pos(sigma), "trk_pdhg_dual_p: sigma must be finite and > 0");
  TRK_REQUIRE(p != w && p != b, "trk_pdhg_dual_p: p must not alias w or b");
  const int grid = stream_grid(m);
  TRK_REQUIRE(grid <= capacity_blocks, "trk_pdhg_dual_p: partial buffer too small (%d blocks needed)", grid);
  *n_blocks = grid;
  with_bools([&](auto VEC) {
    hipLaunchKernelGGL((k_pdhg_dual_p<VEC>), dim3(grid), dim3(NT), 0, (hipStream_t)st, m, (float)sigma, (float)(1.0 / (1.0 + sigma)), w, b,
                       p, partials);
  }, aligned16(w) && aligned16(b) && aligned16(p));
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_pdhg_dual_p_kl(int64_t m, double sigma, double bg, const float* bg_vec, const float* w, const float* b, float* p, double* partials,
                       int capacity_blocks, int* n_blocks, trk_stream st) {
  TRK_REQUIRE(w && b && p && partials && n_blocks, "trk_pdhg_dual_p_kl: NULL argument");
  TRK_REQUIRE(m >= 1, "trk_pdhg_dual_p_kl: need m >= 1");
  TRK_REQUIRE(finite_pos(sigma), "trk_pdhg_dual_p_kl: sigma must be finite and > 0");
  TRK_REQUIRE(bg_vec || (bg >= 0.0 && bg < __builtin_inf()), "trk_pdhg_dual_p_kl: the background must be finite and >= 0");
  TRK_REQUIRE(p != w && p != b && p != bg_vec, "trk_pdhg_dual_p_kl: p must not alias w, b or bg_vec");
  const int grid = stream_grid(m);
  TRK_REQUIRE(grid <= capacity_blocks, "trk_pdhg_dual_p_kl: partial buffer too small (%d blocks needed)", grid);
  *n_blocks = grid;
  with_bools([&](auto VEC, auto BG_VEC) {
    hipLaunchKernelGGL((k_pdhg_dual_p_kl<VEC, BG_VEC>), dim3(grid), dim3(NT), 0, (hipStream_t)st, m, (float)sigma, (float)(2.0 * sigma),
                       (float)(4.0 * sigma), (float)bg, bg_vec, w, b, p, partials);
  }, aligned16(w) && aligned16(b) && aligned16(p) && (!bg_vec || aligned16(bg_vec)), bg_vec != nullptr);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_pdhg_dual_q(int64_t rows, double sigma, double lam, const float* u, float* q, double* partials, int capacity_blocks,
                    int* n_blocks, trk_stream st) {
  TRK_REQUIRE(u && q && partials && n_blocks, "trk_pdhg_dual_q: NULL argument");
  TRK_REQUIRE(rows >= 1, "trk_pdhg_dual_q: need rows >= 1");
  TRK_REQUIRE(finite_pos(sigma), "trk_pdhg_dual_q: sigma must be finite and > 0");
  TRK_REQUIRE(lam >= 0.0 && lam < __builtin_inf(), "trk_pdhg_dual_q: lam must be finite and >= 0");
  TRK_REQUIRE(q != u, "trk_pdhg_dual_q: q must not alias u");
  const int grid = stream_grid(rows);
  TRK_REQUIRE(grid <= capacity_blocks, "trk_pdhg_dual_q: partial buffer too small (%d blocks needed)", grid);
  *n_blocks = grid;
  with_bools([&](auto VEC) {
    hipLaunchKernelGGL((k_pdhg_dual_q<VEC>), dim3(grid), dim3(NT), 0, (hipStream_t)st, rows, (float)sigma, (float)lam, u, q, partials);
  }, aligned16(u) && aligned16(q));
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_pdhg_blocks_iso(int64_t m, int64_t n, int64_t rows, int N, int frames, const trk_op* L_fused, int* blocks) {
  return pdhg_blocks(Groups::kPairs, m, n, rows, N, frames, L_fused, blocks);
}

int trk_pdhg_dual_q_iso(int N, int frames, int64_t rows, double sigma, double lam, const float* u, float* q, double* partials,
                        int capacity_blocks, int* n_blocks, trk_stream st) {
  return grouped_dual_q(Groups::kPairs, N, frames, rows, sigma, lam, u, q, partials, capacity_blocks, n_blocks, st);
}

int trk_pdhg_primal(int64_t n, double tau, double lo, double hi, const float* x, const float* z, const float* v, float* x_new,
                    float* xbar, const float* x_true, double* partials, int capacity_blocks, int* n_blocks, trk_stream st) {
  TRK_REQUIRE(x && z && x_new && xbar && partials && n_blocks, "trk_pdhg_primal: NULL argument");
  TRK_REQUIRE(n >= 1, "trk_pdhg_primal: need n >= 1");
  TRK_REQUIRE(finite_pos(tau), "trk_pdhg_primal: tau must be finite and > 0");
  TRK_REQUIRE(lo <= hi, "trk_pdhg_primal: need lo <= hi (either may be infinite)");
  TRK_REQUIRE(xbar != x && xbar != x_new && xbar != z && xbar != v && xbar != x_true,
              "trk_pdhg_primal: xbar must not alias another operand");
  TRK_REQUIRE(x_new != z && x_new != v && x_new != x_true, "trk_pdhg_primal: x_new may alias x only");
  const int grid = stream_grid(n);
  TRK_REQUIRE(grid <= capacity_blocks, "trk_pdhg_primal: partial buffer too small (%d blocks needed)", grid);
  *n_blocks = grid;
  const bool vec = aligned16(x) && aligned16(z) && aligned16(x_new) && aligned16(xbar) && (!v || aligned16(v)) &&
                   (!x_true || aligned16(x_true));
  with_bools([&](auto HAS_V, auto HAS_XT, auto VEC) {
    hipLaunchKernelGGL((k_pdhg_primal<HAS_V, HAS_XT, VEC>), dim3(grid), dim3(NT), 0, (hipStream_t)st, n, (float)tau, (float)lo, (float)hi,
                       x, z, v, x_new, xbar, x_true, partials);
  }, v != nullptr, x_true != nullptr, vec);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_pdhg_iterate(trk_op* A, trk_op* L, int k_first, int n_iters, double sigma, double tau, double lam, double lo, double hi,
                     int fused, const float* b, float* p, float* q, float* w, float* u, float* z, float* v, float* X, int64_t x_ld,
                     int keep_history, const float* x_prev, float* xbar, const float* x_true, double* NP, int np_capacity_blocks,
                     trk_stream stream) {
  return pdhg_iterate("trk_pdhg_iterate", A, L, Groups::kRows, 0, 0, kDataL2, 0.0, nullptr, k_first, n_iters, sigma, tau, lam, lo, hi,
                      fused, b, p, q, w, u, z, v, X, x_ld, keep_history, x_prev, xbar, x_true, NP, np_capacity_blocks, stream);
}

int trk_pdhg_iterate_iso(trk_op* A, trk_op* L, int N, int frames, int k_first, int n_iters, double sigma, double tau, double lam,
                         double lo, double hi, int fused, const float* b, float* p, float* q, float* w, float* u, float* z, float* v,
                         float* X, int64_t x_ld, int keep_history, const float* x_prev, float* xbar, const float* x_true, double* NP,
                         int np_capacity_blocks, trk_stream stream) {
  TRK_REQUIRE(N >= 2 && frames >= 1, "trk_pdhg_iterate_iso: need N >= 2, frames >= 1");
  return pdhg_iterate("trk_pdhg_iterate_iso", A, L, Groups::kPairs, N, frames, kDataL2, 0.0, nullptr, k_first, n_iters, sigma, tau, lam,
                      lo, hi, fused, b, p, q, w, u, z, v, X, x_ld, keep_history, x_prev, xbar, x_true, NP, np_capacity_blocks, stream);
}

int trk_pdhg_blocks_iso3(int64_t m, int64_t n, int64_t rows, int N, int frames, const trk_op* L_fused, int* blocks) {
  return pdhg_blocks(Groups::kTriples, m, n, rows, N, frames, L_fused, blocks);
}

int trk_pdhg_dual_q_iso3(int N, int frames, int64_t rows, double sigma, double lam, const float* u, float* q, double* partials,
                         int capacity_blocks, int* n_blocks, trk_stream st) {
  return grouped_dual_q(Groups::kTriples, N, frames, rows, sigma, lam, u, q, partials, capacity_blocks, n_blocks, st);
}

int trk_pdhg_iterate_iso3(trk_op* A, trk_op* L, int N, int frames, int k_first, int n_iters, double sigma, double tau, double lam,
                          double lo, double hi, int fused, const float* b, float* p, float* q, float* w, float* u, float* z, float* v,
                          float* X, int64_t x_ld, int keep_history, const float* x_prev, float* xbar, const float* x_true, double* NP,
                          int np_capacity_blocks, trk_stream stream) {
  TRK_REQUIRE(N >= 2 && frames >= 1, "trk_pdhg_iterate_iso3: need N >= 2, frames >= 1");
  return pdhg_iterate("trk_pdhg_iterate_iso3", A, L, Groups::kTriples, N, frames, kDataL2, 0.0, nullptr, k_first, n_iters, sigma, tau,
                      lam, lo, hi, fused, b, p, q, w, u, z, v, X, x_ld, keep_history, x_prev, xbar, x_true, NP, np_capacity_blocks, stream);
}

int trk_pdhg_iterate_data(trk_op* A, trk_op* L, int groups, int N, int frames, int data, double bg, const float* bg_vec, int k_first,
                          int n_iters, double sigma, double tau, double lam, double lo, double hi, int fused, const float* b, float* p,
                          float* q, float* w, float* u, float* z, float* v, float* X, int64_t x_ld, int keep_history, const float* x_prev,
                          float* xbar, const float* x_true, double* NP, int np_capacity_blocks, trk_stream stream) {
  TRK_REQUIRE(groups >= 0 && groups <= 2, "trk_pdhg_iterate_data: groups is 0 (rows), 1 (pairs) or 2 (triples)");
  TRK_REQUIRE(data == kDataL2 || data == kDataKL, "trk_pdhg_iterate_data: data is 0 (least squares) or 1 (Kullback-Leibler)");
  TRK_REQUIRE(groups == 0 || (N >= 2 && frames >= 1), "trk_pdhg_iterate_data: need N >= 2, frames >= 1");
  TRK_REQUIRE(data == kDataL2 || bg_vec || (bg >= 0.0 && bg < __builtin_inf()),
              "trk_pdhg_iterate_data: the background must be finite and >= 0");
  return pdhg_iterate("trk_pdhg_iterate_data", A, L, (Groups)groups, groups ? N : 0, groups ? frames : 0, data, bg, bg_vec, k_first, n_iters,
                      sigma, tau, lam, lo, hi, fused, b, p, q, w, u, z, v, X, x_ld, keep_history, x_prev, xbar, x_true, NP,
                      np_capacity_blocks, stream);
}

}  // extern "C"
