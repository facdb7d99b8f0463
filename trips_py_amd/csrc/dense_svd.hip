// dense_svd.hip — float64 dense SVD by one-sided (Hestenes) block Jacobi, and the two float64 dense products the direct
// solvers need around it (U^T b and V diag(f) c).  Design, measurements and what was tried: docs/kernels/dense_svd.md.
//
//   G = A (m x n, m >= n, column-major), V = I.  Columns in blocks of W = 16, the block count padded to an even nbp (the
//   padding columns are zero and never rotate).  One sweep = nbp - 1 rounds of the round-robin (circle) pairing; in a round
//   every block meets one other and the nbp / 2 pairs are independent.  Before every sweep the columns are ordered by
//   decreasing norm (a permutation `perm` of slots to physical columns; nothing moves), so that a block holds columns of
//   similar size.  A round is three launches:
//     k_svd_gram    the 32 x 32 Gram matrix of every pair, split over row chunks of 128 (partials, no atomics)
//     k_svd_jacobi  one workgroup per pair: the partials summed in chunk order; if some column pair (i, j) of the 32 is not
//                   orthogonal — |g_i^T g_j| > tol ||g_i|| ||g_j|| and > tol max(||g_i||, ||g_j||)^2 — at most two sweeps of
//                   cyclic Jacobi in LDS (16 disjoint rotations per step) on the Gram matrix; the accumulated 32 x 32
//                   rotation, brought back to orthogonality by one Newton-Schulz step, is written out with a flag; otherwise
//                   the flag stays 0.  The second bound is the rounding a rotation leaves in a column (of order eps times the
//                   largest column it is combined with): without it a column far below its partner is never found orthogonal
//                   to it.  What it accepts moves the smaller singular value by at most tol times the larger one.
//     k_svd_apply   [G_I G_J] <- [G_I G_J] R and [V_I V_J] <- [V_I V_J] R for flagged pairs (one row per thread)
//   A sweep in which no pair is flagged ends the iteration.  Then sigma_j = ||G_j|| (k_svd_colnorm); the caller sorts and
//   scales.  Every sum has a fixed order, nothing uses atomics: two runs give the same bits.
//
//   The matrix rotated alongside G need not be the identity: trk_dense_svd_carry_f64 takes a companion C (nc rows, one column
//   per column of G) from the caller and returns C times the accumulated rotation.  The rotations depend on G alone, so the
//   plain SVD is the same driver with C = I.  The GSVD of trips_py_amd/_dense.py is two or three such runs.
#include "trk_internal.h"

#include <cfloat>
#include <algorithm>
#include <cmath>
#include <vector>

using namespace trk;

namespace {

constexpr int W = 16;          // column block width
constexpr int P = 2 * W;       // columns of a pair
constexpr int CH = 128;        // rows per Gram chunk
constexpr int NT = 256;
constexpr int NTJ = 64;        // one wave per pair in the Jacobi step
constexpr int INNER_MAX = 2;   // in-LDS Jacobi sweeps per pair and round (more cost time and save no outer sweeps)

// blocks (bi, bj) of pair k in round r of the circle method on nbp (even) blocks: block nbp-1 stays, the others rotate
__device__ __forceinline__ void pair_blocks(int r, int k, int nbp, int& bi, int& bj) {
  const int M = nbp - 1;
  if (k == 0) {
    bi = r;
    bj = M;
  } else {
    bi = (r + k) % M;
    bj = (r - k + M) % M;
  }
}

__device__ __forceinline__ int64_t pair_col(const int* __restrict__ perm, int c, int bi, int bj) {
  return (int64_t)perm[c < W ? bi * W + c : bj * W + c - W];
}

__global__ __launch_bounds__(NT) void k_svd_gram(const double* __restrict__ G, int64_t ldg, int64_t m, const int* __restrict__ perm,
                                                 int nbp, int r, int nchunks, double* __restrict__ part) {
  __shared__ double tile[CH][P + 1];
  const int pair = blockIdx.x, chunk = blockIdx.y, t = threadIdx.x;
  int bi, bj;
  pair_blocks(r, pair, nbp, bi, bj);
  const int64_t row0 = (int64_t)chunk * CH;
  for (int e = t; e < CH * P; e += NT) {
    const int c = e / CH, rr = e - c * CH;
    const int64_t row = row0 + rr;
    tile[rr][c] = row < m ? G[pair_col(perm, c, bi, bj) * ldg + row] : 0.0;
  }
  __syncthreads();
  const int i0 = (t >> 4) * 2, j0 = (t & 15) * 2;
  double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
  for (int rr = 0; rr < CH; ++rr) {
    const double x0 = tile[rr][i0], x1 = tile[rr][i0 + 1], y0 = tile[rr][j0], y1 = tile[rr][j0 + 1];
    a00 = fma(x0, y0, a00);
    a01 = fma(x0, y1, a01);
    a10 = fma(x1, y0, a10);
    a11 = fma(x1, y1, a11);
  }
  double* out = part + ((int64_t)pair * nchunks + chunk) * (P * P);
  out[i0 * P + j0] = a00;
  out[i0 * P + j0 + 1] = a01;
  out[(i0 + 1) * P + j0] = a10;
  out[(i0 + 1) * P + j0 + 1] = a11;
}

// the 16 disjoint index pairs of step `s` (0..30) of a round-robin sweep over the 32 columns of a pair
__device__ __forceinline__ void inner_pair(int s, int k, int& p, int& q) {
  const int M = P - 1;
  if (k == 0) {
    p = s;
    q = M;
  } else {
    p = (s + k) % M;
    q = (s - k + M) % M;
  }
}

__global__ __launch_bounds__(NTJ) void k_svd_jacobi(const double* __restrict__ part, int nchunks, double tol, double* __restrict__ rot,
                                                    int* __restrict__ flag) {
  __shared__ double a[P][P + 1];
  __shared__ double v[P][P + 1];
  __shared__ double cs[W][2];
  __shared__ int pq[W][2];
  const int pair = blockIdx.x, t = threadIdx.x;
  const double* src = part + (int64_t)pair * nchunks * (P * P);
  for (int e = t; e < P * P; e += NTJ) {
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += src[(int64_t)c * (P * P) + e];
    a[e / P][e % P] = s;
    v[e / P][e % P] = (e / P == e % P) ? 1.0 : 0.0;
  }
  __syncthreads();
  // is some column pair of the 32 not orthogonal to tol?  (zero columns count as orthogonal to everything)
  int off = 0;
  for (int e = t; e < P * P; e += NTJ) {
    const int i = e / P, j = e % P;
    if (i < j && fabs(a[i][j]) > tol * (sqrt(a[i][i]) * sqrt(a[j][j])) && fabs(a[i][j]) > tol * fmax(a[i][i], a[j][j])) off = 1;
  }
  off = __syncthreads_or(off);
  if (!off) {
    if (t == 0) flag[pair] = 0;
    return;
  }
  const double eps_in = fmax(tol * 0.0625, 2.0 * DBL_EPSILON);
  for (int sw = 0; sw < INNER_MAX; ++sw) {
    int changed = 0;
    for (int s = 0; s < P - 1; ++s) {
      if (t < W) {
        int p, q;
        inner_pair(s, t, p, q);
        const double app = a[p][p], aqq = a[q][q], apq = a[p][q];
        double c = 1.0, sn = 0.0;
        if (apq != 0.0 && fabs(apq) > eps_in * (sqrt(app) * sqrt(aqq))) {
          // column p <- c g_p - s g_q, column q <- s g_p + c g_q with (g_p' , g_q') = 0: t = tan(theta) the smaller root of
          // t^2 + 2 tau t - 1 = 0, tau = (a_qq - a_pp) / (2 a_pq)
          const double tau = (aqq - app) / (2.0 * apq);
          const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
          c = 1.0 / sqrt(1.0 + tt * tt);
          sn = tt * c;
          changed = 1;
        }
        cs[t][0] = c;
        cs[t][1] = sn;
        pq[t][0] = p;
        pq[t][1] = q;
      }
      __syncthreads();
      for (int e = t; e < W * P; e += NTJ) {          // rows: a <- R^T a
        const int k = e / P, col = e % P;
        const double sn = cs[k][1];
        if (sn != 0.0) {
          const double c = cs[k][0];
          const int p = pq[k][0], q = pq[k][1];
          const double x = a[p][col], y = a[q][col];
          a[p][col] = c * x - sn * y;
          a[q][col] = sn * x + c * y;
        }
      }
      __syncthreads();
      for (int e = t; e < W * P; e += NTJ) {          // columns: a <- a R, v <- v R
        const int k = e / P, row = e % P;
        const double sn = cs[k][1];
        if (sn != 0.0) {
          const double c = cs[k][0];
          const int p = pq[k][0], q = pq[k][1];
          double x = a[row][p], y = a[row][q];
          a[row][p] = c * x - sn * y;
          a[row][q] = sn * x + c * y;
          x = v[row][p];
          y = v[row][q];
          v[row][p] = c * x - sn * y;
          v[row][q] = sn * x + c * y;
        }
      }
      __syncthreads();
      if (t < W && cs[t][1] != 0.0) {
        a[pq[t][0]][pq[t][1]] = 0.0;
        a[pq[t][1]][pq[t][0]] = 0.0;
      }
      __syncthreads();
    }
    if (!__syncthreads_or(changed)) break;
  }
  // R = v (3 I - v^T v) / 2: the rounding of the accumulated rotations would otherwise add up, round after round, in V and G
  for (int e = t; e < P * P; e += NTJ) {
    const int i = e / P, j = e % P;
    double acc = 0.0;
    for (int k = 0; k < P; ++k) acc = fma(v[k][i], v[k][j], acc);
    a[i][j] = (i == j ? 1.5 : 0.0) - 0.5 * acc;
  }
  __syncthreads();
  double* R = rot + (int64_t)pair * (P * P);
  for (int e = t; e < P * P; e += NTJ) {
    const int i = e / P, j = e % P;
    double acc = 0.0;
    for (int k = 0; k < P; ++k) acc = fma(v[i][k], a[k][j], acc);
    R[e] = acc;
  }
  if (t == 0) flag[pair] = 1;
}

// rows of G (blockIdx.y < gchunks) and of V (the rest): x[0..32) <- x R for the pair's 32 columns
__global__ __launch_bounds__(NT) void k_svd_apply(double* __restrict__ G, int64_t ldg, int64_t m, int gchunks, double* __restrict__ V,
                                                  int64_t ldv, int64_t nv, const int* __restrict__ perm, int nbp, int r,
                                                  const double* __restrict__ rot, const int* __restrict__ flag) {
  const int pair = blockIdx.x;
  if (flag[pair] == 0) return;
  __shared__ double R[P * P];
  for (int e = threadIdx.x; e < P * P; e += NT) R[e] = rot[(int64_t)pair * (P * P) + e];
  __syncthreads();
  int bi, bj;
  pair_blocks(r, pair, nbp, bi, bj);
  double* X;
  int64_t ld, rows, row;
  if ((int)blockIdx.y < gchunks) {
    X = G, ld = ldg, rows = m, row = (int64_t)blockIdx.y * NT + threadIdx.x;
  } else {
    X = V, ld = ldv, rows = nv, row = (int64_t)(blockIdx.y - gchunks) * NT + threadIdx.x;
  }
  if (row >= rows) return;
  double x[P];
#pragma unroll
  for (int c = 0; c < P; ++c) x[c] = X[pair_col(perm, c, bi, bj) * ld + row];
#pragma unroll 4
  for (int j = 0; j < P; ++j) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k) acc = fma(x[k], R[k * P + j], acc);
    X[pair_col(perm, j, bi, bj) * ld + row] = acc;
  }
}

// any[0] <- 1 if some flag of the sweep is set
__global__ __launch_bounds__(NT) void k_svd_any(const int* __restrict__ flags, int64_t count, int* __restrict__ any) {
  int f = 0;
  for (int64_t i = threadIdx.x; i < count; i += NT) f |= flags[i];
  f = __syncthreads_or(f);
  if (threadIdx.x == 0) any[0] = f;
}

// s[j] <- ||G_j||, fixed-order sum (strided per thread, then a tree in LDS)
__global__ __launch_bounds__(NT) void k_svd_colnorm(const double* __restrict__ G, int64_t ldg, int64_t m, double* __restrict__ s) {
  __shared__ double red[NT];
  const double* g = G + (int64_t)blockIdx.x * ldg;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += NT) acc = fma(g[i], g[i], acc);
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) s[blockIdx.x] = sqrt(red[0]);
}

__global__ __launch_bounds__(NT) void k_svd_init(const double* __restrict__ A, int64_t lda, int64_t m, int64_t n, double* __restrict__ G,
                                                 int64_t ldg, int64_t npad, double* __restrict__ V, int64_t ldv) {
  const int64_t j = blockIdx.y;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < ldg; i += (int64_t)gridDim.x * NT)
    G[j * ldg + i] = (j < n && i < m) ? A[j * lda + i] : 0.0;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < ldv; i += (int64_t)gridDim.x * NT)
    V[j * ldv + i] = (i == j) ? 1.0 : 0.0;
  (void)npad;
}

// G as in k_svd_init; the companion's first n columns stay as the caller gave them, its padding columns are zeroed
__global__ __launch_bounds__(NT) void k_svd_init_carry(const double* __restrict__ A, int64_t lda, int64_t m, int64_t n,
                                                       double* __restrict__ G, int64_t ldg, double* __restrict__ C, int64_t ldc) {
  const int64_t j = blockIdx.y;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < ldg; i += (int64_t)gridDim.x * NT)
    G[j * ldg + i] = (j < n && i < m) ? A[j * lda + i] : 0.0;
  if (j >= n)
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < ldc; i += (int64_t)gridDim.x * NT) C[j * ldc + i] = 0.0;
}

// y[j] = beta y[j] + alpha sum_i A[i, j] d[i] x[i]   (one block per column, fixed-order sum)
__global__ __launch_bounds__(NT) void k_gemv_t64(int64_t m, const double* __restrict__ A, int64_t lda, const double* __restrict__ x,
                                                 const double* __restrict__ d, double alpha, double beta, double* __restrict__ y) {
  __shared__ double red[NT];
  const double* a = A + (int64_t)blockIdx.x * lda;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += NT) acc = fma(a[i], d ? d[i] * x[i] : x[i], acc);
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) y[blockIdx.x] = (beta == 0.0 ? 0.0 : beta * y[blockIdx.x]) + alpha * red[0];
}

// y[i] = beta y[i] + alpha sum_j A[i, j] d[j] x[j]   (one row per thread, columns in order)
__global__ __launch_bounds__(NT) void k_gemv_n64(int64_t m, int64_t n, const double* __restrict__ A, int64_t lda,
                                                 const double* __restrict__ x, const double* __restrict__ d, double alpha, double beta,
                                                 double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= m) return;
  double acc = 0.0;
  for (int64_t j = 0; j < n; ++j) acc = fma(A[j * lda + i], d ? d[j] * x[j] : x[j], acc);
  y[i] = (beta == 0.0 ? 0.0 : beta * y[i]) + alpha * acc;
}

struct SvdDims {
  int64_t nbp, npad, npairs, rounds, nchunks;
};

SvdDims svd_dims(int64_t m, int64_t n) {
  SvdDims d;
  d.nbp = (n + W - 1) / W;
  if (d.nbp < 2) d.nbp = 2;
  d.nbp += d.nbp & 1;
  d.npad = d.nbp * W;
  d.npairs = d.nbp / 2;
  d.rounds = d.nbp - 1;
  d.nchunks = (m + CH - 1) / CH;
  return d;
}

}  // namespace

extern "C" {

int trk_dense_svd_f64_dims(int64_t m, int64_t n, int64_t* npad, int64_t* work_doubles) {
  TRK_REQUIRE(m >= 1 && n >= 1 && m >= n, "trk_dense_svd_f64_dims: need m >= n >= 1 (got %lld x %lld)", (long long)m, (long long)n);
  TRK_REQUIRE(n <= TRK_DENSE_SVD_MAX_COLS, "trk_dense_svd_f64_dims: at most %d columns (got %lld)", TRK_DENSE_SVD_MAX_COLS, (long long)n);
  TRK_REQUIRE(npad && work_doubles, "trk_dense_svd_f64_dims: NULL output");
  const SvdDims d = svd_dims(m, n);
  *npad = d.npad;
  // Gram partials, rotations, then as ints the flags of one sweep, the sweep's verdict and the column order
  const int64_t ints = d.rounds * d.npairs + 1 + d.npad;
  *work_doubles = d.npairs * d.nchunks * P * P + d.npairs * P * P + (ints + 1) / 2 + 1;
  return TRK_OK;
}

// The Jacobi iteration on G (already initialised, npad columns) with the companion C (ldc >= nc rows, npad columns) rotated
// alongside; S[0..n) <- the column norms of G.
static int svd_iterate(double* G, int64_t ldg, int64_t m, int64_t n, double* C, int64_t ldc, int64_t nc, double* S, double* work,
                       const SvdDims& d, double tol, int max_sweeps, int* sweeps, int* converged, hipStream_t s) {
  double* part = work;
  double* rot = part + d.npairs * d.nchunks * P * P;
  int* flags = (int*)(rot + d.npairs * P * P);
  int* any = flags + d.rounds * d.npairs;
  int* perm = any + 1;
  const int64_t npad = d.npad;
  std::vector<double> norms((size_t)n);
  std::vector<int> order((size_t)npad);
  const int gchunks = (int)((m + NT - 1) / NT), cchunks = (int)((nc + NT - 1) / NT);
  *sweeps = 0;
  *converged = 0;
  for (int sw = 0; sw < max_sweeps; ++sw) {
    // the sweep's column order: decreasing norm, ties by index; the zero padding columns last
    hipLaunchKernelGGL(k_svd_colnorm, dim3((unsigned)n), dim3(NT), 0, s, G, ldg, m, S);
    TRK_LAUNCH_CHECK();
    TRK_HIP(hipMemcpyAsync(norms.data(), S, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    TRK_HIP(hipStreamSynchronize(s));
    for (int64_t j = 0; j < npad; ++j) order[(size_t)j] = (int)j;
    std::stable_sort(order.begin(), order.begin() + n, [&](int x, int y) { return norms[(size_t)x] > norms[(size_t)y]; });
    TRK_HIP(hipMemcpyAsync(perm, order.data(), sizeof(int) * (size_t)npad, hipMemcpyHostToDevice, s));
    for (int r = 0; r < (int)d.rounds; ++r) {
      int* fr = flags + (int64_t)r * d.npairs;
      hipLaunchKernelGGL(k_svd_gram, dim3((unsigned)d.npairs, (unsigned)d.nchunks), dim3(NT), 0, s, G, ldg, m, perm, (int)d.nbp, r,
                         (int)d.nchunks, part);
      TRK_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_svd_jacobi, dim3((unsigned)d.npairs), dim3(NTJ), 0, s, part, (int)d.nchunks, tol, rot, fr);
      TRK_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_svd_apply, dim3((unsigned)d.npairs, (unsigned)(gchunks + cchunks)), dim3(NT), 0, s, G, ldg, m, gchunks, C,
                         ldc, nc, perm, (int)d.nbp, r, rot, fr);
      TRK_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_svd_any, dim3(1), dim3(NT), 0, s, flags, d.rounds * d.npairs, any);
    TRK_LAUNCH_CHECK();
    int host_any = 1;
    TRK_HIP(hipMemcpyAsync(&host_any, any, sizeof(int), hipMemcpyDeviceToHost, s));
    TRK_HIP(hipStreamSynchronize(s));
    *sweeps = sw + 1;
    if (!host_any) {
      *converged = 1;
      break;
    }
  }
  hipLaunchKernelGGL(k_svd_colnorm, dim3((unsigned)n), dim3(NT), 0, s, G, ldg, m, S);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_dense_svd_f64(const double* A, int64_t m, int64_t n, int64_t lda, double* G, int64_t ldg, double* V, int64_t ldv, double* S,
                      double* work, int64_t work_doubles, double tol, int max_sweeps, int* sweeps, int* converged, trk_stream stream) {
  TRK_REQUIRE(A && G && V && S && work && sweeps && converged, "trk_dense_svd_f64: NULL argument");
  int64_t npad = 0, need = 0;
  if (int rc = trk_dense_svd_f64_dims(m, n, &npad, &need)) return rc;
  TRK_REQUIRE(lda >= m && ldg >= m && ldv >= npad, "trk_dense_svd_f64: leading dimensions too small (lda %lld, ldg %lld >= m %lld; "
              "ldv %lld >= %lld)", (long long)lda, (long long)ldg, (long long)m, (long long)ldv, (long long)npad);
  TRK_REQUIRE(work_doubles >= need, "trk_dense_svd_f64: workspace of %lld doubles, need %lld", (long long)work_doubles, (long long)need);
  TRK_REQUIRE(max_sweeps >= 1 && tol > 0.0, "trk_dense_svd_f64: need max_sweeps >= 1 and tol > 0");
  hipStream_t s = (hipStream_t)stream;
  {
    const int64_t span = ldg > ldv ? ldg : ldv;
    const unsigned gx = (unsigned)((span + NT - 1) / NT < 64 ? (span + NT - 1) / NT : 64);
    hipLaunchKernelGGL(k_svd_init, dim3(gx, (unsigned)npad), dim3(NT), 0, s, A, lda, m, n, G, ldg, npad, V, ldv);
    TRK_LAUNCH_CHECK();
  }
  return svd_iterate(G, ldg, m, n, V, ldv, npad, S, work, svd_dims(m, n), tol, max_sweeps, sweeps, converged, s);
}

int trk_dense_svd_carry_f64_dims(int64_t m, int64_t n, int64_t nc, int64_t* npad, int64_t* work_doubles) {
  TRK_REQUIRE(nc >= 1, "trk_dense_svd_carry_f64_dims: the companion needs at least one row (got %lld)", (long long)nc);
  return trk_dense_svd_f64_dims(m, n, npad, work_doubles);
}

int trk_dense_svd_carry_f64(const double* A, int64_t m, int64_t n, int64_t lda, double* G, int64_t ldg, double* C, int64_t nc,
                            int64_t ldc, double* S, double* work, int64_t work_doubles, double tol, int max_sweeps, int* sweeps,
                            int* converged, trk_stream stream) {
  TRK_REQUIRE(A && G && C && S && work && sweeps && converged, "trk_dense_svd_carry_f64: NULL argument");
  int64_t npad = 0, need = 0;
  if (int rc = trk_dense_svd_carry_f64_dims(m, n, nc, &npad, &need)) return rc;
  TRK_REQUIRE(lda >= m && ldg >= m && ldc >= nc, "trk_dense_svd_carry_f64: leading dimensions too small (lda %lld, ldg %lld >= m "
              "%lld; ldc %lld >= nc %lld)", (long long)lda, (long long)ldg, (long long)m, (long long)ldc, (long long)nc);
  TRK_REQUIRE(work_doubles >= need, "trk_dense_svd_carry_f64: workspace of %lld doubles, need %lld", (long long)work_doubles,
              (long long)need);
  TRK_REQUIRE(max_sweeps >= 1 && tol > 0.0, "trk_dense_svd_carry_f64: need max_sweeps >= 1 and tol > 0");
  hipStream_t s = (hipStream_t)stream;
  {
    const int64_t span = ldg > ldc ? ldg : ldc;
    const unsigned gx = (unsigned)((span + NT - 1) / NT < 64 ? (span + NT - 1) / NT : 64);
    hipLaunchKernelGGL(k_svd_init_carry, dim3(gx, (unsigned)npad), dim3(NT), 0, s, A, lda, m, n, G, ldg, C, ldc);
    TRK_LAUNCH_CHECK();
  }
  return svd_iterate(G, ldg, m, n, C, ldc, nc, S, work, svd_dims(m, n), tol, max_sweeps, sweeps, converged, s);
}

int trk_dense_colnorm_f64(const double* X, int64_t ldx, int64_t rows, int64_t cols, double* out, trk_stream stream) {
  TRK_REQUIRE(X && out, "trk_dense_colnorm_f64: NULL argument");
  TRK_REQUIRE(rows >= 1 && cols >= 1 && ldx >= rows, "trk_dense_colnorm_f64: bad shape %lld x %lld (ldx %lld)", (long long)rows,
              (long long)cols, (long long)ldx);
  hipLaunchKernelGGL(k_svd_colnorm, dim3((unsigned)cols), dim3(NT), 0, (hipStream_t)stream, X, ldx, rows, out);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

int trk_dense_gemv_f64(int trans, int64_t m, int64_t n, const double* A, int64_t lda, const double* x, const double* d, double alpha,
                       double beta, double* y, trk_stream stream) {
  TRK_REQUIRE(A && x && y, "trk_dense_gemv_f64: NULL argument");
  TRK_REQUIRE(m >= 1 && n >= 1 && lda >= m, "trk_dense_gemv_f64: bad shape %lld x %lld (lda %lld)", (long long)m, (long long)n,
              (long long)lda);
  TRK_REQUIRE(y != x && y != d, "trk_dense_gemv_f64: y must not alias x or d");
  hipStream_t s = (hipStream_t)stream;
  if (trans) {
    hipLaunchKernelGGL(k_gemv_t64, dim3((unsigned)n), dim3(NT), 0, s, m, A, lda, x, d, alpha, beta, y);
  } else {
    hipLaunchKernelGGL(k_gemv_n64, dim3((unsigned)((m + NT - 1) / NT)), dim3(NT), 0, s, m, n, A, lda, x, d, alpha, beta, y);
  }
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

}  // extern "C"
