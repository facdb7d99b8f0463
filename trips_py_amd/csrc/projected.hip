// projected.hip — DEVICE code of the projected (k-sized) problems of the Krylov solvers: one-workgroup float64 kernels and their
// launchers, so that an iteration with a numeric regularisation parameter never visits the host.
//   k_bidiag_tikhonov                        Golub-Kahan hybrids: min || [B_k; sqrt(lam) I] y - beta0 e1 || by Givens rotations, resumable
//   k_cgs_coeffs, k_finalize_cgs             repeated Gram-Schmidt from the Gram matrix (finalize_cgs: fused with the sweep's finalize)
//   k_gram_tikhonov, k_gram_tikhonov_border  GKS / MMGKS: (G_A + lam G_L) y = c, by Cholesky in LDS or by a bordered inverse
//   k_gram_row_from_sweep, k_gks_rows_solve  GKS: the new Gram rows from the sweep's products; rows and bordered solve in one launch
//   k_hess_tikhonov                          Hybrid-GMRES: new column of H, its Gram row, (H^T H + lam I) y = beta0 H[0, :]^T
// Their host side: host_regparam.hip (lambda searches), host_worker.hip (the thread that runs them), hybrid_host.hip (iteration drivers).
#include "trk_internal.h"

#include <map>
#include <mutex>

using namespace trk;

namespace {

constexpr int BIDIAG_MAX_K = 2048;   // the back substitution stages 3 k doubles in LDS

// k_bidiag_tikhonov replaces   y = np.linalg.lstsq(vstack((B_k, sqrt(lam) I)), vstack((beta0 e1, 0)))   trips/solvers/Hybrid_LSQR.py:104
// (and GK_Tikhonov.py:60) for the lower-bidiagonal B_k of Golub-Kahan: the stacked matrix is reduced to an upper bidiagonal R by 2k
// Givens rotations (the damped-LSQR elimination of Paige & Saunders 1982, section 2 of "LSQR: an algorithm for sparse linear equations
// and sparse least squares"), then R y = phi is back-substituted.  O(k), backward stable, float64 throughout.
// One workgroup of 64 lanes.  Square roots of the new columns' squared norms are taken in parallel; lane 0 then runs the
// rotation recurrence — per column two square roots and two reciprocals (r^2 = abar^2 + mu^2 + beta^2 needs no second
// hypot) — and the back substitution R y = phi (multiplications by the stored 1/rho) out of LDS, where the dependent chain
// waits ~60 cycles per step instead of an L2 round trip.  With a `work` array the recurrence state survives between
// calls: when mu is unchanged and one column was appended (the fixed-lambda hybrid iteration) only that column is rotated,
// O(1) instead of O(k) expensive operations; any other change restarts from column 0.
// work: [0] columns done, [1] mu, [2] abar, [3] phibar, then invrho[cap], theta[cap], phi[cap].
// y_over_alpha: y_j / alpha_j is written (coefficients with respect to the un-normalised vectors alpha_j v_j).
__global__ __launch_bounds__(64) void k_bidiag_tikhonov(const double* __restrict__ alpha_sq, int64_t a_stride,
                                                        const double* __restrict__ beta_sq, int64_t b_stride, int k,
                                                        double mu, const double* __restrict__ beta0_sq,
                                                        double* __restrict__ y, double* __restrict__ work, int cap,
                                                        double* __restrict__ scratch, int y_over_alpha) {
  extern __shared__ double sm[];
  __shared__ double sh_start;
  double *s_ir = sm, *s_th = sm + k, *s_ph = sm + 2 * k;
  double* st = work ? work : scratch;                          // scratch: same layout, always restarted
  double* invrho = st + 4;
  double* theta = invrho + cap;
  double* phi = theta + cap;
  if (threadIdx.x == 0) {
    const bool resume = work && st[1] == mu && st[0] >= 1.0 && (int)st[0] < k;
    sh_start = resume ? st[0] : 0.0;
  }
  __syncthreads();
  const int j0 = (int)sh_start;
  // al[j] of the columns to process, through y (as scratch) — y is written last
  double* al = y;                                               // al[j] for j in [j0, k)
  for (int j = j0 + (int)threadIdx.x; j < k; j += 64) al[j] = sqrt(alpha_sq[(int64_t)j * a_stride]);
  // columns rotated by earlier launches: their factors go to LDS for the back substitution
  for (int j = threadIdx.x; j < j0; j += 64) {
    s_ir[j] = invrho[j];
    s_th[j] = theta[j];
    s_ph[j] = phi[j];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double mu2 = mu * mu;
    double abar, phibar;
    if (j0 == 0) {
      abar = al[0];
      phibar = sqrt(*beta0_sq);
    } else {
      abar = st[2];
      phibar = st[3];
      // st[2] holds -c2 of the previous last column (its alpha_{j0} factor was not known then)
      abar *= al[j0];
      const double t = theta[j0] * al[j0];
      theta[j0] = t;
      s_th[j0] = t;
    }
    for (int j = j0; j < k; ++j) {
      const double bj2 = beta_sq[(int64_t)j * b_stride];         // B[j+1, j]^2
      const double rhat2 = abar * abar + mu2, r2 = rhat2 + bj2;
      const double rhat = sqrt(rhat2), r = sqrt(r2), bj = sqrt(bj2);
      const double ir = 1.0 / r;
      const double phihat = (abar / rhat) * phibar;
      const double c2 = rhat * ir, s2 = bj * ir;
      invrho[j] = ir;
      s_ir[j] = ir;
      const double ph = c2 * phihat;
      phi[j] = ph;
      s_ph[j] = ph;
      if (j + 1 < k) {
        const double th = s2 * al[j + 1];
        theta[j + 1] = th;
        s_th[j + 1] = th;
        abar = -c2 * al[j + 1];
      } else {
        theta[j + 1] = s2;                                        // completed with alpha_{j+1} on resume (cap >= k + 1)
        abar = -c2;
      }
      phibar = s2 * phihat;
    }
    st[0] = (double)k;
    st[1] = mu;
    st[2] = abar;
    st[3] = phibar;
    // back substitution, the solution left in s_ph
    double yn = s_ph[k - 1] * s_ir[k - 1];
    s_ph[k - 1] = yn;
    for (int j = k - 2; j >= 0; --j) {
      yn = (s_ph[j] - s_th[j + 1] * yn) * s_ir[j];
      s_ph[j] = yn;
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < k; j += 64)
    y[j] = y_over_alpha ? s_ph[j] / sqrt(alpha_sq[(int64_t)j * a_stride]) : s_ph[j];
}

}  // namespace

extern "C" int trk_bidiag_tikhonov(const double* alpha_sq, int64_t alpha_stride, const double* beta_sq,
                                   int64_t beta_stride, int k, double mu, const double* beta0_sq, double* y,
                                   int y_over_alpha, double* work, int work_doubles, trk_stream stream) {
  TRK_REQUIRE(alpha_sq && beta_sq && beta0_sq && y, "trk_bidiag_tikhonov: NULL argument");
  TRK_REQUIRE(k >= 1 && k <= BIDIAG_MAX_K, "trk_bidiag_tikhonov: k must be in [1, 2048]");
  TRK_REQUIRE(mu >= 0.0, "trk_bidiag_tikhonov: mu must be >= 0");
  hipStream_t s = (hipStream_t)stream;
  int cap = k + 1;
  double* scratch = nullptr;
  if (work) {
    cap = (work_doubles - 4) / 3;
    TRK_REQUIRE(cap >= k + 1, "trk_bidiag_tikhonov: work holds %d doubles, %d needed", work_doubles, 3 * (k + 1) + 4);
  } else {
    if (int rc = scratch_doubles(s, (size_t)3 * cap + 4, &scratch)) return rc;
  }
  hipLaunchKernelGGL(k_bidiag_tikhonov, dim3(1), dim3(64), 3 * sizeof(double) * (size_t)k, s, alpha_sq, alpha_stride, beta_sq,
                     beta_stride, k, mu, beta0_sq, y, work, cap, scratch, y_over_alpha);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

// Every kernel BELOW this line is compiled without floating-point contraction (no a * b + c -> fma): k_cgs_coeffs, k_finalize_cgs,
// k_gram_tikhonov, k_gram_tikhonov_border, k_gram_row_from_sweep, k_gks_rows_solve, k_hess_tikhonov; k_bidiag_tikhonov, above, with it.
// This is how they have always been built (the pragma came with host code that once stood here), and the float64 parity tests of the
// GKS, MMGKS and Hybrid-GMRES projected solves were recorded against that build: moving a kernel across this line changes its bits.
#pragma clang fp contract(off)

// (M v)_i, i < k, for a SYMMETRIC k x k matrix in global memory (row stride ld) and v in LDS, by one workgroup: four lanes per
// row, each walking a quarter of COLUMN i (consecutive rows -> consecutive addresses), the four partial sums met by two lane
// exchanges.  These k x k kernels are latency-bound — one thread per row meant k dependent-in-order loads per thread (k = 53:
// 20-30 us per product); a quarter of them per lane, four times the lanes busy.  sink(i, value) is called once per row.
template <class F>
__device__ __forceinline__ void symv4(const double* M, int ld, int k, const double* v, F&& sink) {
  const int part = threadIdx.x & 3;
  for (int base = 0; base < k; base += (int)blockDim.x / 4) {
    const int i = base + ((int)threadIdx.x >> 2);
    double a0 = 0.0, a1 = 0.0;
    if (i < k) {
      int j = part;
      for (; j + 4 < k; j += 8) {
        a0 += M[(size_t)j * ld + i] * v[j];
        a1 += M[(size_t)(j + 4) * ld + i] * v[j + 4];
      }
      if (j < k) a0 += M[(size_t)j * ld + i] * v[j];
    }
    double a = a0 + a1;
    a += __shfl_xor(a, 1, 64);
    a += __shfl_xor(a, 2, 64);
    if (i < k && part == 0) sink(i, a);
  }
}

// ------------------------------------------------------------------------------------------------ repeated Gram-Schmidt by Gram matrix
// `passes` sweeps of block classical Gram-Schmidt, r <- r - V (V^T r), amount to r - V c with
//     c_0 = 0,   c_{p+1} = c_p + (h - G c_p),   h = V^T r,  G = V^T V
// (sweep p+1 projects the result of sweep p: V^T (r - V c_p) = h - G c_p) — any V, orthonormal or not.  With G kept on the
// device (one new row per appended vector) the sweeps cost ONE pass over the basis for h and one for r - V c, instead of two
// per sweep (GKS.py:86-88: three sweeps; MMGKS.py:119-120, decompositions.py:216-218: two).  k x k work, one workgroup.
// rr != nullptr (*rr = r . r): also *rho2_out = || r - V c ||^2 = r.r - 2 c.h + c.(G c), so that the caller knows the norm of the
// orthogonalised vector BEFORE the pass that forms it (trk_gemv_orth_iterate; GKS / MMGKS: r is orthogonal to V but for rounding,
// c.h and c.G c are ~1e-14 of r.r).  Lifted to a tiny positive number should rounding ever drive it to <= 0.
__global__ __launch_bounds__(256) void k_cgs_coeffs(double* __restrict__ G, int ldg, const double* __restrict__ h,
                                                    const double* __restrict__ g_new, int k, int passes, double* __restrict__ c,
                                                    const double* __restrict__ rr = nullptr, double* __restrict__ rho2_out = nullptr) {
  extern __shared__ double sh[];           // c (k) | t (k)
  __shared__ double red[2][4];
  double* cs = sh;
  double* ts = sh + k;
  if (g_new) {                             // install the Gram row / column of the newest vector (index k - 1)
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
      G[(size_t)(k - 1) * ldg + j] = g_new[j];
      G[(size_t)j * ldg + (k - 1)] = g_new[j];
    }
    __threadfence_block();
  }
  for (int j = threadIdx.x; j < k; j += blockDim.x) cs[j] = 0.0;
  __syncthreads();
  __syncthreads();                         // (the installed row is read below by other threads)
  for (int p = 0; p < passes; ++p) {
    if (p == 0) {                          // c_0 = 0: the first sweep's coefficients are h itself
      for (int j = threadIdx.x; j < k; j += blockDim.x) ts[j] = h[j];
    } else {
      symv4(G, ldg, k, cs, [&](int i, double a) { ts[i] = h[i] - a; });
    }
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += blockDim.x) cs[j] += ts[j];
    __syncthreads();
  }
  if (c)
    for (int j = threadIdx.x; j < k; j += blockDim.x) c[j] = cs[j];
  if (rr) {
    double p_ch = 0.0, p_cgc = 0.0;
    symv4(G, ldg, k, cs, [&](int i, double gc) {
      p_ch += cs[i] * h[i];
      p_cgc += cs[i] * gc;
    });
    p_ch = wave_sum(p_ch);
    p_cgc = wave_sum(p_cgc);
    if ((threadIdx.x & 63) == 0) {
      red[0][threadIdx.x >> 6] = p_ch;
      red[1][threadIdx.x >> 6] = p_cgc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const double ch = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
      const double cgc = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
      const double v = *rr - 2.0 * ch + cgc;
      *rho2_out = v > 0.0 ? v : 1e-300;
    }
  }
}

// k_finalize over the 2k sums of a trk_gemv_t2 sweep (h = V^T r | the Gram row of the newest vector) and k_cgs_coeffs in ONE launch:
// workgroup o adds up output o exactly as k_finalize does (finalize_block_256: the same bits) and stores it write-through; the
// workgroup that draws the last ticket then runs the k x k recurrence on the finished sums, which it loads past its L1 / the other
// XCDs' stale L2 lines (sc1) — the hand-off of k_radon_adj_tile's split tiles.  An Arnoldi / GKS step is a chain of dependent
// launches of ~4.5 us each whatever they compute: this takes one out (Hybrid-GMRES on the 512^2 blur: 9 launches per iteration).
__global__ __launch_bounds__(256) void k_finalize_cgs(const double* __restrict__ partials, int nblocks, double* W, unsigned* cnt,
                                                      double* __restrict__ G, int ldg, int k, int passes, double* __restrict__ c) {
  extern __shared__ double sh[];           // c (k) | t (k) | h (k) | g_new (k)
  __shared__ double lds[4];
  __shared__ unsigned ticket;
  const int nout = 2 * k;
  const int o = blockIdx.x;
  const double v = finalize_block_256(partials + o, nblocks, nout, lds);
  if (threadIdx.x == 0) {
    asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" ::"v"(W + o), "v"(v) : "memory");
    ticket = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (ticket != (unsigned)(nout - 1)) return;
  if (threadIdx.x == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // for the next launch
  double* cs = sh;
  double* ts = sh + k;
  double* hs = sh + 2 * k;
  double* gs = sh + 3 * k;
  for (int j = threadIdx.x; j < nout; j += blockDim.x) {
    double t;
    asm volatile("global_load_dwordx2 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(t) : "v"(W + j) : "memory");
    hs[j] = t;                             // (hs and gs are adjacent: W = h | g_new)
  }
  __syncthreads();
  // from here on: k_cgs_coeffs with h and g_new in LDS
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    G[(size_t)(k - 1) * ldg + j] = gs[j];
    G[(size_t)j * ldg + (k - 1)] = gs[j];
  }
  __threadfence_block();
  for (int j = threadIdx.x; j < k; j += blockDim.x) cs[j] = 0.0;
  __syncthreads();
  __syncthreads();
  for (int p = 0; p < passes; ++p) {
    if (p == 0) {
      for (int j = threadIdx.x; j < k; j += blockDim.x) ts[j] = hs[j];
    } else {
      symv4(G, ldg, k, cs, [&](int i, double a) { ts[i] = hs[i] - a; });
    }
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += blockDim.x) cs[j] += ts[j];
    __syncthreads();
  }
  for (int j = threadIdx.x; j < k; j += blockDim.x) c[j] = cs[j];
}

int trk::finalize_cgs(const double* part, int nblk, int k, double* W, double* G, int ldg, int passes, double* c, hipStream_t s) {
  TRK_REQUIRE(part && W && G && c && k >= 1 && k <= 1024 && ldg >= k && passes >= 1 && nblk >= 1, "finalize_cgs: bad argument");
  unsigned* cnt = nullptr;
  if (int rc = stream_ticket(s, &cnt)) return rc;
  hipLaunchKernelGGL(k_finalize_cgs, dim3(2 * k), dim3(256), 4 * (size_t)k * sizeof(double), s, part, nblk, W, cnt, G, ldg, k, passes, c);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

extern "C" int trk_cgs_coeffs(double* G, int ldg, const double* h, const double* g_new, int k, int passes, double* c,
                              trk_stream st) {
  TRK_REQUIRE(G && k >= 1 && ldg >= k && passes >= 0 && (passes == 0 || (h && c)), "trk_cgs_coeffs: bad argument");
  TRK_REQUIRE(k <= 2048, "trk_cgs_coeffs: k <= 2048");
  hipLaunchKernelGGL(k_cgs_coeffs, dim3(1), dim3(256), 2 * (size_t)k * sizeof(double), (hipStream_t)st, G, ldg, h, g_new, k, passes, c, (const double*)nullptr, (double*)nullptr);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

extern "C" int trk_cgs_coeffs_rho(double* G, int ldg, const double* h, const double* g_new, int k, int passes, double* c,
                                  const double* rr, double* rho2_out, trk_stream st) {
  TRK_REQUIRE(G && h && c && rr && rho2_out && k >= 1 && ldg >= k && passes >= 1, "trk_cgs_coeffs_rho: bad argument");
  TRK_REQUIRE(k <= 2048, "trk_cgs_coeffs_rho: k <= 2048");
  hipLaunchKernelGGL(k_cgs_coeffs, dim3(1), dim3(256), 2 * (size_t)k * sizeof(double), (hipStream_t)st, G, ldg, h, g_new, k, passes, c, rr, rho2_out);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

// ------------------------------------------------------------------------------------------------ projected Tikhonov solve from Gram data
// y = argmin ||AV y - b||^2 + lam ||LV y||^2 = (G_A + lam G_L)^-1 c  with G_A = (AV)^T AV, G_L = (LV)^T LV, c = (AV)^T b —
// what `lstsq([R_A; sqrt(lam) R_L], [Q_A^T b; 0])` of GKS.py:74 / MMGKS.py:106 solves (R^T R = G, R_A^T Q_A^T b = c) — on
// the device, from the Gram data the device already holds: with a NUMERIC regparam no scalar visits the host inside the
// loop (GKS / MMGKS each paid a download, two k x k Cholesky factorisations, a stacked least-squares solve and an upload per
// iteration: ~0.15 ms of host time with the GPU idle).  One workgroup; Cholesky in LDS, float64.
// M (k x k, row stride ld, lower triangle read) z = rhs in LDS: Cholesky M = C C^T in place, then C z' = z, C^T y = z'.
// A pivot that rounding drove to <= 0 is lifted to a tiny positive number.  All threads of the workgroup call it.
__device__ __forceinline__ void chol_solve_lds(double* M, int ld, double* z, int k) {
  for (int j = 0; j < k; ++j) {
    if (threadIdx.x == 0) {
      const double d = M[j * ld + j];
      M[j * ld + j] = sqrt(d > 0.0 ? d : 1e-300);
    }
    __syncthreads();
    const double djj = M[j * ld + j];
    for (int i = j + 1 + threadIdx.x; i < k; i += blockDim.x) M[i * ld + j] /= djj;
    __syncthreads();
    const int rem = k - j - 1;
    for (int idx = threadIdx.x; idx < rem * rem; idx += blockDim.x) {
      const int a = j + 1 + idx / rem, b = j + 1 + idx % rem;
      if (b <= a) M[a * ld + b] -= M[a * ld + j] * M[b * ld + j];
    }
    __syncthreads();
  }
  for (int j = 0; j < k; ++j) {
    if (threadIdx.x == 0) z[j] /= M[j * ld + j];
    __syncthreads();
    const double zj = z[j];
    for (int i = j + 1 + threadIdx.x; i < k; i += blockDim.x) z[i] -= M[i * ld + j] * zj;
    __syncthreads();
  }
  for (int j = k - 1; j >= 0; --j) {
    if (threadIdx.x == 0) z[j] /= M[j * ld + j];
    __syncthreads();
    const double zj = z[j];
    for (int i = threadIdx.x; i < j; i += blockDim.x) z[i] -= M[j * ld + i] * zj;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_gram_tikhonov(const double* __restrict__ GA, int lda, const double* __restrict__ GL, int ldl,
                                                       const double* __restrict__ c, int k, double lam, double* __restrict__ y) {
  extern __shared__ double sm[];              // M (k x (k+1)) | z (k)
  const int ld = k + 1;
  double* M = sm;
  double* z = sm + (size_t)k * ld;
  for (int idx = threadIdx.x; idx < k * k; idx += blockDim.x) {
    const int i = idx / k, j = idx - i * k;
    M[i * ld + j] = GA[(size_t)i * lda + j] + lam * GL[(size_t)i * ldl + j];
  }
  for (int i = threadIdx.x; i < k; i += blockDim.x) z[i] = c[i];
  __syncthreads();
  chol_solve_lds(M, ld, z, k);
  for (int i = threadIdx.x; i < k; i += blockDim.x) y[i] = z[i];
}

// The same solve when M = G_A + lam G_L only GROWS between calls (GKS with a numeric regparam: one basis vector, hence one row
// and column of both Gram matrices, per iteration; same lam): Minv holds M^-1 of the leading k_from x k_from block from the
// previous call and is bordered by rows k_from .. k-1 — u = Minv g, s = M[j][j] - g.u, Minv <- [[Minv + u u^T / s, -u / s],
// [-u^T / s, 1 / s]] — then y = Minv c: O(k^2) per new row instead of the O(k^3) Cholesky from scratch (k = 53: 79 -> ~12 us).
// k_from = 0 builds the inverse from nothing (the first call, k = projection_dim).
__device__ __forceinline__ void tikhonov_border_body(const double* GA, int lda, const double* GL, int ldl, const double* c, int k,
                                                     int k_from, double lam, double* Minv, int ldm, double* __restrict__ y, double* sm,
                                                     double* red) {
  double* g = sm;                             // sm: g (k) | u (k) | c (k)
  double* u = sm + k;
  double* cl = sm + 2 * k;
  for (int i = threadIdx.x; i < k; i += blockDim.x) cl[i] = c[i];
  for (int j = k_from; j < k; ++j) {
    for (int i = threadIdx.x; i <= j; i += blockDim.x) g[i] = GA[(size_t)j * lda + i] + lam * GL[(size_t)j * ldl + i];
    __syncthreads();
    double part = 0.0;
    symv4(Minv, ldm, j, g, [&](int i, double a) {             // u = Minv g
      u[i] = a;
      part += a * g[i];
    });
    part = wave_sum(part);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    const double sinv = 1.0 / (g[j] - (red[0] + red[1] + red[2] + red[3]));
    for (int idx = threadIdx.x; idx < j * j; idx += blockDim.x) {
      const int a = idx / j, b = idx - a * j;
      Minv[(size_t)a * ldm + b] += u[a] * u[b] * sinv;
    }
    for (int i = threadIdx.x; i < j; i += blockDim.x) {
      Minv[(size_t)i * ldm + j] = -u[i] * sinv;
      Minv[(size_t)j * ldm + i] = -u[i] * sinv;
    }
    if (threadIdx.x == 0) Minv[(size_t)j * ldm + j] = sinv;
    __syncthreads();                            // (one workgroup: its global writes are visible to it after the barrier)
  }
  __syncthreads();
  symv4(Minv, ldm, k, cl, [&](int i, double a) { y[i] = a; });
}
__global__ __launch_bounds__(256) void k_gram_tikhonov_border(const double* __restrict__ GA, int lda, const double* __restrict__ GL,
                                                              int ldl, const double* __restrict__ c, int k, int k_from, double lam,
                                                              double* Minv, int ldm, double* __restrict__ y) {
  extern __shared__ double sm[];              // g (k) | u (k) | c (k)
  __shared__ double red[4];
  tikhonov_border_body(GA, lda, GL, ldl, c, k, k_from, lam, Minv, ldm, y, sm, red);
}

// GKS: row / column k of a Gram matrix G = V^T M V (M = A^T A or L^T L) for the basis vector v_k = (r - V c) / rho that the sweep
// has just produced, from what the sweep's own pass over V left behind — a = V^T (M r), the coefficients c, s = r . M r and
// rho^2 = ||r - V c||^2 — with no further pass over the basis:
//   G[i][k] = (a_i - (G c)_i) / rho  (i < k),     G[k][k] = (s - 2 c.a + c.(G c)) / rho^2 ;
// optionally the same for a projected right-hand side  rhs_k = (t - c . rhs[0..k)) / rho  (t = r . (A^T b)).
// r is the residual of the projected normal equations, so V^T r = 0 but for rounding and c is of rounding size: nothing cancels.
__device__ __forceinline__ void gram_row_body(double* G, int ldg, int k, const double* __restrict__ a, const double* __restrict__ c,
                                              const double* __restrict__ s_rr, const double* __restrict__ rho2, double* rhs,
                                              const double* tb, double* cl, double (*red)[4]) {
  const double rho = sqrt(*rho2);
  for (int i = threadIdx.x; i < k; i += blockDim.x) cl[i] = c[i];
  __syncthreads();
  double p_ca = 0.0, p_cgc = 0.0, p_cr = 0.0;
  symv4(G, ldg, k, cl, [&](int i, double gc) {
    const double v = (a[i] - gc) / rho;
    G[(size_t)i * ldg + k] = v;              // (row / column k: outside what symv4 reads)
    G[(size_t)k * ldg + i] = v;
    p_ca += cl[i] * a[i];
    p_cgc += cl[i] * gc;
    if (rhs) p_cr += cl[i] * rhs[i];
  });
  p_ca = wave_sum(p_ca);
  p_cgc = wave_sum(p_cgc);
  p_cr = wave_sum(p_cr);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = p_ca;
    red[1][threadIdx.x >> 6] = p_cgc;
    red[2][threadIdx.x >> 6] = p_cr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double ca = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    const double cgc = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    G[(size_t)k * ldg + k] = (*s_rr - 2.0 * ca + cgc) / (rho * rho);
    if (rhs) rhs[k] = (*tb - ((red[2][0] + red[2][1]) + (red[2][2] + red[2][3]))) / rho;
  }
}
__global__ __launch_bounds__(256) void k_gram_row_from_sweep(double* G, int ldg, int k, const double* __restrict__ a,
                                                             const double* __restrict__ c, const double* __restrict__ s_rr,
                                                             const double* __restrict__ rho2, double* rhs, const double* tb) {
  extern __shared__ double cl[];              // c (k)
  __shared__ double red[3][4];
  gram_row_body(G, ldg, k, a, c, s_rr, rho2, rhs, tb, cl, red);
}

// GKS's one-pass form (trk_gemv_orth_iterate): everything between the h-sweep's products and the pass that needs y' is k x k work of
// one workgroup — rows k of G_A and G_L, then the bordered inverse over k + 1 vectors and y' — and was three launches of ~6 us each
// whatever they compute (an install or a row for G_A, a row for G_L, the solve).  One launch: the bodies above, one after the other.
//   A side: ga_new != NULL — the k + 1 entries of row k as a pass over the kept images left them (the Radon operator) — or a_A != NULL —
//           from the sweep's products, with the projected right-hand side's entry k (stencil operators);   L side: from the sweep.
__global__ __launch_bounds__(256) void k_gks_rows_solve(double* GA, double* GL, int ldg, int k, const double* __restrict__ ga_new,
                                                        const double* __restrict__ a_A, const double* __restrict__ s_A,
                                                        const double* __restrict__ tb, const double* __restrict__ a_L,
                                                        const double* __restrict__ s_L, const double* __restrict__ c_sweep,
                                                        const double* __restrict__ rho2, double* c_rhs, double lam, double* Minv, int ldm,
                                                        int k_from, double* __restrict__ y) {
  extern __shared__ double sm[];              // 3 (k + 1) doubles
  __shared__ double red[3][4];
  if (ga_new) {
    for (int j = threadIdx.x; j <= k; j += blockDim.x) {
      GA[(size_t)k * ldg + j] = ga_new[j];
      GA[(size_t)j * ldg + k] = ga_new[j];
    }
  } else {
    gram_row_body(GA, ldg, k, a_A, c_sweep, s_A, rho2, c_rhs, tb, sm, red);
  }
  __syncthreads();
  gram_row_body(GL, ldg, k, a_L, c_sweep, s_L, rho2, nullptr, nullptr, sm, red);
  __threadfence_block();
  __syncthreads();                            // (one workgroup: its own global writes are visible to it after the barrier)
  tikhonov_border_body(GA, ldg, GL, ldg, c_rhs, k + 1, k_from, lam, Minv, ldm, y, sm, &red[0][0]);
}

extern "C" int trk_gks_rows_solve(double* GA, double* GL, int ldg, int k, const double* ga_new, const double* a_A, const double* s_A,
                                  const double* tb, const double* a_L, const double* s_L, const double* c_sweep, const double* rho2,
                                  double* c_rhs, double lam, double* Minv, int ldm, int k_from, double* y, trk_stream st) {
  TRK_REQUIRE(GA && GL && a_L && s_L && c_sweep && rho2 && c_rhs && Minv && y && k >= 1 && ldg >= k + 1 && ldm >= k + 1,
              "trk_gks_rows_solve: bad argument");
  TRK_REQUIRE((ga_new != nullptr) != (a_A != nullptr), "trk_gks_rows_solve: the A-side row either as ga_new or from the sweep (a_A, s_A, tb)");
  TRK_REQUIRE(ga_new || (s_A && tb), "trk_gks_rows_solve: a_A needs s_A = r . A^T A r and tb = r . A^T b");
  TRK_REQUIRE(k_from >= 0 && k_from <= k + 1 && k + 1 <= 2048, "trk_gks_rows_solve: 0 <= k_from <= k + 1 <= 2048");
  hipLaunchKernelGGL(k_gks_rows_solve, dim3(1), dim3(256), 3 * (size_t)(k + 1) * sizeof(double), (hipStream_t)st, GA, GL, ldg, k, ga_new, a_A,
                     s_A, tb, a_L, s_L, c_sweep, rho2, c_rhs, lam, Minv, ldm, k_from, y);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

extern "C" int trk_gram_row_from_sweep(double* G, int ldg, int k, const double* a, const double* c, const double* s_rr,
                                       const double* rho2, double* rhs, const double* tb, trk_stream st) {
  TRK_REQUIRE(G && a && c && s_rr && rho2 && k >= 1 && ldg >= k + 1, "trk_gram_row_from_sweep: bad argument");
  TRK_REQUIRE(!rhs || tb, "trk_gram_row_from_sweep: rhs given without t = r . (A^T b)");
  TRK_REQUIRE(k <= 2048, "trk_gram_row_from_sweep: k <= 2048 (k doubles of LDS)");
  hipLaunchKernelGGL(k_gram_row_from_sweep, dim3(1), dim3(256), (size_t)k * sizeof(double), (hipStream_t)st, G, ldg, k, a, c, s_rr, rho2, rhs, tb);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

// Hybrid-GMRES's projected problem on the device (Hybrid_GMRES.py:69-77 with a numeric regparam):
//   y = argmin || H_k y - beta0 e1 ||^2 + lam || y ||^2 ,   H_k the (k+1) x k Hessenberg matrix of Arnoldi.
// One workgroup appends column k-1 of H from the scalars the orthogonalisation sweep left on the device (its k combined
// Gram-Schmidt coefficients and ||w||^2), extends G = H^T H by its new row/column, and solves (G + lam I) y = beta0 H[0,:]^T.
// H: column-major, column stride ldh >= k+1; G, Minv: row stride ldg.
//   mode 0  Cholesky of G + lam I in LDS, from scratch: O(k^3), any k, any history of lam (what the first version always did:
//           ~50 us per call averaged over k = 1..100 — serial time the host path hides behind the next Arnoldi step);
//   mode 1  M = G + lam I grew by one row and column since the previous call with the same lam, and Minv holds its previous
//           inverse: bordering update  u = Minv g, s = gamma - g.u,  Minv <- [[Minv + u u^T / s, -u / s], [-u^T / s, 1 / s]],
//           then y = Minv c — O(k^2), four barriers, no sequential dependency (cond(M) <= ||G|| / lam: harmless in float64);
//   mode 2  k <= 2: Minv formed directly (the start of the chain; the reference solves its first problem with lam = 0).
__global__ __launch_bounds__(256) void k_hess_tikhonov(double* __restrict__ H, int ldh, double* __restrict__ G, double* Minv,
                                                       int ldg, const double* __restrict__ coef, const double* __restrict__ coef2,
                                                       const double* __restrict__ nrm2_sq, double beta0, int k, double lam,
                                                       int mode, double* __restrict__ y) {
  extern __shared__ double sm[];              // new column (k+1) | g (k) | u (k) | c (k) | [mode 0: M (k x (k+1)) | z (k)]
  double* hc = sm;
  double* g = hc + (k + 1);
  double* u = g + k;
  double* cv = u + k;
  __shared__ double red[4];
  for (int r = threadIdx.x; r <= k; r += blockDim.x) {
    const double v = r < k ? coef[r] + (coef2 ? coef2[r] : 0.0) : sqrt(*nrm2_sq);
    hc[r] = v;
    H[(size_t)(k - 1) * ldh + r] = v;
  }
  __syncthreads();
  // g[i] = G[i][k-1] = sum_r H[r][i] H[r][k-1]; column i of H is non-zero in rows 0 .. i+1
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    double a = 0.0;
    if (i == k - 1) {
      for (int r = 0; r <= k; ++r) a += hc[r] * hc[r];
    } else {
      const double* col = H + (size_t)i * ldh;
      for (int r = 0; r <= i + 1; ++r) a += col[r] * hc[r];
    }
    g[i] = a;
    G[(size_t)i * ldg + (k - 1)] = a;
    G[(size_t)(k - 1) * ldg + i] = a;
    cv[i] = beta0 * (i == k - 1 ? hc[0] : H[(size_t)i * ldh]);
  }
  __syncthreads();                            // (one workgroup: its own global writes are visible to it after the barrier)
  if (mode == 0) {
    const int ld = k + 1;
    double* M = cv + k;
    double* z = M + (size_t)k * ld;
    for (int idx = threadIdx.x; idx < k * k; idx += blockDim.x) {
      const int i = idx / k, j = idx - i * k;
      M[i * ld + j] = G[(size_t)i * ldg + j] + (i == j ? lam : 0.0);
    }
    for (int i = threadIdx.x; i < k; i += blockDim.x) z[i] = cv[i];
    __syncthreads();
    chol_solve_lds(M, ld, z, k);
    for (int i = threadIdx.x; i < k; i += blockDim.x) y[i] = z[i];
    return;
  }
  const double gamma = g[k - 1] + lam;
  if (mode == 2) {                            // k = 1 or 2: the inverse written out
    if (threadIdx.x == 0) {
      if (k == 1) {
        Minv[0] = 1.0 / gamma;
      } else {
        const double a = G[0] + lam, b = g[0], det = a * gamma - b * b;
        Minv[0] = gamma / det;
        Minv[1] = Minv[ldg] = -b / det;
        Minv[ldg + 1] = a / det;
      }
    }
    __syncthreads();
  } else {
    const int m = k - 1;
    // u = Minv g (Minv symmetric: thread i walks column i, consecutive threads read consecutive addresses)
    double part = 0.0;
    symv4(Minv, ldg, m, g, [&](int i, double a) {
      u[i] = a;
      part += a * g[i];
    });
    part = wave_sum(part);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    const double sinv = 1.0 / (gamma - (red[0] + red[1] + red[2] + red[3]));     // Schur complement of the new diagonal entry
    for (int idx = threadIdx.x; idx < m * m; idx += blockDim.x) {
      const int i = idx / m, j = idx - i * m;
      Minv[(size_t)i * ldg + j] += u[i] * u[j] * sinv;
    }
    for (int i = threadIdx.x; i < m; i += blockDim.x) {
      Minv[(size_t)i * ldg + m] = -u[i] * sinv;
      Minv[(size_t)m * ldg + i] = -u[i] * sinv;
    }
    if (threadIdx.x == 0) Minv[(size_t)m * ldg + m] = sinv;
    __syncthreads();
  }
  symv4(Minv, ldg, k, cv, [&](int i, double a) { y[i] = a; });                    // y = Minv c
}

// both kernels keep the k x (k+1) factor in LDS: up to 160 KB per workgroup on gfx950 (opt-in above 64 KB)
static int tikhonov_lds(const void* kernel, size_t bytes) {
  constexpr size_t kMaxDyn = 159 * 1024;        // 160 KB per workgroup minus the kernels' few static bytes
  if (bytes > kMaxDyn) return fail(TRK_EINVAL, "projected Tikhonov solve: k too large for 160 KB of LDS");
  if (bytes > 64 * 1024) {
    static std::mutex mu;
    static std::map<const void*, size_t> granted;
    std::lock_guard<std::mutex> lk(mu);
    if (granted[kernel] < bytes) {
      if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxDyn) != hipSuccess)
        return fail(TRK_EHIP, "projected Tikhonov solve: cannot raise the dynamic LDS limit");
      granted[kernel] = kMaxDyn;
    }
  }
  return TRK_OK;
}

extern "C" int trk_gram_tikhonov(const double* GA, int lda, const double* GL, int ldl, const double* c, int k, double lam,
                                 double* Minv, int ldm, int k_from, double* y, trk_stream st) {
  TRK_REQUIRE(GA && GL && c && y && k >= 1 && lda >= k && ldl >= k, "trk_gram_tikhonov: bad argument");
  if (Minv) {
    TRK_REQUIRE(ldm >= k && k_from >= 0 && k_from <= k, "trk_gram_tikhonov: bordering form needs ldm >= k and 0 <= k_from <= k");
    TRK_REQUIRE(k <= 2048, "trk_gram_tikhonov: bordering form needs k <= 2048 (3 k doubles of LDS)");
    hipLaunchKernelGGL(k_gram_tikhonov_border, dim3(1), dim3(256), 3 * (size_t)k * sizeof(double), (hipStream_t)st, GA, lda, GL, ldl,
                       c, k, k_from, lam, Minv, ldm, y);
    TRK_LAUNCH_CHECK();
    return TRK_OK;
  }
  TRK_REQUIRE(k <= 139, "trk_gram_tikhonov: k <= 139 (the factor lives in LDS)");
  const size_t bytes = ((size_t)k * (k + 1) + k) * sizeof(double);
  if (int rc = tikhonov_lds(reinterpret_cast<const void*>(k_gram_tikhonov), bytes)) return rc;
  hipLaunchKernelGGL(k_gram_tikhonov, dim3(1), dim3(256), bytes, (hipStream_t)st, GA, lda, GL, ldl, c, k, lam, y);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}

extern "C" int trk_hess_tikhonov(double* H, int ldh, double* G, double* Minv, int ldg, const double* coef, const double* coef2,
                                 const double* nrm2_sq, double beta0, int k, double lam, int mode, double* y, trk_stream st) {
  TRK_REQUIRE(H && G && coef && nrm2_sq && y && k >= 1 && ldh >= k + 1 && ldg >= k, "trk_hess_tikhonov: bad argument");
  TRK_REQUIRE(mode >= 0 && mode <= 2 && (mode == 0 || Minv), "trk_hess_tikhonov: mode 0 (Cholesky), 1 (bordering update), 2 (k <= 2) ; modes 1, 2 need Minv");
  TRK_REQUIRE(mode != 2 || k <= 2, "trk_hess_tikhonov: mode 2 starts the chain at k <= 2");
  TRK_REQUIRE(mode != 1 || (k >= 2 && lam > 0.0), "trk_hess_tikhonov: the bordering update needs k >= 2 and lam > 0");
  TRK_REQUIRE(mode != 0 || k <= 139, "trk_hess_tikhonov: Cholesky mode needs k <= 139 (the factor lives in LDS)");
  TRK_REQUIRE(lam >= 0.0, "trk_hess_tikhonov: lam must be >= 0");
  size_t bytes = ((size_t)(k + 1) + 3 * (size_t)k) * sizeof(double);
  if (mode == 0) bytes += ((size_t)k * (k + 1) + k) * sizeof(double);
  if (int rc = tikhonov_lds(reinterpret_cast<const void*>(k_hess_tikhonov), bytes)) return rc;
  hipLaunchKernelGGL(k_hess_tikhonov, dim3(1), dim3(256), bytes, (hipStream_t)st, H, ldh, G, Minv, ldg, coef, coef2, nrm2_sq,
                     beta0, k, lam, mode, y);
  TRK_LAUNCH_CHECK();
  return TRK_OK;
}
