// host_regparam.hip — pure HOST numerics of the projected problems (no HIP call): the Tikhonov solve for a B_k held on the host and the
// searches for the regularisation parameter, GCV by bounded Brent search and the discrepancy principle by Newton's iteration.
// No floating-point contraction in this file, for bit parity with NumPy and SciPy: the searches restate their arithmetic operation
// for operation (pairwise summation order, fminbound's steps) so that lambda agrees with the Python path; an fma would not.
#pragma clang fp contract(off)
#include "projected_internal.h"
#include <cmath>

using namespace trk;

// HOST: the same projected solve for a caller that holds B_k on the host (the hybrid solvers once lambda_k has been chosen there,
// Hybrid_LSQR.py:104): the recurrence of k_bidiag_tikhonov in the same order.  ~10 ns per column on a CPU core against ~400 ns for
// the dependent fp64 square roots and divisions of one GPU lane; the solution reaches the device inside the launch that consumes
// it (trk_gemv_n_hosty).  alpha[k], beta_sub[k] (B[j+1, j]), beta0 = ||b||; y_over_alpha as in trk_bidiag_tikhonov.
extern "C" int trk_host_bidiag_tikhonov(const double* alpha, const double* beta_sub, int k, double beta0, double mu, int y_over_alpha,
                                        double* y) {
  TRK_REQUIRE(alpha && beta_sub && y && k >= 1, "trk_host_bidiag_tikhonov: bad argument");
  TRK_REQUIRE(mu >= 0.0, "trk_host_bidiag_tikhonov: mu must be >= 0");
  std::vector<double> buf(3 * (size_t)k + 1);
  double *ir = buf.data(), *th = ir + k, *ph = th + k + 1;
  const double mu2 = mu * mu;
  double abar = alpha[0], phibar = beta0;
  for (int j = 0; j < k; ++j) {
    const double bj = beta_sub[j];
    const double rhat2 = abar * abar + mu2, r2 = rhat2 + bj * bj;
    const double rhat = std::sqrt(rhat2), r = std::sqrt(r2);
    const double inv = 1.0 / r;
    const double phihat = (abar / rhat) * phibar;
    const double c2 = rhat * inv, s2 = bj * inv;
    ir[j] = inv;
    ph[j] = c2 * phihat;
    if (j + 1 < k) {
      th[j + 1] = s2 * alpha[j + 1];
      abar = -c2 * alpha[j + 1];
    }
    phibar = s2 * phihat;
  }
  double yn = ph[k - 1] * ir[k - 1];
  ph[k - 1] = yn;
  for (int j = k - 2; j >= 0; --j) {
    yn = (ph[j] - th[j + 1] * yn) * ir[j];
    ph[j] = yn;
  }
  for (int j = 0; j < k; ++j) y[j] = y_over_alpha ? ph[j] / alpha[j] : ph[j];
  return TRK_OK;
}

// HOST: generalised cross validation for a diagonalised projected problem, minimised by bounded Brent search.
// Replaces the per-iteration   fminbound(gcv_funct, 1e-9, 1e2, xtol=1e-12, maxfun=1000)   of
// trips/utilities/reg_param/gcv.py:94-95 when the projected pair has been brought to (diag(s), I) — the hybrid solvers'
// SVD of B_k / H_k (Hybrid_LSQR.py:81-84, Hybrid_GMRES.py:55-58) and, after the substitution z = R_L y, the GKS / MMGKS
// pair (R_A, R_L) (GKS.py:60-63, MMGKS.py:97-100).  Objective (gcv.py:25-78 on reduced inputs):
//     G(lam) = sum_i ((1 - f_i) rhs_i)^2 / (m_eff - sum_i f_i)^2 ,   f_i = s_i^2 / (s_i^2 + lam).
// The search restates SciPy's `_minimize_scalar_bounded` (Forsythe-Malcolm-Moler fmin: golden section + successive
// parabolic interpolation) step for step, and the sums use NumPy's pairwise summation order, so that the value agrees
// with the Python path it replaces to the last bit in almost all cases; ~60 objective evaluations of O(k) each cost
// ~20 us here against ~2 ms through scipy.optimize + numpy (measured at k = 50 on the MI355X host).
namespace {

double np_pairwise_sum(const double* a, int n) {
  if (n < 8) {
    double res = 0.;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  if (n <= 128) {
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i;
    for (i = 8; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

struct GcvDiag {
  const double *s, *rhs;
  int k;
  double m_eff;
  double *f, *t;   // work, k each
  double operator()(double lam) const {
    for (int i = 0; i < k; ++i) {
      const double s2 = s[i] * s[i];
      f[i] = s2 / (s2 + lam);
      const double d = (1.0 - f[i]) * rhs[i];
      t[i] = d * d;
    }
    const double num = 0.0 + np_pairwise_sum(t, k);
    const double den = m_eff - (0.0 + np_pairwise_sum(f, k));
    return num / pow(den, 2.0);
  }
};

inline double sign1(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 1.0); }   // np.sign(v) + (v == 0)

// scipy.optimize.fminbound (bounded Brent) restated step for step; `func` is the objective
template <class F>
static void fminbound_brent(const F& func, double x1, double x2, double xatol, int maxfun, double* lam_out, double* fval_out,
                            int* nfev_out) {
  const double sqrt_eps = std::sqrt(2.2e-16);
  const double golden_mean = 0.5 * (3.0 - std::sqrt(5.0));
  double a = x1, b = x2;
  double fulc = a + golden_mean * (b - a);
  double nfc = fulc, xf = fulc;
  double rat = 0.0, e = 0.0;
  double x = xf;
  double fx = func(x);
  int num = 1;
  double fu = INFINITY;
  double ffulc = fx, fnfc = fx;
  double xm = 0.5 * (a + b);
  double tol1 = sqrt_eps * std::fabs(xf) + xatol / 3.0;
  double tol2 = 2.0 * tol1;
  while (std::fabs(xf - xm) > (tol2 - 0.5 * (b - a))) {
    bool golden = true;
    if (std::fabs(e) > tol1) {   // parabolic fit
      golden = false;
      double r = (xf - nfc) * (fx - ffulc);
      double q = (xf - fulc) * (fx - fnfc);
      double p = (xf - fulc) * q - (xf - nfc) * r;
      q = 2.0 * (q - r);
      if (q > 0.0) p = -p;
      q = std::fabs(q);
      r = e;
      e = rat;
      if ((std::fabs(p) < std::fabs(0.5 * q * r)) && (p > q * (a - xf)) && (p < q * (b - xf))) {
        rat = (p + 0.0) / q;
        x = xf + rat;
        if (((x - a) < tol2) || ((b - x) < tol2)) rat = tol1 * sign1(xm - xf);
      } else {
        golden = true;
      }
    }
    if (golden) {
      e = (xf >= xm) ? a - xf : b - xf;
      rat = golden_mean * e;
    }
    x = xf + sign1(rat) * std::fmax(std::fabs(rat), tol1);
    fu = func(x);
    ++num;
    if (fu <= fx) {
      if (x >= xf) a = xf; else b = xf;
      fulc = nfc, ffulc = fnfc;
      nfc = xf, fnfc = fx;
      xf = x, fx = fu;
    } else {
      if (x < xf) a = x; else b = x;
      if ((fu <= fnfc) || (nfc == xf)) {
        fulc = nfc, ffulc = fnfc;
        nfc = x, fnfc = fu;
      } else if ((fu <= ffulc) || (fulc == xf) || (fulc == nfc)) {
        fulc = x, ffulc = fu;
      }
    }
    xm = 0.5 * (a + b);
    tol1 = sqrt_eps * std::fabs(xf) + xatol / 3.0;
    tol2 = 2.0 * tol1;
    if (num >= maxfun) break;
  }
  *lam_out = xf;
  if (fval_out) *fval_out = fx;
  if (nfev_out) *nfev_out = num;
}

// G(lam) of the hybrid solvers' projected problem WITHOUT the SVD of B_k (Hybrid_LSQR.py:81-84): with B = Q [R; 0] (k Givens
// rotations, R upper bidiagonal) and q = the first k entries of Q^T e1,
//   sum_i ((1 - f_i) beta0 u0_i)^2 = beta0^2 lam^2 || (R R^T + lam I)^-1 q ||^2 ,   sum_i f_i = k - lam trace((R R^T + lam I)^-1) ,
// f_i = s_i^2 / (s_i^2 + lam) — the same function of lam that the diagonalised form evaluates (the left null vector of B drops
// out of both), by one LDL^T of a k x k tridiagonal matrix per evaluation: O(k) per lambda and O(k) setup instead of an
// O(k^2) bidiagonal SVD per iteration (dbdsqr with one row of U: 140 us at k ~ 50 on the MI355X host — most of a Hybrid-LSQR
// iteration with regparam = 'gcv').
struct GcvBidiag {
  int k;
  double beta0, m_eff;
  const double *md, *mo, *q;   // R R^T: diagonal (k), off-diagonal (k-1); q (k)
  double *d, *e, *y;           // work, k each
  double operator()(double lam) const {
    // forward / backward pivots of M = R R^T + lam I
    d[0] = md[0] + lam;
    for (int j = 1; j < k; ++j) d[j] = md[j] + lam - mo[j - 1] * mo[j - 1] / d[j - 1];
    e[k - 1] = md[k - 1] + lam;
    for (int j = k - 2; j >= 0; --j) e[j] = md[j] + lam - mo[j] * mo[j] / e[j + 1];
    double tr = 0.0;
    for (int j = 0; j < k; ++j) tr += 1.0 / (d[j] + e[j] - (md[j] + lam));       // (M^-1)_jj
    // M z = q
    y[0] = q[0];
    for (int j = 1; j < k; ++j) y[j] = q[j] - mo[j - 1] / d[j - 1] * y[j - 1];
    double z = y[k - 1] / d[k - 1], zz = z * z;
    for (int j = k - 2; j >= 0; --j) {
      z = (y[j] - mo[j] * z) / d[j];
      zz += z * z;
    }
    const double num = beta0 * beta0 * lam * lam * zz;
    const double den = m_eff - ((double)k - lam * tr);
    return num / (den * den);
  }
};

// B = Q [R; 0] for the lower bidiagonal B (diagonal alpha[k], sub-diagonal beta[k]) by k Givens rotations — rotation j mixes rows j, j+1
// and removes beta[j] — with w (k + 1 entries) <- Q^T w in place.  Leaves the tridiagonal R R^T: md its diagonal (k), mo its off-diagonal.
void bidiag_to_rrt(const double* alpha, const double* beta, int k, double* w, double* md, double* mo) {
  double diag = alpha[0], t_prev = 0.0;
  for (int j = 0; j < k; ++j) {
    const double rr = std::hypot(diag, beta[j]);
    const double c = rr > 0.0 ? diag / rr : 1.0, sn = rr > 0.0 ? beta[j] / rr : 0.0;
    const double wj = c * w[j] + sn * w[j + 1], wn = -sn * w[j] + c * w[j + 1];
    w[j] = wj;
    w[j + 1] = wn;
    const double t = (j + 1 < k) ? sn * alpha[j + 1] : 0.0;          // R[j][j+1]
    md[j] = rr * rr + t * t;
    if (j > 0) mo[j - 1] = t_prev * rr;                                // (R R^T)[j-1][j] = R[j-1][j] R[j][j]
    t_prev = t;
    diag = (j + 1 < k) ? c * alpha[j + 1] : 0.0;
  }
}

// The discrepancy principle's Newton iteration on beta = 1 / alpha (discrepancy_principle.py:80-99): beta_0 = 1e-8, at least 30 steps
// unless the update falls below 1e-12 beta, up to 100 while alpha is still ~0.  eval(beta, &f, &fprime).  *alpha_set = 0 when the loop
// ended before alpha was assigned (the reference then returns None).
template <class F>
void dp_newton_loop(F&& eval, double* alpha_out, int* alpha_set, int* iters_out) {
  double beta = 1e-8, alpha = 0.0;
  int it = 0, have = 0;
  while (it < 30 || (it <= 100 && std::fabs(alpha) < 1e-16)) {
    double f, fp;
    eval(beta, &f, &fp);
    const double beta_new = beta - f / fp;
    if (std::fabs(beta_new - beta) < 1e-12 * beta) break;
    beta = beta_new;
    alpha = 1.0 / beta_new;
    have = 1;
    ++it;
  }
  *alpha_out = alpha;
  *alpha_set = have;
  if (iters_out) *iters_out = it;
}

}  // namespace

// The discrepancy principle's Newton iteration (trk_host_dp_newton) for the bidiagonal projected problem without the SVD of B_k:
// with B = Q [R; 0] and w = Q^T bproj, || bhat / (sv beta + 1) ||^2 = || (beta R R^T + I)^-1 w_{1..k} ||^2 + w_{k+1}^2 — the last entry
// is the component along the left null vector of B, which the Newton step does not move — so every step is one LDL^T of a
// k x k tridiagonal matrix and two solves with it.  The same loop, the same `testzero` branch (discrepancy_principle.py:68-99).
extern "C" int trk_host_dp_bidiag(const double* alpha, const double* beta_sub, int k, const double* bproj, double target,
                                  double extra, double* alpha_out, int* alpha_set, int* iters_out, double* testzero_out) {
  TRK_REQUIRE(alpha && beta_sub && bproj && alpha_out && alpha_set, "trk_host_dp_bidiag: NULL argument");
  TRK_REQUIRE(k >= 1, "trk_host_dp_bidiag: k must be >= 1");
  std::vector<double> wk(7 * (size_t)k + 1);
  double *md = wk.data(), *mo = md + k, *w = mo + k, *d = w + (k + 1), *z = d + k, *y = z + k, *tmp = y + k;
  for (int j = 0; j <= k; ++j) w[j] = bproj[j];
  bidiag_to_rrt(alpha, beta_sub, k, w, md, mo);
  const double null2 = w[k] * w[k];
  const double testzero = null2 - target + extra;                // (:71-76) the discrepancy cannot be reached yet
  if (testzero_out) *testzero_out = testzero;
  *alpha_out = 0.0; *alpha_set = 1;
  if (iters_out) *iters_out = 0;
  if (!(testzero < 0.0)) return TRK_OK;
  auto solve = [&](double bt, const double* rhs, double* out) {  // (bt M + I) out = rhs with the pivots in d (Thomas)
    tmp[0] = rhs[0];
    for (int j = 1; j < k; ++j) tmp[j] = rhs[j] - bt * mo[j - 1] / d[j - 1] * tmp[j - 1];
    out[k - 1] = tmp[k - 1] / d[k - 1];
    for (int j = k - 2; j >= 0; --j) out[j] = (tmp[j] - bt * mo[j] * out[j + 1]) / d[j];
  };
  dp_newton_loop([&](double bt, double* f, double* fp) {
    d[0] = bt * md[0] + 1.0;
    for (int j = 1; j < k; ++j) d[j] = bt * md[j] + 1.0 - (bt * mo[j - 1]) * (bt * mo[j - 1]) / d[j - 1];
    solve(bt, w, z);
    solve(bt, z, y);
    double zz = null2, zwz = 0.0;
    for (int j = 0; j < k; ++j) {
      zz += z[j] * z[j];
      zwz += z[j] * (y[j] - z[j]);
    }
    *f = zz + extra - target;
    *fp = 2.0 / bt * zwz;
  }, alpha_out, alpha_set, iters_out);
  return TRK_OK;
}

extern "C" int trk_host_gcv_fminbound(const double* s, const double* rhs, int k, double m_eff, double x1, double x2,
                                      double xatol, int maxfun, double* lam_out, double* fval_out, int* nfev_out) {
  TRK_REQUIRE(s && rhs && lam_out, "trk_host_gcv_fminbound: NULL argument");
  TRK_REQUIRE(k >= 1 && x1 <= x2 && maxfun >= 1, "trk_host_gcv_fminbound: bad argument");
  std::vector<double> work(2 * (size_t)k);
  const GcvDiag func{s, rhs, k, m_eff, work.data(), work.data() + k};
  fminbound_brent(func, x1, x2, xatol, maxfun, lam_out, fval_out, nfev_out);
  return TRK_OK;
}

extern "C" int trk_host_gcv_bidiag(const double* alpha, const double* beta, int k, double beta0, double m_eff, double x1,
                                   double x2, double xatol, int maxfun, double* lam_out, double* fval_out, int* nfev_out) {
  TRK_REQUIRE(alpha && beta && lam_out, "trk_host_gcv_bidiag: NULL argument");
  TRK_REQUIRE(k >= 1 && x1 <= x2 && maxfun >= 1, "trk_host_gcv_bidiag: bad argument");
  std::vector<double> w(6 * (size_t)k + 1, 0.0);
  double *md = w.data(), *mo = md + k, *d = mo + k, *e = d + k, *y = e + k, *q = y + k;
  q[0] = 1.0;                                   // Q^T e1 (beta0 is factored out); q's entry k, along B's left null vector, drops out
  bidiag_to_rrt(alpha, beta, k, q, md, mo);
  const GcvBidiag func{k, beta0, m_eff, md, mo, q, d, e, y};
  fminbound_brent(func, x1, x2, xatol, maxfun, lam_out, fval_out, nfev_out);
  return TRK_OK;
}

// HOST: the Newton iteration of the discrepancy principle (trips/utilities/reg_param/discrepancy_principle.py:80-99, dptype 'tikhonov')
// on a diagonalised problem:   f(beta) = || bhat / (sv*beta + 1) ||^2 + extra - target   (the norm's square root squared, as there).
extern "C" int trk_host_dp_newton(const double* sv, const double* bhat, int n, double target, double extra,
                                  double* alpha_out, int* alpha_set, int* iters_out) {
  TRK_REQUIRE(sv && bhat && alpha_out && alpha_set, "trk_host_dp_newton: NULL argument");
  TRK_REQUIRE(n >= 1, "trk_host_dp_newton: n must be >= 1");
  dp_newton_loop([&](double beta, double* f, double* fp) {
    double zz = 0.0, zwz = 0.0;
    for (int i = 0; i < n; ++i) {
      const double den = sv[i] * beta + 1.0;
      const double z = bhat[i] / den;
      const double w = z / den;
      zz += z * z;
      zwz += z * (w - z);
    }
    const double nz = std::sqrt(zz);
    *f = nz * nz + extra - target;
    *fp = 2.0 / beta * zwz;
  }, alpha_out, alpha_set, iters_out);
  return TRK_OK;
}

// ------------------------------------------------------------------ GKS / MMGKS with regparam = 'gcv': the host's projected problem in one call
// GKS.py:54-74 / MMGKS.py:94-106 as the engine runs them on the host (the reference's DEFAULT regparam): from the Gram data
// G_A = (AV)^T AV, G_L = (LV)^T LV, c = (AV)^T b — R_A, R_L by Cholesky (the economic QRs' R up to row signs), Q_A^T b = R_A^-T c,
// GCV on (R_A, R_L) brought to (diag(s), I) through M = R_A R_L^-1 = U diag(s) W^T, the Tikhonov minimiser by the stacked
// least-squares problem.  The interpreter's version of this sequence (SciPy wrappers around LAPACK) was 250-300 us per iteration WITH
// THE DEVICE IDLE — the next basis vector needs x = V y.  GCV sees M only through s and U^T rhs: M is bidiagonalised (dgebrd), Q^T is
// applied to rhs (dormbr) and the bidiagonal's singular values are found with the left rotations applied to that ONE vector (dbdsqr,
// ncc = 1) — no singular vectors are formed (the dense SVD with both vector sets, what sla.svd computes, is ~5 x the work).  The caller
// hands the LAPACK routines (SciPy's, as plain C pointers).  *ok_out = 0: a factor failed (semi-definite Gram matrix, singular R_L, no
// convergence) — the caller's own branches take over.
extern "C" int trk_host_gram_gcv(void* const* lapack, const double* GA, const double* GL, int ldg, const double* c_select,
                                 const double* c_solve, int k, double m_eff, double* lam_out, double* y_out, int* ok_out) {
  TRK_REQUIRE(lapack && GA && GL && c_select && c_solve && lam_out && y_out && ok_out && k >= 1 && ldg >= k, "trk_host_gram_gcv: bad argument");
  for (int i = 0; i < 6; ++i) TRK_REQUIRE(lapack[i], "trk_host_gram_gcv: six LAPACK routines (dpotrf, dtrtrs, dgebrd, dormbr, dbdsqr, dgelsy)");
  const potrf_fn dpotrf = (potrf_fn)lapack[0];
  const trtrs_fn dtrtrs = (trtrs_fn)lapack[1];
  const gebrd_fn dgebrd = (gebrd_fn)lapack[2];
  const ormbr_fn dormbr = (ormbr_fn)lapack[3];
  const bdsqr_fn dbdsqr = (bdsqr_fn)lapack[4];
  const gelsy_fn dgelsy = (gelsy_fn)lapack[5];
  *ok_out = 0;
  static thread_local std::vector<double> buf, wk;
  static thread_local std::vector<int> ibuf;
  const size_t kk = (size_t)k * k;
  buf.resize(6 * kk + 16 * (size_t)k + 64);
  ibuf.resize((size_t)k + 8);
  double* RA = buf.data();
  double* RL = RA + kk;
  double* X = RL + kk;           // R_L^-T R_A^T
  double* M = X + kk;            // M = X^T = R_A R_L^-1, overwritten by its bidiagonal form
  double* ST = M + kk;           // stacked [R_A; sqrt(lam) R_L], 2k x k
  double* sv = ST + 2 * kk;      // d of the bidiagonal form, then the singular values
  double* e = sv + k;
  double* tq = e + k;
  double* tp = tq + k;
  double* rs = tp + k;           // R_A^-T c_select, then Q^T of it, then U^T of it
  double* rb = rs + k;           // R_A^-T c_solve
  double* b2 = rb + k;           // 2k
  int n = k, one = 1, zero = 0, info = 0;
  char U_ = 'U', T_ = 'T', N_ = 'N', Q_ = 'Q', L_ = 'L';
  // column-major copies of the symmetrised Gram matrices (symmetric: the layout does not matter), upper Cholesky factors
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < k; ++i) {
      RA[i + (size_t)j * k] = 0.5 * (GA[(size_t)i * ldg + j] + GA[(size_t)j * ldg + i]);
      RL[i + (size_t)j * k] = 0.5 * (GL[(size_t)i * ldg + j] + GL[(size_t)j * ldg + i]);
    }
  dpotrf(&U_, &n, RA, &n, &info);
  if (info != 0) return TRK_OK;
  dpotrf(&U_, &n, RL, &n, &info);
  if (info != 0) return TRK_OK;
  for (int j = 0; j < k; ++j)
    for (int i = j + 1; i < k; ++i) RA[i + (size_t)j * k] = RL[i + (size_t)j * k] = 0.0;      // (dpotrf leaves the other triangle as it was)
  double dmin = fabs(RL[0]), dmax = dmin;
  for (int i = 1; i < k; ++i) {
    const double d = fabs(RL[i + (size_t)i * k]);
    dmin = d < dmin ? d : dmin;
    dmax = d > dmax ? d : dmax;
  }
  if (dmin <= 1e-12 * dmax) return TRK_OK;                                                       // (gcv._diagonalise's test)
  for (int i = 0; i < k; ++i) {
    rs[i] = c_select[i];
    rb[i] = c_solve[i];
  }
  dtrtrs(&U_, &T_, &N_, &n, &one, RA, &n, rs, &n, &info);                                        // Q_A^T b = R_A^-T c
  if (info != 0) return TRK_OK;
  dtrtrs(&U_, &T_, &N_, &n, &one, RA, &n, rb, &n, &info);
  if (info != 0) return TRK_OK;
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < k; ++i) X[i + (size_t)j * k] = RA[j + (size_t)i * k];                    // R_A^T
  dtrtrs(&U_, &T_, &N_, &n, &n, RL, &n, X, &n, &info);                                           // R_L^T X = R_A^T
  if (info != 0) return TRK_OK;
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < k; ++i) M[i + (size_t)j * k] = X[j + (size_t)i * k];                     // M = R_A R_L^-1
  // s and U^T rhs without singular vectors: M = Q B P^T (dgebrd), w = Q^T rhs (dormbr), B = U_B diag(s) V_B^T with w <- U_B^T w (dbdsqr)
  int lwork = 64 * k + 64;
  if ((int)wk.size() < lwork) wk.resize(lwork);
  dgebrd(&n, &n, M, &n, sv, e, tq, tp, wk.data(), &lwork, &info);
  if (info != 0) return TRK_OK;
  dormbr(&Q_, &L_, &T_, &n, &one, &n, M, &n, tq, rs, &n, wk.data(), &lwork, &info);
  if (info != 0) return TRK_OK;
  {
    double dummy = 0.0;
    if ((int)wk.size() < 4 * k + 8) wk.resize(4 * k + 8);
    dbdsqr(&U_, &n, &zero, &zero, &one, sv, e, &dummy, &one, &dummy, &one, rs, &n, wk.data(), &info);
    if (info != 0) return TRK_OK;
  }
  for (int i = 0; i < k; ++i)
    if (!std::isfinite(sv[i]) || !std::isfinite(rs[i])) return TRK_OK;
  double lam = 0.0;
  if (int rc = trk_host_gcv_fminbound(sv, rs, k, m_eff, GCV_X1, GCV_X2, GCV_XATOL, GCV_MAXFUN, &lam, nullptr, nullptr)) return rc;
  // y = argmin || R_A y - Q_A^T b ||^2 + lam || R_L y ||^2 = (G_A + lam G_L)^-1 c: by a Cholesky factorisation of the k x k sum — what the
  // device solves with a numeric lambda (trk_gram_tikhonov); R_A and R_L are Cholesky factors of the Gram matrices themselves, so the
  // stacked least-squares problem on them (the reference's lstsq, SciPy's gelsy with rcond = eps: 2.7 k^3 flops of pivoted QR, a third of
  // this call at k = 50) sees the same conditioning.  A sum that is not positive definite: the stacked problem.
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < k; ++i)
      ST[i + (size_t)j * k] = 0.5 * (GA[(size_t)i * ldg + j] + GA[(size_t)j * ldg + i]) +
                              lam * (0.5 * (GL[(size_t)i * ldg + j] + GL[(size_t)j * ldg + i]));
  dpotrf(&U_, &n, ST, &n, &info);
  if (info == 0) {
    for (int i = 0; i < k; ++i) b2[i] = c_solve[i];
    dtrtrs(&U_, &T_, &N_, &n, &one, ST, &n, b2, &n, &info);                                    // U^T z = c
    if (info == 0) dtrtrs(&U_, &N_, &N_, &n, &one, ST, &n, b2, &n, &info);                     // U y = z
    bool fin = info == 0;
    for (int i = 0; fin && i < k; ++i) fin = std::isfinite(b2[i]);
    if (fin) {
      for (int i = 0; i < k; ++i) y_out[i] = b2[i];
      *lam_out = lam;
      *ok_out = 1;
      return TRK_OK;
    }
  }
  const int m2 = 2 * k;
  const double sl = sqrt(lam);
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < k; ++i) {
      ST[i + (size_t)j * m2] = RA[i + (size_t)j * k];
      ST[k + i + (size_t)j * m2] = sl * RL[i + (size_t)j * k];
    }
  for (int i = 0; i < k; ++i) {
    b2[i] = rb[i];
    b2[k + i] = 0.0;
  }
  int* jpvt = ibuf.data();
  for (int i = 0; i < k; ++i) jpvt[i] = 0;
  double rcond = 2.220446049250313e-16, wq = 0.0;
  int rank = 0, mm = m2;
  lwork = -1;
  dgelsy(&mm, &n, &one, ST, &mm, b2, &mm, jpvt, &rcond, &rank, &wq, &lwork, &info);
  if (info != 0) return TRK_OK;
  lwork = (int)wq + 1;
  if ((int)wk.size() < lwork) wk.resize(lwork);
  dgelsy(&mm, &n, &one, ST, &mm, b2, &mm, jpvt, &rcond, &rank, wk.data(), &lwork, &info);
  if (info != 0) return TRK_OK;
  for (int i = 0; i < k; ++i) y_out[i] = b2[i];
  *lam_out = lam;
  *ok_out = 1;
  return TRK_OK;
}
