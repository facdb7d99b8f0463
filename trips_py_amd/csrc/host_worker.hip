// host_worker.hip — lambda searches on a worker thread.  The hybrid solvers choose lambda_k on the host from B_k while the device runs the
// steps after k; at 512^2 the bounded Brent search for GCV (a dependent chain of divisions, O(k) per evaluation, ~40 evaluations) is 40 of
// the ~100 us the host spends per iteration — more than the device needs for it.  A worker thread of the library takes the search: posting
// and collecting are two cheap calls, the search overlaps the host's enqueueing of the next step.  One job at a time, inputs copied at post.
#pragma clang fp contract(off)   // (as host_regparam.hip: hess_job's residual is compared with NumPy's)
#include "projected_internal.h"
#include <chrono>
#include <cmath>

using namespace trk;

namespace {
// Hybrid_GMRES.py:54-80 for one k, from H_k ((k+1) x k, column-major, ld = k+1) and beta0: M = [beta0 e1 | H] = Q B P^T (dgebrd; the
// first column is a multiple of e1, so Q^T (beta0 e1) = d[0] e1 and P = diag(1, P')): H = Q B[:, 1:] P'^T with B[:, 1:] LOWER bidiagonal,
// diagonal e[0..k), sub-diagonal d[1..k].  lambda by 'standard' GCV on that triple (fullsize k: the k x k diag(s) of :58), z the
// Tikhonov minimiser, y = P' z, and the reference's relResidual (:80: a (k+1,) minus a (k+1, 1) — the Frobenius norm of a matrix).
int hess_job(trk_host_worker* w, HostJob kind) {
  const char* name = kind == HostJob::HessDp ? "hess_dp" : kind == HostJob::HessFixed ? "hess_fixed" : "hess_gcv";
  const int k = w->k, n = k + 1;
  w->y_valid = 0;
  w->M.assign((size_t)n * n, 0.0);
  w->M[0] = w->beta0;
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < n; ++i) w->M[(size_t)(j + 1) * n + i] = w->H[(size_t)j * n + i];
  w->d.resize(n); w->e.resize(n); w->tq.resize(n); w->tp.resize(n);
  int lwork = 64 * n, info = 0, nn = n, one = 1;
  w->work.resize(lwork);
  ((gebrd_fn)w->gebrd)(&nn, &nn, w->M.data(), &nn, w->d.data(), w->e.data(), w->tq.data(), w->tp.data(), w->work.data(), &lwork, &info);
  if (info != 0) return ::trk::fail(TRK_EINVAL, "trk_host_worker (%s): dgebrd failed (info = %d)", name, info);
  const double *alpha = w->e.data(), *beta = w->d.data() + 1;
  const double b0 = w->d[0];
  char vect = 'P', side = 'L', trans = 'N';
  if (kind == HostJob::HessDp) {
    // the discrepancy principle (discrepancy_principle.py:68-99) wants V_{k+1}^T b in the left basis of the bidiagonal form: Q^T bproj
    vect = 'Q'; trans = 'T';
    ((ormbr_fn)w->ormbr)(&vect, &side, &trans, &nn, &one, &nn, w->M.data(), &nn, w->tq.data(), w->c.data(), &nn, w->work.data(), &lwork, &info);
    if (info != 0) return ::trk::fail(TRK_EINVAL, "trk_host_worker (hess_dp): dormbr failed (info = %d)", info);
    w->have = 0;
    if (int rc = trk_host_dp_bidiag(alpha, beta, k, w->c.data(), w->target, w->extra, &w->lam, &w->have, nullptr, nullptr)) return rc;
    // the caller's in-line branches (unassigned / not reachable yet) — unless it asked for the unreachable case's lambda = 0 solve
    if (!w->have || !(w->lam > 0.0 || (w->lam == 0.0 && w->dp_solves_zero))) return TRK_OK;
    vect = 'P'; trans = 'N';
  } else {                                                      // (HessFixed: w->lam is the caller's number — no search)
    if (kind == HostJob::HessGcv)
      if (int rc = trk_host_gcv_bidiag(alpha, beta, k, b0, w->m_eff, w->x1, w->x2, w->xatol, w->maxfun, &w->lam, nullptr, nullptr)) return rc;
    w->have = 1;
  }
  w->y.assign(n, 0.0);
  if (int rc = trk_host_bidiag_tikhonov(alpha, beta, k, b0, sqrt(w->lam), 0, w->y.data() + 1)) return rc;
  ((ormbr_fn)w->ormbr)(&vect, &side, &trans, &nn, &one, &nn, w->M.data(), &nn, w->tp.data(), w->y.data(), &nn, w->work.data(), &lwork, &info);
  if (info != 0) return ::trk::fail(TRK_EINVAL, "trk_host_worker (%s): dormbr failed (info = %d)", name, info);
  double r2 = 0.0;
  for (int i = 0; i < n; ++i) {
    double hy = 0.0;
    for (int j = 0; j < k; ++j) hy += w->H[(size_t)j * n + i] * w->y[1 + j];
    r2 += (w->beta0 - hy) * (w->beta0 - hy) + (double)k * hy * hy;
  }
  w->resid = sqrt(r2);
  w->y_valid = 1;
  return TRK_OK;
}

// wait until ready(state): poll for up to ~0.4 ms, then sleep on the condition variable.  A wake-up through the kernel costs 50-100 us,
// a job 30-150 us — a caller that arrives a little early (the one-call-per-iteration loop does) must not pay for a sleep
template <class F>
void wait_state(trk_host_worker* w, F&& ready) {
  const auto t0 = std::chrono::steady_clock::now();
  do {
    for (int i = 0; i < 512; ++i) {
      if (ready(w->state.load(std::memory_order_acquire))) return;
      __builtin_ia32_pause();
    }
  } while (std::chrono::steady_clock::now() - t0 <= std::chrono::microseconds(400));
  std::unique_lock<std::mutex> lk(w->m);
  w->cv.wait(lk, [&] { return ready(w->state.load(std::memory_order_acquire)); });
}

void host_worker_main(trk_host_worker* w) {
  for (;;) {
    wait_state(w, [](int st) { return st == 1 || st == 3; });        // (jobs arrive every ~60 us inside a solve)
    if (w->state.load(std::memory_order_acquire) == 3) return;
    if (w->kind == HostJob::GcvBidiag) {
      w->have = 1;
      w->rc = trk_host_gcv_bidiag(w->a.data(), w->b.data(), w->k, w->beta0, w->m_eff, w->x1, w->x2, w->xatol, w->maxfun, &w->lam,
                                  nullptr, nullptr);
    } else if (w->kind == HostJob::DpBidiag) {
      w->rc = trk_host_dp_bidiag(w->a.data(), w->b.data(), w->k, w->c.data(), w->target, w->extra, &w->lam, &w->have, nullptr, nullptr);
    } else {
      w->rc = hess_job(w, w->kind);
    }
    {
      std::lock_guard<std::mutex> lk(w->m);
      w->state.store(2, std::memory_order_release);
    }
    w->cv.notify_all();
  }
}
}  // namespace

extern "C" int trk_host_worker_create(trk_host_worker** out) {
  TRK_REQUIRE(out, "trk_host_worker_create: NULL argument");
  auto* w = new trk_host_worker;
  w->th = std::thread(host_worker_main, w);
  *out = w;
  return TRK_OK;
}

extern "C" int trk_host_worker_destroy(trk_host_worker* w) {
  if (!w) return TRK_OK;
  {
    std::unique_lock<std::mutex> lk(w->m);
    w->cv.wait(lk, [&] { return w->state.load() != 1; });          // a running job finishes first
    w->state.store(3, std::memory_order_release);
  }
  w->cv.notify_all();
  w->th.join();
  delete w;
  return TRK_OK;
}

static int host_worker_post(trk_host_worker* w, HostJob kind) {
  {
    std::lock_guard<std::mutex> lk(w->m);
    w->kind = kind;
    w->state.store(1, std::memory_order_release);
  }
  w->cv.notify_all();
  return TRK_OK;
}

extern "C" int trk_host_worker_post_gcv_bidiag(trk_host_worker* w, const double* alpha, const double* beta, int k, double beta0,
                                               double m_eff, double x1, double x2, double xatol, int maxfun) {
  TRK_REQUIRE(w && alpha && beta && k >= 1, "trk_host_worker_post_gcv_bidiag: bad argument");
  TRK_REQUIRE(w->state.load() != 1, "trk_host_worker_post_gcv_bidiag: a job is still running (collect it first)");
  w->a.assign(alpha, alpha + k);
  w->b.assign(beta, beta + k);
  w->k = k;
  w->beta0 = beta0; w->m_eff = m_eff; w->x1 = x1; w->x2 = x2; w->xatol = xatol; w->maxfun = maxfun;
  return host_worker_post(w, HostJob::GcvBidiag);
}

extern "C" int trk_host_worker_post_dp_bidiag(trk_host_worker* w, const double* alpha, const double* beta_sub, int k,
                                              const double* bproj, double target, double extra) {
  TRK_REQUIRE(w && alpha && beta_sub && bproj && k >= 1, "trk_host_worker_post_dp_bidiag: bad argument");
  TRK_REQUIRE(w->state.load() != 1, "trk_host_worker_post_dp_bidiag: a job is still running (collect it first)");
  w->a.assign(alpha, alpha + k);
  w->b.assign(beta_sub, beta_sub + k);
  w->c.assign(bproj, bproj + k + 1);
  w->k = k;
  w->target = target; w->extra = extra;
  return host_worker_post(w, HostJob::DpBidiag);
}

extern "C" int trk_host_worker_set_lapack(trk_host_worker* w, void* dgebrd, void* dormbr) {
  TRK_REQUIRE(w && dgebrd && dormbr, "trk_host_worker_set_lapack: NULL argument");
  TRK_REQUIRE(w->state.load() != 1, "trk_host_worker_set_lapack: a job is running");
  w->gebrd = dgebrd;
  w->ormbr = dormbr;
  return TRK_OK;
}

// what the three Hessenberg posts share: the checks, and H ((k+1) x k, any strides) copied column-major with beta0
static int stage_hess(trk_host_worker* w, const char* who, const double* H, int64_t h_row_stride, int64_t h_col_stride, int k, double beta0) {
  TRK_REQUIRE(w && H && k >= 1, "%s: bad argument", who);
  TRK_REQUIRE(w->gebrd && w->ormbr, "%s: trk_host_worker_set_lapack first", who);
  TRK_REQUIRE(w->state.load() != 1, "%s: a job is still running (collect it first)", who);
  const int n = k + 1;
  w->H.resize((size_t)n * k);
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < n; ++i) w->H[(size_t)j * n + i] = H[i * h_row_stride + j * h_col_stride];
  w->k = k; w->beta0 = beta0;
  return TRK_OK;
}

extern "C" int trk_host_worker_post_hess_gcv(trk_host_worker* w, const double* H, int64_t h_row_stride, int64_t h_col_stride, int k,
                                             double beta0, double m_eff, double x1, double x2, double xatol, int maxfun) {
  if (int rc = stage_hess(w, "trk_host_worker_post_hess_gcv", H, h_row_stride, h_col_stride, k, beta0)) return rc;
  w->m_eff = m_eff; w->x1 = x1; w->x2 = x2; w->xatol = xatol; w->maxfun = maxfun;
  return host_worker_post(w, HostJob::HessGcv);
}

extern "C" int trk_host_worker_post_hess_fixed(trk_host_worker* w, const double* H, int64_t h_row_stride, int64_t h_col_stride, int k,
                                               double beta0, double lam) {
  TRK_REQUIRE(lam >= 0.0, "trk_host_worker_post_hess_fixed: bad argument");
  if (int rc = stage_hess(w, "trk_host_worker_post_hess_fixed", H, h_row_stride, h_col_stride, k, beta0)) return rc;
  w->lam = lam;
  return host_worker_post(w, HostJob::HessFixed);
}

extern "C" int trk_host_worker_post_hess_dp(trk_host_worker* w, const double* H, int64_t h_row_stride, int64_t h_col_stride, int k,
                                            double beta0, const double* bproj, double target, double extra) {
  TRK_REQUIRE(bproj, "trk_host_worker_post_hess_dp: bad argument");
  if (int rc = stage_hess(w, "trk_host_worker_post_hess_dp", H, h_row_stride, h_col_stride, k, beta0)) return rc;
  w->c.assign(bproj, bproj + k + 1);
  w->target = target; w->extra = extra;
  return host_worker_post(w, HostJob::HessDp);
}

extern "C" int trk_host_worker_collect_vec(trk_host_worker* w, double* lam_out, int* have_out, double* y, int k, double* resid_out) {
  TRK_REQUIRE(w && lam_out && have_out && y && resid_out, "trk_host_worker_collect_vec: NULL argument");
  TRK_REQUIRE(w->state.load() != 0, "trk_host_worker_collect_vec: nothing was posted");
  TRK_REQUIRE(w->kind >= HostJob::HessGcv && k == w->k, "trk_host_worker_collect_vec: the posted job is not a Hessenberg job of this size");
  const int rc = trk_host_worker_collect(w, lam_out, have_out);
  if (rc == TRK_OK && *have_out && w->y_valid) {
    for (int j = 0; j < k; ++j) y[j] = w->y[1 + j];
    *resid_out = w->resid;
  }
  return rc;
}

extern "C" int trk_host_worker_collect(trk_host_worker* w, double* lam_out, int* have_out) {
  TRK_REQUIRE(w && lam_out && have_out, "trk_host_worker_collect: NULL argument");
  TRK_REQUIRE(w->state.load() != 0, "trk_host_worker_collect: nothing was posted");
  wait_state(w, [](int st) { return st == 2; });
  *lam_out = w->lam;
  *have_out = w->have;
  const int rc = w->rc;
  w->state.store(0, std::memory_order_release);
  return rc;
}
