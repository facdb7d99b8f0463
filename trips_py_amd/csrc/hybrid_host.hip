// hybrid_host.hip — the host's turn of a Hybrid-LSQR / Hybrid-GMRES iteration in one library call each: post and collect the lambda
// searches on the worker threads (host_worker.hip), keep the device's steps enqueued, launch the iterate.
#include "projected_internal.h"
#include <chrono>
#include <cmath>
#include <deque>

using namespace trk;

// ------------------------------------------------------------------ Hybrid-LSQR with automatic lambda: the host's turn of an iteration
// Hybrid_LSQR.py:80-110 as the engine runs it (the search for lambda_k on the worker thread, the iterate of the step before formed when its
// lambda is collected): collect the search posted by the call before, post the search for step k_post (mode 0: gcv, 1: the discrepancy
// principle; B_k's entries and U^T b are the caller's host arrays, read before this returns), and — when k_done > 0 and x_out != NULL —
// solve the projected Tikhonov problem of step k_done with the collected lambda (trk_host_bidiag_tikhonov, y over alpha) and launch
// x_out = V_{k_done} y with y in the kernel's arguments (trk_gemv_n_hosty; ref != NULL: with the error partials).  Four library calls and
// three NumPy temporaries of the interpreter's loop in one.  *have_out = 0: nothing was collected (k_done == 0) or the search set no lambda.
extern "C" int trk_hlsqr_select(trk_host_worker* w, int mode, const double* alphas, const double* betas, int k_post, double beta0,
                                double m_eff_or_target, const double* bproj, double extra, int k_done, const float* V, int64_t ld,
                                int64_t n, float* x_out, const float* ref, double* err_partials, int err_cap, int* n_blocks,
                                double* lam_out, int* have_out, trk_stream stream) {
  TRK_REQUIRE(w && alphas && betas && lam_out && have_out && n_blocks && k_post >= 0 && k_done >= 0, "trk_hlsqr_select: bad argument");
  TRK_REQUIRE(mode == 0 || (mode == 1 && (bproj || k_post == 0)), "trk_hlsqr_select: mode 0 (gcv) or 1 (dp, with U^T b)");
  *have_out = 0;
  *n_blocks = 0;
  double lam = 0.0;
  int have = 0;
  if (k_done > 0) {
    if (int rc = trk_host_worker_collect(w, &lam, &have)) return rc;
    *lam_out = lam;
    *have_out = have;
  }
  if (k_post > 0) {
    if (mode == 0) {
      if (int rc = trk_host_worker_post_gcv_bidiag(w, alphas, betas, k_post, beta0, m_eff_or_target, GCV_X1, GCV_X2, GCV_XATOL, GCV_MAXFUN)) return rc;
    } else if (int rc = trk_host_worker_post_dp_bidiag(w, alphas, betas, k_post, bproj, m_eff_or_target, extra)) return rc;
  }
  if (k_done > 0 && have && x_out) {
    TRK_REQUIRE(V && n >= 0 && ld >= n, "trk_hlsqr_select: x_out given without the basis");
    static thread_local std::vector<double> y;
    y.resize((size_t)k_done);
    if (int rc = trk_host_bidiag_tikhonov(alphas, betas, k_done, beta0, sqrt(lam), 1, y.data())) return rc;
    if (int rc = trk_gemv_n_hosty(V, ld, k_done, n, y.data(), x_out, ref, err_partials, err_cap, n_blocks, stream)) return rc;
  }
  return TRK_OK;
}

// ------------------------------------------------------------------ Hybrid-GMRES: the host side of one iteration in one call
// Hybrid_GMRES.py:46-80 with regparam = 'gcv' as this library runs it: the Arnoldi steps run ahead on the stream (each posts its column
// of H from its last kernel), iterate k's projected problem — bidiagonalisation of [beta0 e1 | H_k], the GCV search, the Tikhonov solve —
// is one job of a worker thread, and x_k = V_k y_k is launched with y_k in the kernel's arguments when the job is collected.  Nothing
// in the Arnoldi process waits for a projected solution, so the jobs of consecutive iterates run on SEVERAL workers side by side (a job
// is O(k^3): ~150 us at k = 60 against ~55 us of kernels per step) and are collected in order, `workers` iterations late.  What the
// interpreter did per iteration (seven library calls, three NumPy temporaries, ~70 us) is one call here.
struct trk_hgmres {
  trk_op* op;
  float* V;
  int64_t ld;
  int cap;                 // Arnoldi steps at most (H is (cap + 1) x cap)
  float* w;
  double *G, *W, *S;
  int ldg;
  trk_mailbox* mb;         // borrowed: 2 slots, a region of 2 cap + 4 doubles each
  double* mb_host;
  std::vector<trk_host_worker*> ws;   // borrowed
  double beta0;
  std::vector<double> H;   // column-major, column stride ldh
  int ldh;
  int k_enq, k_abs;        // steps enqueued / columns of H installed
  std::deque<int> posted;  // iterates (0-based) whose projected problems the workers hold, oldest first
  unsigned long long post_seq, collect_seq;
  std::vector<double> y;
  hipStream_t stream;
  double t_wait_step = 0, t_enqueue = 0, t_collect = 0, t_post = 0, t_launch = 0;     // host seconds by phase (trk_hgmres_stats)
  double fixed_lam = -1.0;                                                              // >= 0: the jobs solve with this lambda (no search)
  // the discrepancy principle: V_{k+1}^T b grows by one entry per step (taken by the step's normalising pass, posted with its scalars)
  const float* bvec = nullptr;
  std::vector<double> bproj;
  double dp_target = 0.0, dp_extra = 0.0;
};
static inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

extern "C" int trk_hgmres_fixed_lambda(trk_hgmres* g, double lam) {
  TRK_REQUIRE(g, "trk_hgmres_fixed_lambda: NULL handle");
  g->fixed_lam = lam;                          // (< 0: back to gcv)
  return TRK_OK;
}

extern "C" int trk_hgmres_dp(trk_hgmres* g, const float* bvec, double bproj0, double target, double extra, double** bproj_out) {
  TRK_REQUIRE(g && bvec && g->k_enq == 0, "trk_hgmres_dp: before trk_hgmres_start, with the right-hand side on the device");
  g->bvec = bvec;
  g->bproj.assign((size_t)g->cap + 2, 0.0);
  g->bproj[0] = bproj0;
  g->dp_target = target;
  g->dp_extra = extra;
  for (trk_host_worker* w : g->ws) w->dp_solves_zero = 1;      // (reset by trk_hgmres_destroy: the workers are borrowed)
  if (bproj_out) *bproj_out = g->bproj.data();
  return TRK_OK;
}

extern "C" int trk_hgmres_stats(trk_hgmres* g, double* seconds5) {
  TRK_REQUIRE(g && seconds5, "trk_hgmres_stats: NULL argument");
  seconds5[0] = g->t_wait_step; seconds5[1] = g->t_enqueue; seconds5[2] = g->t_collect; seconds5[3] = g->t_post; seconds5[4] = g->t_launch;
  return TRK_OK;
}

extern "C" int trk_hgmres_create(trk_op* op, float* V, int64_t ld, int capacity, float* w, double* G, int ldg, double* W, double* S,
                                 trk_mailbox* mb, trk_host_worker* const* workers, int n_workers, double beta0, trk_stream stream,
                                 trk_hgmres** out) {
  TRK_REQUIRE(op && V && w && G && W && S && out && mb && workers && capacity >= 1 && ldg >= capacity, "trk_hgmres_create: bad argument");
  TRK_REQUIRE(op->rows == op->cols && ld >= op->rows, "trk_hgmres_create: square operator, ld >= n");
  TRK_REQUIRE(n_workers >= 1 && n_workers <= 16, "trk_hgmres_create: 1..16 workers");
  for (int i = 0; i < n_workers; ++i)
    TRK_REQUIRE(workers[i] && workers[i]->gebrd && workers[i]->ormbr, "trk_hgmres_create: every worker with trk_host_worker_set_lapack done");
  auto* g = new trk_hgmres{};
  g->op = op; g->V = V; g->ld = ld; g->cap = capacity; g->w = w; g->G = G; g->W = W; g->S = S; g->ldg = ldg;
  g->beta0 = beta0; g->ldh = capacity + 2; g->stream = (hipStream_t)stream;
  g->H.assign((size_t)g->ldh * (size_t)(capacity + 1), 0.0);
  g->y.assign((size_t)capacity + 1, 0.0);
  g->ws.assign(workers, workers + n_workers);
  g->mb = mb;
  int rc = trk_mailbox_host(mb, &g->mb_host);
  if (!rc && (trk_mailbox_doubles(mb) < 2 * (2 * capacity + 4) || trk_mailbox_slots(mb) < 2))
    rc = fail(TRK_EINVAL, "trk_hgmres_create: the mailbox needs 2 slots and 2 (2 capacity + 4) doubles (a region per slot: two steps are in flight)");
  if (rc) {
    delete g;
    return rc;
  }
  *out = g;
  return TRK_OK;
}

// (the mailbox and the workers are the caller's: pinned memory and threads are pooled above the library — creating and freeing them
// per solve costs more than the iterations of a short solve)
extern "C" int trk_hgmres_destroy(trk_hgmres* g) {
  if (!g) return TRK_OK;
  if (g->k_enq > g->k_abs) (void)trk_mailbox_wait(g->mb, g->k_enq & 1);              // a posted step still writes to the mailbox
  while (!g->posted.empty()) {                                                        // jobs nobody collected: the workers go back idle
    double lam, r;
    int have;
    (void)trk_host_worker_collect_vec(g->ws[g->collect_seq % g->ws.size()], &lam, &have, g->y.data(), g->posted.front() + 1, &r);
    g->posted.pop_front();
    ++g->collect_seq;
  }
  for (trk_host_worker* w : g->ws) w->dp_solves_zero = 0;
  delete g;
  return TRK_OK;
}

extern "C" int trk_hgmres_hessenberg(trk_hgmres* g, double** H, int* ldh, int* columns) {
  TRK_REQUIRE(g && H && ldh && columns, "trk_hgmres_hessenberg: NULL argument");
  *H = g->H.data();
  *ldh = g->ldh;
  *columns = g->k_abs;
  return TRK_OK;
}

// the next Arnoldi step, its scalars posted to slot (k & 1)
static int hgmres_enqueue(trk_hgmres* g) {
  const int k = g->k_enq + 1;
  TRK_REQUIRE(k <= g->cap, "trk_hgmres: more steps than the basis was planned for");
  if (int rc = trk_arnoldi_step_post_dot(g->op, g->V, g->ld, k, g->w, g->G, g->ldg, g->W, g->S, g->mb, k & 1, 0, 1 + 2 * k,
                                         (k & 1) * (2 * g->cap + 4), g->bvec, 2 * g->cap + 2, g->stream))
    return rc;
  g->k_enq = k;
  return TRK_OK;
}
// Two steps ahead of the columns installed: step k + 1 needs nothing from the host, and enqueued only once step k's scalars had
// arrived it left the device idle for a launch latency per step (S is rewritten by step k + 1 only after step k's last kernel has
// posted it: stream order)
static int hgmres_keep_ahead(trk_hgmres* g) {
  while (g->k_enq < g->cap && g->k_enq < g->k_abs + 2)
    if (int rc = hgmres_enqueue(g)) return rc;
  return TRK_OK;
}

extern "C" int trk_hgmres_start(trk_hgmres* g) {
  TRK_REQUIRE(g && g->k_enq == 0, "trk_hgmres_start: once, first");
  return hgmres_keep_ahead(g);
}

/* One pass of the loop: absorb, enqueue_next (two steps stay on the stream ahead of the columns installed), x_done, post_job as trk.h
 * describes them.  The collect comes before the post (with every worker busy the caller collects in the same call), the launch after it. */
extern "C" int trk_hgmres_iter(trk_hgmres* g, int absorb, int enqueue_next, int post_job, float* x_done, const float* ref,
                               double* err_partials, int err_cap, int* done_ii, double* done_lam, double* done_resid, int* done_blocks) {
  TRK_REQUIRE(g && done_ii && done_lam && done_resid && done_blocks, "trk_hgmres_iter: NULL argument");
  *done_ii = -1;
  *done_blocks = 0;
  const size_t nw = g->ws.size();
  if (absorb) {
    TRK_REQUIRE(g->k_enq > g->k_abs, "trk_hgmres_iter: no step is pending");
    const int k = g->k_abs + 1;
    const double t0 = now_s();
    if (int rc = trk_mailbox_wait(g->mb, k & 1)) return rc;
    g->t_wait_step += now_s() - t0;
    const double* h = g->mb_host + (size_t)(k & 1) * (2 * g->cap + 4);   // S[0] = h_{k+1,k}^2, S[1..1+k) + S[1+k..1+2k) = the column above it
    double* col = g->H.data() + (size_t)(k - 1) * g->ldh;
    for (int i = 0; i < k; ++i) col[i] = h[1 + i] + h[1 + k + i];
    col[k] = sqrt(h[0]);
    if (g->bvec) g->bproj[k] = h[1 + 2 * k];
    g->k_abs = k;
  }
  double t1 = now_s();
  if (enqueue_next)
    if (int rc = hgmres_keep_ahead(g)) return rc;
  g->t_enqueue += now_s() - t1;
  t1 = now_s();
  int done = -1;
  if (x_done) {
    TRK_REQUIRE(!g->posted.empty(), "trk_hgmres_iter: x_done given but no job is posted");
    int have = 0;
    done = g->posted.front();
    if (int rc = trk_host_worker_collect_vec(g->ws[g->collect_seq % nw], done_lam, &have, g->y.data(), done + 1, done_resid)) return rc;
    g->posted.pop_front();
    ++g->collect_seq;
    if (!have || (g->bvec && !g->ws[(g->collect_seq - 1) % nw]->y_valid)) {   // the discrepancy principle's "unassigned": the caller's branch
      TRK_REQUIRE(g->bvec, "trk_hgmres_iter: the worker returned no lambda");
      *done_ii = done;
      *done_blocks = -1;
      done = -1;
    }
  }
  g->t_collect += now_s() - t1;
  t1 = now_s();
  if (post_job) {
    TRK_REQUIRE(g->k_abs >= 1 && g->posted.size() < nw, "trk_hgmres_iter: post_job needs a column of H and a free worker (collect first)");
    const int k = g->k_abs;
    if (g->bvec) {
      if (int rc = trk_host_worker_post_hess_dp(g->ws[g->post_seq % nw], g->H.data(), 1, g->ldh, k, g->beta0, g->bproj.data(), g->dp_target, g->dp_extra))
        return rc;
    } else if (g->fixed_lam >= 0.0) {
      if (int rc = trk_host_worker_post_hess_fixed(g->ws[g->post_seq % nw], g->H.data(), 1, g->ldh, k, g->beta0, g->fixed_lam)) return rc;
    } else if (int rc = trk_host_worker_post_hess_gcv(g->ws[g->post_seq % nw], g->H.data(), 1, g->ldh, k, g->beta0, (double)k, GCV_X1, GCV_X2, GCV_XATOL, GCV_MAXFUN))
      return rc;
    g->posted.push_back(k - 1);
    ++g->post_seq;
  }
  g->t_post += now_s() - t1;
  t1 = now_s();
  if (done >= 0) {
    if (int rc = trk_gemv_n_hosty(g->V, g->ld, done + 1, g->op->rows, g->y.data(), x_done, ref, err_partials, err_cap, done_blocks,
                                  g->stream))
      return rc;
    *done_ii = done;
  }
  g->t_launch += now_s() - t1;
  return TRK_OK;
}
