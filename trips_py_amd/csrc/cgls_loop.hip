// cgls_loop.hip — whole stretches of CGLS iterations enqueued by ONE library call.
//
// With tol = 0 the recurrence of trips/solvers/CGLS.py:56-80 never needs a value on the host, so nothing but call
// overhead separates consecutive kernels.  Driving the 3-6 launches of an iteration from Python costs ~10 us of
// interpreter + ctypes time per launch — more than the kernels themselves for images up to ~1024^2 (a 512^2 blur runs in
// 3 us).  These two entry points run the same launch sequence as trips_py_amd.solvers.CGLS.CGLSRun.step /
// CGLSRunFused.step in a C loop (same kernels, same scalar layout, bit-identical results), leaving one call per solve.
#include "trk_internal.h"

using namespace trk;

extern "C" {

// Which pair of kernels carries the updates between the operator applies of the raw-partials iteration:
//   0: [x' = x + a p ; r -= a w] after A p, [p = t + b p] after A^T r           (36n bytes; trk_cgls_update_xr_src, trk_cgls_p_update)
//   1: [r -= a w] after A p, [x' = x + a p ; p = t + b p] after A^T r            (32n bytes: p is read once; trk_cgls_r_update,
//                                                                                 trk_cgls_xp_update)
// Measured (iterations/s, 0 vs 1): 512^2 39.1 k vs 38.3 k, 1536^2 23.7 k vs 23.4 k | 3072^2 10.6 k vs 11.1 k, 3584^2 8.30 k vs
// 8.72 k, 4096^2 6.85 k vs 7.26 k, 4608^2 5.48 k vs 5.70 k, 5120^2 4.45 k vs 4.36 k, 6144^2 2.82 k vs 2.74 k, 8192^2 1.53 k vs
// 1.64 k: the saved pass pays from ~8 M unknowns on (small images are launch-bound and the five-stream kernel is the
// slower one per byte).
int trk_cgls_update_grouping(int64_t n) {
  return n >= ((int64_t)8 << 20) ? 1 : 0;
}

int trk_cgls_iterate(trk_op* A, int k_first, int n_iters, float* p, float* r, float* t, float* w, float* X, int64_t x_ld,
                     int keep_history, const float* x_prev, const float* x_true, double* S, double* NP,
                     int np_capacity_blocks, int* n_np_inout, double* PG, double* PD, int pcap, int grouping,
                     trk_stream stream) {
  TRK_REQUIRE(A && p && r && t && w && X && x_prev && S && NP && n_np_inout, "trk_cgls_iterate: NULL argument");
  TRK_REQUIRE(k_first >= 1 && n_iters >= 0, "trk_cgls_iterate: need k_first >= 1, n_iters >= 0");
  const int64_t m = A->rows, n = A->cols;
  int n_np = *n_np_inout;
  // raw-partials form: the operator leaves ||w||^2, ||t||^2 as block partials and the consumers add them up —
  // four launches per iteration instead of six (no reduction-finalize launches)
  const bool raw = PG && PD && pcap > 0 && A->apply_fused;
  const bool xp_form = (grouping < 0 ? trk_cgls_update_grouping(n) : grouping) == 1;
  for (int k = k_first; k < k_first + n_iters; ++k) {
    double* row = S + 5 * (int64_t)k;                       // [delta, gamma, ||x||^2, ||dx||^2, ||x-xt||^2]
    double *delta = row, *gamma = row + 1;
    const double* gamma_old = (k == 1) ? S : row - 4;
    float* x_new = X + (int64_t)(keep_history ? (k - 1) : ((k - 1) & 1)) * x_ld;
    int rc;
    if (raw && xp_form) {
      int n_d = 0, n_g = 0;
      rc = trk_op_apply_fused(A, 0, p, nullptr, 0.0, nullptr, 0, nullptr, 0, nullptr, w, PD, pcap, &n_d, stream);
      if (rc) return rc;
      rc = trk_cgls_r_update(m, gamma_old, PD, n_d, r, w, delta, stream);
      if (rc) return rc;
      rc = trk_op_apply_fused(A, 1, r, nullptr, 0.0, nullptr, 0, nullptr, 0, nullptr, t, PG, pcap, &n_g, stream);
      if (rc) return rc;
      rc = trk_cgls_xp_update(n, gamma_old, delta, PG, n_g, x_prev, p, t, x_new, x_true, gamma,
                              NP + 3 * (int64_t)n_np * (k - 1), np_capacity_blocks, &n_np, stream);
      if (rc) return rc;
      x_prev = x_new;
      continue;
    }
    if (raw) {
      int n_d = 0, n_g = 0;
      rc = trk_op_apply_fused(A, 0, p, nullptr, 0.0, nullptr, 0, nullptr, 0, nullptr, w, PD, pcap, &n_d, stream);
      if (rc) return rc;
      rc = trk_cgls_update_xr_src(n, m, gamma_old, 1, PD, n_d, x_prev, p, x_new, r, w, x_true, delta,
                                  NP + 3 * (int64_t)n_np * (k - 1), np_capacity_blocks, &n_np, stream);
      if (rc) return rc;
      rc = trk_op_apply_fused(A, 1, r, nullptr, 0.0, nullptr, 0, nullptr, 0, nullptr, t, PG, pcap, &n_g, stream);
      if (rc) return rc;
      rc = trk_cgls_p_update(n, t, p, PG, n_g, gamma_old, gamma, stream);
      if (rc) return rc;
      x_prev = x_new;
      continue;
    }
    rc = trk_op_apply(A, 0, p, 0, w, 0, 1, delta, stream);                                      // w = A p, ||w||^2   (:60-61)
    if (rc) return rc;
    rc = trk_cgls_update_xr_deferred(n, m, gamma_old, delta, x_prev, p, x_new, r, w, x_true,      // x, r updates   (:64-67)
                                     NP + 3 * (int64_t)n_np * (k - 1), np_capacity_blocks, &n_np, stream);
    if (rc) return rc;
    rc = trk_op_apply(A, 1, r, 0, t, 0, 1, gamma, stream);                                      // t = A^T r, ||t||^2 (:68-70)
    if (rc) return rc;
    rc = trk_axpby(n, 1.0, nullptr, nullptr, 0, t, 1.0, gamma, gamma_old, 0, p, p, nullptr, stream);   // p = t + (g/g_old) p (:72)
    if (rc) return rc;
    x_prev = x_new;
  }
  *n_np_inout = n_np;
  return TRK_OK;
}

// How many x updates the history-less raw-partials iteration (grouping 1) defers and then makes in ONE pass (trk_cgls_iterate_xbatch);
// 1 = off.  Measured (iterations/s, s = 1 / 2 / 4 / 8, median of three):
//   3072^2 12.0 k / 12.3 k / 12.6 k / 12.6 k | 3584^2 9.32 k / 9.57 k / 9.73 k / 9.81 k | 4096^2 7.64 k / 7.87 k / 8.06 k / 8.09 k |
//   4608^2 6.12 k / 6.26 k / 6.34 k / 6.44 k | 5120^2 5.09 k / 5.28 k / 5.32 k / 5.31 k | 6144^2 3.17 k / 3.18 k / 3.19 k / 3.17 k |
//   8192^2 1.75 k / 1.77 k / 1.77 k / 1.79 k
// (profiles/xbatch/sweep.txt).
// s = 8 is the fastest or level at every size the regrouped updates are used at, so the threshold is theirs (trk_cgls_update_grouping);
// the ten-stream k_cgls_xs_update<8> streams a little below <4> (805 MB in 140 us = 5.8 TB/s against 537 MB in 88 us = 6.1 TB/s at
// 4096^2) and still pays for the writes it saves.
int trk_cgls_x_batch(int64_t n) {
  return n >= ((int64_t)8 << 20) ? 8 : 1;
}

int trk_cgls_iterate_xbatch(trk_op* A, int k_first, int n_iters, float* p, float* ring, int64_t ring_ld, int s, float* r, float* t,
                            float* w, float* X, int64_t x_ld, const float* x_prev, const float* x_true, double* S, double* NP,
                            int np_capacity_blocks, int* n_np_inout, double* PG, double* PD, int pcap, trk_stream stream) {
  TRK_REQUIRE(A && p && r && t && w && X && x_prev && S && NP && n_np_inout && PG && PD && pcap > 0,
              "trk_cgls_iterate_xbatch: NULL argument");
  TRK_REQUIRE(A->apply_fused, "trk_cgls_iterate_xbatch: the operator has no fused apply (trk_op_fused_caps)");
  TRK_REQUIRE(k_first >= 1 && n_iters >= 0, "trk_cgls_iterate_xbatch: need k_first >= 1, n_iters >= 0");
  TRK_REQUIRE(s >= 1 && (s == 1 || (ring && ring_ld >= A->cols)), "trk_cgls_iterate_xbatch: s > 1 needs a ring of s - 1 directions");
  const int64_t m = A->rows, n = A->cols;
  int n_np = *n_np_inout;
  // the directions live in s slots (0: the caller's p, j: ring row j - 1) used round-robin; `cur` holds p_k, the `pending` slots up to
  // it the directions of the iterations whose x update is still to be made
  auto slot = [&](int j) { return j == 0 ? p : ring + (int64_t)(j - 1) * ring_ld; };
  int cur = 0, pending = 0;
  const int k_end = k_first + n_iters;
  for (int k = k_first; k < k_end; ++k) {
    double* row = S + 5 * (int64_t)k;                     // [delta, gamma, ||x||^2, ||dx||^2, ||x-xt||^2]
    const double* gamma_old = (k == 1) ? S : row - 4;
    float* p_k = slot(cur);
    int n_d = 0, n_g = 0;
    int rc = trk_op_apply_fused(A, 0, p_k, nullptr, 0.0, nullptr, 0, nullptr, 0, nullptr, w, PD, pcap, &n_d, stream);
    if (rc) return rc;
    rc = trk_cgls_r_update(m, gamma_old, PD, n_d, r, w, row, stream);
    if (rc) return rc;
    rc = trk_op_apply_fused(A, 1, r, nullptr, 0.0, nullptr, 0, nullptr, 0, nullptr, t, PG, pcap, &n_g, stream);
    if (rc) return rc;
    const bool last = k + 1 == k_end;
    if (++pending < s && !last) {                         // p_{k+1} into the next slot; x waits
      cur = (cur + 1) % s;
      rc = trk_cgls_p_update_to(n, t, p_k, slot(cur), PG, n_g, gamma_old, row + 1, stream);
      if (rc) return rc;
      continue;
    }
    // x_{k-pending+1} .. x_k in one pass, x_k written to the slot trk_cgls_iterate writes it to; p_{k+1} over p_k (in place: it stays
    // cached for the next forward apply), at the end of the call into the caller's p
    float* x_new = X + (int64_t)((k - 1) & 1) * x_ld;
    rc = trk_cgls_xs_update(n, pending, k, S, PG, n_g, x_prev, p, ring, ring_ld, s, (cur - pending + 1 + s) % s, t, x_new,
                            last ? p : p_k, x_true, NP, np_capacity_blocks, &n_np, stream);
    if (rc) return rc;
    x_prev = x_new;
    pending = 0;
    if (last) cur = 0;
  }
  *n_np_inout = n_np;
  return TRK_OK;
}

// Where the recomputing loop below replaces trk_cgls_iterate_xbatch (1 = on).  Measured (iterations/s at s = 8, x-batch loop vs recompute,
// median of three, spread of the runs below 0.4 % everywhere; profiles/recompute/sweep.txt):
//   3072^2 12.74 k vs 13.11 k (+2.9 %) | 3584^2 9.87 k vs 10.27 k (+4.0 %) | 4096^2 8.14 k vs 8.85 k (+8.7 %) | 4608^2 6.44 k vs 6.82 k (+5.9 %) |
//   5120^2 5.23 k vs 5.60 k (+7.1 %) | 6144^2 3.12 k vs 3.92 k (+25.8 %) | 8192^2 1.77 k vs 2.01 k (+13.9 %)
// faster at every size the x-batch loop is used at, so the threshold is that loop's (trk_cgls_x_batch); nothing was measured below it.
int trk_cgls_recompute(int64_t n) {
  return n >= ((int64_t)8 << 20) ? 1 : 0;
}

// trk_cgls_iterate_xbatch without the two temporaries: w = A p_k and t = A^T r are never stored.  Each product is applied twice — once
// for its norm alone (the reduction that must be finished before the coefficient exists), once with the update it feeds as the kernel's
// own epilogue: r <- r - alpha (A p_k) in place, p_{k+1} <- (A^T r) + beta p_k.  Same launch count, same S / NP / PG / PD layout and slot
// arithmetic, the same fp32 operations on every entry (k_blur_slide RC_RATIO), 37n bytes per iteration at s = 8 instead of 44.5n.
// The x update cannot ride on the p update any more (there is no t to read): it is made alone (trk_cgls_xs_update_x) between F1, which
// publishes the delta_k its last step needs, and A0 — before A1 writes a new direction, so that the ring is free by then and p_{k+1}
// may go over p_k.
int trk_cgls_iterate_recompute(trk_op* A, int k_first, int n_iters, float* p, float* ring, int64_t ring_ld, int s, float* r, float* t,
                               float* w, float* X, int64_t x_ld, const float* x_prev, const float* x_true, double* S, double* NP,
                               int np_capacity_blocks, int* n_np_inout, double* PG, double* PD, int pcap, trk_stream stream) {
  (void)t;
  (void)w;
  TRK_REQUIRE(A && p && r && X && x_prev && S && NP && n_np_inout && PG && PD && pcap > 0, "trk_cgls_iterate_recompute: NULL argument");
  TRK_REQUIRE(A->apply_norm && A->apply_ratio, "trk_cgls_iterate_recompute: the operator has no recompute forms (trk_op_recompute_caps)");
  TRK_REQUIRE(A->rows == A->cols, "trk_cgls_iterate_recompute: square operators only");
  TRK_REQUIRE(k_first >= 1 && n_iters >= 0, "trk_cgls_iterate_recompute: need k_first >= 1, n_iters >= 0");
  TRK_REQUIRE(s >= 1 && (s == 1 || (ring && ring_ld >= A->cols)), "trk_cgls_iterate_recompute: s > 1 needs a ring of s - 1 directions");
  const int64_t n = A->cols;
  int n_np = *n_np_inout;
  auto slot = [&](int j) { return j == 0 ? p : ring + (int64_t)(j - 1) * ring_ld; };   // as trk_cgls_iterate_xbatch
  int cur = 0, pending = 0;
  const int k_end = k_first + n_iters;
  for (int k = k_first; k < k_end; ++k) {
    double* row = S + 5 * (int64_t)k;                     // [delta, gamma, ||x||^2, ||dx||^2, ||x-xt||^2]
    const double* gamma_old = (k == 1) ? S : row - 4;
    float* p_k = slot(cur);
    int n_d = 0, n_g = 0;
    int rc = trk_op_apply_sumsq_raw(A, 0, p_k, PD, pcap, &n_d, stream);                                        // F0
    if (rc) return rc;
    rc = trk_op_apply_ratio(A, 0, p_k, 0, -1.0, gamma_old, 1, PD, n_d, r, r, row, 1, stream);                   // F1
    if (rc) return rc;
    const bool last = k + 1 == k_end;
    const bool batch = ++pending >= s || last;
    if (batch) {                                          // x_{k-pending+1} .. x_k in one pass, x_k where trk_cgls_iterate writes it
      float* x_new = X + (int64_t)((k - 1) & 1) * x_ld;
      rc = trk_cgls_xs_update_x(n, pending, k, S, x_prev, p, ring, ring_ld, s, (cur - pending + 1 + s) % s, x_new, x_true, NP,
                                np_capacity_blocks, &n_np, stream);
      if (rc) return rc;
      x_prev = x_new;
      pending = 0;
    }
    rc = trk_op_apply_sumsq_raw(A, 1, r, PG, pcap, &n_g, stream);                                              // A0
    if (rc) return rc;
    // p_{k+1}: behind an x update over p_k (it stays cached for F0), at the end of the call into the caller's p; else the next slot
    float* p_next = batch ? (last ? p : p_k) : slot((cur + 1) % s);
    rc = trk_op_apply_ratio(A, 1, r, 1, 1.0, PG, n_g, gamma_old, 1, p_k, p_next, row + 1, 0, stream);           // A1
    if (rc) return rc;
    if (!batch) cur = (cur + 1) % s;
    if (last) cur = 0;
  }
  *n_np_inout = n_np;
  return TRK_OK;
}

int trk_cgls_iterate_fused(trk_op* A, int k_first, int n_iters, float* P, int64_t p_ld, float* R, int64_t r_ld, float* t,
                           float* w, float* X, int64_t x_ld, int keep_history, const float* x_prev, const float* x_true,
                           double* S, double* PG, double* PD, int pcap, double* NP, int np_capacity_blocks,
                           int* n_g_inout, int* n_np_inout, trk_stream stream) {
  TRK_REQUIRE(A && P && R && t && w && X && x_prev && S && PG && PD && NP && n_g_inout && n_np_inout,
              "trk_cgls_iterate_fused: NULL argument");
  TRK_REQUIRE(k_first >= 1 && n_iters >= 0, "trk_cgls_iterate_fused: need k_first >= 1, n_iters >= 0");
  const int64_t n = A->cols;
  int n_g = *n_g_inout, n_np = *n_np_inout, n_d = 0;
  for (int k = k_first; k < k_first + n_iters; ++k) {
    const int64_t b = 5 * (int64_t)k;
    float *p_old = P + (int64_t)((k - 1) & 1) * p_ld, *p_new = P + (int64_t)(k & 1) * p_ld;
    float *r_old = R + (int64_t)((k - 1) & 1) * r_ld, *r_new = R + (int64_t)(k & 1) * r_ld;
    const double* gprev = (k <= 2) ? S : S + 5 * (int64_t)(k - 2) + 1;      // gamma_{k-2}, published by K2 of iteration k-1
    // K1: p_k = t + (gamma_{k-1}/gamma_{k-2}) p_{k-1} ; w = A p_k
    int rc = trk_op_apply_fused(A, 0, t, p_old, k == 1 ? 0.0 : 1.0, PG, n_g, gprev, 1, p_new, w, PD, pcap, &n_d, stream);
    if (rc) return rc;
    // K2: x_k = x_{k-1} + (gamma_{k-1}/delta_k) p_k ; publishes delta_k -> S[5k], gamma_{k-1} -> S[5(k-1)+1] (S[0] for k = 1)
    float* x_new = X + (int64_t)(keep_history ? (k - 1) : ((k - 1) & 1)) * x_ld;
    double* gpub = (k == 1) ? S : S + b - 4;
    rc = trk_cgls_x_update(n, PG, n_g, PD, n_d, x_prev, p_new, x_new, x_true, S + b, gpub,
                           NP + 3 * (int64_t)n_np * (k - 1), np_capacity_blocks, &n_np, stream);
    if (rc) return rc;
    // K3: r_k = r_{k-1} - (gamma_{k-1}/delta_k) w ; t = A^T r_k ; ||t||^2 partials = gamma_k
    rc = trk_op_apply_fused(A, 1, r_old, w, -1.0, gpub, 1, S + b, 1, r_new, t, PG, pcap, &n_g, stream);
    if (rc) return rc;
    x_prev = x_new;
  }
  *n_g_inout = n_g;
  *n_np_inout = n_np;
  return TRK_OK;
}

}  // extern "C"
