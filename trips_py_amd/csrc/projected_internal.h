// projected_internal.h — shared by the host side of the projected problems: host_regparam.hip, host_worker.hip, hybrid_host.hip
#pragma once
#include "trk_internal.h"
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

namespace trk {
// the caller's LAPACK (SciPy's), handed over as plain C pointers: Fortran convention, every argument by reference
typedef void (*potrf_fn)(char*, int*, double*, int*, int*);
typedef void (*trtrs_fn)(char*, char*, char*, int*, int*, double*, int*, double*, int*, int*);
typedef void (*gebrd_fn)(int*, int*, double*, int*, double*, double*, double*, double*, double*, int*, int*);
typedef void (*ormbr_fn)(char*, char*, char*, int*, int*, int*, double*, int*, double*, double*, int*, double*, int*, int*);
typedef void (*bdsqr_fn)(char*, int*, int*, int*, int*, double*, double*, double*, int*, double*, int*, double*, int*, double*, int*);
typedef void (*gelsy_fn)(int*, int*, int*, double*, int*, double*, int*, int*, double*, int*, double*, int*, int*);

constexpr double GCV_X1 = 1e-9, GCV_X2 = 1e2, GCV_XATOL = 1e-12;   // the box of every GCV search (reg_param/gcv.py:94-95):
constexpr int GCV_MAXFUN = 1000;                                   //   fminbound(gcv_funct, 1e-9, 1e2, xtol=1e-12, maxfun=1000)

enum class HostJob {
  GcvBidiag,   // trk_host_gcv_bidiag on (a, b) = B_k
  DpBidiag,    // trk_host_dp_bidiag on B_k and c = U^T b
  HessGcv,     // Hybrid-GMRES (these three stay last): the whole projected problem of one iterate from H_k, lambda by GCV
  HessDp,      //   ... lambda by the discrepancy principle (c = V_{k+1}^T b)
  HessFixed,   //   ... lambda is the caller's number: no search
};
}  // namespace trk

struct trk_host_worker {
  std::thread th;
  std::mutex m;
  std::condition_variable cv;
  std::atomic<int> state{0};      // 0 idle, 1 posted, 2 done, 3 stop
  trk::HostJob kind = trk::HostJob::GcvBidiag;
  std::vector<double> a, b, c;    // B_k: diagonal, sub-diagonal; the projected right-hand side of a DP job
  int k = 0;
  double beta0 = 0.0;                                   // every kind but DpBidiag
  double m_eff = 0.0, x1 = 0.0, x2 = 0.0, xatol = 0.0;  // the GCV kinds: the objective's m and the search box
  int maxfun = 0;
  double target = 0.0, extra = 0.0;                     // the DP kinds
  double lam = 0.0;               // the job's result; HessFixed: posted with the caller's lambda
  int have = 0, rc = 0;
  // the Hessenberg kinds: [beta0 e1 | H] bidiagonalised by the caller's LAPACK (dgebrd / dormbr), lambda, the Tikhonov solve, the residual
  void *gebrd = nullptr, *ormbr = nullptr;
  std::vector<double> M, H, d, e, tq, tp, work, y;
  double resid = 0.0;
  int dp_solves_zero = 0;         // HessDp: "the discrepancy cannot be reached yet" (lambda = 0) is solved here too (trk_hgmres's workers)
  int y_valid = 0;                // the last Hessenberg job left y and resid
};
