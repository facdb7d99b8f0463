"""The library's host worker thread (trk_host_worker_*) as the hybrid solvers use it: lambda searches and whole projected problems
posted to it, collected one iteration later; idle workers are pooled between solves."""
import atexit
import ctypes
import threading

import numpy as np

_SEARCHER_LOCK = threading.Lock()


class _Searcher:
    """The library's worker thread for the lambda searches (trk_host_worker_*): post copies B_k's entries and returns, collect
    waits for the result.  One per solve."""

    def __init__(self, lib):
        self._ct, self.lib = ctypes, lib
        self.h = ctypes.c_void_p()
        if lib.trk_host_worker_create(ctypes.byref(self.h)) != 0:
            raise RuntimeError("trk_host_worker_create failed")

    def post_gcv(self, alphas, betas, beta0, m_eff, x1=1e-9, x2=1e2, xtol=1e-12, maxfun=1000):
        al = np.ascontiguousarray(alphas, dtype=np.float64)
        be = np.ascontiguousarray(betas, dtype=np.float64)
        if self.lib.trk_host_worker_post_gcv_bidiag(self.h, al.ctypes.data, be.ctypes.data, int(al.size), float(beta0), float(m_eff),
                                                    float(x1), float(x2), float(xtol), int(maxfun)) != 0:
            raise RuntimeError("trk_host_worker_post_gcv_bidiag failed")

    def post_dp(self, alphas, betas, bproj, delta, eta=1.01):
        al = np.ascontiguousarray(alphas, dtype=np.float64)
        be = np.ascontiguousarray(betas, dtype=np.float64)
        bp = np.ascontiguousarray(np.asarray(bproj, dtype=np.float64).reshape(-1))
        if self.lib.trk_host_worker_post_dp_bidiag(self.h, al.ctypes.data, be.ctypes.data, int(al.size), bp.ctypes.data,
                                                   float((eta * delta) ** 2), 0.0) != 0:
            raise RuntimeError("trk_host_worker_post_dp_bidiag failed")

    def post_hess_gcv(self, H, beta0, k, x1=1e-9, x2=1e2, xtol=1e-12, maxfun=1000):
        """Hybrid-GMRES: the whole projected problem of iterate k (bidiagonalisation, GCV, Tikhonov solve, back-transformation) as one
        job; H: a float64 array view of the (k+1) x k Hessenberg matrix (any strides: copied by the library before this returns)."""
        self._need_lapack()
        if H.dtype != np.float64 or H.shape != (k + 1, k):
            raise ValueError("post_hess_gcv: H must be a float64 (k+1) x k array")
        if self.lib.trk_host_worker_post_hess_gcv(self.h, H.ctypes.data, H.strides[0] // 8, H.strides[1] // 8, int(k), float(beta0),
                                                  float(k), float(x1), float(x2), float(xtol), int(maxfun)) != 0:
            raise RuntimeError("trk_host_worker_post_hess_gcv failed")

    def _need_lapack(self):
        if not getattr(self, "_lapack", False):
            from ..reg_param._bidiag import lapack_pointers
            ptrs = lapack_pointers()
            if ptrs is None or self.lib.trk_host_worker_set_lapack(self.h, ptrs[0], ptrs[1]) != 0:
                raise RuntimeError("trk_host_worker_set_lapack failed")
            self._lapack = True

    def post_hess_dp(self, H, beta0, k, bproj, delta, eta=1.01):
        """The same job with the discrepancy principle: bproj = V_{k+1}^T b (k + 1 values, copied)."""
        self._need_lapack()
        bp = np.ascontiguousarray(np.asarray(bproj, dtype=np.float64).reshape(-1))
        if H.dtype != np.float64 or H.shape != (k + 1, k) or bp.size != k + 1:
            raise ValueError("post_hess_dp: H must be a float64 (k+1) x k array, bproj k + 1 values")
        if self.lib.trk_host_worker_post_hess_dp(self.h, H.ctypes.data, H.strides[0] // 8, H.strides[1] // 8, int(k), float(beta0),
                                                 bp.ctypes.data, float((eta * delta) ** 2), 0.0) != 0:
            raise RuntimeError("trk_host_worker_post_hess_dp failed")

    def collect_vec(self, k):
        """(lambda or None, y, relResidual); y and the residual are meaningful only for a positive lambda."""
        lam, have, r = self._ct.c_double(0.0), self._ct.c_int(0), self._ct.c_double(0.0)
        y = np.empty(k, dtype=np.float64)
        if self.lib.trk_host_worker_collect_vec(self.h, self._ct.byref(lam), self._ct.byref(have), y.ctypes.data, int(k),
                                                self._ct.byref(r)) != 0:
            raise RuntimeError("the projected problem failed on the worker thread")
        return (lam.value if have.value else None), y, r.value

    def collect(self):
        lam, have = self._ct.c_double(0.0), self._ct.c_int(0)
        if self.lib.trk_host_worker_collect(self.h, self._ct.byref(lam), self._ct.byref(have)) != 0:
            raise RuntimeError("lambda search failed on the worker thread")
        return lam.value if have.value else None

    def close(self):
        h, self.h = self.h, None
        if h:
            self.lib.trk_host_worker_destroy(h)

    # a solve borrows a worker and hands it back: creating and joining a thread per solve was ~0.1 ms of a 7 ms solve
    _idle = []
    _idle_max = 4

    @classmethod
    def borrow(cls, lib):
        with _SEARCHER_LOCK:
            while cls._idle:
                w = cls._idle.pop()
                if w.h and w.lib is lib:
                    return w
        return cls(lib)

    def give_back(self):
        """After a clean solve (nothing posted and not collected); anything else: close()."""
        with _SEARCHER_LOCK:
            keep = bool(self.h) and len(_Searcher._idle) < _Searcher._idle_max
            if keep:
                _Searcher._idle.append(self)
        if not keep:
            self.close()


@atexit.register
def _close_idle_searchers():
    with _SEARCHER_LOCK:
        idle, _Searcher._idle = _Searcher._idle, []
    for w in idle:
        try:
            w.close()
        except Exception:      # noqa: BLE001  (interpreter shutdown)
            pass
