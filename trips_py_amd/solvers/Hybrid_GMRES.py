"""Hybrid GMRES on the HIP engine — signature, iteration structure and `info` of trips/solvers/Hybrid_GMRES.py:23-87.

Device: Arnoldi steps (1 operator apply + two passes of block Gram-Schmidt against the whole basis = 2 tall-skinny
GEMV-T / GEMV-N pairs), x = V_k y.  Host: H_k, lambda selection, stacked Tikhonov solve.
  `_plan` names a solve's route, `_Run` has one method per route."""
import ctypes as ct
from collections import namedtuple

import numpy as np
import scipy.linalg as sla

from .. import _lib
from .._io import Formatter, History, as_operator
from ..krylov import ArnoldiState, GramSchmidtByGram, _plain_handle_apply
from ..reg_param._bidiag import HessenbergBidiag, bidiag_tikhonov_host
from ..reg_param.discrepancy_principle import discrepancy_principle, discrepancy_principle_bidiag
from ..reg_param.gcv import fminbound_gcv_bidiag
from ._common import check_delta, choose_lambda, tikhonov_lstsq, small_host_blas
from ._iterate import CAPACITY, Iterates
from ._worker import _Searcher

# basis size from which Hybrid-GMRES's GCV goes through the bidiagonal form instead of the dense SVD (below it the SVD is the
# cheaper call: 20 us at k = 10 against 25-60 us of ctypes and NumPy overhead around dgebrd)
BIDIAG_FROM_K = 12
# (the same threshold in the one-call-per-iteration loop: the two routes evaluate one GCV function a rounding apart, and below
# k ~ 10 its minimum can be flat enough for the two answers to differ visibly — 56 % at one iterate of the 512^2 blur with a
# threshold of 2 — so the reference's route, the SVD, keeps the small iterates)
WORKER_FROM_K = BIDIAG_FROM_K


# what the choice of a route depends on (`_caps` below says where each comes from)
Caps = namedtuple("Caps", "world handle one_call device_solve err_ok lapack gram_max_k")
# route: 'library' | 'device' | 'host'; selector: 'number' | 'gcv' | 'dp' | 'l_curve'; worker: the projected problems from k = from_k on are
# jobs of a worker thread; bidiag: an iterate k >= BIDIAG_FROM_K selected in this thread goes through the bidiagonal form, not the SVD
Plan = namedtuple("Plan", "route selector worker from_k bidiag")


def _plan(regparam, n_iter, kwargs, caps):
    """The route of Hybrid_GMRES(…, n_iter, regparam, **kwargs) on an engine with `caps`: touches no device and no library."""
    number = not isinstance(regparam, str)
    deep = n_iter > BIDIAG_FROM_K
    # gcv, a number or dp with delta; one rank, a plain library operator: the host side of an iteration is ONE library call
    # (trk_hgmres_iter: absorb the step that ran ahead, enqueue the next, collect the worker's answer for the iterate before, post this
    # one, launch x = V y) — kwarg c_loop
    c_ok = bool(kwargs.get("c_loop", True) and n_iter >= 2 and caps.world == 1 and caps.handle and caps.one_call and caps.err_ok
                and caps.lapack)
    solvable = number and kwargs.get("device_solve", True) and (regparam > 0 or n_iter < caps.gram_max_k)
    c_fixed = bool(c_ok and number and float(regparam) >= 0.0 and solvable)
    on_dev = bool(number and caps.device_solve and 0 < n_iter and solvable and not c_fixed)
    search = bool(kwargs.get("async_search", True) and caps.lapack and deep)
    # gcv through the bidiagonal form: the search itself on the library's worker thread, one iteration behind (kwarg async_search)
    async_gcv = regparam == "gcv" and kwargs.get("gcv_by_bidiag", True) and search
    # dp the same way
    dp_async = regparam == "dp" and kwargs.get("dp_by_bidiag", True) and search and "explicitProj" not in kwargs
    c_dp = c_ok and dp_async and kwargs.get("delta") is not None
    bidiag = bool(caps.lapack and ((regparam == "gcv" and kwargs.get("gcv_by_bidiag", True))
                                   or (regparam == "dp" and kwargs.get("dp_by_bidiag", True) and "explicitProj" not in kwargs)))
    selector = "number" if number else regparam
    if c_fixed:                                     # a number: no search, no flat minimum — every iterate but the first
        return Plan("library", selector, True, 2, bidiag)
    if async_gcv and c_ok:
        return Plan("library", selector, True, WORKER_FROM_K, bidiag)
    if c_dp:                                        # (from 2: measured, no gain — the early iterates come back unassigned)
        return Plan("library", selector, True, BIDIAG_FROM_K, bidiag)
    if on_dev:
        return Plan("device", selector, False, None, bidiag)
    worker = bool(async_gcv or dp_async)
    return Plan("host", selector, worker, BIDIAG_FROM_K if worker else None, bidiag)


def _caps(A, eng, ar, n, err_ok):
    return Caps(world=getattr(eng, "world", 1), handle=bool(getattr(A, "_h", None)) and _plain_handle_apply(A),
                one_call=(hasattr(eng, "cgs_coeffs") and hasattr(eng, "gemv_n_hosty")
                          and hasattr(getattr(eng, "lib", None), "trk_hgmres_create") and ar.V.data.stride(0) >= n),
                device_solve=hasattr(eng, "hess_tikhonov") and hasattr(eng, "cgs_coeffs"), err_ok=err_ok,
                lapack=HessenbergBidiag.available(), gram_max_k=getattr(eng, "GRAM_TIKHONOV_MAX_K", 0))


class _Run:
    """One Hybrid_GMRES solve: what the steps of a route share, and one method per route (`library`, `device`, `host`)."""

    def __init__(self, A, ar, bv, n_iter, regparam, kwargs, plan, it):
        self.A, self.eng, self.ar, self.bv, self.regparam, self.kwargs, self.plan, self.it = A, A.engine, ar, bv, regparam, kwargs, plan, it
        self.n_iter = n_iter
        self.is_dp = plan.selector == "dp"
        self.Y = self.eng.scalars(max(1, n_iter))
        self.P = self.eng.scalars(n_iter + 2)          # V^T b for the discrepancy principle
        self.lams, self.res = [], []

    def _rel_residual(self, bhat, H, y):
        # reference quirk (:80): `bhat - H@y` broadcasts a (k+1,) against a (k+1,1) -> Frobenius norm of a matrix
        hy = (H @ y).reshape(-1, 1)
        return float(np.linalg.norm(bhat.reshape(1, -1) - hy))

    def solve(self, ii, k, H, Pk=None):
        """Everything the host owes iterate k once H_k is known — lambda_k, y_k, the reference's relResidual — as a function of H_k
        (and, for dp, Pk = V_{k+1}^T b) alone.  (Round 5 measured the obvious next step — several k at once on a small thread pool,
        LAPACK releasing the interpreter lock — and it LOSES: 3.3 k iterations/s against 5.2 k on the 512^2 blur, the hand-over of the
        interpreter lock between the pool and the enqueueing thread costs more than the SVDs overlap.  The SVD of a 61 x 60 H is 0.45 ms
        on a host core, 0.17 ms on average over a 60-step solve, against 66 us of kernels per iteration: that is the 5.2 k with gcv
        against 15.4 k with a number.)"""
        regparam, kwargs, beta0 = self.regparam, self.kwargs, self.ar.beta0
        bidiag = k >= BIDIAG_FROM_K and self.plan.bidiag
        bhat = np.zeros(k + 1)
        bhat[0] = beta0
        hb, svd, lam = None, None, 0               # (:55-56: the first projected problem is unregularised)
        if ii == 0:
            pass
        elif regparam == "gcv" and bidiag:
            # no SVD: [bhat | H] bidiagonalised once (LAPACK dgebrd, a third of the dense SVD's cost), then the O(k)-per-evaluation
            # GCV search and the O(k) Tikhonov solve of the Golub-Kahan form (reg_param/_bidiag.HessenbergBidiag); 'standard' GCV
            # on the k x k diag(s) of (:58) = fullsize k.  Same singular values, same products with bhat: lambda agrees with the
            # SVD route to ~3e-8 at an interior minimum (two evaluations of one smooth function a rounding apart), y to 1e-14.
            hb = HessenbergBidiag(H, beta0)
            lam = fminbound_gcv_bidiag(hb.alphas, hb.betas, hb.beta0, k)
        elif regparam in ("gcv", "l_curve"):
            Qh, sv, Vh = sla.svd(H, full_matrices=False, check_finite=False)
            qb = Qh.T @ bhat
            lam = choose_lambda(regparam, np.diag(sv), np.eye(k), qb, 0.0, kwargs)   # 'standard' GCV here (:58)
            svd = (sv, Vh, qb)
        elif self.is_dp:                           # (the first steps, and whatever the worker hands back: the reference's unassigned /
            if bidiag:                             #  not-reachable-yet branches)
                # the same Newton iteration on the bidiagonal form of [bhat | H] (as 'gcv' above): V^T b in the left basis'
                # coordinates; lambda agrees with the SVD route to 1e-15 (tests/test_host_regparam.py)
                hb = HessenbergBidiag(np.array(H, copy=True), beta0)
                extra = {key: kwargs[key] for key in ("eta",) if key in kwargs}
                lam = discrepancy_principle_bidiag(hb.alphas, hb.betas, hb.left_t(Pk), delta=kwargs.get("delta"), **extra)
                if lam is None or not lam > 0:
                    hb = None
            if hb is None:
                # the SVD discrepancy_principle() takes of H (discrepancy_principle.py:68-70), taken here so that the Tikhonov solve
                # below can share it
                Uf, sv, Vh = sla.svd(H)
                extra = {key: kwargs[key] for key in ("eta", "explicitProj") if key in kwargs}
                lam = discrepancy_principle(None, None, None, 0.0, delta=kwargs.get("delta"), L_is_identity=True,
                                            spectrum=(sv, Uf.T @ np.array(Pk).reshape(-1, 1), (k + 1, k)), **extra)
                svd = (sv, Vh, Uf[:, :k].T @ bhat)
        else:
            lam = regparam
        if hb is not None:
            y = hb.back(bidiag_tikhonov_host(hb.alphas, hb.betas, hb.beta0, np.sqrt(lam)))
        elif svd is not None and lam > 0:
            # the Tikhonov minimiser of (:76) from the SVD the selector needed anyway: y = V diag(s / (s^2 + lam)) U^T bhat — O(k^2)
            # where the stacked least-squares problem is another O(k^3) factorisation per iteration
            sv, Vh, qb = svd
            y = Vh.T @ ((sv / (sv * sv + lam)) * qb)
        else:
            y = tikhonov_lstsq(H, np.eye(k), lam, bhat)
        return lam, y, self._rel_residual(bhat, H, y)

    def inline(self, ii, H, Pk=None):
        self.form(ii, *self.solve(ii, ii + 1, H, Pk))              # iterate ii selected, solved and formed in this thread

    def form(self, ii, lam, y, r):
        self.lams.append(lam)
        self.res.append(r)
        if self.plan.route == "library":           # (the one-call loop: every iterate through the same kernel and partial count)
            self.it.from_host_y(ii + 1, np.ascontiguousarray(y, dtype=np.float64).reshape(-1))
        else:
            self.Y.set(0, y)
            self.it.from_device_y(ii + 1, self.Y.ref(0))                     # x = V[:, :-1] @ y (:77)

    # ---- route 'device'
    def device(self, workers):
        """A numeric regparam: the projected problem stays on the device (trk_hess_tikhonov appends the new column of H from the
        sweep's scalars and solves the k x k normal equations) — nothing visits the host inside the loop; H and every y are
        downloaded once at the end for `relResidual`."""
        eng, ar, it, regparam, kmax = self.eng, self.ar, self.it, self.regparam, self.n_iter
        Hd = eng.scalars((kmax + 1) * kmax)          # column-major, column stride kmax + 1
        Gd = eng.scalars(kmax * kmax)
        Mi = eng.scalars(kmax * kmax)                # (H^T H + lam I)^-1, bordered by one row and column per step
        Yall = eng.scalars(kmax * kmax)              # y of iteration ii in row ii
        for ii in range(kmax):
            k = ar._enqueue()                        # Arnoldi step k = ii + 1: its coefficients sit in ar.S[1 .. 1+2k), ||w||^2 in S[0]
            lam = 0 if ii == 0 else regparam                                # (:55-56: the first projected problem is unregularised)
            self.lams.append(lam)
            # steps 1 (lam = 0) and 2 start the chain, every later step borders the inverse it inherits (same lam)
            mode = 2 if k <= 2 else (1 if lam > 0 else 0)
            eng.hess_tikhonov(Hd.ref(0), kmax + 1, Gd.ref(0), Mi.ref(0), kmax, ar.S.ref(1), None, ar.S.ref(0), ar.beta0, k,
                              lam, mode, Yall.ref(ii * kmax))
            it.from_device_y(k, Yall.ref(ii * kmax))                        # x = V[:, :-1] @ y (:77)
        Hh = Hd.host(0, (kmax + 1) * kmax).reshape(kmax, kmax + 1).T         # (kmax+1) x kmax
        Yh = Yall.host(0, kmax * kmax).reshape(kmax, kmax)
        ar.Hcols = [Hh[:j + 2, j].copy() for j in range(kmax)]
        bhat = np.zeros(kmax + 1)
        bhat[0] = ar.beta0
        for ii in range(kmax):
            k = ii + 1
            self.res.append(self._rel_residual(bhat[:k + 1], Hh[:k + 1, :k], Yh[ii, :k]))

    # ---- route 'host'
    def _enqueue_proj(self, j0, j1):
        """V_{k+1}^T b grows by ONE entry per step (the earlier basis vectors do not change): one dot per step, enqueued behind
        the step and downloaded with it, instead of a sweep over the whole basis and a blocking read per iteration."""
        eng, P = self.eng, self.P
        for j in range(j0, j1):
            eng.dot(self.ar.V[j], self.bv, P.ref(j))
        eng.allreduce(P, j0, j1)
        return j0, j1, P.host_later(j0, j1)

    def _finish(self, jj, lam_w, y, r, Ph):
        """Iterate jj back from the worker: formed from its answer, or (dp without a positive lambda) in this thread."""
        if self.is_dp and not (lam_w is not None and lam_w > 0):
            self.inline(jj, self.ar.H_view()[:jj + 2, :jj + 1], Ph[:jj + 2])
        else:
            self.form(jj, lam_w, y, r)

    def host(self, workers):
        """The Arnoldi step one ahead of the projected problem; from k = plan.from_k on the projected problem of iterate k —
        bidiagonalisation of [bhat | H_k], the search, the Tikhonov solve, y = P' z — is ONE job of the library's worker thread
        (trk_host_worker_post_hess_gcv / _dp), collected one iteration later: this thread only absorbs a step, enqueues the next and
        launches x_{k-1} = V y_{k-1} while the worker and the device run."""
        ar, n_iter, is_dp, kwargs = self.ar, self.n_iter, self.is_dp, self.kwargs
        searcher = workers[0] if workers else None
        Ph = np.zeros(n_iter + 2)
        pend = ar.step_prefetch() if n_iter > 0 else None
        ppend = self._enqueue_proj(0, 2) if (is_dp and pend is not None) else None
        waiting = None                               # the iterate whose job the worker holds
        for ii in range(n_iter):
            k = ii + 1
            ar.absorb(pend)                      # column k of H; step k+1 runs while the host works on the projected problem
            if ppend is not None:
                j0, j1, hnd = ppend
                Ph[j0:j1] = hnd.get()
            pend = ar.step_prefetch() if k < n_iter else None
            ppend = self._enqueue_proj(k + 1, k + 2) if (is_dp and pend is not None) else None
            H = ar.H_view()
            done = None
            if waiting is not None:
                done, waiting = (waiting,) + searcher.collect_vec(waiting + 1), None
            if searcher is not None and k >= BIDIAG_FROM_K and (ii > 0 or not is_dp):
                if is_dp:
                    searcher.post_hess_dp(H, ar.beta0, k, Ph[:k + 1], kwargs.get("delta"), kwargs.get("eta", 1.01))
                else:
                    searcher.post_hess_gcv(H, ar.beta0, k)           # (H is copied before this returns)
                waiting = ii
            if done is not None:
                self._finish(*done, Ph)
            if waiting is None:
                self.inline(ii, H, Ph[:k + 1])
        if waiting is not None:
            self._finish(waiting, *searcher.collect_vec(waiting + 1), Ph)

    # ---- route 'library'
    def library(self, workers):
        """One library call per iteration (trk_hgmres_iter); the projected problems are jobs of the worker threads — with the caller's
        lambda instead of a search when regparam is a number — and the device runs nothing but the Arnoldi steps and x = V y (the ~8 us
        k_hess_tikhonov left every iteration's critical path: 17-18 k -> 20 k iterations/s on the 512^2 blur).  Worker threads: the
        projected problems of consecutive iterates side by side (each O(k^3): ~150 us at k = 60 against ~55 us of kernels per step on
        the 512^2 blur), collected in order."""
        eng, ar, n_iter, lib = self.eng, self.ar, self.n_iter, self.eng.lib
        for w in workers:
            w._need_lapack()
        ar.gram = GramSchmidtByGram(eng, ar.V, ar.capacity + 1)          # (installs the Gram row of V[0])
        wh = (ct.c_void_p * len(workers))(*[w.h for w in workers])
        cap_mb = 64
        while cap_mb < 2 * (2 * n_iter + 4):
            cap_mb *= 2
        mb, mb_view = eng._mailbox_take(cap_mb, 32)                      # pinned memory from the engine's pool
        drv = ct.c_void_p()
        try:
            _lib.check(lib.trk_hgmres_create(self.A._h, ar.V.data.data_ptr(), ar.V.data.stride(0), n_iter, ar.w.data_ptr(), ar.gram.G.ref(0),
                                             ar.gram.kmax, ar.gram.W.ref(0), ar.S.ref(0), mb, wh, len(workers), float(ar.beta0),
                                             eng.stream(), ct.byref(drv)), "trk_hgmres_create")
        except Exception:
            eng._mailbox_give(cap_mb, mb, mb_view)
            raise
        try:
            self._library_loop(lib, drv, len(workers))
            if "host_phases" in self.kwargs:                             # (a list the caller wants the library's phase timers in)
                t5 = (ct.c_double * 5)()
                lib.trk_hgmres_stats(drv, t5)
                self.kwargs["host_phases"][:] = list(t5)
        finally:
            lib.trk_hgmres_destroy(drv)                                  # (waits for what is still posted: then the mailbox may go back)
            eng._mailbox_give(cap_mb, mb, mb_view)

    def _library_loop(self, lib, drv, nw):
        n_iter, kwargs, plan = self.n_iter, self.kwargs, self.plan
        Hp, ldh, ncol = ct.POINTER(ct.c_double)(), ct.c_int(), ct.c_int()
        _lib.check(lib.trk_hgmres_hessenberg(drv, ct.byref(Hp), ct.byref(ldh), ct.byref(ncol)), "trk_hgmres_hessenberg")
        Ht = np.ctypeslib.as_array(Hp, shape=(n_iter + 1, ldh.value))      # Ht[j, i] = H[i, j]: the library's array, filled as steps arrive
        bp = None
        if plan.selector == "number":
            _lib.check(lib.trk_hgmres_fixed_lambda(drv, float(self.regparam)), "trk_hgmres_fixed_lambda")
        elif self.is_dp:
            # V_{k+1}^T b: the first entry here, every further one by the step's own normalising pass (trk_arnoldi_step_post_dot)
            self.eng.dot(self.ar.V[0], self.bv, self.P.ref(0))
            bpp = ct.POINTER(ct.c_double)()
            _lib.check(lib.trk_hgmres_dp(drv, self.bv.data_ptr(), float(self.P.host(0, 1)[0]),
                                         float((kwargs.get("eta", 1.01) * kwargs["delta"]) ** 2), 0.0, ct.byref(bpp)), "trk_hgmres_dp")
            bp = np.ctypeslib.as_array(bpp, shape=(n_iter + 2,))
        _lib.check(lib.trk_hgmres_start(drv), "trk_hgmres_start")
        it, inline, lams, res, iterate = self.it, self.inline, self.lams, self.res, lib.trk_hgmres_iter
        d_ii, d_lam, d_res, d_blk = ct.c_int(), ct.c_double(), ct.c_double(), ct.c_int()
        ref = None if it.xt is None else it.xt.data_ptr()
        posted = []                                                      # iterates whose jobs the workers hold, oldest first

        def one(absorb, more, post, collect):
            """Absorb a step, enqueue `more`, post this iterate's job and (collect) take the oldest posted iterate back, its x = V y
            launched into the next row of the history."""
            jj = posted.pop(0) if collect else None
            row = it.row() if collect else None
            _lib.check(iterate(drv, absorb, more, post, None if row is None else row.data_ptr(), ref, it.partials() if collect else None,
                               CAPACITY, ct.byref(d_ii), ct.byref(d_lam), ct.byref(d_res), ct.byref(d_blk)), "trk_hgmres_iter")
            if not collect:
                return
            if d_ii.value != jj or jj != it.done:
                raise RuntimeError("trk_hgmres_iter: the collected iterate is not the oldest one posted")
            if d_blk.value < 0:                              # dp: no positive lambda from the worker — the reference's other branches, here
                inline(jj, np.ascontiguousarray(Ht[:jj + 1, :jj + 2].T), bp[:jj + 2].copy())
                return
            lams.append(d_lam.value)
            res.append(d_res.value)
            it.wrote(row, d_blk.value)

        for ii in range(n_iter):
            k = ii + 1
            post = k >= plan.from_k
            one(1, 1, int(post), post and len(posted) == nw)              # (the library keeps two steps ahead, n_iter in all)
            if post:
                posted.append(ii)
            else:                                                        # the first iterates: in this thread (SVD route), as before
                # (row-major copies: the layout the Python loop hands to LAPACK — the discrepancy principle's lambda is ill-conditioned
                #  enough at small k for a transposed input's other rounding to show at 1e-6)
                inline(ii, np.ascontiguousarray(Ht[:k, :k + 1].T), bp[:k + 1].copy() if self.is_dp else None)
        while posted:
            one(0, 0, 0, True)


@small_host_blas
def Hybrid_GMRES(A, b, n_iter, regparam="gcv", x_true=None, **kwargs):
    """Returns (x, info); info keys: xHistory (n_iter iterates), regParam, regParam_history (first entry 0),
    relError (if x_true), relResidual, its (= n_iter-1).  Engine-only kwarg: history (True, False, a stride, 'host' or a .npy path: _io.History)."""
    A = as_operator(A)
    check_delta(regparam, kwargs)
    if kwargs.get("dp_stop", False):
        # the reference's dp_stop branch multiplies V[:, :-1] (k-1 columns) by a k-vector and raises (:87-93 / :60-66)
        raise NotImplementedError("dp_stop=True: the reference branch is shape-inconsistent; not reproduced")
    eng = A.engine
    m, n = A.shape
    if m != n:
        raise Exception("Please check the size of the matrx A: it should be square in order to apply hybrid GMRES")
    n_iter = int(n_iter)
    fmt = Formatter(b)
    xt = None if x_true is None else eng.to_vec(x_true, n)

    ar = ArnoldiState(A, b, n_iter)
    bv = eng.to_vec(b, m) if (isinstance(regparam, str) and regparam == "dp") else None
    Hs = History(eng, kwargs.get("history", True), max(1, n_iter), n, "Hybrid_GMRES xHistory")
    it = Iterates(eng, Hs, ar.V, xt, max(1, n_iter))
    plan = _plan(regparam, n_iter, kwargs, _caps(A, eng, ar, n, xt is None or it.err_fused))
    run = _Run(A, ar, bv, n_iter, regparam, kwargs, plan, it)
    # the library route: two worker threads; the host route with searches off this thread: one (host-only entry points: no GPU involved)
    workers = [_Searcher.borrow(_lib.load()) for _ in range(2 if plan.route == "library" else int(plan.worker))]
    clean = False
    try:
        getattr(run, plan.route)(workers)
        clean = True
    finally:
        for w in workers:                            # (after anything but a clean solve a job may still be posted: destroy waits for it)
            w.give_back() if clean else w.close()
    if it.x_dev is None:
        raise UnboundLocalError("Hybrid_GMRES with n_iter < 1 forms no iterate")
    info = {"xHistory": Hs.collect(fmt, n_iter), "regParam": run.lams[-1], "regParam_history": run.lams,
            "relResidual": run.res, "its": n_iter - 1}
    if xt is not None:
        info["relError"] = it.relError()
    return fmt.vec(it.x_dev), info
