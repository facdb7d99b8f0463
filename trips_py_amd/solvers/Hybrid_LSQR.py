"""Hybrid LSQR on the HIP engine — signature, iteration structure and `info` of trips/solvers/Hybrid_LSQR.py:25-114.

Device: Golub-Kahan steps (2 operator applies + fused axpby/norm kernels), the projected Tikhonov solve on the
bidiagonal (trk_bidiag_tikhonov), x = V y (one tall-skinny GEMV over the row-per-vector basis), ||x - x_true||.
Host (float64, k-sized): lambda selection only.  With a numeric `regparam` nothing is read back inside the loop: the
whole solve is enqueued asynchronously.
`_plan` names the route; a numeric regparam runs `_fixed_lambda`, an automatic one `_AutoLambda`: they share nothing inside the loop.
"""
import ctypes as ct
from collections import namedtuple

import numpy as np
import scipy.linalg as sla

from .. import _lib, _trace
from .._io import Formatter, History, as_operator
from ..krylov import GKState
from ..reg_param.discrepancy_principle import discrepancy_principle_bidiag
from ..reg_param.gcv import fminbound_gcv_bidiag
from ._common import check_delta, choose_lambda, small_host_blas
from ._iterate import CAPACITY, Iterates
from ._worker import _Searcher


# what the choice of a route depends on (`_caps` below says where each comes from)
Caps = namedtuple("Caps", "damped_update step_update hosty err_ok lib select")
# recur: fixed lambda, the iterates by damped LSQR's short recurrence; fuse_update: each update inside the next step's adjoint half;
# host_y: automatic lambda, the projected solve on the host and y in the launch's arguments; worker: the search for lambda on a worker
# thread, one iteration behind; one_call: the host's turn of an iteration as one library call (trk_hlsqr_select)
Plan = namedtuple("Plan", "recur fuse_update host_y worker one_call")


def _plan(regparam, n_iter, kwargs, keep, have_xt, caps):
    """The route of Hybrid_LSQR(…, n_iter, regparam, **kwargs) whose history keeps iterates (`keep`) or not, with or without
    x_true, on an engine with `caps`: touches no device and no library."""
    on_host = isinstance(regparam, str)          # lambda selection needs B_k on the host
    # fixed lambda with every iterate formed: x_k = V_k y_k is the damped-LSQR iterate, which follows from x_{k-1} by Paige &
    # Saunders' short recurrence (an identity in B_k, whatever the orthogonality of V): one pass over three vectors per iterate
    # instead of the projected solve plus a k-term combination (4 k n bytes) — and nothing reads AB, so no norm is flushed
    recur = bool(not on_host and caps.damped_update and kwargs.get("x_by_recurrence", True) and (keep or have_xt) and n_iter >= 2
                 and float(regparam) >= 0.0)
    fuse_update = bool(recur and kwargs.get("update_on_the_step", True) and caps.step_update)
    host_y = bool(on_host and caps.hosty and kwargs.get("host_projected_solve", True) and caps.err_ok)
    # gcv / dp: the search for lambda_k runs on a worker thread of the library (trk_host_worker_*) while this thread enqueues the
    # next step; the iterate of step k is formed one trip later, when its lambda is collected.  (The searches were 20-45 us of
    # the ~100 us this loop spent per iteration at 512^2 x 180 — more than the device needs for an iteration's kernels.)
    worker = bool(on_host and regparam in ("gcv", "dp") and kwargs.get("async_search", True) and caps.lib and n_iter > 2)
    # kwarg one_call (default on): the host's turn of an iteration as one library call (trk_hlsqr_select)
    one_call = bool(worker and host_y and kwargs.get("one_call", True) and caps.select
                    and (regparam == "gcv" or kwargs.get("delta") is not None))
    return Plan(recur, fuse_update, host_y, worker, one_call)


def _caps(eng, gk, xt):
    return Caps(damped_update=hasattr(eng, "lsqr_damped_update"), step_update=gk.native_axpby and hasattr(eng, "gk_step_lsqr"),
                hosty=hasattr(eng, "gemv_n_hosty"), err_ok=xt is None or hasattr(eng, "gemv_n_err"), lib=hasattr(eng, "lib"),
                select=hasattr(getattr(eng, "lib", None), "trk_hlsqr_select"))


def _progress(n_iter, kwargs):
    return _trace.progress(range(n_iter), "running Golub-Kahan bidiagonalization algorithm...", kwargs.get("progress"))   # (Hybrid_LSQR.py:73)


def _solve_on_device(eng, gk, it, Y, W, k, lam):
    """y = lstsq([B; sqrt(lam) I], [beta0 e1; 0]) (:104), on the device from the squared norms in gk.AB (as y_j / alpha_j: the rows
    of V are alpha_j v_j), and x = V y."""
    eng.bidiag_tikhonov(gk.AB.ref(1), 2, gk.AB.ref(2), 2, k, np.sqrt(lam), gk.AB.ref(0), Y.ref(0), W, y_over_alpha=True)
    it.from_device_y(k, Y.ref(0))


def _fixed_lambda(eng, gk, it, plan, regparam, n_iter, keep, kwargs, lams):
    """A numeric regparam: nothing on the host needs B_k.  Iterates that nobody looks at are not formed and the step's last norm stays
    inside the operator (defer); when every iterate IS formed, step k+1 is enqueued BEFORE x_k — its adjoint kernel finishes
    beta_{k+1}^2 on the way (GKState.step(defer=True)), which the projected solve of x_k reads — so that no reduction launch is
    spent on it.  With plan.recur x_k follows from x_{k-1}, and with plan.fuse_update that update rides step k+1's adjoint half,
    whose second operand is the V[k-1] the update needs (trk_gk_step_lsqr: the iteration is three launches on the projector)."""
    xt = it.xt
    wanted = keep or xt is not None
    if plan.recur:
        n = gk.A.shape[1]
        w, x1, st = eng.empty(n), eng.empty(n), eng.scalars(8)
        x_prev, mu = None, np.sqrt(float(regparam))
    else:
        Y = eng.scalars(max(1, n_iter))          # projected solution
        W = eng.scalars(3 * (n_iter + 1) + 4)    # rotation state of the projected solve, resumed while lambda stays the same
    for ii in _progress(n_iter, kwargs):
        _trace.mark("Hybrid_LSQR: Golub-Kahan step, projected problem, iterate")
        k = ii + 1
        if gk.V.k < k:
            gk.step(sync=False, defer=True)
        ahead = k < n_iter and wanted            # step k+1 ahead of x_k
        if not plan.recur:
            if ahead:
                gk.step(sync=False, defer=True)
            if ii > 0:                           # (the reference forms no iterate at the first step)
                lams.append(regparam)
                if wanted or k == n_iter:        # (else nobody looks at this iterate: history=False, no x_true)
                    gk.flush()
                    _solve_on_device(eng, gk, it, Y, W, k, regparam)
        else:
            # step k of the recurrence (the reference reports no iterate for k = 1, the recurrence needs it all the same)
            x = x1 if ii == 0 else it.row()
            ref, partials = (None, None) if ii == 0 else (xt, it.partials())
            st_in, st_out = st.ref(4 * ((ii + 1) & 1)), st.ref(4 * (ii & 1))
            rode = False
            if ahead:
                req = (w, x_prev, x, ref, partials, CAPACITY, mu, st_in, st_out) if plan.fuse_update else None
                gk.step(sync=False, defer=True, lsqr=req)
                rode = req is not None and gk.lsqr_taken
            if rode:
                got = gk.lsqr_blocks
            else:
                # alpha_k^2 = AB[2k-1] and beta_{k+1}^2 = AB[2k] are final: the step enqueued ahead finished the latter
                if k == n_iter:
                    gk.flush()                   # no step was enqueued ahead of the last iterate
                got = eng.lsqr_damped_update(gk.V[ii], w, x_prev, x, gk.AB.ref(2 * k - 1), gk.AB.ref(2 * k), gk.AB.ref(0), mu, st_in, st_out,
                                             ii == 0, ref=ref, partials=partials, capacity=CAPACITY)
            x_prev = x
            if ii > 0:
                lams.append(regparam)
                it.wrote(x, got)


class _AutoLambda:
    """regparam = 'gcv' | 'dp' | 'l_curve': lambda_k is chosen on the host from B_k.  The Golub-Kahan steps do not depend on lambda:
    they are enqueued `ahead` steps in front of the iterate the host is choosing lambda for, each followed by the download of its two
    norms.  One step ahead, the device idled every iteration between the kernels of x_k and the enqueue of step k+2, which waited for
    step k+1's norms (gcv: 115 us per iteration for 75 us of kernels).  The host's turn of an iteration is one of `_inline`, `_posted`
    and `_one_call` (plan.worker, plan.one_call)."""

    def __init__(self, eng, gk, it, plan, regparam, n_iter, keep, kwargs, lams, bv):
        self.eng, self.gk, self.it, self.plan, self.regparam, self.n_iter, self.kwargs, self.lams = eng, gk, it, plan, regparam, n_iter, kwargs, lams
        self.bv = bv                             # the discrepancy principle wants U^T b (None otherwise)
        self.wanted = keep or it.xt is not None
        self.m = gk.A.shape[0]
        self.ahead = max(1, int(kwargs.get("steps_ahead", 3)))
        self.pending, self.n_enq = [], 0
        # B_k's entries (and U^T b in the left basis' scale) as float64 ARRAYS grown in place: the calls below take views of them — the lists
        # of krylov.GKState converted to arrays four times per iteration were O(k) interpreter work each (20 us of a 70 us iteration at k = 100)
        self.al, self.be, self.bp = np.empty(n_iter + 1), np.empty(n_iter + 1), np.empty(n_iter + 2)
        self.n_ab, self.n_bp = 0, 0
        if not plan.host_y:
            self.Y = eng.scalars(max(1, n_iter))          # projected solution
            self.W = eng.scalars(3 * (n_iter + 1) + 4)    # rotation state of the projected solve, resumed while lambda stays the same
        if plan.one_call:
            self.out = ct.c_int(0), ct.c_double(0.0), ct.c_int(0)
            self.dp_target = float((kwargs.get("eta", 1.01) * kwargs["delta"]) ** 2) if regparam == "dp" else 0.0

    def _enqueue_ahead(self):
        gk, n_iter = self.gk, self.n_iter
        while self.n_enq < n_iter and len(self.pending) < self.ahead:
            # (a step's download starts behind the next step: its last norm rides there)
            self.pending.extend(gk.step_prefetch(project=self.bv, more_follow=self.n_enq + 1 < n_iter))
            self.n_enq += 1

    def _grow_host_arrays(self):
        gk, al, be, bp = self.gk, self.al, self.be, self.bp
        n_ab, n_bp = self.n_ab, self.n_bp
        while n_ab < len(gk._alphas):
            al[n_ab], be[n_ab] = gk._alphas[n_ab], gk._betas[n_ab]
            n_ab += 1
        if gk.uproj is not None:
            while n_bp < len(gk.uproj) and n_bp <= n_ab:                 # rows of U are beta_j u_j (beta_0 := beta0)
                bp[n_bp] = gk.uproj[n_bp] / (gk.beta0 if n_bp == 0 else be[n_bp - 1])
                n_bp += 1
        self.n_ab, self.n_bp = n_ab, n_bp

    def run(self, searcher):
        gk, n_iter = self.gk, self.n_iter
        self.searcher = searcher
        turn = self._one_call if self.plan.one_call else self._posted if searcher is not None else self._inline
        waiting = None                           # the step whose lambda the worker is looking for
        self._enqueue_ahead()
        for ii in _progress(n_iter, self.kwargs):
            _trace.mark("Hybrid_LSQR: Golub-Kahan step, projected problem, iterate")
            gk.absorb(self.pending.pop(0))       # alpha_k, beta_{k+1}; the steps behind it run while the host chooses lambda_k
            self._enqueue_ahead()
            self._grow_host_arrays()
            if ii > 0:                           # (the reference forms no iterate at the first step)
                waiting = turn(ii + 1, waiting)
        if waiting is not None:
            self.form(waiting, searcher.collect())

    def form(self, k, lam):
        eng, gk = self.eng, self.gk
        self.lams.append(lam)
        if not self.wanted and k < self.n_iter:
            return                               # nobody looks at this iterate (history=False, no x_true)
        if self.plan.host_y:
            # B_k is on the host already (lambda_k was chosen from it), and so is the projected solve — O(k) on a CPU core, where one
            # GPU lane spent 5-25 us on the dependent square roots and divisions of a recurrence that restarts whenever lambda moves;
            # the k coefficients reach the device in the arguments of the launch that forms x_k
            self.it.from_host_y(k, eng.host_bidiag_tikhonov(self.al[:k], self.be[:k], gk.beta0, np.sqrt(lam), y_over_alpha=True))
        else:
            # (the norms of step k were downloaded, hence finished, before this)
            _solve_on_device(eng, gk, self.it, self.Y, self.W, k, lam)

    def _one_call(self, k, waiting):
        """Collect lambda of the step before, post the search for lambda_k, solve and launch the iterate of the step before: ONE
        library call (trk_hlsqr_select) for what `_posted` does in four."""
        eng, gk, it, regparam = self.eng, self.gk, self.it, self.regparam
        c_nblk, c_lam, c_have = self.out
        kd = waiting if waiting is not None else 0
        form = kd > 0 and (self.wanted or kd >= self.n_iter)
        row = it.row() if form else None
        if regparam == "dp" and self.n_bp < k + 1:
            raise RuntimeError("Hybrid_LSQR: U^T b is behind the bidiagonal")
        _lib.check(eng.lib.trk_hlsqr_select(
            self.searcher.h, 0 if regparam == "gcv" else 1, self.al.ctypes.data, self.be.ctypes.data, k, float(gk.beta0),
            float(self.m) if regparam == "gcv" else self.dp_target, self.bp.ctypes.data, 0.0, kd, gk.V.data.data_ptr(), gk.V.data.stride(0),
            gk.A.shape[1], None if row is None else row.data_ptr(), None if (row is None or it.xt is None) else it.xt.data_ptr(),
            None if row is None else it.partials(), CAPACITY, ct.byref(c_nblk), ct.byref(c_lam), ct.byref(c_have), eng.stream()),
            "trk_hlsqr_select")
        if kd > 0:
            if not c_have.value:
                raise RuntimeError("Hybrid_LSQR: the search on the worker thread set no lambda")
            self.lams.append(c_lam.value)
            if form:
                it.wrote(row, c_nblk.value)
        return k

    def _posted(self, k, waiting):
        """Post the search for lambda_k first, then form the iterate of the step before it."""
        searcher, kwargs = self.searcher, self.kwargs
        lam = searcher.collect() if waiting is not None else None
        if self.regparam == "gcv":
            searcher.post_gcv(self.al[:k], self.be[:k], self.gk.beta0, self.m)
        else:
            if self.n_bp < k + 1:
                raise RuntimeError("Hybrid_LSQR: U^T b is behind the bidiagonal")
            searcher.post_dp(self.al[:k], self.be[:k], self.bp[:k + 1], kwargs.get("delta"), kwargs.get("eta", 1.01))
        if waiting is not None:
            self.form(waiting, lam)
        return k

    def _inline(self, k, waiting):
        """The search for lambda_k in this thread, then iterate k."""
        gk, regparam, kwargs = self.gk, self.regparam, self.kwargs
        if regparam == "gcv":
            # svd(B) (:81) enters GCV through s and Q_A^T bhat = beta0 * (first row of the left vectors) only — and G(lam) is a
            # resolvent of the tridiagonal B B^T: evaluated without the SVD (trk_host_gcv_bidiag); variant 'modified', fullsize = m (:84)
            lam = fminbound_gcv_bidiag(gk._alphas[:k], gk._betas[:k], gk.beta0, self.m)
        elif regparam == "l_curve":
            bhat = np.zeros(k + 1)
            bhat[0] = gk.beta0
            Qb, s, _ = sla.svd(gk.B(k), full_matrices=False)
            lam = choose_lambda(regparam, np.diag(s), np.eye(k), Qb.T @ bhat, 0.0, kwargs, variant="modified", fullsize=self.m)
        elif regparam == "dp":
            # discrepancy_principle(U, B, L, b): projects b on the (no longer exactly orthonormal) computed U (:86)
            # U^T b row by row, downloaded with each step's norms (krylov.GKState.step_prefetch): no pass over U, no blocking copy
            bproj = np.asarray(gk.uproj[:k + 1]) / np.concatenate(([gk.beta0], gk._betas[:k]))   # rows of U are beta_j u_j
            extra = {key: kwargs[key] for key in ("eta", "explicitProj") if key in kwargs}
            # the Newton iteration of discrepancy_principle() (:68-70) on the tridiagonal resolvent: no SVD of B_k
            lam = discrepancy_principle_bidiag(gk._alphas[:k], gk._betas[:k], bproj, delta=kwargs.get("delta"), **extra)
        else:
            lam = regparam
        self.form(k, lam)
        return None


@small_host_blas(when=lambda rp: rp == "l_curve")
def Hybrid_LSQR(A, b, n_iter=100, regparam="gcv", x_true=None, **kwargs):
    """Returns (x, info); info keys: xHistory (n_iter-1 iterates: none is formed at the first step, :77-78), regParam,
    regParam_history, relError (if x_true), relResidual (empty list, as in the reference), its (= n_iter-1).
    Engine-only kwarg: history (True, False, a stride, 'host' or a .npy path: _io.History)."""
    A = as_operator(A)
    check_delta(regparam, kwargs)
    if kwargs.get("dtype") is not None and np.dtype(kwargs["dtype"]) != np.dtype("float32"):
        return _hybrid_lsqr_float64(A, b, int(n_iter), regparam, x_true, kwargs)
    if kwargs.get("dp_stop", False):
        # the reference's dp_stop branch multiplies V[:, :-1] (k-1 columns) by a k-vector and raises (:87-93 / :60-66)
        raise NotImplementedError("dp_stop=True: the reference branch is shape-inconsistent; not reproduced")
    eng = A.engine
    m, n = A.shape
    n_iter = int(n_iter)
    fmt = Formatter(b)
    xt = None if x_true is None else eng.to_vec(x_true, n)

    gk = GKState(A, b, n_iter, normalized=False)     # U[j] = beta_j u_j, V[j] = alpha_j v_j (krylov.GKState)
    bv = eng.to_vec(b, m) if (isinstance(regparam, str) and regparam == "dp") else None
    H = History(eng, kwargs.get("history", True), max(1, n_iter - 1), n, "Hybrid_LSQR xHistory")
    plan = _plan(regparam, n_iter, kwargs, H.keeps_any, xt is not None, _caps(eng, gk, xt))
    # (the recurrence's iterates come from two kernels with different partial counts — the adjoint's tiles or the update's own
    #  grid: each iterate owns 1024 zero-initialised places, all of them are summed)
    it = Iterates(eng, H, gk.V, xt, max(1, n_iter), fixed_stride=plan.recur)
    lams = []
    workers = [_Searcher.borrow(eng.lib)] if plan.worker else []
    clean = False
    try:
        if isinstance(regparam, str):
            _AutoLambda(eng, gk, it, plan, regparam, n_iter, H.keeps_any, kwargs, lams, bv).run(workers[0] if workers else None)
        else:
            _fixed_lambda(eng, gk, it, plan, regparam, n_iter, H.keeps_any, kwargs, lams)
        clean = True
    finally:
        _trace.mark(None)
        for w in workers:                            # (after anything but a clean solve a job may still be posted: destroy waits for it)
            w.give_back() if clean else w.close()
    if it.x_dev is None:
        raise UnboundLocalError("Hybrid_LSQR with n_iter < 2 forms no iterate (the reference fails the same way, "
                                "Hybrid_LSQR.py:114)")
    info = {"xHistory": H.collect(fmt, it.done), "regParam": lams[-1], "regParam_history": lams,
            "relResidual": [], "its": n_iter - 1}
    if xt is not None:
        info["relError"] = it.relError()
    return fmt.vec(it.x_dev), info


def _hybrid_lsqr_float64(A, b, n_iter, regparam, x_true, kwargs):
    """Hybrid_LSQR(..., dtype='float64'): the float64 INSTRUMENT (csrc/ref64.hip, trk_gk_lsqr_chain) — the engine's own arrangement
    of the solver (Golub-Kahan on unnormalised vectors, the iterate by damped LSQR's short recurrence) with its vectors stored in
    float64 and the projector's weights and sums in float64.  For checking the fast path against, not for speed: a numeric
    `regparam` and a parallel-beam operator only.  kwargs: storage ('float64' | 'float32': the element type of the vectors; the
    arithmetic stays float64), weights ('float64' | 'tables64': see Radon2DParallel.set_arithmetic)."""
    import torch
    from .. import _lib
    from ..operators import Radon2DParallel
    if np.dtype(kwargs["dtype"]) != np.dtype("float64"):
        raise ValueError("Hybrid_LSQR: dtype must be 'float32' (the engine) or 'float64' (the instrument)")
    if isinstance(regparam, str) or not isinstance(A, Radon2DParallel):
        raise NotImplementedError("Hybrid_LSQR(dtype='float64') is the diagnostic chain: numeric regparam, Radon2DParallel operator")
    if n_iter < 2:
        raise UnboundLocalError("Hybrid_LSQR with n_iter < 2 forms no iterate (the reference fails the same way, Hybrid_LSQR.py:114)")
    eng = A.engine
    m, n = A.shape
    tdt = torch.float64 if kwargs.get("storage", "float64") == "float64" else torch.float32
    fmt = Formatter(b)
    bv = torch.as_tensor(np.asarray(b, dtype=np.float64).reshape(-1) if not isinstance(b, torch.Tensor) else b.reshape(-1)).to(device=eng.device, dtype=tdt)
    if bv.numel() != m:
        raise ValueError(f"dimension mismatch: b has {bv.numel()} entries, the operator {m} rows")
    X = torch.empty((n_iter, n), dtype=tdt, device=eng.device)
    work = torch.empty(2 * m + 3 * n, dtype=tdt, device=eng.device)
    AB = torch.zeros(2 * n_iter + 1, dtype=torch.float64, device=eng.device)
    st = torch.zeros(8, dtype=torch.float64, device=eng.device)
    rc = eng.lib.trk_gk_lsqr_chain(A._h, bv.element_size(), {"float64": 0, "tables64": 1}[kwargs.get("weights", "float64")], bv.data_ptr(),
                                   n_iter, float(regparam), X.data_ptr(), work.data_ptr(), AB.data_ptr(), st.data_ptr(), eng.stream())
    _lib.check(rc, "trk_gk_lsqr_chain")
    hist = [X[k].to("cpu").numpy().astype(np.float64).reshape(-1, 1) for k in range(1, n_iter)]   # none at the first step (:77-78)
    info = {"xHistory": hist, "regParam": regparam, "regParam_history": [regparam] * (n_iter - 1), "relResidual": [],
            "its": n_iter - 1, "B_squared": AB.to("cpu").numpy()}
    if x_true is not None:
        xt = (x_true.detach().to("cpu").numpy() if isinstance(x_true, torch.Tensor) else np.asarray(x_true)).astype(np.float64).reshape(-1, 1)
        info["relError"] = [float(np.linalg.norm(h - xt) / np.linalg.norm(xt)) for h in hist]
    return (hist[-1] if fmt.numpy else X[n_iter - 1].clone().reshape(-1, 1)), info
