"""MRNSD on the HIP engine: min ||b - A x|| over x >= 0 — the modified residual norm steepest descent of Nagy and Strakos, IR Tools'
IRmrnsd, called like `CGLS(A, b, x0, max_iter, tol)` on the same operators.

With r = b - A x, g = -A^T r and s = -(x . g) (steepest descent in the metric scaled by x), per iteration, all on the GPU:
    u = A s ; ||u||^2 from the operator (a finished scalar, or raw block partials where trk_op_fused_caps says so)
    z = A^T u
    one kernel (trk_mrnsd_update): alpha = min(gamma / ||u||^2, bound) ; x = max(x + alpha s, 0) ; g += alpha z ; s = -(x . g) ;
        r -= alpha u ; the next gamma = -<g, s> and bound = min_{s_i < 0} x_i / -s_i, and the reported norms
Vectors are fp32, scalars and reductions fp64; nothing visits the host unless a stopping rule asks (include/trk.h: the layout of S).
Not built: sharded MRNSD, a periodic refresh of g from a true product, the s / r updates fused into the blur's two-operand form,
weighted variants (Poisson data: solvers.MLEM), box constraints (solvers.PDHG takes a box).
"""
import numpy as np

from .._io import Formatter, _host, as_operator
from ._run import IterationRun


def default_x0(A, bv, background=None):
    """The constant start sum(b) / sum(A 1) when that is positive, else 1 (a device vector).  background (solvers.MLEM): a number or
    an m-vector on the host that is taken off b first, sum(b - background) / sum(A 1)."""
    eng = A.engine
    ones = eng.to_vec(np.ones(A.shape[1], dtype=np.float32))
    a1 = A.apply(ones)
    sb, sa = float(_host(bv).astype(np.float64).sum()), float(_host(a1).astype(np.float64).sum())
    if background is not None:
        sb -= float(np.broadcast_to(np.asarray(background, dtype=np.float64), (A.shape[0],)).sum())
    c = sb / sa if sa != 0.0 else 0.0
    if not (np.isfinite(c) and c > 0.0):
        c = 1.0
    return eng.to_vec(np.full(A.shape[1], c, dtype=np.float32))


class MRNSDRun(IterationRun):
    """The MRNSD recurrence as an object, like CGLSRun: `step()` enqueues one iteration from Python, `run(n)` n of them in one
    library call (trk_mrnsd_iterate: the same kernels, the same bits), `rows()` / `row(k)` download the scalars.

    S[0..2] = gamma_0, bound_0, ||r_0||^2 ; row k at 8k = [||u||^2, alpha, gamma_k, bound_k, ||x||^2, ||dx||^2, ||x - x_true||^2, ||r||^2]
    with gamma_k, bound_k what iteration k leaves.  x0 must be >= 0 (MRNSD() checks it)."""

    PCAP = 4096                            # room for an operator's raw block partials
    CAP = 1024                             # blocks of a streaming kernel at most (gamma / bound / norm partials)

    def __init__(self, A, b, x0, max_iter, x_true=None, history=True):
        A = as_operator(A)
        if A.engine.world > 1:
            raise NotImplementedError("MRNSD is not built for unknowns spread over ranks (eng.world > 1)")
        super().__init__(A, b, max_iter, x_true, history, "MRNSD xHistory")
        eng, max_iter = self.eng, self.max_iter
        m, n = A.shape
        x_start = default_x0(A, self.bv) if x0 is None else eng.to_vec(x0, n)
        self.g, self.s, self.z = eng.empty(n), eng.empty(n), eng.empty(n)
        self.r, self.u = eng.empty(m), eng.empty(m)
        self.S = S = eng.scalars(8 * (max_iter + 1))
        self.GB = eng.scalars(4 * self.CAP)            # two gb buffers: iteration k reads half (k-1) & 1, writes half k & 1
        self.B = eng.scalars(1)                        # ||b||^2
        # operators that leave ||A s||^2 as raw block partials (the blur, the projectors): the update kernel adds them up itself
        self.raw = bool(hasattr(A, "_h") and hasattr(eng, "op_can_fuse") and eng.op_can_fuse(A._h))
        self.PU = eng.scalars(self.PCAP) if self.raw else None
        self._final = 0
        # r = b - A x0 ; g = -A^T r ; s, gamma_0, bound_0, ||r_0||^2
        A.apply(x_start, out=self.r)
        eng.axpby(1.0, self.bv, -1.0, self.r, self.r)
        A.apply(self.r, out=self.g, transpose=True)
        eng.scale(-1.0, self.g, self.g)
        eng.nrm2sq(self.bv, self.B.ref(0))
        self.n_np = eng.mrnsd_init(x_start, self.g, self.r, self.s, self.GB.ref(0), self.CAP, S.ref(0))
        self.NP = eng.scalars(4 * self.n_np * max(1, max_iter))
        self.x_cur = x_start

    def _half(self, k):
        return 2 * self.CAP * (k & 1)

    def _step(self):
        eng, A, S = self.eng, self.A, self.S
        self.k += 1
        k = self.k
        row = 8 * k
        x_new = self.hist.row(k - 1)
        if self.raw:
            n_u = eng.op_apply_fused(A._h, False, self.s, None, 0.0, None, 0, None, 0, None, self.u, self.PU.ref(0), self.PCAP)
            unorm = self.PU.ref(0)
        else:
            A.apply(self.s, out=self.u, sumsq=S.ref(row))
            n_u, unorm = 1, S.ref(row)
        A.apply(self.u, out=self.z, transpose=True)
        src, dst = self._half(k - 1), self._half(k)
        self.n_np = eng.mrnsd_update(self.GB.ref(src), self.n_np, self.GB.ref(src + self.CAP), self.n_np, unorm, n_u, self.x_cur, x_new,
                                     self.g, self.s, self.z, self.r, self.u, self.xt, self.GB.ref(dst), self.CAP, S.ref(row),
                                     S.ref(0) if k == 1 else S.ref(row - 6), self.NP.ref(4 * self.n_np * (k - 1)), self.CAP)
        self.x_cur = x_new

    def _c_loop(self):
        """One library call on the HIP engine (trk_mrnsd_iterate)."""
        eng = self.eng
        if not (hasattr(self.A, "_h") and hasattr(eng, "mrnsd_iterate")):
            return None

        def call(k_first, n, X, keep):
            self.n_np = eng.mrnsd_iterate(self.A._h, k_first, n, self.g, self.s, self.z, self.r, self.u, X, keep, self.x_cur,
                                          self.xt, self.S.ref(0), self.GB.ref(0), self.CAP, self.NP.ref(0), self.CAP, self.n_np,
                                          None if not self.raw else self.PU.ref(0), self.PCAP if self.raw else 0)
        return call

    def _finish(self):
        """gamma_k, bound_k of the last iteration (still block partials) and the reported sums of every iteration into S."""
        k = self.k
        if k == 0 or self._final == k:
            return
        eng, h = self.eng, self._half(k)
        eng.mrnsd_finish(self.GB.ref(h), self.n_np, self.GB.ref(h + self.CAP), self.n_np, self.S.ref(8 * k + 2))
        eng.finalize_batched(self.NP.ref(0), self.n_np, 4, k, self.S.ref(12), 8)
        self._final = k

    def row(self, k):
        """Row k of S (host sync)."""
        self._finish()
        return self.S.host(8 * k, 8 * k + 8)

    def rows(self):
        """([gamma_0, bound_0, ||r_0||^2], the k rows) on the host."""
        self._finish()
        Sh = self.S.host()
        return Sh[0:3].copy(), Sh[8:8 * (self.k + 1)].reshape(self.k, 8)

    def b_norm(self):
        return float(np.sqrt(self.B.host(0, 1)[0]))


def MRNSD(A, b, x0, max_iter, tol, x_true=None, **kwargs):
    """Modified residual norm steepest descent: min ||b - A x|| subject to x >= 0.

    A: LinearOperator; b: (m,) / (m,1); x0: (n,) / (n,1), entrywise >= 0 with at least one positive entry (ValueError otherwise), or
    None for the constant sum(b) / sum(A 1) (1 if that is not positive).  Returns (x, info) with info keys
        xHistory, its,
        relResidual   ||x_k - x_{k-1}|| / ||x_k|| as in CGLS here (the step is taken as alpha_k s, also where the clamp at 0 cut it),
        Rnrm          ||r_k|| / ||b||,
        stepLength    alpha_k,
        bounded       per step: alpha_k < theta_k = gamma_{k-1} / ||A s||^2 — the step was cut where an entry reaches zero,
        relError      ||x_k - x_true|| / ||x_true|| when x_true is given.  This differs from CGLS, which keeps the reference's quirk of
                      dividing by ||x_k||.
    Stopping: tol = 0 runs max_iter iterations in one enqueue and honours a breakdown (gamma_k <= 0 or ||A s||^2 <= 0: the iterate
    cannot move any more) after the fact, as CGLS does; tol > 0 stops when sqrt(gamma_k) <= tol sqrt(gamma_0); with delta= (and
    eta=1.01, the names of the hybrid solvers) it stops when ||r_k|| <= eta delta.
    Engine-only kwarg: history — as for CGLS (trips_py_amd._io.History).
    """
    max_iter = int(max_iter)
    if max_iter <= 0:
        raise ValueError("MRNSD needs max_iter >= 1")
    fmt = Formatter(b)
    A = as_operator(A)
    if A.engine.world > 1:
        raise NotImplementedError("MRNSD is not built for unknowns spread over ranks (eng.world > 1)")
    if x0 is not None:
        x0h = _host(x0).reshape(-1)
        if x0h.size != A.shape[1]:
            raise ValueError(f"x0 has {x0h.size} entries, expected {A.shape[1]}")
        if not np.all(np.isfinite(x0h)) or np.any(x0h < 0) or not np.any(x0h > 0):
            raise ValueError("MRNSD: x0 must be finite and >= 0 with at least one positive entry")
    delta = kwargs.get("delta", None)
    eta = float(kwargs.get("eta", 1.01))
    history = kwargs.get("history", True)
    run = MRNSDRun(A, b, x0, max_iter, x_true, history)
    sync_each = (tol != 0) or delta is not None
    if not sync_each:
        run.run(max_iter)                       # nothing is read back inside the loop -> one enqueue
    else:
        g0 = None
        while run.k < max_iter:
            run.step()
            h = run.row(run.k)
            if g0 is None:
                g0 = float(run.S.host(0, 1)[0])
            if h[0] <= 0.0 or h[2] <= 0.0:                                          # breakdown: nothing moves any more
                break
            if tol != 0 and np.sqrt(h[2]) <= tol * np.sqrt(g0):
                break
            if delta is not None and np.sqrt(h[7]) <= eta * float(delta):
                break
    s0, rows = run.rows()
    k, x_fin = run.k, run.x_cur
    if not sync_each:
        # iteration j broke down if it met ||u||^2 <= 0 or consumed gamma_{j-1} <= 0: it and every later one left the state as it was.
        # The last iteration that moved is j - 1 (at least one is reported).
        g_prev = np.concatenate(([s0[0]], rows[:-1, 2]))
        dead = np.nonzero((rows[:, 0] <= 0.0) | (g_prev <= 0.0))[0]
        if dead.size and max(1, int(dead[0])) < k:
            k = max(1, int(dead[0]))
            if run.hist.mode == "device":
                rows, x_fin = rows[:k], run.slot(k - 1)
            else:
                # the iterate is gone (no / streamed history): solve again for exactly k iterations (deterministic: the same iterates)
                return MRNSD(A, b, x0, k, tol, x_true, **kwargs)
    norm_x = np.sqrt(rows[:, 4])
    with np.errstate(divide="ignore", invalid="ignore"):
        theta = np.concatenate(([s0[0]], rows[:-1, 2])) / rows[:, 0]
        info = {"xHistory": run.hist.collect(fmt, k), "its": k,
                "relResidual": list(np.sqrt(rows[:, 5]) / norm_x),
                "Rnrm": list(np.sqrt(rows[:, 7]) / run.b_norm()),
                "stepLength": list(rows[:, 1]),
                "bounded": [bool(v) for v in rows[:, 1] < theta]}
    if run.xt is not None:
        nxt = float(np.linalg.norm(_host(run.xt).astype(np.float64)))
        info["relError"] = list(np.sqrt(rows[:, 6]) / nxt)
    return fmt.vec(x_fin), info
