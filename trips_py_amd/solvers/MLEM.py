"""MLEM on the HIP engine — Richardson-Lucy to the deblurring community, MLEM to tomographers: maximise the Poisson likelihood of
b ~ Poisson(A x + beta) over x >= 0, beta >= 0 a known background, called like `MRNSD(A, b, x0, max_iter, tol)` on the same operators.
That is min KL(b, A x + beta) with KL(b, y) = sum_i y_i - b_i + b_i log(b_i / y_i), by the multiplicative iteration
    x_k = x_{k-1} . A^T(b / (A x_{k-1} + beta)) / (A^T 1).
A^T is the operator's own transpose throughout, also behind s = A^T 1: for the blur modes whose flipped-PSF transpose is not the
adjoint the method is defined with that transpose, as MRNSD's is.  Per iteration, all on the GPU:
    w = A x ; one kernel over the data (trk_mlem_ratio): rho = b / (w + beta) written over w, KL(b, w + beta), ||w + beta - b||^2
    t = A^T rho ; one kernel over the unknowns (trk_mlem_update): x = max(x t / s, 0) and the reported norms
No device scalar steers the loop, so a whole solve is one enqueue (trk_mlem_iterate).  Vectors are fp32, the reported sums fp64
(include/trk.h: the operations and the layout of S).  An unknown no datum sees (s_i = 0: a masked detector) is set to 0 by the first
iteration and stays there; where A x + beta <= 0 under a positive count the ratio is taken as 0 and KL reports inf.
Ordered subsets: solvers.OSEM.  Not built: sharded MLEM, the ratio fused into the operator's epilogue, acceleration or line search, KL for MMGKS
(solvers.PDHG takes data='kl' for a regularised fit).
"""
import numpy as np

from .._io import Formatter, _host, as_operator
from ._run import IterationRun
from .MRNSD import default_x0


def poisson_data(b, background, m, who):
    """(b, background) on the host as float64, checked: b an m-vector, finite and >= 0; background a number or an m-vector, finite and
    >= 0 (returned as a float or as an m-vector)."""
    bh = _host(b).astype(np.float64).reshape(-1)
    if bh.size != m:
        raise ValueError(f"b has {bh.size} entries, expected {m}")
    if not np.all(np.isfinite(bh)) or np.any(bh < 0):
        raise ValueError(f"{who}: b must be finite and >= 0 — Poisson counts cannot be negative (clip data that carries Gaussian noise, "
                         "e.g. np.maximum(b, 0), before it gets here)")
    bg = _host(background).astype(np.float64)
    if bg.size != 1:
        bg = bg.reshape(-1)
        if bg.size != m:
            raise ValueError(f"{who}: background has {bg.size} entries, expected 1 or {m}")
    if not np.all(np.isfinite(bg)) or np.any(bg < 0):
        raise ValueError(f"{who}: background must be finite and >= 0")
    return bh, (float(bg.reshape(-1)[0]) if bg.size == 1 else bg)


class MLEMRun(IterationRun):
    """The MLEM iteration as an object, like MRNSDRun: `step()` enqueues one iteration from Python, `run(n)` n of them in one library
    call (trk_mlem_iterate: the same kernels, the same bits), `rows()` / `row(k)` download the sums.

    Row k (1-based) at S + 8k = [KL(b, A x_{k-1} + beta), ||A x_{k-1} + beta - b||^2, 0, 0, ||x_k||^2, ||x_k - x_{k-1}||^2,
    ||x_k - x_true||^2, entries of x_k equal to 0]: the first two at x_{k-1}, the point iteration k applies A to.
    b and background must be >= 0 and x0 > 0 (MLEM() checks them); x0 = None: the constant sum(b - beta) / sum(A 1), 1 if that is not
    positive."""

    def __init__(self, A, b, x0, max_iter, x_true=None, history=True, background=0.0):
        A = as_operator(A)
        if A.engine.world > 1:
            raise NotImplementedError("MLEM is not built for unknowns spread over ranks (eng.world > 1)")
        super().__init__(A, b, max_iter, x_true, history, "MLEM xHistory")
        eng, max_iter = self.eng, self.max_iter
        m, n = A.shape
        bg = _host(background).astype(np.float64)
        self.bg = float(bg.reshape(-1)[0]) if bg.size == 1 else eng.to_vec(bg, m)       # a number, or a device vector
        self.x_cur = default_x0(A, self.bv, bg) if x0 is None else eng.to_vec(x0, n)
        self.w, self.t = eng.empty(m), eng.empty(n)
        # sinv = 1 / (A^T 1), 0 where an unknown is seen by no datum; s never visits the host
        self.sinv = eng.empty(n)
        A.apply(eng.to_vec(np.ones(m, dtype=np.float32)), out=self.sinv, transpose=True)
        eng.mlem_sinv(self.sinv, self.sinv)
        self.cap = eng.mlem_blocks(m, n)
        self.NP = eng.scalars(8 * self.cap * max(1, max_iter))     # zeroed: a kernel writes only its slots of its blocks' rows
        self.S = eng.scalars(8 * (max_iter + 1))
        self.B = eng.scalars(1)                                    # ||b||^2
        eng.nrm2sq(self.bv, self.B.ref(0))
        self._final = 0

    def _step(self):
        eng, A = self.eng, self.A
        self.k += 1
        k = self.k
        part = self.NP.ref(8 * self.cap * (k - 1))
        x_new = self.hist.row(k - 1)
        A.apply(self.x_cur, out=self.w)
        eng.mlem_ratio(self.bg, self.w, self.bv, self.w, part, self.cap)          # rho over w
        A.apply(self.w, out=self.t, transpose=True)
        eng.mlem_update(self.x_cur, self.t, self.sinv, self.xt, x_new, part, self.cap)
        self.x_cur = x_new

    def _c_loop(self):
        """One library call on the HIP engine (trk_mlem_iterate)."""
        eng = self.eng
        if not (hasattr(self.A, "_h") and hasattr(eng, "mlem_iterate")):
            return None

        def call(k_first, n, X, keep):
            eng.mlem_iterate(self.A._h, k_first, n, self.bg, self.bv, self.sinv, self.w, self.t, X, keep, self.x_cur, self.xt,
                             self.NP.ref(0), self.cap)
        return call

    def _finish(self):
        """The block partials of the iterations not summed yet into their rows of S."""
        if self._final == self.k:
            return
        f = self._final
        self.eng.finalize_batched(self.NP.ref(8 * self.cap * f), self.cap, 8, self.k - f, self.S.ref(8 * (f + 1)), 8)
        self._final = self.k

    def row(self, k):
        """Row k of S (host sync)."""
        self._finish()
        return self.S.host(8 * k, 8 * k + 8)

    def rows(self):
        """The k rows on the host."""
        self._finish()
        return self.S.host()[8:8 * (self.k + 1)].reshape(self.k, 8)

    def b_norm(self):
        return float(np.sqrt(self.B.host(0, 1)[0]))

    def objective_at(self, x):
        """KL(b, A x + beta) at a device vector x, from one product (the sum of the ratio kernel on scratch; the state of the run is
        left alone)."""
        eng = self.eng
        w = self.A.apply(x)
        part, out = eng.scalars(8 * self.cap), eng.scalars(8)
        eng.mlem_ratio(self.bg, w, self.bv, w, part.ref(0), self.cap)
        eng.finalize_batched(part.ref(0), self.cap, 8, 1, out.ref(0), 8)
        return float(out.host()[0])


def MLEM(A, b, x0, max_iter, tol, x_true=None, background=0.0, **kwargs):
    """MLEM / Richardson-Lucy: min KL(b, A x + background) over x >= 0, the maximum-likelihood fit of Poisson counts b.

    A: LinearOperator; b: (m,) / (m,1), finite and >= 0 (ValueError otherwise: counts cannot be negative, and clipping data that carries
    Gaussian noise is left to the caller); background: a number or an m-vector, finite and >= 0; x0: (n,) / (n,1), finite and > 0
    everywhere (ValueError otherwise: a zero entry never moves), or None for the constant sum(b - background) / sum(A 1) (1 if that
    is not positive).  An unknown with (A^T 1)_i = 0 becomes 0.  Returns (x, info) with info keys
        xHistory, its,
        relResidual   ||x_k - x_{k-1}|| / ||x_k||,
        KL            KL(b, A x_{k-1} + background)   and
        Rnrm          ||A x_{k-1} + background - b|| / ||b|| — both AT x_{k-1}, the point iteration k applies A to (they cost no
                      product of their own; PDHG's convention for `objective`); inf where A x + background <= 0 under a count,
        zeros         the number of entries of x_k equal to 0,
        relError      ||x_k - x_true|| / ||x_true|| when x_true is given (as MRNSD),
        objectiveFinal  KL at the returned x, from one extra product after the loop.
    Stopping: tol = 0 runs max_iter iterations in one enqueue; tol > 0 reads a row back every iteration and stops at
    relResidual <= tol; with delta= (and eta=1.01, the names of the hybrid solvers) the discrepancy rule is read from row k, which
    describes x_{k-1}: when ||A x_{k-1} + background - b|| <= eta delta at k >= 2 the solve returns x_{k-1} with its = k - 1.
    Engine-only kwarg: history — as for CGLS (trips_py_amd._io.History).
    """
    max_iter = int(max_iter)
    if max_iter <= 0:
        raise ValueError("MLEM needs max_iter >= 1")
    fmt = Formatter(b)
    A = as_operator(A)
    if A.engine.world > 1:
        raise NotImplementedError("MLEM is not built for unknowns spread over ranks (eng.world > 1)")
    _bh, bg = poisson_data(b, background, A.shape[0], "MLEM")
    if x0 is not None:
        x0h = _host(x0).reshape(-1)
        if x0h.size != A.shape[1]:
            raise ValueError(f"x0 has {x0h.size} entries, expected {A.shape[1]}")
        if not np.all(np.isfinite(x0h)) or not np.all(x0h.astype(np.float32) > 0):
            raise ValueError("MLEM: x0 must be finite and > 0 everywhere (the iteration is multiplicative: a zero entry never moves)")
    delta = kwargs.get("delta", None)
    eta = float(kwargs.get("eta", 1.01))
    run = MLEMRun(A, b, x0, max_iter, x_true, kwargs.get("history", True), bg)
    k_ret = None
    if tol == 0 and delta is None:
        run.run(max_iter)                       # nothing is read back inside the loop -> one enqueue
    else:
        while run.k < max_iter:
            run.step()
            h = run.row(run.k)
            if delta is not None and run.k >= 2 and np.sqrt(h[1]) <= eta * float(delta):
                k_ret = run.k - 1               # the row describes x_{k-1}: that iterate is the one returned
                break
            if tol != 0 and np.sqrt(h[5]) <= tol * np.sqrt(h[4]):
                break
    rows = run.rows()
    k, x_fin = run.k, run.x_cur
    if k_ret is not None:
        k, rows, x_fin = k_ret, rows[:k_ret], run.slot(k_ret - 1)       # still in its slot: iteration k_ret + 1 wrote the next one
    with np.errstate(divide="ignore", invalid="ignore"):
        info = {"xHistory": run.hist.collect(fmt, k), "its": k,
                "relResidual": list(np.sqrt(rows[:, 5]) / np.sqrt(rows[:, 4])),
                "KL": list(rows[:, 0]),
                "Rnrm": list(np.sqrt(rows[:, 1]) / run.b_norm()),
                "zeros": [int(c) for c in rows[:, 7]],
                "objectiveFinal": run.objective_at(x_fin)}
    if run.xt is not None:
        nxt = float(np.linalg.norm(_host(run.xt).astype(np.float64)))
        info["relError"] = list(np.sqrt(rows[:, 6]) / nxt)
    return fmt.vec(x_fin), info


RichardsonLucy = MLEM
