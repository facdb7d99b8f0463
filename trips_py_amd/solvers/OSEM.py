"""OSEM on the HIP engine — ordered-subsets expectation maximisation (Hudson and Larkin 1994), the form of MLEM (solvers.MLEM) that
emission tomography runs in practice: the data are dealt into S row subsets (operators.RowSubsets: every S-th view of a projector,
every S-th row or given index sets of a sparse matrix) and a PASS applies MLEM's multiplicative update once per subset,
    x <- x . A_s^T(b_s / (A_s x + beta_s)) / (A_s^T 1),        s in the visiting order (bit-reversed by default),
so that one pass over the data moves x about as far as S MLEM iterations.  S = 1 is MLEM, bit for bit.  Per sub-step, all on the GPU:
    w = A_s x ; one kernel over the subset's data (trk_mlem_ratio on its slice): rho over w, KL and the residual of the subset
    t = A_s^T rho ; one kernel over the unknowns (trk_osem_update): x' = max(x t / s_s, 0), kept where the subset sees nothing
No device scalar steers the loop, so a whole solve is one enqueue (trk_osem_iterate).  THE KEEP RULE: an unknown the current subset
does not see ((A_s^T 1)_i = 0, common with one view per subset) keeps its value in that sub-step — MLEM's kernel would set it to 0 and
a multiplicative iteration never moves a 0 again.  An unknown NO subset sees therefore stays at x0 (MLEM sets it to 0).  OSEM does
not converge to the maximum-likelihood point for S > 1 (it enters a limit cycle near it); that is the method, not the arithmetic.
Not built: relaxation schedules (RAMLA, DRAMA), sharded OSEM, the ratio fused into the operator's epilogue, subsets of dynamic or
block-diagonal operators.  docs/kernels/ordered_subsets.md.
"""
import numpy as np

from .._io import Formatter, _host, as_operator
from ._run import SubsetRun
from .MLEM import poisson_data
from .MRNSD import default_x0


class OSEMRun(SubsetRun):
    """The OSEM iteration as an object, like MLEMRun: `step()` enqueues one PASS from Python, `run(n)` n of them in one library call
    (trk_osem_iterate: the same kernels, the same bits), `rows()` / `row(k)` download the sums (SubsetRun: slots 0 and 1 of a pass row
    are RUNNING sums, subset s contributing KL(b_s, A_s x + beta_s) and ||A_s x + beta_s - b_s||^2 at the sub-iterate it saw; slot 7
    counts the zeros of x_k).  b, background >= 0 and x0 > 0 (OSEM() checks them); b and a background vector are given in the
    operator's row order and held subset-major."""

    def __init__(self, A, b, x0, max_iter, x_true=None, history=True, background=0.0, subsets=1, order="bitrev"):
        super().__init__(A, b, max_iter, x_true, history, "OSEM xHistory", subsets, order)
        eng, sub = self.eng, self.sub
        m, n = sub.shape
        bg = _host(background).astype(np.float64)
        self.bg = float(bg.reshape(-1)[0]) if bg.size == 1 else eng.to_vec(sub.split(bg), m)       # a number, or a device vector
        self.x_cur = default_x0(sub if sub.A is None else sub.A, self.bv, bg) if x0 is None else eng.to_vec(x0, n)
        # SINV[s] = 1 / (A_s^T 1), 0 where subset s sees nothing of an unknown
        self.SINV = self.subset_sums(transpose=True)
        eng.mlem_sinv(self.SINV.reshape(-1), self.SINV.reshape(-1))

    def _bg(self, lo, hi):
        return self.bg if isinstance(self.bg, float) else self.bg[lo:hi]

    def _data(self, s, w, lo, hi, part):
        self.eng.mlem_ratio(self._bg(lo, hi), w, self.bv[lo:hi], w, part, self.cap)

    def _update(self, s, x_in, x_ref, x_true, x_out, part):
        self.eng.osem_update(x_in, self.t, self.SINV[s], x_ref, x_true, x_out, part, self.cap)

    def _c_loop(self):
        """One library call on the HIP engine (trk_osem_iterate)."""
        eng, args = self.eng, self._subset_args()
        if args is None or not hasattr(eng, "osem_iterate"):
            return None

        def call(k_first, n, X, keep):
            eng.osem_iterate(*args, k_first, n, self.bg, self.bv, self.SINV, self.w, self.t, self.xw, X, keep, self.x_cur, self.xt,
                             self.NP.ref(0), self.cap)
        return call

    def objective_at(self, x):
        """KL(b, A x + beta) over ALL the data at a device vector x, from one product per subset (the sums of the ratio kernel on
        scratch, added on the host in subset order; the state of the run is left alone)."""
        eng, sub, S = self.eng, self.sub, self.nS
        part, out = eng.scalars(8 * self.cap * S), eng.scalars(8 * S)
        for s, op in enumerate(sub.ops):
            lo, hi = int(sub.offsets[s]), int(sub.offsets[s + 1])
            w = op.apply(x)
            eng.mlem_ratio(self._bg(lo, hi), w, self.bv[lo:hi], w, part.ref(8 * self.cap * s), self.cap)
        eng.finalize_batched(part.ref(0), self.cap, 8, S, out.ref(0), 8)
        total = 0.0
        for v in out.host()[0::8]:
            total += float(v)
        return total


def OSEM(A, b, x0, max_iter, tol, x_true=None, subsets=1, background=0.0, order="bitrev", **kwargs):
    """OSEM: MLEM's multiplicative update applied subset by subset, `max_iter` PASSES over the data.

    A, b, background, x0: as for MLEM (b finite and >= 0, x0 finite and > 0 or None, ValueError otherwise).  subsets: the number S of
    row subsets (operators.RowSubsets(A, S, order): every S-th view of a Radon2DParallel / FanBeam2D, every S-th row of a SparseOp;
    other operators take S = 1 only) or a RowSubsets; order: "bitrev" (default), "sequential" or a permutation.  An unknown the
    current subset does not see keeps its value; one that no subset sees stays at x0.  Returns (x, info) with MLEM's keys plus
        subsets       S,
        KL, Rnrm      RUNNING values of pass k: the sums over the subsets of KL(b_s, A_s x + background_s) and (under the root, over
                      ||b||) ||A_s x + background_s - b_s||^2, each subset's term taken at the sub-iterate it saw — they cost no
                      product of their own and describe no single point,
        relResidual   ||x_k - x_{k-1}|| / ||x_k|| over the whole pass,
        zeros, relError   of x_k,
        objectiveFinal  KL over all the data at the returned x, from one product per subset after the loop.
    Stopping: tol = 0 runs max_iter passes in one enqueue; tol > 0 reads a row back every pass and stops at relResidual <= tol;
    with delta= (and eta=1.01) the solve stops after the first pass whose running residual is <= eta delta and returns that pass's
    iterate.  Engine-only kwarg: history — as for CGLS (trips_py_amd._io.History).
    """
    max_iter = int(max_iter)
    if max_iter <= 0:
        raise ValueError("OSEM needs max_iter >= 1")
    fmt = Formatter(b)
    A = as_operator(A)
    _bh, bg = poisson_data(b, background, A.shape[0], "OSEM")
    if x0 is not None:
        x0h = _host(x0).reshape(-1)
        if x0h.size != A.shape[1]:
            raise ValueError(f"x0 has {x0h.size} entries, expected {A.shape[1]}")
        if not np.all(np.isfinite(x0h)) or not np.all(x0h.astype(np.float32) > 0):
            raise ValueError("OSEM: x0 must be finite and > 0 everywhere (the iteration is multiplicative: a zero entry never moves)")
    delta = kwargs.get("delta", None)
    eta = float(kwargs.get("eta", 1.01))
    run = OSEMRun(A, b, x0, max_iter, x_true, kwargs.get("history", True), bg, subsets, order)
    if tol == 0 and delta is None:
        run.run(max_iter)                       # nothing is read back inside the loop -> one enqueue
    else:
        while run.k < max_iter:
            run.step()
            h = run.row(run.k)
            if delta is not None and np.sqrt(h[1]) <= eta * float(delta):
                break
            if tol != 0 and np.sqrt(h[5]) <= tol * np.sqrt(h[4]):
                break
    rows, k = run.rows(), run.k
    with np.errstate(divide="ignore", invalid="ignore"):
        info = {"xHistory": run.hist.collect(fmt, k), "its": k, "subsets": run.nS,
                "relResidual": list(np.sqrt(rows[:, 5]) / np.sqrt(rows[:, 4])),
                "KL": list(rows[:, 0]),
                "Rnrm": list(np.sqrt(rows[:, 1]) / run.b_norm()),
                "zeros": [int(c) for c in rows[:, 7]],
                "objectiveFinal": run.objective_at(run.x_cur)}
    if run.xt is not None:
        nxt = float(np.linalg.norm(_host(run.xt).astype(np.float64)))
        info["relError"] = list(np.sqrt(rows[:, 6]) / nxt)
    return fmt.vec(run.x_cur), info
