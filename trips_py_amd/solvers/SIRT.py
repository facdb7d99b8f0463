"""SIRT, OS-SIRT and SART on the HIP engine — the additive, least-squares twin of MLEM / OSEM and the default solver of the ASTRA
toolbox whose projectors the reference wraps:
    x <- P_box(x + omega C_s A_s^T R_s (b_s - A_s x)),     R_s = 1 / (A_s 1),  C_s = 1 / (A_s^T 1)
over the row subsets of operators.RowSubsets in their visiting order.  One subset is SIRT (Gilbert 1972; with these weights
||b - A x||_R never increases for 0 < omega < 2 and A >= 0), S subsets OS-SIRT, one view per subset SART (Andersen and Kak 1984).
The weights are each subset's OWN row and column sums, 0 where a sum is not positive (an unknown the subset does not see does not
move, a ray that meets no pixel gives nothing).  The method assumes A >= 0, as MLEM does.  weights=None is the plain projected
Landweber step x <- P_box(x + (relax / ||A||^2) A^T (b - A x)), one subset only.  Per sub-step, all on the GPU:
    w = A_s x ; one kernel over the subset's data (trk_sirt_residual): rho = (b_s - w) R_s over w, ||b_s - w||^2 plain and R-weighted
    t = A_s^T rho ; one kernel over the unknowns (trk_sirt_update): x' = clip(fma(omega, t C_s, x), lower, upper) and the norms
No device scalar steers the loop, so a whole solve is one enqueue (trk_sirt_iterate).  Vectors fp32, sums fp64 (include/trk.h).
Not built: relaxation schedules, Cimmino and DROP weights, sharded runs, fused epilogues, subsets of dynamic or block-diagonal
operators.  docs/kernels/ordered_subsets.md.
"""
import numpy as np

from .._io import Formatter, _host, as_operator
from ._run import SubsetRun


class SIRTRun(SubsetRun):
    """The SIRT iteration as an object, like OSEMRun: `step()` one PASS from Python, `run(n)` n of them in one library call
    (trk_sirt_iterate: the same kernels, the same bits).  Pass row k (SubsetRun): slot 0 the running ||b - A x||^2, slot 1 the running
    R-weighted one (both sums over the subsets, each term at the sub-iterate the subset saw; with S = 1 they describe x_{k-1}),
    slots 4..6 as MLEM's, slot 7 the entries of x_k on a finite bound.  x0 = None: zeros clipped into the box."""

    def __init__(self, A, b, x0, max_iter, x_true=None, history=True, subsets=1, order="bitrev", relax=1.0, lower=-np.inf, upper=np.inf,
                 weights="sirt", normA2=None):
        super().__init__(A, b, max_iter, x_true, history, "SIRT xHistory", subsets, order)
        eng, sub = self.eng, self.sub
        self.lo, self.hi = float(lower), float(upper)
        start = np.zeros(sub.shape[1]) if x0 is None else _host(x0).astype(np.float64).reshape(-1)
        self.x_cur = eng.to_vec(np.clip(start, self.lo, self.hi), sub.shape[1])
        if weights == "sirt":
            self.omega = float(relax)
            self.RINV, self.CINV = self.subset_sums(transpose=False), self.subset_sums(transpose=True)
            eng.mlem_sinv(self.RINV, self.RINV)
            eng.mlem_sinv(self.CINV.reshape(-1), self.CINV.reshape(-1))
        else:
            from ..operators import operator_norm_sq
            self.omega = float(relax) / float(operator_norm_sq(sub.ops[0]) if normA2 is None else normA2)
            self.RINV = self.CINV = None

    def _data(self, s, w, lo, hi, part):
        self.eng.sirt_residual(None if self.RINV is None else self.RINV[lo:hi], w, self.bv[lo:hi], w, part, self.cap)

    def _update(self, s, x_in, x_ref, x_true, x_out, part):
        self.eng.sirt_update(self.omega, self.lo, self.hi, x_in, self.t, None if self.CINV is None else self.CINV[s], x_ref, x_true,
                             x_out, part, self.cap)

    def _c_loop(self):
        """One library call on the HIP engine (trk_sirt_iterate)."""
        eng, args = self.eng, self._subset_args()
        if args is None or not hasattr(eng, "sirt_iterate"):
            return None

        def call(k_first, n, X, keep):
            eng.sirt_iterate(*args, k_first, n, self.bv, self.RINV, self.CINV, self.omega, self.lo, self.hi, self.w, self.t, self.xw, X,
                             keep, self.x_cur, self.xt, self.NP.ref(0), self.cap)
        return call


def SIRT(A, b, x0, max_iter, tol, x_true=None, subsets=1, relax=1.0, lower=-np.inf, upper=np.inf, weights="sirt", order="bitrev",
         **kwargs):
    """SIRT / OS-SIRT: min ||A x - b|| over lower <= x <= upper by x <- P_box(x + relax C_s A_s^T R_s (b_s - A_s x)), `max_iter`
    PASSES over the subsets.

    A: LinearOperator with entries >= 0 (a projector, a blur, a sparse system matrix); b: (m,) / (m,1); x0: (n,) / (n,1) or None
    (zeros), clipped into the box; subsets, order: as for OSEM (an int S or an operators.RowSubsets); lower <= upper, -inf / +inf
    allowed.  weights="sirt": R_s, C_s the reciprocal row and column sums of each subset, relax in (0, 2) (ValueError otherwise).
    weights=None: projected Landweber with the step relax / normA2, normA2= an estimate of ||A||^2 (default:
    operators.operator_norm_sq(A)); one subset only (ValueError for more).  Returns (x, info) with info keys
        xHistory, its, subsets,
        relResidual       ||x_k - x_{k-1}|| / ||x_k|| over the whole pass,
        Rnrm              the running ||b - A x|| / ||b|| of pass k and
        weightedResidual  the running ||b - A x||_R^2 = sum_i R_i (b - A x)_i^2 (weights=None: the plain sum of squares) — sums over
                          the subsets, each term at the sub-iterate the subset saw; with one subset both describe x_{k-1},
        atBound           the number of entries of x_k on a finite bound,
        relError          ||x_k - x_true|| / ||x_true|| when x_true is given.
    Stopping: tol = 0 runs max_iter passes in one enqueue; tol > 0 reads a row back every pass and stops at relResidual <= tol; with
    delta= (and eta=1.01) the solve stops after the first pass whose running residual is <= eta delta and returns that pass's
    iterate.  Engine-only kwargs: history — as for CGLS; normA2.
    """
    max_iter = int(max_iter)
    if max_iter <= 0:
        raise ValueError("SIRT needs max_iter >= 1")
    fmt = Formatter(b)
    A = as_operator(A)
    bh = _host(b).astype(np.float64).reshape(-1)
    if bh.size != A.shape[0]:
        raise ValueError(f"b has {bh.size} entries, expected {A.shape[0]}")
    if not np.all(np.isfinite(bh)):
        raise ValueError("SIRT: b must be finite")
    if x0 is not None and (_host(x0).size != A.shape[1] or not np.all(np.isfinite(_host(x0)))):
        raise ValueError(f"SIRT: x0 must be finite with {A.shape[1]} entries")
    if not float(lower) <= float(upper):
        raise ValueError("SIRT: need lower <= upper")
    if weights not in ("sirt", None):
        raise ValueError(f"SIRT: weights is 'sirt' or None, got {weights!r}")
    relax = float(relax)
    if not 0.0 < relax < 2.0:
        raise ValueError(f"SIRT: relax must lie in (0, 2), got {relax}")
    n_sub = len(subsets.ops) if hasattr(subsets, "ops") else int(subsets)
    if weights is None and n_sub > 1:
        raise ValueError("SIRT: weights=None (Landweber) has one step length for the whole operator: subsets=1 only")
    delta = kwargs.get("delta", None)
    eta = float(kwargs.get("eta", 1.01))
    run = SIRTRun(A, b, x0, max_iter, x_true, kwargs.get("history", True), subsets, order, relax, lower, upper, weights,
                  kwargs.get("normA2", None))
    if tol == 0 and delta is None:
        run.run(max_iter)                       # nothing is read back inside the loop -> one enqueue
    else:
        while run.k < max_iter:
            run.step()
            h = run.row(run.k)
            if delta is not None and np.sqrt(h[0]) <= eta * float(delta):
                break
            if tol != 0 and np.sqrt(h[5]) <= tol * np.sqrt(h[4]):
                break
    rows, k = run.rows(), run.k
    with np.errstate(divide="ignore", invalid="ignore"):
        info = {"xHistory": run.hist.collect(fmt, k), "its": k, "subsets": run.nS,
                "relResidual": list(np.sqrt(rows[:, 5]) / np.sqrt(rows[:, 4])),
                "Rnrm": list(np.sqrt(rows[:, 0]) / run.b_norm()),
                "weightedResidual": list(rows[:, 1]),
                "atBound": [int(c) for c in rows[:, 7]]}
    if run.xt is not None:
        nxt = float(np.linalg.norm(_host(run.xt).astype(np.float64)))
        info["relError"] = list(np.sqrt(rows[:, 6]) / nxt)
    return fmt.vec(run.x_cur), info


def SART(A, b, x0, max_iter, tol, x_true=None, **kwargs):
    """SART: SIRT with one view per subset (subsets = the number of views of a Radon2DParallel or FanBeam2D); every other argument
    as SIRT's.  ValueError for operators without views."""
    A = as_operator(A)
    if not hasattr(A, "angles"):
        raise ValueError(f"SART: a {type(A).__name__} has no views (built for Radon2DParallel and FanBeam2D); use SIRT with subsets=")
    if "subsets" in kwargs:
        raise ValueError("SART: the subsets are the views; use SIRT for another choice")
    return SIRT(A, b, x0, max_iter, tol, x_true=x_true, subsets=len(A.angles), **kwargs)
