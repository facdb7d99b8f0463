"""PDHG on the HIP engine: min_x 1/2 ||A x - b||^2 + lam ||L x||_1 subject to lower <= x <= upper — the exact l1 / anisotropic TV term
and a box in one solve, by the primal-dual hybrid gradient iteration (Chambolle and Pock 2011, algorithm 1, theta = 1; CIL's PDHG).
With tv='iso' the term is lam sum_g ||(L x)_g||_2, isotropic TV (Rudin, Osher and Fatemi): the horizontal and the vertical difference
of a pixel form one group, every other row of L a group of its own (include/trk.h: the groups of a geometry (N, frames)).
With tv='iso3' it is isotropic in space and time, lam sum over voxels of sqrt(h^2 + v^2 + t^2) on the rows of a space-time first
difference operator: the group of voxel (t, i, j) holds whichever of H_t[i][j], V_t[i][j] and T_t[i][j] exist (CIL's TotalVariation
on a 2-D + time volume); 'iso' on such an operator is spatially isotropic and temporally l1.

With K = [A; L], duals p and q (zero at the start), x_0 the caller's start projected onto the box and xbar_0 = x_0, per iteration:
    w = A xbar ; p = (p + sigma (w - b)) / (1 + sigma)                      (trk_pdhg_dual_p)
    u = L xbar ; q = clip(q + sigma u, -lam, lam)                           (trk_pdhg_dual_q, or trk_pdhg_tv_dual: u in registers)
                 tv='iso': q = each group of q + sigma u projected onto the 2-norm ball of radius lam
                                                                            (trk_pdhg_dual_q_iso, or trk_pdhg_tv_dual_iso)
                 tv='iso3': the same with the groups (h, v, t)              (trk_pdhg_dual_q_iso3, or trk_pdhg_st_dual_iso3)
    z = A^T p ; v = L^T q ; x = clip(x - tau (z + v), lower, upper) ; xbar = 2 x - x_previous
                                                                            (trk_pdhg_primal, or trk_pdhg_tv_primal: v gathered;
                                                                             tv='iso3' on SpaceTimeDerivative: trk_pdhg_st_primal)
sigma, tau and lam are host constants, so nothing is read back inside the loop: a whole solve is one enqueue (trk_pdhg_iterate).
Vectors are fp32, the reported sums fp64 (include/trk.h: the operations and the layout of S).  It converges for
sigma tau ||K||^2 < 1.
Not built: the fused space-time kernels for tv='aniso' / 'iso' (SpaceTimeDerivative runs those two on the generic path), time-sharded
space-time handles and sharded PDHG, rectangular images and frames, fused forms for Framelet2D, cache hints on the fused kernels'
loads and stores, diagonal preconditioning or adaptive step balancing (`ratio` is the only knob), data terms other than the two below.

With data='kl' the data term is the Kullback-Leibler fit of Poisson counts, min_x KL(b, A x + background) + lam R(L x) over the box,
KL(b, y) = sum_i y_i - b_i + b_i log(b_i / y_i) (solvers.MLEM minimises it without a regulariser).  Only the dual update of p changes:
    p = 1/2 (1 + z - sqrt((z - 1)^2 + 4 sigma b)),  z = p + sigma (w + background)         (trk_pdhg_dual_p_kl)
the prox of sigma F* for F(y) = KL(b, y + background), F*(p) = sum -b log(1 - p) - background p; every fused TV path comes with it.
"""
import numpy as np

from .._io import Formatter, _host, as_operator
from ..operators import operator_norm_sq
from ._run import IterationRun
from .MLEM import poisson_data

_GROUPS = {"aniso": 0, "iso": 1, "iso3": 2}        # trk_pdhg_iterate_data's spelling of the grouping


def _iso_geometry(L, tv, tv_dims):
    """None for tv='aniso'; for 'iso' and 'iso3' (N, frames) of the groups on L's rows: the operator's own, or the caller's tv_dims,
    checked against L.shape ('iso': a tail of further rows may follow the frames' blocks; 'iso3': the space-time rows exactly)."""
    from ..operators import FirstDerivative2D, SpaceTimeDerivative
    if tv not in ("aniso", "iso", "iso3"):
        raise ValueError(f"PDHG: tv must be 'aniso', 'iso' or 'iso3', not {tv!r}")
    if tv == "aniso":
        if tv_dims is not None:
            raise ValueError("PDHG: tv_dims belongs to tv='iso' and tv='iso3'")
        return None
    if tv_dims is not None:
        try:
            N, frames = (int(d) for d in tv_dims)
        except (TypeError, ValueError):
            raise ValueError("PDHG: tv_dims must be (N, frames)") from None
    elif isinstance(L, FirstDerivative2D):
        N, frames = L.N, 1
    elif isinstance(L, SpaceTimeDerivative):
        N, frames = L.N, L.nt_global
    else:
        raise ValueError(f"PDHG: tv={tv!r} needs tv_dims=(N, frames) for a {type(L).__name__} regulariser: only FirstDerivative2D and "
                         "SpaceTimeDerivative carry the geometry of their rows")
    if N < 2 or frames < 1:
        raise ValueError("PDHG: tv_dims needs N >= 2 and frames >= 1")
    rows, cols = L.shape
    if tv == "iso3":
        if rows != frames * 2 * N * (N - 1) + (frames - 1) * N * N or cols != frames * N * N:
            raise ValueError(f"PDHG: L is {rows} x {cols}, not the space-time first differences of {frames} images of {N} x {N} "
                             "(tv='iso3' takes no further rows)")
        return N, frames
    if rows < frames * 2 * N * (N - 1) or cols != frames * N * N:
        raise ValueError(f"PDHG: L is {rows} x {cols}, not the first differences of {frames} images of {N} x {N} (and a tail of further rows)")
    return N, frames


class PDHGRun(IterationRun):
    """The PDHG iteration as an object, like MRNSDRun: `step()` enqueues one iteration from Python, `run(n)` n of them in one library
    call when A and L both have handles (trk_pdhg_iterate: the same kernels, the same bits), `rows()` / `row(k)` download the sums.

    Row k (1-based) at S + 8k = [||A xbar - b||^2, sum |L xbar|, ||p_k - p_{k-1}||^2, ||q_k - q_{k-1}||^2, ||x_k||^2,
    ||x_k - x_{k-1}||^2, ||x_k - x_true||^2, entries of x_k on a bound], the first two at xbar_{k-1} = 2 x_{k-1} - x_{k-2}: the point
    iteration k applies A and L to.  `fused`: None = the fused first-difference kernels where L takes them, True / False forces.
    tv='iso': the isotropic term — sum |L xbar| becomes the sum of the groups' 2-norms; the geometry (N, frames) is
    FirstDerivative2D's (N, 1), SpaceTimeDerivative's (N, nt) or, for any other operator with that row layout, `tv_dims`.
    tv='iso3': the groups (h, v, t) of a voxel on the space-time row layout; fused=None takes the fused space-time kernels where L is
    a SpaceTimeDerivative with every frame on this rank whose own geometry it is, every other L the unfused dual behind L.apply.
    data='kl': the Kullback-Leibler data term with `background` (a number or an m-vector; b and background >= 0, which PDHG()
    checks) — slot 0 of a row becomes KL(b, A xbar + background), inf where that point leaves the domain of the likelihood."""

    def __init__(self, A, b, L, lam, sigma, tau, lower, upper, x0, max_iter, x_true=None, history=True, fused=None, tv="aniso",
                 tv_dims=None, data="l2", background=0.0):
        A = as_operator(A)
        if data not in ("l2", "kl"):
            raise ValueError(f"PDHG: data must be 'l2' or 'kl', not {data!r}")
        self.data = data
        self.L = L = as_operator(L, "L")
        if A.engine.world > 1:
            raise NotImplementedError("PDHG is not built for unknowns spread over ranks (eng.world > 1)")
        m, n = A.shape
        rows = L.shape[0]
        if L.shape[1] != n:
            raise ValueError(f"L has {L.shape[1]} columns, A has {n}")
        self.lam, self.sigma, self.tau = float(lam), float(sigma), float(tau)
        self.lo, self.hi = float(lower), float(upper)
        if not (np.isfinite(self.lam) and self.lam >= 0):
            raise ValueError("PDHG: lam must be finite and >= 0")
        if not (np.isfinite(self.sigma) and np.isfinite(self.tau) and self.sigma > 0 and self.tau > 0):
            raise ValueError("PDHG: sigma and tau must be finite and > 0")
        if not self.lo <= self.hi:
            raise ValueError("PDHG: need lower <= upper")
        self.tv = tv
        self.geo = _iso_geometry(L, tv, tv_dims)
        super().__init__(A, b, max_iter, x_true, history, "PDHG xHistory")
        eng, max_iter = self.eng, self.max_iter
        self.bg = None
        if data == "kl":
            bg = _host(background).astype(np.float64)
            self.bg = float(bg.reshape(-1)[0]) if bg.size == 1 else eng.to_vec(bg, m)       # a number, or a device vector
        if tv == "iso3":                                           # the fused space-time pair groups the rows as its handle lays them out
            from ..operators import SpaceTimeDerivative
            can = bool(isinstance(L, SpaceTimeDerivative) and hasattr(L, "_h") and hasattr(eng, "pdhg_st_dual_iso3")
                       and not L.sharded and self.geo == (L.N, L.nt_global))
            if fused and not can:
                raise ValueError("PDHG: fused=True with tv='iso3' needs a SpaceTimeDerivative regulariser of that geometry, every frame "
                                 "on one rank, on the HIP engine")
        else:
            can = bool(hasattr(L, "_h") and hasattr(eng, "pdhg_fused_caps") and eng.pdhg_fused_caps(L._h))
            if self.geo is not None:                               # the fused isotropic dual pairs the rows as its handle lays them out
                can = can and self.geo == (L.N, 1)
            if fused and not can:
                raise ValueError("PDHG: fused=True needs a FirstDerivative2D regulariser on the HIP engine")
        self.fused = can if fused is None else bool(fused)
        # the start, projected onto the box in fp32 (the bounds as the kernels round them)
        x0h = np.zeros(n, dtype=np.float32) if x0 is None else _host(x0).astype(np.float32).reshape(-1)
        if x0h.size != n:
            raise ValueError(f"x0 has {x0h.size} entries, expected {n}")
        self.x_cur = eng.to_vec(np.clip(x0h, np.float32(self.lo), np.float32(self.hi)))
        self.xbar = self.x_cur.clone()
        self.p, self.w = eng.zeros(m), eng.empty(m)
        self.q, self.z = eng.zeros(rows), eng.empty(n)
        self.u, self.v = (None, None) if self.fused else (eng.empty(rows), eng.empty(n))
        if self.geo is None:
            self.cap = eng.pdhg_blocks(m, n, rows, L._h if self.fused else None)
        elif tv == "iso3":
            self.cap = eng.pdhg_blocks_iso3(m, n, rows, *self.geo, L._h if self.fused else None)
        else:
            self.cap = eng.pdhg_blocks_iso(m, n, rows, *self.geo, L._h if self.fused else None)
        self.NP = eng.scalars(8 * self.cap * max(1, max_iter))     # zeroed: a kernel writes only its slots of its blocks' rows
        self.S = eng.scalars(8 * (max_iter + 1))
        self.B = eng.scalars(1)                                    # ||b||^2
        eng.nrm2sq(self.bv, self.B.ref(0))
        self._final = 0

    def _step(self):
        eng, A, L = self.eng, self.A, self.L
        self.k += 1
        k = self.k
        part = self.NP.ref(8 * self.cap * (k - 1))
        x_new = self.hist.row(k - 1)
        A.apply(self.xbar, out=self.w)
        self._dual_p(self.w, self.p, part)
        if self.fused:
            dual = {"aniso": eng.pdhg_tv_dual, "iso": eng.pdhg_tv_dual_iso, "iso3": eng.pdhg_st_dual_iso3}[self.tv]
            dual(L._h, self.sigma, self.lam, self.xbar, self.q, part, self.cap)
        else:
            L.apply(self.xbar, out=self.u)
            self._dual_q(self.u, self.q, part)
        A.apply(self.p, out=self.z, transpose=True)
        if self.fused:
            primal = eng.pdhg_st_primal if self.tv == "iso3" else eng.pdhg_tv_primal
            primal(L._h, self.tau, self.lo, self.hi, self.x_cur, self.z, self.q, x_new, self.xbar, self.xt, part, self.cap)
        else:
            L.apply(self.q, out=self.v, transpose=True)
            eng.pdhg_primal(self.tau, self.lo, self.hi, self.x_cur, self.z, self.v, x_new, self.xbar, self.xt, part, self.cap)
        self.x_cur = x_new

    def _dual_p(self, w, p, part):
        if self.data == "kl":
            self.eng.pdhg_dual_p_kl(self.sigma, self.bg, w, self.bv, p, part, self.cap)
        else:
            self.eng.pdhg_dual_p(self.sigma, w, self.bv, p, part, self.cap)

    def _dual_q(self, u, q, part):
        if self.geo is None:
            self.eng.pdhg_dual_q(self.sigma, self.lam, u, q, part, self.cap)
        elif self.tv == "iso3":
            self.eng.pdhg_dual_q_iso3(*self.geo, self.sigma, self.lam, u, q, part, self.cap)
        else:
            self.eng.pdhg_dual_q_iso(*self.geo, self.sigma, self.lam, u, q, part, self.cap)

    def _c_loop(self):
        """One library call where A and L both have handles (trk_pdhg_iterate, trk_pdhg_iterate_iso, trk_pdhg_iterate_iso3; data='kl':
        trk_pdhg_iterate_data)."""
        eng = self.eng
        loop = "pdhg_iterate_data" if self.data == "kl" else \
            {"aniso": "pdhg_iterate", "iso": "pdhg_iterate_iso", "iso3": "pdhg_iterate_iso3"}[self.tv]
        if not (hasattr(self.A, "_h") and hasattr(self.L, "_h") and hasattr(eng, loop)):
            return None

        def call(k_first, n, X, keep):
            rest = (k_first, n, self.sigma, self.tau, self.lam, self.lo, self.hi, self.fused, self.bv, self.p, self.q, self.w, self.u,
                    self.z, self.v, X, keep, self.x_cur, self.xbar, self.xt, self.NP.ref(0), self.cap)
            if self.data == "kl":
                eng.pdhg_iterate_data(self.A._h, self.L._h, _GROUPS[self.tv], *(self.geo or (0, 0)), 1, self.bg, *rest)
            elif self.geo is None:
                eng.pdhg_iterate(self.A._h, self.L._h, *rest)
            else:
                getattr(eng, loop)(self.A._h, self.L._h, *self.geo, *rest)
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
        """1/2 ||A x - b||^2 + lam ||L x||_1 (tv='iso', 'iso3': lam sum_g ||(L x)_g||_2; data='kl': KL(b, A x + background) in place of
        the least-squares term, no factor 1/2) at a device vector x, from one pair of products (the sums of the dual kernels on
        scratch duals; the state of the run is left alone)."""
        eng = self.eng
        w, u = self.A.apply(x), self.L.apply(x)
        part, out = eng.scalars(8 * self.cap), eng.scalars(8)
        self._dual_p(w, eng.zeros(w.numel()), part.ref(0))
        self._dual_q(u, eng.zeros(u.numel()), part.ref(0))
        eng.finalize_batched(part.ref(0), self.cap, 8, 1, out.ref(0), 8)
        s = out.host()
        return (1.0 if self.data == "kl" else 0.5) * float(s[0]) + self.lam * float(s[1])


def pdhg_steps(normK2, ratio=1.0):
    """(sigma, tau) with sigma tau normK2 = 0.95^2 and sigma / tau = ratio."""
    tau = 0.95 / np.sqrt(float(normK2) * float(ratio))
    return float(ratio) * tau, tau


def PDHG(A, b, L, lam, max_iter, tol=0, x0=None, x_true=None, lower=0.0, upper=np.inf, sigma=None, tau=None, normK2=None, ratio=1.0,
         tv="aniso", tv_dims=None, data="l2", background=0.0, **kwargs):
    """Primal-dual hybrid gradient: min 1/2 ||A x - b||^2 + lam ||L x||_1 subject to lower <= x <= upper.

    A, L: LinearOperators with the same column count (L = Identity: plain l1; FirstDerivative2D: anisotropic TV, on fused kernels);
    tv: 'aniso' (the l1 norm of L x), 'iso' — lam sum over pixels of sqrt(h^2 + v^2), isotropic TV: the rows H[i][j] and V[i][j] of
        the first differences of an image form one group, the last row's H, the last column's V and every further row (the temporal
        rows of SpaceTimeDerivative: spatially isotropic, temporally l1) a group of their own.  The geometry is FirstDerivative2D's
        (fused kernels) and SpaceTimeDerivative's own; tv_dims=(N, frames) gives it for any other operator whose rows are `frames`
        blocks [H ; V] of N x N images and then a tail, such as SparseOp(first_derivative_2d(N, N)).  ValueError where it is missing
        or disagrees with L.shape.  The objectives below then carry the group norms, and info['tv'] = 'iso';
        'iso3' — lam sum over voxels of sqrt(h^2 + v^2 + t^2), isotropic in space and time: L's rows must be exactly those of
        SpaceTimeDerivative(N, frames) (its own geometry, on fused kernels; tv_dims for SparseOp(spacetime_derivative(N, N, frames));
        FirstDerivative2D is (N, 1): 'iso' bit for bit).  The groups are triples, the pairs and singles of the volume's three far
        faces, and info['tv'] = 'iso3';
    data: 'l2' (the least-squares term above) or 'kl' — min KL(b, A x + background) + lam R(L x) over the box, the fit of Poisson
        counts b (finite and >= 0: ValueError otherwise; clipping Gaussian-noisy data is left to the caller) over a known background
        (a number or an m-vector, finite and >= 0).  Then `objective` and `objectiveFinal` are KL + lam R with no factor 1/2,
        info['KL'] = KL(b, A xbar_{k-1} + background) replaces info['Rnrm'] (inf where A xbar + background <= 0 under a count: xbar
        is not confined to the box; the iteration itself is unaffected), info['data'] = 'kl', and delta= is refused (ValueError: the
        discrepancy rule is a least-squares notion).  A start with A x0 + background > 0 is advisable (x0 = None is the zero vector);
    b: (m,) / (m,1); x0: (n,) / (n,1) or None (zeros), projected onto the box; lower / upper: scalars, -inf / +inf allowed.
    Steps: sigma and tau as given; if not both are, sigma tau normK2 = 0.95^2 and sigma / tau = ratio, with normK2 the caller's number
    or else operator_norm_sq([A, L], iters=30, seed=0) — an estimate from below, for which the 0.95 leaves room down to 0.9025 of the
    true ||K||^2.  Returns (x, info) with info keys
        xHistory, its,
        relResidual   ||x_k - x_{k-1}|| / ||x_k||,
        Rnrm          ||A xbar_{k-1} - b|| / ||b||   and
        objective     1/2 ||A xbar_{k-1} - b||^2 + lam ||L xbar_{k-1}||_1 — both AT THE EXTRAPOLATED POINT xbar_{k-1} = 2 x_{k-1} - x_{k-2}
                      iteration k applies A and L to (they cost no product of their own), not at x_k,
        dualChange    sqrt(||p_k - p_{k-1}||^2 + ||q_k - q_{k-1}||^2),
        active        the number of entries of x_k on a bound,
        relError      ||x_k - x_true|| / ||x_true|| when x_true is given (as MRNSD),
        sigma, tau, normK2 (None when both steps were given without it),
        objectiveFinal  the objective at the returned x, from one extra pair of products after the loop.
    Stopping: tol = 0 runs max_iter iterations in one enqueue; tol > 0 reads a row back every iteration and stops at
    relResidual <= tol; with delta= (and eta=1.01) it stops when ||A xbar - b|| <= eta delta.
    Engine-only kwargs: history — as for CGLS (trips_py_amd._io.History); fused — None / True / False (PDHGRun); delta, eta.
    """
    max_iter = int(max_iter)
    if max_iter <= 0:
        raise ValueError("PDHG needs max_iter >= 1")
    fmt = Formatter(b)
    A, L = as_operator(A), as_operator(L, "L")
    if A.engine.world > 1:
        raise NotImplementedError("PDHG is not built for unknowns spread over ranks (eng.world > 1)")
    if L.shape[1] != A.shape[1]:
        raise ValueError(f"L has {L.shape[1]} columns, A has {A.shape[1]}")
    _iso_geometry(L, tv, tv_dims)                # refused before the norm estimate is paid for
    if data not in ("l2", "kl"):
        raise ValueError(f"PDHG: data must be 'l2' or 'kl', not {data!r}")
    if data == "kl":
        _bh, background = poisson_data(b, background, A.shape[0], "PDHG(data='kl')")
        if kwargs.get("delta", None) is not None:
            raise ValueError("PDHG(data='kl'): delta= is refused — the discrepancy rule is a least-squares notion")
    lam = float(lam)
    if not (np.isfinite(lam) and lam >= 0):
        raise ValueError("PDHG: lam must be finite and >= 0")
    if not float(lower) <= float(upper):
        raise ValueError("PDHG: need lower <= upper")
    for name, val in (("sigma", sigma), ("tau", tau), ("normK2", normK2), ("ratio", ratio)):
        if val is not None and not (np.isfinite(val) and val > 0):
            raise ValueError(f"PDHG: {name} must be finite and > 0")
    if sigma is None or tau is None:
        if normK2 is None:
            normK2 = operator_norm_sq([A, L], iters=30, seed=0)
            if not (np.isfinite(normK2) and normK2 > 0):
                raise ValueError("PDHG: the estimate of ||K||^2 is not positive: A and L are both zero?")
        sigma, tau = pdhg_steps(normK2, ratio)
    delta = kwargs.get("delta", None)
    eta = float(kwargs.get("eta", 1.01))
    run = PDHGRun(A, b, L, lam, sigma, tau, lower, upper, x0, max_iter, x_true, kwargs.get("history", True), kwargs.get("fused", None),
                  tv, tv_dims, data, background)
    if tol == 0 and delta is None:
        run.run(max_iter)                       # nothing is read back inside the loop -> one enqueue
    else:
        while run.k < max_iter:
            run.step()
            h = run.row(run.k)
            if tol != 0 and np.sqrt(h[5]) <= tol * np.sqrt(h[4]):
                break
            if delta is not None and np.sqrt(h[0]) <= eta * float(delta):
                break
    rows = run.rows()
    k, x_fin = run.k, run.x_cur
    with np.errstate(divide="ignore", invalid="ignore"):
        fit = {"KL": list(rows[:, 0]), "data": "kl"} if data == "kl" else {"Rnrm": list(np.sqrt(rows[:, 0]) / run.b_norm())}
        info = {"xHistory": run.hist.collect(fmt, k), "its": k,
                "relResidual": list(np.sqrt(rows[:, 5]) / np.sqrt(rows[:, 4])),
                **fit,
                "objective": list((1.0 if data == "kl" else 0.5) * rows[:, 0] + lam * rows[:, 1]),
                "dualChange": list(np.sqrt(rows[:, 2] + rows[:, 3])),
                "active": [int(c) for c in rows[:, 7]],
                "sigma": float(sigma), "tau": float(tau), "normK2": None if normK2 is None else float(normK2),
                "objectiveFinal": run.objective_at(x_fin)}
    if run.geo is not None:
        info["tv"] = run.tv
    if run.xt is not None:
        nxt = float(np.linalg.norm(_host(run.xt).astype(np.float64)))
        info["relError"] = list(np.sqrt(rows[:, 6]) / nxt)
    return fmt.vec(x_fin), info
