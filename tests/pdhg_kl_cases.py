"""PDHG with the Kullback-Leibler data term (solvers.PDHG(..., data='kl'), csrc/pdhg.hip: k_pdhg_dual_p_kl) restated in NumPy on top
of tests/pdhg_cases.py, tests/pdhg_iso_cases.py and tests/pdhg_iso3_cases.py, and the seeded Poisson problems its tests share
(tests/test_pdhg_kl_host.py, tests/test_gpu_pdhg_kl.py).

Only the dual update of p differs from the least-squares program: `prox_kl_f64` is its float64 form, `dual_p_kl_f32` ONE launch of the
kernel on fp32 vectors (include/trk.h: the operations and their order).  The loops take tv = 'aniso', 'iso' or 'iso3' and borrow the
dual of q, the projections and the primal update from the three case files."""
import numpy as np

import pdhg_cases as C
import pdhg_iso3_cases as T
import pdhg_iso_cases as I
from mlem_cases import kl_terms
from pdhg_cases import F32, F64, _sq, _start, fma32, primal_f32

TVS = ["aniso", "iso", "iso3"]


def prox_kl_f64(sigma, bg, z, b):
    """prox_{sigma F*}(z) for F(y) = KL(b, y + bg): with d = z + sigma bg - 1 and r = sqrt(d^2 + 4 sigma b),
    1 + (d - r) / 2 for d <= 0 and 1 - 2 sigma b / (d + r) for d > 0 — the same number, the form that does not cancel."""
    d = np.asarray(z, dtype=F64) + sigma * bg - 1.0
    r = np.sqrt(d * d + 4.0 * sigma * b)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d <= 0, 1.0 + 0.5 * (d - r), 1.0 - (2.0 * sigma * b) / (d + r))


def dual_p_kl_f32(sigma, bg, w, b, p):
    """y = w + bg ; z = fmaf(sf, y, p) ; d = z - 1 ; r = sqrtf(fmaf(d, d, c4 * b)) ; p' = (d <= 0) ? fmaf(0.5, d - r, 1) :
    1 - (c2 * b) / (d + r) with c2 = (float)(2 sigma), c4 = (float)(4 sigma).  Returns (p', KL(b, y), ||p' - p||^2)."""
    sf, c2, c4 = F32(sigma), F32(2.0 * F64(sigma)), F32(4.0 * F64(sigma))
    w, b, p = (np.asarray(v, dtype=F32) for v in (w, b, p))
    y = w + np.broadcast_to(np.asarray(bg, dtype=F32), w.shape)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z = fma32(sf, y, p)
        d = z - F32(1)
        r = np.sqrt(I.fma32_arrays(d, d, c4 * b))
        assert r.dtype == F32
        pn = np.where(d <= 0, I.fma32_arrays(np.full(d.shape, 0.5, dtype=F32), d - r, np.ones(d.shape, dtype=F32)),
                      F32(1) - (c2 * b) / (d + r)).astype(F32)
    return pn, float(np.sum(kl_terms(b, y))), _sq(pn.astype(F64) - p.astype(F64))


def _geo_of(tv, geo):
    assert tv in TVS and (tv == "aniso") == (geo is None)
    return geo


def project_f64(tv, geo, lam, t):
    if tv == "aniso":
        return np.clip(t, -lam, lam)
    return (I if tv == "iso" else T).project_f64(*geo, lam, t)


def norm_sum_f64(tv, geo, u):
    if tv == "aniso":
        return float(np.abs(u).sum())
    return float(I.group_norms(*geo, u).sum()) if tv == "iso" else T.norm_sum(*geo, u)


def dual_q_f32(tv, geo, sigma, lam, u, q):
    if tv == "aniso":
        return C.dual_q_f32(sigma, lam, u, q)
    return (I.dual_q_iso_f32 if tv == "iso" else T.dual_q_iso3_f32)(*geo, sigma, lam, u, q)


def pdhg_kl_f64(A, L, b, bg, lam, sigma, tau, lo, hi, x0, iters, tv="aniso", geo=None, x_true=None, stop_step=None):
    """PDHG for min KL(b, A x + bg) + lam R(L x) over the box in float64 throughout; pdhg_cases.pdhg_f64's dictionary, slot 0 of S the
    KL value at xbar."""
    (Amv, Armv), (Lmv, Lrmv) = A, L
    _geo_of(tv, geo)
    b = np.asarray(b, dtype=F64).reshape(-1)
    bgv = np.broadcast_to(np.asarray(bg, dtype=F64), b.shape)
    x = _start(x0, Armv(b).size, lo, hi, F64)
    xbar = x.copy()
    p, q = np.zeros(b.size), np.zeros(Lmv(x).size)
    X, S = [], []
    for _ in range(iters):
        w = Amv(xbar)
        pn = prox_kl_f64(sigma, bgv, p + sigma * w, b)
        u = Lmv(xbar)
        qn = project_f64(tv, geo, lam, q + sigma * u)
        xn = np.minimum(np.maximum(x - tau * (Armv(pn) + Lrmv(qn)), lo), hi)
        S.append([float(np.sum(kl_terms(b, w + bgv))), norm_sum_f64(tv, geo, u), _sq(pn - p), _sq(qn - q), _sq(xn), _sq(xn - x),
                  0.0 if x_true is None else _sq(xn - x_true), float(np.count_nonzero((xn == lo) | (xn == hi)))])
        xbar = 2.0 * xn - x
        x, p, q = xn, pn, qn
        X.append(x.copy())
        if stop_step is not None and S[-1][5] <= stop_step ** 2 * S[-1][4]:
            break
    return {"X": X, "S": np.array(S), "p": p, "q": q}


def pdhg_kl_f32(A, L, b, bg, lam, sigma, tau, lo, hi, x0, iters, tv="aniso", geo=None, x_true=None):
    """The storage-faithful form on the generic path: fp32 vectors (an operator's float64 product rounded to fp32 once), float64 sums,
    the updates by dual_p_kl_f32 and the three case files' one-kernel functions."""
    (Amv, Armv), (Lmv, Lrmv) = A, L
    _geo_of(tv, geo)

    def f(fn, v):
        return fn(v.astype(F64)).astype(F32)
    b = np.asarray(b, dtype=F32).reshape(-1)
    xt = None if x_true is None else np.asarray(x_true, dtype=F32).reshape(-1)
    x = _start(x0, Armv(b.astype(F64)).size, lo, hi, F32)
    xbar = x.copy()
    p, q = np.zeros(b.size, dtype=F32), np.zeros(Lmv(x.astype(F64)).size, dtype=F32)
    X, S = [], []
    for _ in range(iters):
        p, s0, s2 = dual_p_kl_f32(sigma, bg, f(Amv, xbar), b, p)
        q, s1, s3 = dual_q_f32(tv, geo, sigma, lam, f(Lmv, xbar), q)
        x, xbar, tail = primal_f32(tau, lo, hi, x, f(Armv, p), f(Lrmv, q), xt)
        S.append([s0, s1, s2, s3] + tail)
        X.append(x.copy())
    return {"X": X, "S": np.array(S), "p": p, "q": q}


def objective_kl(A, L, b, bg, lam, x, tv="aniso", geo=None):
    """KL(b, A x + bg) + lam R(L x) in float64 (no factor 1/2)."""
    x = np.asarray(x, dtype=F64).reshape(-1)
    b = np.asarray(b, dtype=F64).reshape(-1)
    return float(np.sum(kl_terms(b, A[0](x) + bg))) + lam * norm_sum_f64(tv, geo, L[0](x))


# ------------------------------------------------------------------ the seeded problems
# For every tv the smallest problem of its case file that has the fused kernels: pdhg_cases' Q1 (32^2 Gaussian blur, FirstDerivative2D)
# for 'aniso' and 'iso', pdhg_iso3_cases' Q5 (three 16^2 Radon frames, SpaceTimeDerivative) for 'iso3'.
PROBLEM_OF = {"aniso": "Q1", "iso": "Q1", "iso3": "Q5"}
GEOMETRY = {"aniso": None, "iso": I.GEOMETRY["Q1"], "iso3": T.GEOMETRY["Q5"]}
BACKGROUND = 5.0
SCALE = 200.0
LAM = 0.2


class KlProblem:
    """The operators, box and steps of a pdhg_cases problem with photon counts: x_true is 200 x that problem's truth,
    b = poisson(A x_true + 5) from a fixed seed, lam = 0.2, and the start the constant sum(b - bg) / sum(A 1) (A x0 + bg > 0)."""

    def __init__(self, name):
        self.base = P = C.problem(name)
        self.name, self.shape, self.lo, self.hi, self.sigma, self.tau = name, P.shape, P.lo, P.hi, P.sigma, P.tau
        o = P.oracle()
        self.bg, self.lam = BACKGROUND, LAM
        self.x_true = SCALE * P.x_true
        mean = np.maximum(o.matvec(self.x_true), 0.0) + self.bg
        self.b = np.random.default_rng(50 + C.NAMES.index(name)).poisson(mean).astype(F64)
        self.x0 = np.full(self.shape[1], (self.b - self.bg).sum() / o.matvec(np.ones(self.shape[1])).sum())

    def pairs(self):
        return C.pair(self.base.oracle()), C.pair(self.base.oracle_L())

    def f64(self, tv, iters, A=None, **kw):
        Ao, Lo = self.pairs()
        return pdhg_kl_f64(A or Ao, Lo, self.b, self.bg, self.lam, self.sigma, self.tau, self.lo, self.hi, self.x0, iters, tv,
                           GEOMETRY[tv], **kw)

    def f32(self, tv, iters, A=None, **kw):
        Ao, Lo = self.pairs()
        return pdhg_kl_f32(A or Ao, Lo, self.b, self.bg, self.lam, self.sigma, self.tau, self.lo, self.hi, self.x0, iters, tv,
                           GEOMETRY[tv], **kw)


_problems = {}


def problem(tv):
    name = PROBLEM_OF[tv]
    if name not in _problems:
        _problems[name] = KlProblem(name)
    return _problems[name]
