"""MLEM / Richardson-Lucy (trips_py_amd/solvers/MLEM.py, csrc/mlem.hip) restated in NumPy, and the seeded Poisson problems its
tests share (tests/test_mlem_host.py, tests/test_gpu_mlem.py).

The restatement takes any (matvec, rmatvec) and comes in two forms: float64 throughout, and storage-faithful — fp32 vectors, an
operator's float64 product rounded to fp32 once, fp64 sums, the operations of the two kernels in the kernels' order (include/trk.h).
`ratio_f32`, `update_f32` and `sinv_f32` are ONE launch each on given vectors: the storage-faithful loop is built from them, the CPU
test engine calls them, and the GPU tests compare one launch with them."""
import numpy as np

import mrnsd_cases as MC

F32, F64 = np.float32, np.float64


def kl_terms(b, y):
    """kl(b_i, y_i) in float64 from the values given: (y - b) + b log(b / y) for b > 0, y > 0 (both finite); y for b == 0, y >= 0;
    +inf otherwise.  Never a NaN."""
    b, y = np.asarray(b).astype(F64), np.asarray(y).astype(F64)
    out = np.full(b.shape, np.inf)
    ok = (b > 0) & (y > 0) & np.isfinite(b) & np.isfinite(y)
    out[ok] = (y[ok] - b[ok]) + b[ok] * np.log(b[ok] / y[ok])
    z = (b == 0) & (y >= 0)
    out[z] = y[z]
    return out


def _bg32(bg, m):
    return np.broadcast_to(np.asarray(bg, dtype=F32), (m,))


def sinv_f32(s):
    """sinv = (s > 0) ? 1 / s : 0, one correctly rounded fp32 division."""
    s = np.asarray(s, dtype=F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, F32(1) / s, F32(0)).astype(F32)


def ratio_f32(w, bg, b):
    """One launch of the ratio kernel on fp32 vectors: y = w + bg (one fp32 add), rho = (y > 0) ? b / y : 0, and the two sums."""
    w, b = np.asarray(w, dtype=F32), np.asarray(b, dtype=F32)
    y = w + _bg32(bg, w.size)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.where(y > 0, b / y, F32(0)).astype(F32)
        kl = float(np.sum(kl_terms(b, y)))
        rr = float(np.sum((y.astype(F64) - b.astype(F64)) ** 2))
    return {"rho": rho, "kl": kl, "rr": rr}


def update_f32(x, t, sinv, x_true=None):
    """One launch of the update kernel: x' = max((x * t) * sinv, 0), two fp32 products in that order, d = x' - x in fp32."""
    x, t, sinv = (np.asarray(v, dtype=F32) for v in (x, t, sinv))
    with np.errstate(over="ignore", invalid="ignore"):
        xn = np.maximum((x * t) * sinv, F32(0)).astype(F32)
        d = (xn - x).astype(F64)
    xn64 = xn.astype(F64)
    return {"x": xn, "xx": float(np.dot(xn64, xn64)), "dd": float(np.dot(d, d)),
            "ee": 0.0 if x_true is None else float(np.sum((xn64 - np.asarray(x_true, dtype=F32).astype(F64)) ** 2)),
            "zeros": int(np.count_nonzero(xn == 0))}


def _new_out():
    return {"X": [], "kl": [], "rr": [], "zeros": [], "dd": [], "xx": []}


def mlem_f64(matvec, rmatvec, b, x0, iters, bg=0.0):
    """MLEM in float64 throughout.  Lists per iteration: X (the iterates x_k), kl and rr (KL(b, A x_{k-1} + bg) and
    ||A x_{k-1} + bg - b||^2: at the point iteration k applies A to), zeros, dd = ||x_k - x_{k-1}||^2, xx = ||x_k||^2."""
    b = np.asarray(b, dtype=F64).reshape(-1)
    x = np.asarray(x0, dtype=F64).reshape(-1).copy()
    bgv = np.broadcast_to(np.asarray(bg, dtype=F64), b.shape)
    s = rmatvec(np.ones(b.size))
    with np.errstate(divide="ignore"):
        sinv = np.where(s > 0, 1.0 / s, 0.0)
    out = _new_out()
    out["s"] = s
    for _ in range(iters):
        y = matvec(x) + bgv
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = np.where(y > 0, b / y, 0.0)
        xn = np.maximum(x * rmatvec(rho) * sinv, 0.0)
        out["kl"].append(float(np.sum(kl_terms(b, y))))
        out["rr"].append(float(np.sum((y - b) ** 2)))
        out["dd"].append(float(np.sum((xn - x) ** 2)))
        out["xx"].append(float(np.dot(xn, xn)))
        out["zeros"].append(int(np.count_nonzero(xn == 0)))
        out["X"].append(xn.copy())
        x = xn
    return out


def mlem_f32(matvec, rmatvec, b, x0, iters, bg=0.0, x_true=None):
    """The storage-faithful form: every vector is fp32 (an operator's float64 product is rounded to fp32 once), the sums float64,
    the updates by ratio_f32 and update_f32."""
    def mv(v):
        return matvec(v.astype(F64)).astype(F32)

    def rmv(v):
        return rmatvec(v.astype(F64)).astype(F32)
    b = np.asarray(b, dtype=F32).reshape(-1)
    x = np.asarray(x0, dtype=F32).reshape(-1).copy()
    bg = np.asarray(bg, dtype=F32)
    sinv = sinv_f32(rmv(np.ones(b.size, dtype=F32)))
    out = _new_out()
    out["ee"] = []
    for _ in range(iters):
        r = ratio_f32(mv(x), bg, b)
        u = update_f32(x, rmv(r["rho"]), sinv, x_true)
        for key, v in (("kl", r["kl"]), ("rr", r["rr"]), ("dd", u["dd"]), ("xx", u["xx"]), ("ee", u["ee"]), ("zeros", u["zeros"])):
            out[key].append(v)
        x = u["x"]
        out["X"].append(x.copy())
    return out


def worst_distance(a, b):
    """The worst relative 2-norm distance of the iterates of run `a` from those of run `b`."""
    return MC.worst_distance(a, b)


def worst_scalar(a, b):
    """max_k |a_k / b_k - 1| of two scalar histories."""
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    return float(np.max(np.abs(a / b - 1.0)))


# ------------------------------------------------------------------ the seeded problems
NAMES = MC.NAMES
EXACT_ADJOINT = MC.EXACT_ADJOINT
BACKGROUND = {"P1": 5.0, "P2": 0.0, "P3": 5.0, "P4": 0.0}
SCALE = 200.0


class Problem(MC.Problem):
    """mrnsd_cases.Problem's geometry (P1: 32^2 Gaussian blur, reflect; P2: 33 x 17 motion PSF, nearest; P3: Radon 24^2 x 12 angles;
    P4: sparse 150 x 120) with photon counts: x_true is 200 x that problem's truth, b = poisson(A x_true + bg) from a fixed seed,
    bg = 5 on P1 and P3 and 0 on P2 and P4, x0 the constant sum(b - bg) / sum(A 1)."""

    def __init__(self, name):
        super().__init__(name)
        o = self.oracle()
        self.bg = BACKGROUND[name]
        self.x_true = SCALE * self.x_true
        mean = np.maximum(o.matvec(self.x_true), 0.0) + self.bg
        self.b = np.random.default_rng({"P1": 31, "P2": 32, "P3": 33, "P4": 34}[name]).poisson(mean).astype(F64)
        c = (self.b - self.bg).sum() / o.matvec(np.ones(self.shape[1])).sum()
        self.x0 = np.full(self.shape[1], c if c > 0 else 1.0)


_problems = {}


def problem(name):
    if name not in _problems:
        _problems[name] = Problem(name)
    return _problems[name]
