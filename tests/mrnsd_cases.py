"""MRNSD (trips_py_amd/solvers/MRNSD.py, csrc/mrnsd.hip) restated in NumPy, and the seeded problems its tests share
(tests/test_mrnsd_host.py, tests/test_gpu_mrnsd.py).

The restatement takes any (matvec, rmatvec) and comes in two forms: float64 throughout, and storage-faithful — fp32 vectors, fp64
scalars, the operations of the update kernel in the kernel's order (include/trk.h).  `update_f32` is ONE such update on given
vectors: the storage-faithful loop is built from it, the CPU test engine calls it, and the GPU tests compare one launch with it."""
import numpy as np

F32, F64 = np.float32, np.float64


def bound_of(x, s):
    """min over {i : s_i < 0} of x_i / -s_i in float64, +inf when no s_i is negative."""
    neg = s < 0
    if not np.any(neg):
        return np.inf
    return float(np.min(x[neg].astype(F64) / -s[neg].astype(F64)))


def alpha_of(gamma, bound, uu):
    """(theta, alpha): alpha = min(theta, bound), 0 if ||u||^2 <= 0 or gamma <= 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        theta = F64(gamma) / F64(uu)
    if uu <= 0 or gamma <= 0:
        return float(theta), 0.0
    return float(theta), float(min(theta, bound))


def fma32(a, x, y):
    """fmaf(a, x, y) on fp32 operands, correctly rounded: the product is exact in float64; the float64 sum is made round-to-odd
    (its rounding error from TwoSum: where the sum is inexact and its last bit is even, the neighbour on the error's side is taken),
    after which the rounding to fp32 is the rounding of the exact value — no double rounding."""
    p = F64(a) * np.asarray(x, dtype=F32).astype(F64)
    y = np.asarray(y, dtype=F32).astype(F64)
    s = p + y
    bb = s - p
    err = (p - (s - bb)) + (y - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def update_f32(gamma, bound, uu, x, g, s, z, r, u, x_true=None):
    """One update of the kernel on fp32 vectors with float64 scalars; returns a dict of the new state, scalars and sums."""
    theta, alpha = alpha_of(gamma, bound, uu)
    step = F32(alpha)
    xn = np.maximum(fma32(step, s, x), F32(0))
    gn = fma32(step, z, g)
    sn = -(xn * gn)                                   # one fp32 product
    rn = fma32(-step, u, r)
    d = step * s                                      # fp32
    xn64, gn64, sn64 = xn.astype(F64), gn.astype(F64), sn.astype(F64)
    return {"theta": theta, "alpha": alpha, "x": xn, "g": gn, "s": sn, "r": rn,
            "gamma": float(-np.dot(gn64, sn64)), "bound": bound_of(xn, sn),
            "xx": float(np.dot(xn64, xn64)), "dd": float(np.dot(d.astype(F64), d.astype(F64))),
            "ee": 0.0 if x_true is None else float(np.sum((xn64 - x_true.astype(F64)) ** 2)),
            "rr": float(np.dot(rn.astype(F64), rn.astype(F64)))}


def _record(out, x, theta, alpha, gamma, bound, uu, rr):
    out["X"].append(x.copy())
    for key, v in (("theta", theta), ("alpha", alpha), ("gamma", gamma), ("bound", bound), ("uu", uu), ("rr", rr)):
        out[key].append(v)


def _new_out(gamma, bound, rr):
    return {"X": [], "theta": [], "alpha": [], "gamma": [], "bound": [], "uu": [], "rr": [], "gamma0": gamma, "bound0": bound,
            "rr0": rr}


def mrnsd_f64(matvec, rmatvec, b, x0, iters, force_theta=False):
    """MRNSD in float64 throughout.  Returns lists per iteration (X: the iterates; gamma, bound: what the iteration leaves; bounded
    step k: alpha[k] < theta[k]).  force_theta: alpha = theta whatever the bound (and no clamp) — plain steepest descent in the
    x-scaled metric, for the test that says what the method is."""
    x = np.asarray(x0, dtype=F64).reshape(-1).copy()
    r = np.asarray(b, dtype=F64).reshape(-1) - matvec(x)
    g = -rmatvec(r)
    s = -(x * g)
    gamma, bound = float(-np.dot(g, s)), bound_of(x, s)
    out = _new_out(gamma, bound, float(np.dot(r, r)))
    for _ in range(iters):
        u = matvec(s)
        z = rmatvec(u)
        uu = float(np.dot(u, u))
        theta, alpha = alpha_of(gamma, bound, uu)
        if force_theta:
            alpha = theta
            x = x + alpha * s
        else:
            x = np.maximum(x + alpha * s, 0.0)
        g = g + alpha * z
        s = -(x * g)
        r = r - alpha * u
        gamma, bound = float(-np.dot(g, s)), bound_of(x, s)
        _record(out, x, theta, alpha, gamma, bound, uu, float(np.dot(r, r)))
    return out


def mrnsd_f32(matvec, rmatvec, b, x0, iters, x_true=None):
    """The storage-faithful form: every vector is fp32 (an operator's float64 product is rounded to fp32 once, ||u||^2 is the
    float64 sum over the rounded u), scalars float64, the update by update_f32."""
    def mv(v):
        return matvec(v.astype(F64)).astype(F32)

    def rmv(v):
        return rmatvec(v.astype(F64)).astype(F32)
    x = np.asarray(x0, dtype=F32).reshape(-1).copy()
    r = np.asarray(b, dtype=F32).reshape(-1) - mv(x)
    g = -rmv(r)
    s = -(x * g)
    gamma, bound = float(-np.dot(g.astype(F64), s.astype(F64))), bound_of(x, s)
    out = _new_out(gamma, bound, float(np.dot(r.astype(F64), r.astype(F64))))
    xt = None if x_true is None else np.asarray(x_true, dtype=F32).reshape(-1)
    for _ in range(iters):
        u = mv(s)
        z = rmv(u)
        uu = float(np.dot(u.astype(F64), u.astype(F64)))
        st = update_f32(gamma, bound, uu, x, g, s, z, r, u, xt)
        x, g, s, r, gamma, bound = st["x"], st["g"], st["s"], st["r"], st["gamma"], st["bound"]
        _record(out, x, st["theta"], st["alpha"], gamma, bound, uu, st["rr"])
    return out


def worst_distance(a, b):
    """The worst relative 2-norm distance of the iterates of run `a` from those of run `b`."""
    return max(float(np.linalg.norm(xa.astype(F64) - xb) / np.linalg.norm(xb)) for xa, xb in zip(a["X"], b["X"]))


# ------------------------------------------------------------------ the seeded problems
NAMES = ["P1", "P2", "P3", "P4"]
EXACT_ADJOINT = ["P1", "P3", "P4"]          # P2's flipped-PSF "transpose" under 'nearest' is not the adjoint


def _truth(nx, ny, seed):
    """A few positive points plus a plateau on a zero background."""
    rng = np.random.default_rng(seed)
    img = np.zeros((nx, ny))
    img[nx // 4: nx // 4 + max(2, nx // 4), ny // 3: ny // 3 + max(2, ny // 4)] = 1.0
    for _ in range(5):
        img[rng.integers(1, nx - 1), rng.integers(1, ny - 1)] += 2.0 + 2.0 * rng.random()
    return img.reshape(-1)


def _sparse_matrix():
    import scipy.sparse as sp
    rng = np.random.default_rng(404)
    M = sp.random(150, 120, density=0.08, random_state=rng, data_rvs=lambda k: rng.random(k)).tocsr()
    return (M + sp.eye(150, 120, format="csr")).tocsr()


class Problem:
    """name, shape (m, n), x_true, b (1 % noise), x0 (the constant start) as float64 arrays; `oracle()` = the float64 operator of
    the oracle (oracle/cpu_ref.py's protocol: matvec, rmatvec, _fwd, _adj); `device(engine)` = the engine's operator."""

    def __init__(self, name):
        self.name = name
        o = self.oracle()
        self.shape = o.shape
        if name == "P1":
            self.x_true = _truth(32, 32, 11)
        elif name == "P2":
            self.x_true = _truth(33, 17, 12)
        elif name == "P3":
            self.x_true = _truth(24, 24, 13)
        else:
            rng = np.random.default_rng(14)
            self.x_true = np.where(rng.random(120) < 0.3, 1.0 + rng.random(120), 0.0)
            self.x_true[40:60] = 1.0
        rng = np.random.default_rng({"P1": 21, "P2": 22, "P3": 23, "P4": 24}[name])
        bt = o.matvec(self.x_true)
        e = rng.standard_normal(bt.size)
        self.b = bt + 0.01 * np.linalg.norm(bt) / np.linalg.norm(e) * e
        c = self.b.sum() / o.matvec(np.ones(self.shape[1])).sum()
        self.x0 = np.full(self.shape[1], c if c > 0 else 1.0)

    def psf(self):
        from oracle import cpu_ref as O
        from trips_py_amd.problems import motion_psf
        return O.gauss_psf((9, 9), 1.5)[0] if self.name == "P1" else motion_psf((7, 7), 5.0, 30.0)[0]

    def oracle(self):
        from blur_psf_cases import scipy_operator
        from oracle import cpu_ref as O
        if self.name == "P1":
            return scipy_operator(self.psf(), 32, 32, "reflect")
        if self.name == "P2":
            return scipy_operator(self.psf(), 33, 17, "nearest")
        if self.name == "P3":
            return O.Radon2D(24, np.linspace(0, np.pi, 12, endpoint=False))
        return O.MatrixOp(_sparse_matrix())

    def device(self, engine=None):
        from trips_py_amd.operators import Blur2D, Radon2DParallel, SparseOp
        if self.name == "P1":
            return Blur2D(self.psf(), 32, 32, engine=engine, boundary="reflect")
        if self.name == "P2":
            return Blur2D(self.psf(), 33, 17, engine=engine, boundary="nearest")
        if self.name == "P3":
            return Radon2DParallel(24, np.linspace(0, np.pi, 12, endpoint=False), engine=engine)
        return SparseOp(_sparse_matrix(), engine=engine)


_problems = {}


def problem(name):
    if name not in _problems:
        _problems[name] = Problem(name)
    return _problems[name]
