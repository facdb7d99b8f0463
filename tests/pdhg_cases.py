"""PDHG (trips_py_amd/solvers/PDHG.py, csrc/pdhg.hip, the fused forms in csrc/pdhg_tv.hip) restated in NumPy, and the seeded problems
its tests share (tests/test_pdhg_host.py, tests/test_gpu_pdhg.py).

The restatement takes any (matvec, rmatvec) pair for A and for L and comes in two forms: float64 throughout (`pdhg_f64`), and
storage-faithful (`pdhg_f32`) — fp32 vectors, float64 sums, the operations of the kernels in the kernels' order (include/trk.h).  The
storage-faithful loop is built from one-kernel functions (`dual_p_f32`, `dual_q_f32`, `tv_dual_f32`, `primal_f32`, `tv_primal_f32`): the
CPU test engine calls them and the GPU tests compare one launch with each."""
import numpy as np

from mrnsd_cases import _sparse_matrix, _truth, fma32

F32, F64 = np.float32, np.float64


def _sq(a):
    a = np.asarray(a, dtype=F64)
    return float(np.dot(a, a))


# ------------------------------------------------------------------ one kernel each, storage-faithful
def dual_p_f32(sigma, w, b, p):
    """p' = fmaf(sf, w - b, p) * cf ; returns (p', ||w - b||^2, ||p' - p||^2)."""
    sf, cf = F32(sigma), F32(1.0 / (1.0 + F64(sigma)))
    e = w - b
    pn = fma32(sf, e, p) * cf
    return pn, _sq(e), _sq(pn.astype(F64) - p.astype(F64))


def dual_q_f32(sigma, lam, u, q):
    """q' = min(max(fmaf(sf, u, q), -lf), lf) ; returns (q', sum |u|, ||q' - q||^2)."""
    sf, lf = F32(sigma), F32(lam)
    qn = np.minimum(np.maximum(fma32(sf, u, q), -lf), lf)
    return qn, float(np.sum(np.abs(u.astype(F64)))), _sq(qn.astype(F64) - q.astype(F64))


def primal_f32(tau, lo, hi, x, z, v, x_true=None):
    """g = z + v (v None: g = z) ; x' = min(max(fmaf(-tf, g, x), lof), hif) ; xbar' = fmaf(2, x', -x) ; d = x' - x.
    Returns (x', xbar', [||x'||^2, ||d||^2, ||x' - x_true||^2, entries on a bound])."""
    tf, lof, hif = F32(tau), F32(lo), F32(hi)
    g = z if v is None else z + v
    xn = np.minimum(np.maximum(fma32(-tf, g, x), lof), hif)
    xb = fma32(F32(2), xn, -x)
    d = xn - x
    ee = 0.0 if x_true is None else _sq(xn.astype(F64) - x_true.astype(F64))
    return xn, xb, [_sq(xn), _sq(d), ee, float(np.count_nonzero((xn == lof) | (xn == hif)))]


def d2_fwd_f32(N, x):
    """The 2-D first differences of an N x N image in fp32, in the rows' order: x[i][j] - x[i][j+1], then x[i][j] - x[i+1][j]."""
    X = x.reshape(N, N)
    return np.concatenate(((X[:, :-1] - X[:, 1:]).reshape(-1), (X[:-1, :] - X[1:, :]).reshape(-1)))


def d2_adj_f32(N, q):
    """The gather of the operator's transpose in fp32, per pixel in this order: 0, + H[i][j], - H[i][j-1], + V[i][j], - V[i-1][j],
    absent terms skipped."""
    H, V = q[:N * (N - 1)].reshape(N, N - 1), q[N * (N - 1):].reshape(N - 1, N)
    acc = np.zeros((N, N), dtype=F32)
    acc[:, :-1] = acc[:, :-1] + H
    acc[:, 1:] = acc[:, 1:] - H
    acc[:-1, :] = acc[:-1, :] + V
    acc[1:, :] = acc[1:, :] - V
    return acc.reshape(-1)


def tv_dual_f32(N, sigma, lam, xbar, q):
    return dual_q_f32(sigma, lam, d2_fwd_f32(N, xbar), q)


def tv_primal_f32(N, tau, lo, hi, x, z, q, x_true=None):
    return primal_f32(tau, lo, hi, x, z, d2_adj_f32(N, q), x_true)


# ------------------------------------------------------------------ the loops
def _start(x0, n, lo, hi, dtype):
    x = np.zeros(n, dtype=dtype) if x0 is None else np.asarray(x0, dtype=dtype).reshape(-1).copy()
    return np.minimum(np.maximum(x, dtype(lo)), dtype(hi))


def pdhg_f64(A, L, b, lam, sigma, tau, lo, hi, x0, iters, x_true=None, stop_step=None):
    """PDHG in float64 throughout.  A, L: (matvec, rmatvec) pairs.  Returns X (the iterates), S (iters x 8, the rows of the scalar
    block), and the last p, q.  stop_step: stop once ||x' - x|| <= stop_step ||x'||."""
    (Amv, Armv), (Lmv, Lrmv) = A, L
    b = np.asarray(b, dtype=F64).reshape(-1)
    x = _start(x0, Armv(b).size, lo, hi, F64)
    xbar = x.copy()
    p, q = np.zeros(b.size), np.zeros(Lmv(x).size)
    X, S = [], []
    for _ in range(iters):
        e = Amv(xbar) - b
        pn = (p + sigma * e) / (1.0 + sigma)
        u = Lmv(xbar)
        qn = np.clip(q + sigma * u, -lam, lam)
        xn = np.minimum(np.maximum(x - tau * (Armv(pn) + Lrmv(qn)), lo), hi)
        S.append([_sq(e), float(np.abs(u).sum()), _sq(pn - p), _sq(qn - q), _sq(xn), _sq(xn - x),
                  0.0 if x_true is None else _sq(xn - x_true), float(np.count_nonzero((xn == lo) | (xn == hi)))])
        xbar = 2.0 * xn - x
        x, p, q = xn, pn, qn
        X.append(x.copy())
        if stop_step is not None and S[-1][5] <= stop_step ** 2 * S[-1][4]:
            break
    return {"X": X, "S": np.array(S), "p": p, "q": q}


def pdhg_f32(A, L, b, lam, sigma, tau, lo, hi, x0, iters, x_true=None, tv_N=None):
    """The storage-faithful form: every vector is fp32 (an operator's float64 product is rounded to fp32 once), the sums float64,
    the updates by the one-kernel functions above.  tv_N: L is the 2-D first-difference operator of an N x N image and the fused
    forms are taken (the same bits: differences of fp32 numbers in fp32 are what rounding the float64 product gives)."""
    (Amv, Armv), (Lmv, Lrmv) = A, L

    def f(fn, v):
        return fn(v.astype(F64)).astype(F32)
    b = np.asarray(b, dtype=F32).reshape(-1)
    xt = None if x_true is None else np.asarray(x_true, dtype=F32).reshape(-1)
    x = _start(x0, Armv(b.astype(F64)).size, lo, hi, F32)
    xbar = x.copy()
    p, q = np.zeros(b.size, dtype=F32), np.zeros(Lmv(x.astype(F64)).size, dtype=F32)
    X, S = [], []
    for _ in range(iters):
        p, s0, s2 = dual_p_f32(sigma, f(Amv, xbar), b, p)
        if tv_N:
            q, s1, s3 = tv_dual_f32(tv_N, sigma, lam, xbar, q)
            x, xbar, tail = tv_primal_f32(tv_N, tau, lo, hi, x, f(Armv, p), q, xt)
        else:
            q, s1, s3 = dual_q_f32(sigma, lam, f(Lmv, xbar), q)
            x, xbar, tail = primal_f32(tau, lo, hi, x, f(Armv, p), f(Lrmv, q), xt)
        S.append([s0, s1, s2, s3] + tail)
        X.append(x.copy())
    return {"X": X, "S": np.array(S), "p": p, "q": q}


def objective(A, L, b, lam, x):
    """1/2 ||A x - b||^2 + lam ||L x||_1 in float64."""
    x = np.asarray(x, dtype=F64).reshape(-1)
    return 0.5 * _sq(A[0](x) - np.asarray(b, dtype=F64).reshape(-1)) + lam * float(np.abs(L[0](x)).sum())


def operator_norm_sq(ops, n, iters=30, seed=0):
    """trips_py_amd.operators.operator_norm_sq restated in float64: power iteration on sum O^T O from the seeded normal start rounded
    to fp32; the last Rayleigh quotient sum ||O v||^2 / ||v||^2."""
    y = np.random.default_rng(seed).standard_normal(n).astype(F32).astype(F64)
    rq = 0.0
    for _ in range(iters):
        v = y / np.linalg.norm(y)
        outs = [mv(v) for mv, _ in ops]
        rq = sum(_sq(o) for o in outs) / _sq(v)
        y = sum(rmv(o) for (_, rmv), o in zip(ops, outs))
    return float(rq)


def worst_distance(a, b):
    """The worst relative 2-norm distance of the iterates of run `a` from those of run `b`."""
    return max(float(np.linalg.norm(xa.astype(F64) - xb) / np.linalg.norm(xb)) for xa, xb in zip(a["X"], b["X"]))


def pair(o):
    return (o.matvec, o.rmatvec)


# ------------------------------------------------------------------ the seeded problems
NAMES = ["Q1", "Q2", "Q3", "Q4", "Q5"]
FUSED = ["Q1", "Q2"]                        # L = FirstDerivative2D: the fused kernels
EXACT_ADJOINT = ["Q1", "Q3", "Q4", "Q5"]    # Q2's flipped-PSF "transpose" under 'nearest' is not the adjoint
_BOX = {"Q1": (0.0, np.inf), "Q2": (0.0, 3.0), "Q3": (0.0, np.inf), "Q4": (-np.inf, np.inf), "Q5": (0.0, np.inf)}
_Q5_ANGLES = [np.linspace(0, np.pi, 8, endpoint=False) + 0.1 * t for t in range(3)]


class Problem:
    """name, shape (m, n), x_true, b (1 % noise), the box (lo, hi), lam = 0.01 ||A||^2 (from the dense matrix), normK2 (the dense
    ||[A; L]||^2), est (operator_norm_sq restated, 30 steps) and the steps sigma = tau = 0.95 / sqrt(est), as float64; `oracle()` /
    `oracle_L()` = the float64 operators of the oracle (oracle/cpu_ref.py's protocol); `device(engine)` / `device_L(engine)` = the
    engine's operators; tv_N = N where L is the 2-D first-difference operator."""

    def __init__(self, name):
        self.name = name
        o, oL = self.oracle(), self.oracle_L()
        self.shape = o.shape
        n = o.shape[1]
        self.tv_N = {"Q1": 32, "Q2": 33}.get(name)
        if name == "Q1":
            self.x_true = _truth(32, 32, 31)
        elif name == "Q2":
            self.x_true = 4.0 * _truth(33, 33, 32)           # peaks far above the upper bound of 3
        elif name == "Q3":
            self.x_true = _truth(24, 24, 33)
        elif name == "Q4":
            rng = np.random.default_rng(34)
            self.x_true = np.where(rng.random(120) < 0.2, rng.standard_normal(120) * 2.0, 0.0)
        else:
            self.x_true = np.concatenate([_truth(16, 16, 35 + t) for t in range(3)])
        rng = np.random.default_rng(40 + NAMES.index(name))
        bt = o.matvec(self.x_true)
        e = rng.standard_normal(bt.size)
        self.b = bt + 0.01 * np.linalg.norm(bt) / np.linalg.norm(e) * e
        self.lo, self.hi = _BOX[name]
        M, Lm = o.todense(), oL.todense()
        self.normA2 = float(np.linalg.norm(M, 2) ** 2)
        self.lam = 0.01 * self.normA2
        self.normK2 = float(np.linalg.eigvalsh(M.T @ M + Lm.T @ Lm)[-1])
        self.est = operator_norm_sq([pair(o), pair(oL)], n)
        self.sigma = self.tau = 0.95 / np.sqrt(self.est)

    def psf(self):
        from oracle import cpu_ref as O
        from trips_py_amd.problems import motion_psf
        return O.gauss_psf((9, 9), 1.5)[0] if self.name == "Q1" else motion_psf((7, 7), 5.0, 30.0)[0]

    def oracle(self):
        from blur_psf_cases import scipy_operator
        from oracle import cpu_ref as O
        if self.name == "Q1":
            return scipy_operator(self.psf(), 32, 32, "reflect")
        if self.name == "Q2":
            return scipy_operator(self.psf(), 33, 33, "nearest")
        if self.name == "Q3":
            return O.Radon2D(24, np.linspace(0, np.pi, 12, endpoint=False))
        if self.name == "Q4":
            return O.MatrixOp(_sparse_matrix())
        return O.BlockDiag([O.Radon2D(16, a) for a in _Q5_ANGLES])

    def oracle_L(self):
        import scipy.sparse as sp
        from oracle import cpu_ref as O
        if self.name in ("Q1", "Q2"):
            return O.FirstDerivative2D(32 if self.name == "Q1" else 33)
        if self.name == "Q3":
            return O.MatrixOp(O.first_derivative_2d(24, 24))
        if self.name == "Q4":
            return O.MatrixOp(sp.identity(120, format="csr"))
        return O.SpaceTimeDerivative(16, 3)

    def device(self, engine=None):
        from trips_py_amd.operators import BlockDiagOp, Blur2D, Radon2DParallel, SparseOp
        if self.name == "Q1":
            return Blur2D(self.psf(), 32, 32, engine=engine, boundary="reflect")
        if self.name == "Q2":
            return Blur2D(self.psf(), 33, 33, engine=engine, boundary="nearest")
        if self.name == "Q3":
            return Radon2DParallel(24, np.linspace(0, np.pi, 12, endpoint=False), engine=engine)
        if self.name == "Q4":
            return SparseOp(_sparse_matrix(), engine=engine)
        return BlockDiagOp([Radon2DParallel(16, a, engine=engine) for a in _Q5_ANGLES], engine=engine)

    def device_L(self, engine=None):
        from oracle import cpu_ref as O
        from trips_py_amd.operators import FirstDerivative2D, Identity, SpaceTimeDerivative, SparseOp
        if self.name in ("Q1", "Q2"):
            return FirstDerivative2D(self.tv_N, engine=engine)
        if self.name == "Q3":
            return SparseOp(O.first_derivative_2d(24, 24), engine=engine)
        if self.name == "Q4":
            return Identity(120, engine=engine)
        return SpaceTimeDerivative(16, 3, engine=engine)

    def f64(self, iters, A=None, **kw):
        """pdhg_f64 on the oracle's operators (A: another (matvec, rmatvec) pair for the data operator), the problem's steps."""
        return pdhg_f64(A or pair(self.oracle()), pair(self.oracle_L()), self.b, self.lam, self.sigma, self.tau, self.lo, self.hi, None,
                        iters, **kw)

    def f32(self, iters, **kw):
        return pdhg_f32(pair(self.oracle()), pair(self.oracle_L()), self.b, self.lam, self.sigma, self.tau, self.lo, self.hi, None,
                        iters, **kw)


_problems = {}


def problem(name):
    if name not in _problems:
        _problems[name] = Problem(name)
    return _problems[name]
