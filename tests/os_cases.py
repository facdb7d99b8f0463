"""The ordered-subsets iterations (trips_py_amd/solvers/OSEM.py, SIRT.py, csrc/subsets.hip) restated in NumPy, and the seeded
problems their tests share (tests/test_os_host.py, tests/test_gpu_os.py).

`osem_update_*`, `sirt_residual_*` and `sirt_update_*` are ONE launch each on given vectors, in two forms: storage-faithful (fp32
vectors, the operations of the kernels in the kernels' order — include/trk.h — with the fmaf restated with one rounding, sums in fp64)
and float64 throughout.  The loops `osem_f64 / osem_f32 / sirt_f64 / sirt_f32` run over a list of per-subset (matvec, rmatvec) with
the keep rule; the storage-faithful ones round an operator's float64 product to fp32 once, are built from the launches, and are what
the CPU test engine calls."""
import numpy as np

import mlem_cases as LC
import mrnsd_cases as MC

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------ the visiting order
BITREV = {1: [0], 2: [0, 1], 3: [0, 2, 1], 4: [0, 2, 1, 3], 5: [0, 4, 2, 1, 3], 6: [0, 4, 2, 1, 5, 3], 7: [0, 4, 2, 6, 1, 5, 3],
          8: [0, 4, 2, 6, 1, 5, 3, 7], 12: [0, 8, 4, 2, 10, 6, 1, 9, 5, 3, 11, 7]}


def bitrev_order(S):
    """The subsets sorted by the bit-reversed value of their number in ceil(log2 S) bits, by shifting bits (the product sorts strings)."""
    bits = 0
    while (1 << bits) < S:
        bits += 1

    def rev(s):
        r = 0
        for i in range(bits):
            r |= ((s >> i) & 1) << (bits - 1 - i)
        return r
    return sorted(range(S), key=rev)


# ------------------------------------------------------------------ one launch, storage-faithful and float64
def _x_sums(xn, d, x_true, count):
    xn64, d64 = xn.astype(F64), d.astype(F64)
    return {"x": xn, "xx": float(np.dot(xn64, xn64)), "dd": float(np.sum(d64 ** 2)),          # (the sums as mlem_cases.mlem_f64 forms them)
            "ee": 0.0 if x_true is None else float(np.sum((xn64 - np.asarray(x_true, dtype=xn.dtype).astype(F64)) ** 2)), "count": int(count)}


def osem_update_f32(x, t, sinv, x_ref=None, x_true=None):
    """x' = (sinv > 0) ? max((x * t) * sinv, 0) : x, two fp32 products in that order; d = x' - (x_ref or x) in fp32; count: x' == 0."""
    x, t, sinv = (np.asarray(v, dtype=F32) for v in (x, t, sinv))
    with np.errstate(over="ignore", invalid="ignore"):
        xn = np.where(sinv > 0, np.maximum((x * t) * sinv, F32(0)), x).astype(F32)
        d = xn - (x if x_ref is None else np.asarray(x_ref, dtype=F32))
    return _x_sums(xn, d, x_true, np.count_nonzero(xn == 0))


def osem_update_f64(x, t, sinv, x_ref=None, x_true=None):
    x, t, sinv = (np.asarray(v, dtype=F64) for v in (x, t, sinv))
    xn = np.where(sinv > 0, np.maximum(x * t * sinv, 0.0), x)
    return _x_sums(xn, xn - (x if x_ref is None else np.asarray(x_ref, dtype=F64)), x_true, np.count_nonzero(xn == 0))


def sirt_residual_f32(w, b, rinv=None):
    """d = b - w ; rho = d * rinv (d without rinv) in fp32 ; dd = sum d^2, wd = sum rho d in fp64 from the fp32 values."""
    w, b = np.asarray(w, dtype=F32), np.asarray(b, dtype=F32)
    d = b - w
    rho = d if rinv is None else d * np.asarray(rinv, dtype=F32)
    d64 = d.astype(F64)
    return {"rho": rho.astype(F32), "dd": float(np.dot(d64, d64)), "wd": float(np.dot(rho.astype(F64), d64))}


def sirt_residual_f64(w, b, rinv=None):
    d = np.asarray(b, dtype=F64) - np.asarray(w, dtype=F64)
    rho = d if rinv is None else d * np.asarray(rinv, dtype=F64)
    return {"rho": rho, "dd": float(np.dot(d, d)), "wd": float(np.dot(rho, d))}


def _on_finite_bound(xn, lo, hi):
    return np.count_nonzero(((xn == lo) & np.isfinite(lo)) | ((xn == hi) & np.isfinite(hi)))


def sirt_update_f32(omega, lo, hi, x, t, cinv=None, x_ref=None, x_true=None):
    """u = t * cinv (t without cinv) ; x' = min(max(fmaf(omega32, u, x), lo32), hi32), the fmaf with ONE rounding (mrnsd_cases.fma32) ;
    d = x' - (x_ref or x) in fp32 ; count: x' on a finite bound."""
    x, t = np.asarray(x, dtype=F32), np.asarray(t, dtype=F32)
    lo, hi = F32(lo), F32(hi)
    u = t if cinv is None else (t * np.asarray(cinv, dtype=F32)).astype(F32)
    xn = np.minimum(np.maximum(MC.fma32(F32(omega), u, x), lo), hi).astype(F32)
    d = xn - (x if x_ref is None else np.asarray(x_ref, dtype=F32))
    return _x_sums(xn, d, x_true, _on_finite_bound(xn, lo, hi))


def sirt_update_f64(omega, lo, hi, x, t, cinv=None, x_ref=None, x_true=None):
    x, t = np.asarray(x, dtype=F64), np.asarray(t, dtype=F64)
    u = t if cinv is None else t * np.asarray(cinv, dtype=F64)
    xn = np.minimum(np.maximum(x + omega * u, lo), hi)
    return _x_sums(xn, xn - (x if x_ref is None else np.asarray(x_ref, dtype=F64)), x_true, _on_finite_bound(xn, F64(lo), F64(hi)))


# ------------------------------------------------------------------ the loops
def _recip(s, dt):
    s = np.asarray(s, dtype=dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, dt(1) / s, dt(0)).astype(dt)


def _passes(ops, rows, order, x0, passes, dt, data, update, x_true):
    """`passes` passes over the subsets.  ops: per subset (matvec, rmatvec) in float64; data(s, w) -> (rho, slot 0, slot 1);
    update(s, x, t, x_ref, x_true) -> a launch's dict.  Per pass: X (x_k), s0 / s1 (the running sums of slots 0 / 1, in visiting
    order), xx, dd (over the whole pass), ee, count; `seen`: per sub-step (pass, s, x before, x after)."""
    x = np.asarray(x0, dtype=dt).reshape(-1).copy()
    out = {"X": [], "s0": [], "s1": [], "xx": [], "dd": [], "ee": [], "count": [], "seen": []}
    S = len(order)
    for k in range(passes):
        start, s0, s1 = x, 0.0, 0.0
        for pos, s in enumerate(order):
            last = pos == S - 1
            w = ops[s][0](x.astype(F64)).astype(dt)
            rho, a0, a1 = data(s, w)
            t = ops[s][1](rho.astype(F64)).astype(dt)
            u = update(s, x, t, start if (last and pos > 0) else None, x_true if last else None)
            out["seen"].append((k, s, x, u["x"]))
            x, s0, s1 = u["x"], s0 + a0, s1 + a1
        out["X"].append(x.copy())
        for key, v in (("s0", s0), ("s1", s1), ("xx", u["xx"]), ("dd", u["dd"]), ("ee", u["ee"]), ("count", u["count"])):
            out[key].append(v)
    return out


def _osem(ops, rows, order, b, x0, passes, bg, x_true, dt):
    b = np.asarray(b, dtype=dt).reshape(-1)
    bgv = np.broadcast_to(np.asarray(bg, dtype=dt), b.shape)
    sinv = [_recip(op[1](np.ones(len(r))).astype(dt), dt) for op, r in zip(ops, rows)]

    def data(s, w):
        if dt is F32:
            r = LC.ratio_f32(w, bgv[rows[s]], b[rows[s]])
            return r["rho"], r["kl"], r["rr"]
        y = w + bgv[rows[s]]
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = np.where(y > 0, b[rows[s]] / y, 0.0)
        return rho, float(np.sum(LC.kl_terms(b[rows[s]], y))), float(np.sum((y - b[rows[s]]) ** 2))

    upd = osem_update_f32 if dt is F32 else osem_update_f64
    out = _passes(ops, rows, order, x0, passes, dt, data, lambda s, x, t, xr, xt: upd(x, t, sinv[s], xr, xt), x_true)
    out.update(kl=out["s0"], rr=out["s1"], zeros=out["count"], sinv=sinv)
    return out


def osem_f64(ops, rows, order, b, x0, passes, bg=0.0, x_true=None):
    """OSEM in float64.  Per pass: X, kl and rr (the running sums), zeros, dd = ||x_k - x_{k-1}||^2 over the pass, xx; sinv per subset."""
    return _osem(ops, rows, order, b, x0, passes, bg, x_true, F64)


def osem_f32(ops, rows, order, b, x0, passes, bg=0.0, x_true=None):
    """The storage-faithful form: every vector fp32, the launches mlem_cases.ratio_f32 and osem_update_f32."""
    return _osem(ops, rows, order, b, x0, passes, bg, x_true, F32)


def _sirt(ops, rows, order, b, x0, passes, relax, lo, hi, x_true, dt):
    b = np.asarray(b, dtype=dt).reshape(-1)
    n = np.asarray(x0).size
    rinv = [_recip(op[0](np.ones(n)).astype(dt), dt) for op in ops]
    cinv = [_recip(op[1](np.ones(len(r))).astype(dt), dt) for op, r in zip(ops, rows)]
    res, upd = (sirt_residual_f32, sirt_update_f32) if dt is F32 else (sirt_residual_f64, sirt_update_f64)

    def data(s, w):
        r = res(w, b[rows[s]], rinv[s])
        return r["rho"], r["dd"], r["wd"]

    x0 = np.clip(np.asarray(x0, dtype=F64), lo, hi)
    out = _passes(ops, rows, order, x0, passes, dt, data, lambda s, x, t, xr, xt: upd(relax, lo, hi, x, t, cinv[s], xr, xt), x_true)
    out.update(rr=out["s0"], wr=out["s1"], at_bound=out["count"])
    return out


def sirt_f64(ops, rows, order, b, x0, passes, relax=1.0, lo=-np.inf, hi=np.inf, x_true=None):
    """SIRT / OS-SIRT in float64 with each subset's own reciprocal row and column sums.  Per pass: X, rr (running ||b - A x||^2), wr
    (running R-weighted), at_bound, dd, xx."""
    return _sirt(ops, rows, order, b, x0, passes, relax, lo, hi, x_true, F64)


def sirt_f32(ops, rows, order, b, x0, passes, relax=1.0, lo=-np.inf, hi=np.inf, x_true=None):
    return _sirt(ops, rows, order, b, x0, passes, relax, lo, hi, x_true, F32)


worst_distance = MC.worst_distance
worst_scalar = LC.worst_scalar


# ------------------------------------------------------------------ the seeded problems and their subsets
SUBSETS = {"P3": [1, 2, 3, 5, 12], "P4": [1, 3], "F1": [1, 3]}
F1_N, F1_VIEWS = 16, 8


class FanProblem:
    """F1: a fan-beam case of 16^2 pixels x 8 views with the default geometry, Gaussian data (1 % noise) or photon counts (200 x the
    truth, background 2)."""
    name = "F1"

    def __init__(self, poisson):
        self.angles = np.linspace(0, np.pi, F1_VIEWS, endpoint=False)
        o = self.oracle()
        self.shape = o.shape
        self._M = o.todense()
        self.x_true = MC._truth(F1_N, F1_N, 15) * (LC.SCALE if poisson else 1.0)
        bt = self._M @ self.x_true
        if poisson:
            self.bg = 2.0
            self.b = np.random.default_rng(35).poisson(bt + self.bg).astype(F64)
        else:
            self.bg = 0.0
            e = np.random.default_rng(25).standard_normal(bt.size)
            self.b = bt + 0.01 * np.linalg.norm(bt) / np.linalg.norm(e) * e
        c = (self.b - self.bg).sum() / (self._M @ np.ones(self.shape[1])).sum()
        self.x0 = np.full(self.shape[1], c if c > 0 else 1.0)

    def oracle(self):
        from oracle import cpu_ref as O
        return O.FanBeam2D(F1_N, self.angles)

    def device(self, engine=None):
        from trips_py_amd.operators import FanBeam2D
        return FanBeam2D(F1_N, angles=self.angles, engine=engine)


_problems = {}


def problem(name, poisson):
    """P3 / P4 of mlem_cases (poisson) or of mrnsd_cases (Gaussian), or F1."""
    key = (name, bool(poisson))
    if key not in _problems:
        _problems[key] = FanProblem(poisson) if name == "F1" else (LC if poisson else MC).problem(name)
    return _problems[key]


def subset_rows(name, S):
    """The rows of subset s: the views s, s + S, ... of a projector (P3, F1), the rows s::S of the sparse matrix (P4)."""
    P = problem(name, False)
    m = P.shape[0]
    if name == "P4":
        return [np.arange(s, m, S) for s in range(S)]
    n_ang = {"P3": 12, "F1": F1_VIEWS}[name]
    views = np.arange(m).reshape(n_ang, m // n_ang)
    return [views[s::S].reshape(-1) for s in range(S)]


_oracles = {}


def subset_oracles(name, S):
    """The float64 operator of every subset, made from ITS angles / rows (oracle/cpu_ref.py), computed once."""
    from oracle import cpu_ref as O
    if (name, S) not in _oracles:
        if name == "P3":
            ang = np.linspace(0, np.pi, 12, endpoint=False)
            ops = [O.Radon2D(24, ang[s::S]) for s in range(S)]
        elif name == "F1":
            ang = np.linspace(0, np.pi, F1_VIEWS, endpoint=False)
            ops = [O.FanBeam2D(F1_N, ang[s::S]) for s in range(S)]
        else:
            M = MC._sparse_matrix()
            ops = [O.MatrixOp(M[r]) for r in subset_rows(name, S)]
        _oracles[(name, S)] = ops
    return _oracles[(name, S)]


_dense = {}


def dense_pairs(name, S):
    """[(matvec, rmatvec)] of the subset oracles through their dense float64 matrices (fast to iterate with), computed once."""
    if (name, S) not in _dense:
        Ms = [np.asarray(o.todense() if not hasattr(o, "M") else o.M.toarray(), dtype=F64) for o in subset_oracles(name, S)]
        _dense[(name, S)] = [((lambda v, M=M: M @ v), (lambda v, M=M: M.T @ v)) for M in Ms]
    return _dense[(name, S)]
