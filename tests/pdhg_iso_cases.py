"""PDHG with the isotropic TV term (solvers/PDHG.py tv='iso', csrc/pdhg.hip, csrc/pdhg_tv.hip) restated in NumPy, on the problems of
tests/pdhg_cases.py: the groups of a geometry (N, frames), the isotropic dual in the kernels' operations (include/trk.h: the fp32
operations of a pair) and the float64 / storage-faithful loops, which return what pdhg_cases.pdhg_f64 returns.  Only the dual update
of q and slot 1 of the sums differ from the anisotropic restatement; everything else is taken from pdhg_cases."""
import numpy as np

import pdhg_cases as C
from pdhg_cases import F32, F64, _sq, _start, dual_p_f32, dual_q_f32, d2_fwd_f32, fma32, primal_f32, tv_primal_f32

NAMES = ["Q1", "Q2", "Q3", "Q5"]
GEOMETRY = {"Q1": (32, 1), "Q2": (33, 1), "Q3": (24, 1), "Q5": (16, 3)}     # (N, frames); Q5's tail: the 2 * 16^2 temporal rows
FUSED = C.FUSED


# ------------------------------------------------------------------ the groups
def groups(N, frames, rows):
    """(ph, pv, singles): index arrays into the rows of L.  Pair g is {ph[g], pv[g]} = {H[i][j], V[i][j]} of a frame for i, j < N - 1;
    singles are the last image row's H, the last image column's V and every row from frames * 2 N (N - 1) on."""
    blk = 2 * N * (N - 1)
    assert N >= 2 and frames >= 1 and rows >= frames * blk
    i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(N - 1), np.arange(N - 1), indexing="ij"))
    base = (np.arange(frames) * blk)[:, None]
    ph = (base + (i * (N - 1) + j)[None, :]).reshape(-1)
    pv = (base + (N * (N - 1) + i * N + j)[None, :]).reshape(-1)
    edge = np.concatenate(((N - 1) * (N - 1) + np.arange(N - 1), N * (N - 1) + np.arange(N - 1) * N + N - 1))
    singles = np.concatenate(((base + edge[None, :]).reshape(-1), np.arange(frames * blk, rows)))
    return ph, pv, singles


def group_norms(N, frames, u):
    """The 2-norms of the groups of u in float64: pairs, then singles."""
    u = np.asarray(u, dtype=F64).reshape(-1)
    ph, pv, sg = groups(N, frames, u.size)
    return np.concatenate((np.sqrt(u[ph] * u[ph] + u[pv] * u[pv]), np.abs(u[sg])))


def project_f64(N, frames, lam, t):
    """Every group of t projected onto the 2-norm ball of radius lam, float64."""
    ph, pv, sg = groups(N, frames, t.size)
    out = t.copy()
    m = np.sqrt(t[ph] ** 2 + t[pv] ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(m <= lam, 1.0, lam / m)
    out[ph], out[pv] = t[ph] * s, t[pv] * s
    out[sg] = np.clip(t[sg], -lam, lam)
    return out


# ------------------------------------------------------------------ one kernel each, storage-faithful
def fma32_arrays(a, x, y):
    """fma32 with an array as its first operand too.  fma32 passes `a` through np.float64(), which turns a ONE-element array into a
    scalar (deprecated): such operands go through as two copies."""
    a = np.asarray(a, dtype=F32)
    if a.size == 1:
        return fma32(np.repeat(a, 2), np.repeat(x, 2), np.repeat(y, 2))[:1].reshape(a.shape)
    return fma32(a, x, y)


def dual_q_iso_f32(N, frames, sigma, lam, u, q):
    """The isotropic dual on fp32 u and q.  A pair: th = fmaf(sf, uh, qh) ; tv = fmaf(sf, uv, qv) ; m = sqrtf(fmaf(th, th, tv * tv)) ;
    m <= lf keeps (th, tv), else s = lf / m scales both.  A single: dual_q_f32's clip.  Returns (q', sum of the groups' 2-norms of u,
    ||q' - q||^2)."""
    sf, lf = F32(sigma), F32(lam)
    ph, pv, sg = groups(N, frames, u.size)
    th, tv = fma32(sf, u[ph], q[ph]), fma32(sf, u[pv], q[pv])
    m = np.sqrt(fma32_arrays(th, th, tv * tv))
    assert m.dtype == F32
    keep = m <= lf
    with np.errstate(divide="ignore", invalid="ignore"):
        s = lf / m
        sh, sv = th * s, tv * s
    qn = q.copy()
    qn[ph], qn[pv] = np.where(keep, th, sh), np.where(keep, tv, sv)
    qn[sg], s1_single, _ = dual_q_f32(sigma, lam, u[sg], q[sg])
    uh, uv = u[ph].astype(F64), u[pv].astype(F64)
    return qn, float(np.sum(np.sqrt(uh * uh + uv * uv))) + s1_single, _sq(qn.astype(F64) - q.astype(F64))


def tv_dual_iso_f32(N, sigma, lam, xbar, q):
    return dual_q_iso_f32(N, 1, sigma, lam, d2_fwd_f32(N, xbar), q)


# ------------------------------------------------------------------ the loops
def pdhg_iso_f64(A, L, b, lam, sigma, tau, lo, hi, x0, iters, geo, x_true=None, stop_step=None):
    """pdhg_cases.pdhg_f64 with the isotropic dual of geometry geo = (N, frames): the same dictionary, slot 1 of S the sum of the
    groups' 2-norms of L xbar."""
    (Amv, Armv), (Lmv, Lrmv) = A, L
    N, frames = geo
    b = np.asarray(b, dtype=F64).reshape(-1)
    x = _start(x0, Armv(b).size, lo, hi, F64)
    xbar = x.copy()
    p, q = np.zeros(b.size), np.zeros(Lmv(x).size)
    X, S = [], []
    for _ in range(iters):
        e = Amv(xbar) - b
        pn = (p + sigma * e) / (1.0 + sigma)
        u = Lmv(xbar)
        qn = project_f64(N, frames, lam, q + sigma * u)
        xn = np.minimum(np.maximum(x - tau * (Armv(pn) + Lrmv(qn)), lo), hi)
        S.append([_sq(e), float(group_norms(N, frames, u).sum()), _sq(pn - p), _sq(qn - q), _sq(xn), _sq(xn - x),
                  0.0 if x_true is None else _sq(xn - x_true), float(np.count_nonzero((xn == lo) | (xn == hi)))])
        xbar = 2.0 * xn - x
        x, p, q = xn, pn, qn
        X.append(x.copy())
        if stop_step is not None and S[-1][5] <= stop_step ** 2 * S[-1][4]:
            break
    return {"X": X, "S": np.array(S), "p": p, "q": q}


def pdhg_iso_f32(A, L, b, lam, sigma, tau, lo, hi, x0, iters, geo, x_true=None, tv_N=None):
    """pdhg_cases.pdhg_f32 with the isotropic dual.  tv_N: the fused forms on the 2-D operator (geo = (tv_N, 1))."""
    (Amv, Armv), (Lmv, Lrmv) = A, L
    N, frames = geo
    assert not tv_N or geo == (tv_N, 1)

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
            q, s1, s3 = tv_dual_iso_f32(tv_N, sigma, lam, xbar, q)
            x, xbar, tail = tv_primal_f32(tv_N, tau, lo, hi, x, f(Armv, p), q, xt)
        else:
            q, s1, s3 = dual_q_iso_f32(N, frames, sigma, lam, f(Lmv, xbar), q)
            x, xbar, tail = primal_f32(tau, lo, hi, x, f(Armv, p), f(Lrmv, q), xt)
        S.append([s0, s1, s2, s3] + tail)
        X.append(x.copy())
    return {"X": X, "S": np.array(S), "p": p, "q": q}


def objective_iso(A, L, b, lam, x, geo):
    """1/2 ||A x - b||^2 + lam sum_g ||(L x)_g||_2 in float64."""
    x = np.asarray(x, dtype=F64).reshape(-1)
    return 0.5 * _sq(A[0](x) - np.asarray(b, dtype=F64).reshape(-1)) + lam * float(group_norms(*geo, L[0](x)).sum())


# ------------------------------------------------------------------ the problems: pdhg_cases' b, lam, steps and box
def problem(name):
    assert name in NAMES
    return C.problem(name)


def f64(name, iters, A=None, **kw):
    P = problem(name)
    return pdhg_iso_f64(A or C.pair(P.oracle()), C.pair(P.oracle_L()), P.b, P.lam, P.sigma, P.tau, P.lo, P.hi, None, iters,
                        GEOMETRY[name], **kw)


def f32(name, iters, **kw):
    P = problem(name)
    return pdhg_iso_f32(C.pair(P.oracle()), C.pair(P.oracle_L()), P.b, P.lam, P.sigma, P.tau, P.lo, P.hi, None, iters,
                        GEOMETRY[name], **kw)
