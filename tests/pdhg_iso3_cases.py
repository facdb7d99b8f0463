"""PDHG with the isotropic space-time TV term (solvers/PDHG.py tv='iso3', csrc/pdhg.hip, csrc/pdhg_tv.hip; the operator: csrc/tvops.hip) restated in NumPy: the
groups (h, v, t) of a geometry (N, frames) on the space-time row layout, the dual in the kernels' operations (include/trk.h: the fp32
operations of a triple), the space-time differences and their transpose in the kernels' order, and the float64 / storage-faithful
loops, which return what pdhg_cases.pdhg_f64 returns.  Only the dual update of q and slot 1 of the sums differ from the anisotropic
restatement.  Two-member groups go through pdhg_iso_cases.dual_q_iso_f32 and singles through pdhg_cases.dual_q_f32."""
import numpy as np

import pdhg_cases as C
import pdhg_iso_cases as I
from pdhg_cases import F32, F64, _sq, _start, d2_adj_f32, d2_fwd_f32, dual_p_f32, dual_q_f32, fma32, primal_f32

NAMES = ["Q5", "Q5u"]
GEOMETRY = {"Q5": (16, 3), "Q5u": (16, 3)}
KINDS = ("hvt", "hv", "ht", "vt", "single")


def rows_of(N, frames):
    return frames * 2 * N * (N - 1) + (frames - 1) * N * N


# ------------------------------------------------------------------ the groups
def groups3(N, frames):
    """Index arrays into the rows of the space-time operator, by kind of group: 'hvt' a (3, k) array of triples, 'hv', 'ht', 'vt'
    (2, k) arrays of pairs with the members in row order, 'single' a (k,) array.  The group of voxel (t, i, j) holds whichever of
    H_t[i][j] (j < N - 1), V_t[i][j] (i < N - 1) and T_t[i][j] (t < frames - 1) exist; voxel (frames-1, N-1, N-1) has no row."""
    assert N >= 2 and frames >= 1
    blk, npix = 2 * N * (N - 1), N * N
    t, i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(frames), np.arange(N), np.arange(N), indexing="ij"))
    has = {"h": j < N - 1, "v": i < N - 1, "t": t < frames - 1}
    row = {"h": t * blk + i * (N - 1) + j, "v": t * blk + N * (N - 1) + i * N + j, "t": frames * blk + t * npix + i * N + j}
    out = {}
    for kind in ("hvt", "hv", "ht", "vt"):
        mask = np.ones(t.size, dtype=bool)
        for c in "hvt":
            mask &= has[c] if c in kind else ~has[c]
        out[kind] = np.stack([row[c][mask] for c in kind])
    out["single"] = np.concatenate([row[c][has[c] & ~has[a] & ~has[b]] for c, a, b in ("hvt", "vht", "thv")])
    return out


def group_counts(N, frames):
    """The closed forms of the number of groups of every kind."""
    return {"hvt": (frames - 1) * (N - 1) ** 2, "hv": (N - 1) ** 2, "ht": (frames - 1) * (N - 1), "vt": (frames - 1) * (N - 1),
            "single": 2 * (N - 1) + frames - 1}


def group_norms(N, frames, u):
    """kind -> the float64 2-norms of the groups of u."""
    u = np.asarray(u, dtype=F64).reshape(-1)
    g = groups3(N, frames)
    out = {k: np.sqrt(sum(u[r] * u[r] for r in g[k])) for k in ("hvt", "hv", "ht", "vt")}
    out["single"] = np.abs(u[g["single"]])
    return out


def norm_sum(N, frames, u):
    return float(sum(v.sum() for v in group_norms(N, frames, u).values()))


def project_f64(N, frames, lam, t):
    """Every group of t projected onto the 2-norm ball of radius lam, float64."""
    g = groups3(N, frames)
    out = t.copy()
    for k in ("hvt", "hv", "ht", "vt"):
        m = np.sqrt(sum(t[r] ** 2 for r in g[k]))
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(m <= lam, 1.0, lam / m)
        for r in g[k]:
            out[r] = t[r] * s
    out[g["single"]] = np.clip(t[g["single"]], -lam, lam)
    return out


# ------------------------------------------------------------------ one kernel each, storage-faithful
def _pairs_f32(sigma, lam, ua, ub, qa, qb):
    """pdhg_iso_cases.dual_q_iso_f32's pair arithmetic on k pairs (a, b): they are laid out as the pairs (H00, V00) of k images of
    2 x 2, whose two singles are zero.  Returns (qa', qb', the pairs' sum of 2-norms of u, their ||q' - q||^2)."""
    k = ua.size
    if k == 0:
        return qa.copy(), qb.copy(), 0.0, 0.0
    u, q = np.zeros(4 * k, dtype=F32), np.zeros(4 * k, dtype=F32)
    u[0::4], u[2::4], q[0::4], q[2::4] = ua, ub, qa, qb
    qn, s1, s3 = I.dual_q_iso_f32(2, k, sigma, lam, u, q)
    assert not qn[1::4].any() and not qn[3::4].any()
    return qn[0::4], qn[2::4], s1, s3


def triple_keep_mask(sigma, lam, uh, uv, ut, qh, qv, qt):
    """(th, tv, tt, m <= lf) of the triples in the kernels' operations."""
    sf, lf = F32(sigma), F32(lam)
    th, tv, tt = fma32(sf, uh, qh), fma32(sf, uv, qv), fma32(sf, ut, qt)
    m = np.sqrt(I.fma32_arrays(th, th, I.fma32_arrays(tv, tv, tt * tt)))
    assert m.dtype == F32
    return th, tv, tt, m, m <= lf


def dual_q_iso3_f32(N, frames, sigma, lam, u, q):
    """The space-time isotropic dual on fp32 u and q.  A triple: th, tv, tt = fmaf(sf, u., q.) ; m = sqrtf(fmaf(th, th, fmaf(tv, tv,
    tt * tt))) ; m <= lf keeps t, else s = lf / m scales all three.  Pairs: dual_q_iso_f32's; singles: dual_q_f32's clip.  Returns
    (q', sum of the groups' 2-norms of u, ||q' - q||^2)."""
    lf = F32(lam)
    assert u.size == q.size == rows_of(N, frames) and u.dtype == q.dtype == F32
    g = groups3(N, frames)
    qn = q.copy()
    s1 = s3 = 0.0
    rh, rv, rt = g["hvt"]
    if rh.size:
        th, tv, tt, m, keep = triple_keep_mask(sigma, lam, u[rh], u[rv], u[rt], q[rh], q[rv], q[rt])
        with np.errstate(divide="ignore", invalid="ignore"):
            s = lf / m
            sh, sv, st = th * s, tv * s, tt * s
        qn[rh], qn[rv], qn[rt] = np.where(keep, th, sh), np.where(keep, tv, sv), np.where(keep, tt, st)
        a, b, c = u[rh].astype(F64), u[rv].astype(F64), u[rt].astype(F64)
        s1 += float(np.sum(np.sqrt(a * a + b * b + c * c)))
        s3 += sum(_sq(qn[r].astype(F64) - q[r].astype(F64)) for r in (rh, rv, rt))
    for kind in ("hv", "ht", "vt"):
        ra, rb = g[kind]
        qn[ra], qn[rb], p1, p3 = _pairs_f32(sigma, lam, u[ra], u[rb], q[ra], q[rb])
        s1, s3 = s1 + p1, s3 + p3
    sg = g["single"]
    qn[sg], p1, p3 = dual_q_f32(sigma, lam, u[sg], q[sg])
    return qn, s1 + p1, s3 + p3


def st_fwd_f32(N, frames, x):
    """The space-time first differences in fp32 in the rows' order: every frame's [H ; V] (k_d2_fwd), then x_t - x_{t+1}."""
    X = x.reshape(frames, N * N)
    return np.concatenate([d2_fwd_f32(N, X[t]) for t in range(frames)] + [(X[:-1] - X[1:]).reshape(-1)])


def st_adj_f32(N, frames, q):
    """The gather of the operator's transpose in fp32, per voxel in the order of k_d2_adj<., true>: the four spatial terms of
    d2_adj_f32, then + T_t, then - T_{t-1}, absent terms skipped."""
    blk, npix = 2 * N * (N - 1), N * N
    acc = np.stack([d2_adj_f32(N, q[t * blk:(t + 1) * blk]) for t in range(frames)])
    T = q[frames * blk:].reshape(frames - 1, npix)
    acc[:-1] = acc[:-1] + T
    acc[1:] = acc[1:] - T
    return acc.reshape(-1)


def st_dual_iso3_f32(N, frames, sigma, lam, xbar, q):
    return dual_q_iso3_f32(N, frames, sigma, lam, st_fwd_f32(N, frames, xbar), q)


def st_primal_f32(N, frames, tau, lo, hi, x, z, q, x_true=None):
    return primal_f32(tau, lo, hi, x, z, st_adj_f32(N, frames, q), x_true)


# ------------------------------------------------------------------ the loops
def pdhg_iso3_f64(A, L, b, lam, sigma, tau, lo, hi, x0, iters, geo, x_true=None, stop_step=None):
    """pdhg_cases.pdhg_f64 with the space-time isotropic dual of geometry geo = (N, frames): the same dictionary, slot 1 of S the sum
    of the groups' 2-norms of L xbar."""
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
        S.append([_sq(e), norm_sum(N, frames, u), _sq(pn - p), _sq(qn - q), _sq(xn), _sq(xn - x),
                  0.0 if x_true is None else _sq(xn - x_true), float(np.count_nonzero((xn == lo) | (xn == hi)))])
        xbar = 2.0 * xn - x
        x, p, q = xn, pn, qn
        X.append(x.copy())
        if stop_step is not None and S[-1][5] <= stop_step ** 2 * S[-1][4]:
            break
    return {"X": X, "S": np.array(S), "p": p, "q": q}


def pdhg_iso3_f32(A, L, b, lam, sigma, tau, lo, hi, x0, iters, geo, x_true=None, fused=False):
    """pdhg_cases.pdhg_f32 with the space-time isotropic dual.  fused: the differences and the gather in fp32 as the fused kernels
    form them (the same bits as rounding the float64 products of fp32 operands)."""
    (Amv, Armv), (Lmv, Lrmv) = A, L
    N, frames = geo

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
        if fused:
            q, s1, s3 = st_dual_iso3_f32(N, frames, sigma, lam, xbar, q)
            x, xbar, tail = st_primal_f32(N, frames, tau, lo, hi, x, f(Armv, p), q, xt)
        else:
            q, s1, s3 = dual_q_iso3_f32(N, frames, sigma, lam, f(Lmv, xbar), q)
            x, xbar, tail = primal_f32(tau, lo, hi, x, f(Armv, p), f(Lrmv, q), xt)
        S.append([s0, s1, s2, s3] + tail)
        X.append(x.copy())
    return {"X": X, "S": np.array(S), "p": p, "q": q}


def objective_iso3(A, L, b, lam, x, geo):
    """1/2 ||A x - b||^2 + lam sum_g ||(L x)_g||_2 with the groups (h, v, t), in float64."""
    x = np.asarray(x, dtype=F64).reshape(-1)
    return 0.5 * _sq(A[0](x) - np.asarray(b, dtype=F64).reshape(-1)) + lam * norm_sum(*geo, L[0](x))


# ------------------------------------------------------------------ the problems
Q5U_MIN_AT_UPPER = 10


class _Q5u:
    """Q5 of pdhg_cases (16 x 16 x 3 dynamic Radon, the same b, lam and steps) under the box [0, c].  c is chosen here, on the CPU,
    from the float64 restatement alone: the value 25 places below the top of the 30th iterate of the solve with c = inf, so that the
    bounded solve has more than Q5U_MIN_AT_UPPER entries on the upper bound (asserted in tests/test_pdhg_iso3_host.py)."""

    def __init__(self):
        P = C.problem("Q5")
        self.__dict__.update(P.__dict__)
        self.name = "Q5u"
        free = pdhg_iso3_f64(C.pair(P.oracle()), C.pair(P.oracle_L()), P.b, P.lam, P.sigma, P.tau, P.lo, np.inf, None, 30, (16, 3))
        self.hi = float(F32(np.sort(free["X"][-1])[-25]))
        self._P = P

    def oracle(self):
        return self._P.oracle()

    def oracle_L(self):
        return self._P.oracle_L()

    def device(self, engine=None):
        return self._P.device(engine)

    def device_L(self, engine=None):
        return self._P.device_L(engine)


_problems = {}


def problem(name):
    assert name in NAMES
    if name == "Q5":
        return C.problem("Q5")
    if name not in _problems:
        _problems[name] = _Q5u()
    return _problems[name]


def f64(name, iters, A=None, **kw):
    P = problem(name)
    return pdhg_iso3_f64(A or C.pair(P.oracle()), C.pair(P.oracle_L()), P.b, P.lam, P.sigma, P.tau, P.lo, P.hi, None, iters,
                         GEOMETRY[name], **kw)


def f32(name, iters, **kw):
    P = problem(name)
    return pdhg_iso3_f32(C.pair(P.oracle()), C.pair(P.oracle_L()), P.b, P.lam, P.sigma, P.tau, P.lo, P.hi, None, iters,
                         GEOMETRY[name], **kw)
