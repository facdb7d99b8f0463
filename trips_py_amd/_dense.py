"""Dense float64 matrices on the device for the direct solvers (tSVD, tGSVD, Tikhonov): operand conversion, the one-sided Jacobi
SVD of csrc/dense_svd.hip (trk_dense_svd_f64), the same iteration with a carried companion (trk_dense_svd_carry_f64) and the GSVD
built on it, and the two float64 products (trk_dense_gemv_f64).

A device matrix is held as a torch float64 tensor `At` of shape (n, m), contiguous: row j of `At` is column j of the m x n matrix,
i.e. the column-major layout the kernels read (leading dimension m)."""
import ctypes
import math
import warnings

import numpy as np
import torch

from . import _lib
from .engine import default_engine
from .operators import LinearOperator

MAX_COLS = 8192          # TRK_DENSE_SVD_MAX_COLS
MAX_SWEEPS = 30


def _engine():
    return default_engine()


def dense_host(A, role="A"):
    """A as a float64 NumPy 2-D array: ndarray / np.matrix / scipy.sparse / engine operator (through todense()) / torch tensor."""
    if isinstance(A, LinearOperator):
        return np.asarray(A.todense(), dtype=np.float64)
    if isinstance(A, torch.Tensor):
        return A.detach().to("cpu", torch.float64).numpy()
    try:
        import scipy.sparse as sp
        if sp.issparse(A):
            return np.asarray(A.toarray(), dtype=np.float64)
    except ImportError:        # pragma: no cover
        pass
    if hasattr(A, "todense") and not isinstance(A, np.ndarray):
        return np.asarray(A.todense(), dtype=np.float64)
    a = np.asarray(A, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError(f"{role} must be a 2-D matrix, got shape {a.shape}")
    return a


def to_device_t(A, role="A"):
    """A (any kind dense_host accepts) -> (At, m, n): At the (n, m) contiguous float64 device tensor (column-major A)."""
    eng = _engine()
    if isinstance(A, torch.Tensor):
        if A.dim() != 2:
            raise ValueError(f"{role} must be a 2-D matrix, got shape {tuple(A.shape)}")
        At = A.detach().to(device=eng.device, dtype=torch.float64).T.contiguous()
    else:
        a = dense_host(A, role)
        At = torch.from_numpy(np.ascontiguousarray(a.T)).to(eng.device)
    return At, int(At.shape[1]), int(At.shape[0])


def amax_finite(Xt, role):
    """The largest |entry| of a device matrix as a host float (one synchronisation); ValueError naming `role` when the matrix
    holds a NaN or an Inf, which no sweep of the Jacobi iteration would notice: every comparison with a NaN is false, so the
    iteration reports convergence."""
    amax = float(Xt.abs().max()) if Xt.numel() else 0.0
    if not np.isfinite(amax):
        raise ValueError(f"dense SVD: the matrix {role} has a NaN or Inf entry")
    return amax


def pow2_exponent(amax):
    """e with amax in [2^e, 2^(e + 1)); 0 for amax = 0."""
    return math.frexp(amax)[1] - 1 if amax > 0.0 else 0


def scale_pow2(X, k):
    """X * 2^k, exact (short of the ends of the float64 range).  In two factors: 2^k itself leaves the range for |k| > 1023."""
    if k == 0:
        return X
    h = k // 2
    return (X * math.ldexp(1.0, h)) * math.ldexp(1.0, k - h)


def _svd_tall(At, m, n, max_sweeps=MAX_SWEEPS, role="A", amax=None):
    """One-sided Jacobi on the m x n (m >= n) column-major At -> (Ut (n, m), S (n,), Vt (n, n), sweeps), sorted descending:
    row j of Ut / Vt is the j-th left / right singular vector.

    The kernels square entries, so the iteration runs on At scaled by the power of two that brings its largest |entry| (`amax`;
    taken here when not given) into [1, 2), and S is scaled back: exact, and the factors of 2^k A are those of A bit for bit
    with S times 2^k.  ValueError for a matrix with a NaN or Inf entry."""
    eng = _engine()
    e = pow2_exponent(amax_finite(At, role) if amax is None else amax)
    At = scale_pow2(At, -e).contiguous()
    lib = eng.lib
    npad, need = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.trk_dense_svd_f64_dims(m, n, ctypes.byref(npad), ctypes.byref(need)), "trk_dense_svd_f64_dims")
    npad = npad.value
    G = torch.empty((npad, m), dtype=torch.float64, device=eng.device)
    V = torch.empty((npad, npad), dtype=torch.float64, device=eng.device)
    S = torch.empty(n, dtype=torch.float64, device=eng.device)
    work = torch.empty(need.value, dtype=torch.float64, device=eng.device)
    sweeps, conv = ctypes.c_int(0), ctypes.c_int(0)
    tol = max(m, 64) * np.finfo(np.float64).eps
    _lib.check(lib.trk_dense_svd_f64(At.data_ptr(), m, n, m, G.data_ptr(), m, V.data_ptr(), npad, S.data_ptr(), work.data_ptr(),
                                     need.value, float(tol), int(max_sweeps), ctypes.byref(sweeps), ctypes.byref(conv), eng.stream()),
               "trk_dense_svd_f64")
    if not conv.value:
        warnings.warn(f"dense SVD: {m} x {n} not converged after {sweeps.value} Jacobi sweeps", RuntimeWarning)
    S, perm = torch.sort(S, descending=True, stable=True)
    Gt = G[:n].index_select(0, perm)
    inv = torch.where(S > 0, 1.0 / torch.where(S > 0, S, torch.ones_like(S)), torch.zeros_like(S))
    Ut = Gt * inv.reshape(-1, 1)
    Vt = V[:n, :n].index_select(0, perm)          # row j of V^T = column perm[j] of V (V is column-major: row = column)
    return Ut, scale_pow2(S, e), Vt.contiguous(), sweeps.value


def svd_device(A, max_sweeps=MAX_SWEEPS, role="A"):
    """Thin SVD of A on the device: (Ut (k, m), S (k,), Vt (k, n), sweeps) as float64 device tensors, k = min(m, n), singular values
    descending; A = Ut^T diag(S) Vt.  A wide matrix runs on A^T with the factors swapped.  Any finite float64 matrix is accepted
    (see _svd_tall); ValueError naming `role` for one with a NaN or Inf entry."""
    At, m, n = to_device_t(A, role)
    return svd_device_t(At, m, n, max_sweeps, role)


def svd_device_t(At, m, n, max_sweeps=MAX_SWEEPS, role="A"):
    if min(m, n) > MAX_COLS:
        raise ValueError(f"dense SVD: at most {MAX_COLS} columns (of the matrix or of its transpose); got {m} x {n}")
    if m >= n:
        return _svd_tall(At, m, n, max_sweeps, role)
    Ut, S, Vt, sw = _svd_tall(At.T.contiguous(), n, m, max_sweeps, role)   # A^T = U' S V'^T  ->  A = V' S U'^T
    return Vt, S, Ut, sw


def svd_carry_t(At, m, n, Ct, max_sweeps=MAX_SWEEPS):
    """One-sided Jacobi on the m x n (m >= n) column-major At with a carried companion (trk_dense_svd_carry_f64): Ct is (n, nc),
    row j the companion's column j.  With W the accumulated rotation, returns (Gt (n, m) = (A W)^T, S (n,) = its column norms,
    (C W)^T (n, nc), sweeps) — in the order of A's columns, neither sorted nor normalised.  As in _svd_tall the iteration runs
    on At scaled by a power of two to a largest |entry| in [1, 2), and Gt and S are scaled back; ValueError for a NaN or Inf."""
    eng = _engine()
    e = pow2_exponent(amax_finite(At, "A"))
    lib = eng.lib
    nc = int(Ct.shape[1])
    if tuple(At.shape) != (n, m) or int(Ct.shape[0]) != n:
        raise ValueError(f"svd_carry_t: At {tuple(At.shape)} and Ct {tuple(Ct.shape)} do not fit an {m} x {n} matrix")
    npad, need = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.trk_dense_svd_carry_f64_dims(m, n, nc, ctypes.byref(npad), ctypes.byref(need)), "trk_dense_svd_carry_f64_dims")
    npad = npad.value
    At = scale_pow2(At, -e).contiguous()
    G = torch.empty((npad, m), dtype=torch.float64, device=eng.device)
    C = torch.empty((npad, nc), dtype=torch.float64, device=eng.device)
    C[:n].copy_(Ct)
    S = torch.empty(n, dtype=torch.float64, device=eng.device)
    work = torch.empty(need.value, dtype=torch.float64, device=eng.device)
    sweeps, conv = ctypes.c_int(0), ctypes.c_int(0)
    tol = max(m, 64) * np.finfo(np.float64).eps
    _lib.check(lib.trk_dense_svd_carry_f64(At.data_ptr(), m, n, m, G.data_ptr(), m, C.data_ptr(), nc, nc, S.data_ptr(),
                                           work.data_ptr(), need.value, float(tol), int(max_sweeps), ctypes.byref(sweeps),
                                           ctypes.byref(conv), eng.stream()), "trk_dense_svd_carry_f64")
    if not conv.value:
        warnings.warn(f"dense SVD: {m} x {n} not converged after {sweeps.value} Jacobi sweeps", RuntimeWarning)
    return scale_pow2(G[:n], e), scale_pow2(S, e), C[:n], sweeps.value


def colnorm(Xt, row0, rows):
    """Norms of the columns of rows [row0, row0 + rows) of the column-major matrix Xt (cols, ld): the fixed-order sum of the SVD's
    own singular values (trk_dense_colnorm_f64), where a torch reduction would not promise the same bits twice."""
    eng = _engine()
    cols, ld = int(Xt.shape[0]), int(Xt.shape[1])
    if not Xt.is_contiguous() or row0 < 0 or rows < 1 or row0 + rows > ld:
        raise ValueError(f"colnorm: rows [{row0}, {row0 + rows}) of a contiguous ({cols}, {ld}) tensor")
    out = torch.empty(cols, dtype=torch.float64, device=eng.device)
    _lib.check(eng.lib.trk_dense_colnorm_f64(Xt.data_ptr() + 8 * row0, ld, rows, cols, out.data_ptr(), eng.stream()),
               "trk_dense_colnorm_f64")
    return out


def gsvd_shapes(A, L):
    """(m, p, n) of the pair A (m x n), L (p x n), from the operands' `.shape` alone (nothing touches the engine): ValueError
    unless both are 2-D with the same column count, m >= n, p >= n and n <= MAX_COLS."""
    shapes = []
    for X, role in ((A, "A"), (L, "L")):
        shp = tuple(int(v) for v in (X.shape if hasattr(X, "shape") else np.shape(X)))
        if len(shp) != 2:
            raise ValueError(f"gsvd: {role} must be a 2-D matrix, got shape {shp}")
        shapes.append(shp)
    (m, n), (p, n2) = shapes
    if n != n2:
        raise ValueError(f"gsvd: A is {m} x {n} and L is {p} x {n2}: the column counts differ")
    if n < 1 or m < n or p < n:
        raise ValueError(f"gsvd: need m >= n, p >= n and n >= 1 for A m x n and L p x n (A is {m} x {n}, L is {p} x {n})")
    if n > MAX_COLS:
        raise ValueError(f"gsvd: at most {MAX_COLS} columns; got {n}")
    return m, p, n


class GSVD:
    """The factors of gsvd_device as float64 device tensors, every matrix column-major (row i = column i):
        Gt (n, m) = (U diag(c))^T,  Ht (n, p) = (V diag(s))^T,  Xt (n, n) = X^T,  Yt (n, n) = (X^-T)^T,  c ascending, s,
    so that A = G X^T, L = H X^T and Y^T X = I; sweeps = Jacobi sweeps of the stages (0 for a stage that did not run)."""

    def __init__(self, m, p, n, Gt, Ht, Xt, Yt, c, s, sweeps):
        self.m, self.p, self.n = m, p, n
        self.Gt, self.Ht, self.Xt, self.Yt, self.c, self.s, self.sweeps = Gt, Ht, Xt, Yt, c, s, sweeps

    def _inv(self, d):
        ok = d > self.n * np.finfo(np.float64).eps
        return torch.where(ok, 1.0 / torch.where(ok, d, torch.ones_like(d)), torch.zeros_like(d))

    def inv_c(self):
        """1 / c, and 0 where c <= n eps (the columns of U that are zero by convention)."""
        return self._inv(self.c)

    def Ut(self):
        return self.Gt * self.inv_c().reshape(-1, 1)

    def Vt(self):
        return self.Ht * self._inv(self.s).reshape(-1, 1)


def gsvd_device(A, L, max_sweeps=MAX_SWEEPS):
    """GSVD of the pair (A m x n, L p x n; m >= n, p >= n, [A; L] of full column rank) on the device -> GSVD.
    Three runs of the one-sided Jacobi (docs/kernels/dense_svd.md, "GSVD"):
      1. M = [A; L] = Q diag(sigma) Vm^T; ValueError when sigma_min <= max(m + p, n) eps sigma_max (A and L share a null space).
      2. Q1 = Q[:m] with the companion [Q2; Vm diag(sigma); Vm diag(1 / sigma)]: G = Q1 W, Q2 W, X = Vm diag(sigma) W and
         Y = X^-T come back together; c, s = column norms of G and Q2 W.
      3. on the columns J with c > 1 / sqrt(2), where Q2 W has small and poorly orthogonal columns: Q2 W_J with the companion
         [G_J; X_J; Y_J]; c and s on J again from the column norms.  Skipped when J is empty.
    Then the columns are sorted by c ascending (s descending), the reference's order.
    An s that should be zero (L has a null vector) comes out of the rotations as rounding of its O(1) neighbours, of order
    sqrt(n) tol, not n eps.  What lies within 8 (m + p) eps cond(M) of zero — the accuracy of every s here — is returned as
    exactly 0, with a zero column in H."""
    m, p, n = gsvd_shapes(A, L)
    At, _, _ = to_device_t(A, "A")
    Lt, _, _ = to_device_t(L, "L")
    eps = np.finfo(np.float64).eps
    amax = max(amax_finite(At, "A"), amax_finite(Lt, "L"))
    Qt, sig, Vmt, sw1 = _svd_tall(torch.cat((At, Lt), dim=1), m + p, n, max_sweeps, "[A; L]", amax)
    smax, smin = float(sig[0]), float(sig[-1])
    if not smin > max(m + p, n) * eps * smax:
        raise ValueError(f"gsvd: [A; L] has no full column rank to working precision (sigma_min = {smin:.3e}, sigma_max = "
                         f"{smax:.3e}): A and L share a null space")
    sc = sig.reshape(-1, 1)
    Gt, c, Ct, sw2 = svd_carry_t(Qt[:, :m].contiguous(), m, n, torch.cat((Qt[:, m:], Vmt * sc, Vmt / sc), dim=1), max_sweeps)
    Ht, XYt = Ct[:, :p].contiguous(), Ct[:, p:]
    s = colnorm(Ht, 0, p)
    J = torch.nonzero(c > np.sqrt(0.5)).reshape(-1)
    sw3 = 0
    if J.numel() > 0:
        nJ = int(J.numel())
        comp = torch.cat((Gt.index_select(0, J), XYt.index_select(0, J)), dim=1)
        HJ, sJ, comp, sw3 = svd_carry_t(Ht.index_select(0, J), p, nJ, comp, max_sweeps)
        comp = comp.contiguous()
        Gt, XYt = Gt.clone(), XYt.clone()
        Gt.index_copy_(0, J, comp[:, :m])
        XYt.index_copy_(0, J, comp[:, m:])
        Ht.index_copy_(0, J, HJ)
        c = c.index_copy(0, J, colnorm(comp, 0, m))
        s = s.index_copy(0, J, sJ)
    live = s > 8 * (m + p) * eps * (smax / smin)
    s, Ht = torch.where(live, s, torch.zeros_like(s)), Ht * live.reshape(-1, 1)
    c, order = torch.sort(c, stable=True)
    Gt, Ht, XYt, s = Gt.index_select(0, order), Ht.index_select(0, order), XYt.index_select(0, order), s.index_select(0, order)
    return GSVD(m, p, n, Gt, Ht, XYt[:, :n].contiguous(), XYt[:, n:].contiguous(), c, s, (sw1, sw2, sw3))


def gemv(trans, At, m, n, x, d=None, alpha=1.0, beta=0.0, y=None):
    """y = beta y + alpha op(A) (d .* x) with A given as its column-major (n, m) tensor At (trk_dense_gemv_f64): op(A) = A^T for
    trans (x, d have m entries, y n), A otherwise (x, d n entries, y m).  float64 device vectors."""
    eng = _engine()
    out_len = n if trans else m
    if y is None:
        y = torch.empty(out_len, dtype=torch.float64, device=eng.device)
    x = x.reshape(-1).contiguous()
    d = None if d is None else d.reshape(-1).contiguous()
    _lib.check(eng.lib.trk_dense_gemv_f64(1 if trans else 0, m, n, At.data_ptr(), m, x.data_ptr(), 0 if d is None else d.data_ptr(),
                                          float(alpha), float(beta), y.data_ptr(), eng.stream()), "trk_dense_gemv_f64")
    return y


def vec_device(b, n):
    """b (NumPy / np.matrix / torch, any shape with n entries) -> float64 device vector."""
    eng = _engine()
    if isinstance(b, torch.Tensor):
        v = b.detach().to(device=eng.device, dtype=torch.float64).reshape(-1)
    else:
        v = torch.from_numpy(np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1))).to(eng.device)
    if v.numel() != n:
        raise ValueError(f"vector of {v.numel()} entries where {n} are needed")
    return v.contiguous()


# ------------------------------------------------------------------------------------------- pieces of the direct solvers
# the reference's message when regparam='dp' comes without delta (tSVD.py, Tikhonov.py through discrepancy_principle.py)
NO_DELTA_MSG = ("A value for the noise level delta was not provided and the discrepancy principle cannot be applied. \n"
                "                    Please supply a value of delta based on the estimated noise level of the problem, or choose the "
                "regularization parameter according to gcv.")


def check_delta(regparam, kwargs):
    if isinstance(regparam, str) and regparam in ("dp", "DP", "Dp", "Discrepancy Principle", "Discrepancy principle",
                                                  "discrepancy principle") and kwargs.get("delta", None) is None:
        raise Exception(NO_DELTA_MSG)


class Spectrum:
    """Thin SVD of an m x n device matrix and the projection of one right-hand side on it:
        c = U^T b (k = min(m, n) entries, device),  resid2 = ||b - U c||^2 (host float; 0 when U is square)."""

    def __init__(self, At, m, n, bv):
        self.m, self.n = m, n
        self.Ut, self.S, self.Vt, self.sweeps = svd_device_t(At, m, n)
        self.k = int(self.S.numel())
        self.c = gemv(True, self.Ut, m, self.k, bv)
        if m > self.k:
            r = gemv(False, self.Ut, m, self.k, self.c, alpha=-1.0, beta=1.0, y=bv.clone())
            self.resid2 = float(torch.dot(r, r))
        else:
            self.resid2 = 0.0
        self.s_host = self.S.cpu().numpy()
        self.c_host = self.c.cpu().numpy()

    def bhat_with_tail(self):
        """c, followed by sqrt(resid2) when b has a part outside the columns of U: the sums of squares of the reference's m-entry
        U^T b (full U) over any trailing range are those of this vector."""
        if self.m > self.k:
            return np.append(self.c_host, np.sqrt(self.resid2))
        return self.c_host

    def solve(self, d_host):
        """V diag(d) c for a host filter vector d (k entries) -> device vector (n)."""
        d = torch.from_numpy(np.ascontiguousarray(d_host, dtype=np.float64)).to(self.c.device)
        return gemv(False, self.Vt, self.n, self.k, self.c, d=d)
