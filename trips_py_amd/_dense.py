"""Dense float64 matrices on the device for the direct solvers (tSVD, Tikhonov): operand conversion, the one-sided Jacobi
SVD of csrc/dense_svd.hip (trk_dense_svd_f64) and its two float64 products (trk_dense_gemv_f64).

A device matrix is held as a torch float64 tensor `At` of shape (n, m), contiguous: row j of `At` is column j of the m x n matrix,
i.e. the column-major layout the kernels read (leading dimension m)."""
import ctypes
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


def _svd_tall(At, m, n, max_sweeps=MAX_SWEEPS):
    """One-sided Jacobi on the m x n (m >= n) column-major At -> (Ut (n, m), S (n,), Vt (n, n), sweeps), sorted descending:
    row j of Ut / Vt is the j-th left / right singular vector."""
    eng = _engine()
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
    return Ut, S, Vt.contiguous(), sweeps.value


def svd_device(A, max_sweeps=MAX_SWEEPS):
    """Thin SVD of A on the device: (Ut (k, m), S (k,), Vt (k, n), sweeps) as float64 device tensors, k = min(m, n), singular values
    descending; A = Ut^T diag(S) Vt.  A wide matrix runs on A^T with the factors swapped."""
    At, m, n = to_device_t(A)
    return svd_device_t(At, m, n, max_sweeps)


def svd_device_t(At, m, n, max_sweeps=MAX_SWEEPS):
    if min(m, n) > MAX_COLS:
        raise ValueError(f"dense SVD: at most {MAX_COLS} columns (of the matrix or of its transpose); got {m} x {n}")
    if m >= n:
        return _svd_tall(At, m, n, max_sweeps)
    Ut, S, Vt, sw = _svd_tall(At.T.contiguous(), n, m, max_sweeps)   # A^T = U' S V'^T  ->  A = V' S U'^T
    return Vt, S, Ut, sw


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
