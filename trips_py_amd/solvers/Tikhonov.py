"""Dense Tikhonov with the reference's signature (trips/solvers/Tikhonov.py): x = argmin ||A x - b||^2 + lambda ||L x||^2, lambda by
GCV (gcv.py:25-95 with Q_A = I), by the discrepancy principle (discrepancy_principle.py:19-99) or given.

Everything goes through the spectrum of the standard-form matrix, one device SVD (csrc/dense_svd.hip), instead of a dense solve
of the normal equations per evaluation of the selection function:

    L = I        Abar = A, bbar = b, x = y.
    otherwise    L^T L = R^T R with R = diag(s_r) W_r^T from the device SVD of L (zero rows appended when L has fewer rows than
                 columns), r = its numerical rank and N = the remaining right singular vectors (the null space of L).  With
                 x = R^+ y + N z and the N-part chosen to fit the data (A N = Q_N T_N):
                     Abar = (I - Q_N Q_N^T) A R^+,  bbar = (I - Q_N Q_N^T) b,
                     x = R^+ y - N T_N^-1 Q_N^T (A R^+ y - b)
                 (the A-weighted pseudo-inverse of L, as the discrepancy principle's null-space branch has it, :45-66).
    Abar = U diag(s) V^T, c = U^T bbar, t = ||bbar - U c||^2:
        ||A x_lambda - b||^2         = sum (lambda / (s^2 + lambda))^2 c^2 + t
        trace of the influence matrix = dim N + sum s^2 / (s^2 + lambda)
        y_lambda                     = V diag(s / (s^2 + lambda)) c
The reference's selection functions are these expressions of lambda; the minimiser (fminbound on [1e-9, 1e2]) and the Newton
iteration of the discrepancy principle are the engine's existing ones (reg_param/)."""
import numpy as np
import torch

from .. import _dense
from ..operators import Identity, is_identity
from ..reg_param.discrepancy_principle import discrepancy_principle
from ..reg_param.gcv import fminbound_gcv_diag

_GCV = ("gcv", "GCV", "Gcv")
_DP = ("DP", "dp", "Dp", "Discrepancy Principle", "Discrepancy principle", "discrepancy principle")


def _standard_form(At, m, n, L, bv):
    """-> (Abar_t (r, m), r, dim N, back(y) -> x) for a general L (see the module docstring)."""
    Lh = _dense.dense_host(L, "L")
    if Lh.shape[1] != n:
        raise ValueError(f"Tikhonov: L has {Lh.shape[1]} columns, A has {n}")
    if Lh.shape[0] < n:
        Lh = np.vstack((Lh, np.zeros((n - Lh.shape[0], n))))
    _, SL, WLt, _ = _dense.svd_device(Lh, role="L")
    tol = max(Lh.shape) * np.finfo(np.float64).eps * float(SL[0]) if SL.numel() else 0.0
    r = int((SL > tol).sum())
    Rp_t = WLt[:r] / SL[:r].reshape(-1, 1)                 # (r, n): rows = columns of R^+ = W_r diag(1/s_r)
    M = (At.T @ Rp_t.T)                                    # A R^+  (m x r), row-major
    if r == n:
        Abar = M
        bbar = bv

        def back(y):
            return Rp_t.T @ y
    else:
        N = WLt[r:].T                                      # n x (n - r)
        AN = At.T @ N                                      # m x (n - r)
        QN, TN = torch.linalg.qr(AN, mode="reduced")
        Abar = M - QN @ (QN.T @ M)
        bbar = bv - QN @ (QN.T @ bv)

        def back(y):
            Ay = M @ y
            z = torch.linalg.solve_triangular(TN, (QN.T @ (Ay - bv)).reshape(-1, 1), upper=True).reshape(-1)
            return Rp_t.T @ y - N @ z
    return Abar.T.contiguous(), r, n - r, back, bbar.contiguous()


def Tikhonov(A, b, L, x_true, regparam="gcv", **kwargs):
    """Returns (x (n, 1), lambda).  `x_true` is accepted and not used, as in the reference.  A, L: ndarray, np.matrix,
    scipy.sparse, engine operators (densified) or torch tensors; x comes back as float64 NumPy, or as a float64 device tensor
    when b is a torch tensor."""
    _dense.check_delta(regparam, kwargs)
    if isinstance(regparam, str) and regparam not in _GCV + _DP:
        raise TypeError(f"Tikhonov: regparam must be 'gcv', 'dp' or a number, got {regparam!r}")
    At, m, n = _dense.to_device_t(A)
    bv = _dense.vec_device(b, m)
    if isinstance(L, Identity) or (not isinstance(L, torch.Tensor) and is_identity(L) and np.shape(L) == (n, n)):
        Abar_t, r, dim_null, bbar = At, n, 0, bv
        back = None
    else:
        Abar_t, r, dim_null, back, bbar = _standard_form(At, m, n, L, bv)
    sp = _dense.Spectrum(Abar_t, m, r, bbar)
    s, c = sp.s_host, sp.c_host
    tall = m > sp.k
    if isinstance(regparam, str) and regparam in _GCV:
        s_ext = np.append(s, 0.0) if tall else s
        c_ext = sp.bhat_with_tail()
        lam = fminbound_gcv_diag(s_ext, c_ext, m - dim_null)
    elif isinstance(regparam, str):
        shape = (sp.k + 1, sp.k) if tall else (sp.k, sp.k)
        lam = discrepancy_principle(None, None, None, 0.0, spectrum=(s, sp.bhat_with_tail(), shape),
                                    **{k_: v_ for k_, v_ in kwargs.items() if k_ in ("delta", "eta")})
    else:
        lam = regparam
    den = s * s + float(lam)
    y = sp.solve(np.divide(s, den, out=np.zeros_like(s), where=den > 0))
    x = y if back is None else back(y)
    if isinstance(b, torch.Tensor):
        return x.reshape(-1, 1), lam
    return x.cpu().numpy().reshape(-1, 1), lam
