"""Truncated SVD with the reference's signature (trips/solvers/tSVD.py): x = V_k diag(1 / s_k) U_k^T b on the device SVD.

The reference takes a full SVD (U m x m); the truncation rules see the tail of U^T b past column n only through its sum of
squares, so a thin U and ||b - U U^T b||^2 give the same index without the m x m factor."""
import numpy as np
import torch

from .. import _dense
from ..reg_param.discrepancy_principle import discrepancy_principle
from ..reg_param.gcv import truncation_gcv


def tSVD_sol(A, b, regparam="gcv", **kwargs):
    """Returns (x (n, 1), k).  regparam: 'gcv' (gcv.py:96-112), 'dp' (needs delta; discrepancy_principle.py:100-118) or the
    truncation index itself.  A: ndarray, np.matrix, scipy.sparse, an engine operator (densified) or a torch tensor; x comes back
    as float64 NumPy, or as a float64 device tensor when b is a torch tensor."""
    if regparam == "dp" and kwargs.get("delta", None) is None:
        raise Exception(_dense.NO_DELTA_MSG)
    At, m, n = _dense.to_device_t(A)
    bv = _dense.vec_device(b, m)
    sp = _dense.Spectrum(At, m, n, bv)
    if isinstance(regparam, str) and regparam in ("gcv", "dp"):
        if m < n:
            raise ValueError(f"tSVD_sol: regparam={regparam!r} needs at least as many rows as columns (A is {m} x {n})")
        bhat = sp.bhat_with_tail()
        if regparam == "gcv":
            k = truncation_gcv(bhat, n, "tsvd", rows=m)
        else:
            k = discrepancy_principle(None, np.empty((0, n)), bhat, 0.0, dptype="tsvd",
                                      **{k_: v_ for k_, v_ in kwargs.items() if k_ in ("delta", "eta")})
    else:
        k = regparam
    kk = max(0, min(int(k), sp.k))
    if kk == 0:
        x = torch.zeros(n, dtype=torch.float64, device=bv.device)
    else:
        x = _dense.gemv(False, sp.Vt[:kk], n, kk, sp.c[:kk], d=1.0 / sp.S[:kk])
    if isinstance(b, torch.Tensor):
        return x.reshape(-1, 1), k
    return x.cpu().numpy().reshape(-1, 1), k
