"""Truncated GSVD with the reference's signature (trips/solvers/tGSVD.py) on the device GSVD (_dense.gsvd_device):
x = Y C_k U^T b, where A = U C X^T, L = V S X^T, Y = X^-T, c ascending, and C_k is C with its first k diagonal entries zeroed.

The reference multiplies by C where a pseudo-inverse of A restricted to the kept columns would divide by it; this is that
formula as written (docs/kernels/dense_svd.md, "GSVD").  It is evaluated as Y (keep .* (G^T b)) with G = U C, the matrix the
decomposition produces, so nothing is divided by a small c."""
import numpy as np
import torch

from .. import _dense
from ..reg_param.discrepancy_principle import discrepancy_principle
from ..reg_param.gcv import truncation_gcv


def tGSVD_sol(A, L, b, regparam="gcv", **kwargs):
    """Returns (x (n, 1), k).  regparam: 'gcv' (gcv.py:113-123), 'dp' (needs delta; discrepancy_principle.py:119-129) or the
    index k itself, used as the reference uses it: C[:k, :k] = 0, a Python slice.  A (m x n), L (p x n) with m >= n, p >= n:
    ndarray, np.matrix, scipy.sparse, an engine operator (densified) or a torch tensor; x comes back as float64 NumPy, or as a
    float64 device tensor when b is a torch tensor.  The rules see bhat = U^T b, n entries (U is thin, as the reference's is)."""
    if regparam == "dp" and kwargs.get("delta", None) is None:
        raise Exception(_dense.NO_DELTA_MSG)
    m, p, n = _dense.gsvd_shapes(A, L)
    f = _dense.gsvd_device(A, L)
    bv = _dense.vec_device(b, m)
    gb = _dense.gemv(True, f.Gt, m, n, bv)                       # G^T b = C U^T b
    if isinstance(regparam, str) and regparam in ("gcv", "dp"):
        bhat = (gb * f.inv_c()).cpu().numpy()
        if regparam == "gcv":
            k = truncation_gcv(bhat, n, "tgsvd", p=n)
        else:
            k = discrepancy_principle(None, np.empty((0, n)), bhat, 0.0, dptype="tgsvd",
                                      **{k_: v_ for k_, v_ in kwargs.items() if k_ in ("delta", "eta")})
    else:
        k = regparam
    keep = np.ones(n)
    keep[:k] = 0
    x = _dense.gemv(False, f.Yt, n, n, gb, d=torch.from_numpy(keep).to(gb.device))
    if isinstance(b, torch.Tensor):
        return x.reshape(-1, 1), k
    return x.cpu().numpy().reshape(-1, 1), k
