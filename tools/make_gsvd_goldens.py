#!/usr/bin/env python
"""Generate tests/golden/direct_tgsvd_deblur1d.npz by RUNNING THE REFERENCE: its `gsvd` (trips/utilities/decompositions.py) and
`tGSVD_sol` on the 1-D deblurring demo's problem: n = 200, Gauss sigma = 30, L = gen_first_derivative_operator(200) densified
plus a zero row, as the notebook builds it; b and delta are those of tests/golden/direct_deblur1d.npz (same seeds).

TEST TOOLING, NOT PRODUCT.  Run only where the reference checkout exists (TRIPS_REFERENCE, default /root/reference):

    python tools/make_gsvd_goldens.py

ONE FUNCTION OF THE REFERENCE IS REPLACED AT RUN TIME.  Its `decompositions.diagp` builds the sign flips as a matrix product whose
shapes do not agree under current NumPy as soon as one diagonal entry is negative (`Y[:, np.ix_(j)]` is 3-D), and this problem
has negative entries.  `diagp` below does what that function is for — negate the columns of Y and the rows of X where the k-th
diagonal of X is negative — and nothing else of the reference is touched.

Stored, numbers only: diag C and diag S of the reference's gsvd; x and k of tGSVD_sol for 'gcv', 'dp' and k = 150; b, delta; the
reference's own residuals ||A - U C X^T||_F / ||M||_F and ||L - V S X^T||_F / ||M||_F, M = [A; L]."""
import contextlib
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("TRIPS_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(HERE, "oracle_shim"))
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

np.int0 = np.intp  # removed in NumPy 2; Deblurring1D.py still uses it
from trips.solvers.tGSVD import tGSVD_sol  # noqa: E402
from trips.test_problems.Deblurring1D import Deblurring1D  # noqa: E402
from trips.utilities import decompositions as refdec  # noqa: E402
from trips.utilities import operators as refops  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
K_NUM = 150


def diagp(Y, X, k):
    j = np.where(np.diagonal(X, k) < 0)[0]
    Y[:, j] = -Y[:, j]
    X[j, :] = -X[j, :]
    return Y, X + 0


refdec.diagp = diagp


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*a, **k)


def main():
    n = 200
    with np.load(os.path.join(OUT, "direct_deblur1d.npz")) as g:
        b, delta = g["b"].reshape(-1, 1), float(g["delta"])
        assert int(g["n"]) == n and float(g["sigma"]) == 30.0
    A = np.asarray(Deblurring1D(CommitCrime=True).forward_Op_1D(parameter=30.0, nx=n).todense())
    L = np.vstack((np.asarray(refops.gen_first_derivative_operator(n).todense()), np.zeros((1, n))))
    U, V, X, C, S = quiet(refdec.gsvd, A.copy(), L.copy())
    nM = np.sqrt(np.linalg.norm(A) ** 2 + np.linalg.norm(L) ** 2)
    out = dict(n=n, sigma=30.0, b=b.reshape(-1), delta=delta, c=np.diag(C).copy(), s=np.diag(S).copy(),
               res_A=np.linalg.norm(A - U @ C @ X.T) / nM, res_L=np.linalg.norm(L - V @ S @ X.T) / nM)
    print(f"residuals {out['res_A']:.3e} {out['res_L']:.3e}")
    for rp in ("gcv", "dp", K_NUM):
        x, k = quiet(tGSVD_sol, A.copy(), L.copy(), b.copy(), regparam=rp, **({"delta": delta} if rp == "dp" else {}))
        key = rp if isinstance(rp, str) else "num"
        out[f"{key}_x"], out[f"{key}_k"] = np.asarray(x, dtype=np.float64).reshape(-1), np.int64(k)
        print(f"  {str(rp):4s} -> k = {int(k)}, ||x|| = {np.linalg.norm(x):.6g}")
    np.savez_compressed(os.path.join(OUT, "direct_tgsvd_deblur1d.npz"), **{k: np.asarray(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
