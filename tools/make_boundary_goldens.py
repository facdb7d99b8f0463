#!/usr/bin/env python
"""Generate tests/golden/deblur1d_bc_<mode>.npz by RUNNING THE REFERENCE's 1-D deblurring problem under the four boundary
modes besides 'reflect' (Deblurring1D.forward_Op_1D(parameter, nx, boundary_condition=mode), Deblurring1D.py:93-102).

TEST TOOLING, NOT PRODUCT.  Run only where the reference exists (the build container), with the same shim as
tools/make_goldens.py (whose path setup and helpers are imported from it):

    python tools/make_boundary_goldens.py

Per mode: the length-n PSF, a seeded signal `x` with the reference's forward and backward (flipped-PSF) applies of it, and
the reference's CGLS (50 iterations, tol 0) and Hybrid_LSQR (fixed lambda) on the BASELINE C1 signal with seeded 1 % noise.
Only numeric arrays are stored.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import CGLS, Deblurring1D, Hybrid_LSQR, np, quiet, save  # noqa: E402

MODES = ("constant", "nearest", "mirror", "wrap")
N, SIGMA, CGLS_ITS, HYB_ITS, HYB_LAM = 256, 3, 50, 20, 1e-2


def deblur1d_bc(mode):
    print("1-D deblurring,", mode)
    D1 = Deblurring1D(CommitCrime=True)
    A = D1.forward_Op_1D(SIGMA, N, boundary_condition=mode)
    rng = np.random.default_rng(2024)
    x = rng.standard_normal(N)
    Ax = np.asarray(A @ x).reshape(-1)
    ATx = np.asarray(A.T @ x).reshape(-1)
    x_true = D1.gen_xtrue(N, "curve0").reshape(-1, 1)
    b_true = np.asarray(A @ x_true).reshape(-1, 1)
    e = np.random.default_rng(81).standard_normal(b_true.shape)
    e *= 0.01 * np.linalg.norm(b_true) / np.linalg.norm(e)
    b = b_true + e
    xc, ic = quiet(CGLS, A, b, np.zeros((N, 1)), CGLS_ITS, 0, x_true=x_true)
    xh, ih = quiet(Hybrid_LSQR, A, b, HYB_ITS, HYB_LAM, x_true)
    save("deblur1d_bc_" + mode, psf=D1.PSF, n=N, x=x, Ax=Ax, ATx=ATx, x_true=x_true, b=b,
         cgls_max_iter=CGLS_ITS, cgls_x=xc, cgls_relError=ic["relError"], cgls_relResidual=ic["relResidual"], cgls_its=ic["its"],
         hlsqr_n_iter=HYB_ITS, hlsqr_lam=HYB_LAM, hlsqr_x=xh, hlsqr_relError=ih["relError"])


if __name__ == "__main__":
    for m in MODES:
        deblur1d_bc(m)
