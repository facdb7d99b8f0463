#!/usr/bin/env python
"""Generate the direct-solver fixtures tests/golden/direct_*.npz by RUNNING THE REFERENCE: its Deblurring1D / Deblurring2D
operators, tSVD_sol, Tikhonov and the GCV truncation rules (gcv.py:96-123).

TEST TOOLING, NOT PRODUCT.  Run only where the reference checkout exists (TRIPS_REFERENCE, default /root/reference):

    python tools/make_direct_goldens.py

Like tools/make_goldens.py it puts tools/oracle_shim (stand-ins for the absent pylops / astra / h5py / resizeimage) and the
reference on sys.path and stores plain numbers: the problem's kind, sizes and seeds, b, delta, the singular values of the
reference's A, and the reference's x, k and lambda for regparam 'gcv', 'dp' and a number.  A is not stored: the tests rebuild
it (tests/direct_cases.py) and check the rebuild against the stored singular values.  Cases:
    deblur1d   the 1-D demo's problem: n = 200, Gauss sigma = 30, reflect; tSVD, Tikhonov with I and with the (n-1) x n difference
    blur2d     a 24^2 image, Gauss PSF 9 x 9 with spread (2, 3) (no tied singular values); tSVD, Tikhonov with I and with
               gen_first_derivative_operator_2D densified
    tall       a small parallel-beam system, 323 rows > 144 columns, no tied singular values; tSVD
    gcv_tgsvd  the 'tgsvd' GCV rule on hand-made projections (p = n with an interior minimum, p < n)
"""
import io
import os
import sys
import contextlib

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("TRIPS_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(HERE, "oracle_shim"))
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

np.int0 = np.intp  # removed in NumPy 2; Deblurring1D.py still uses it
import direct_cases as dc  # noqa: E402
from trips.solvers.tSVD import tSVD_sol  # noqa: E402
from trips.solvers.Tikhonov import Tikhonov  # noqa: E402
from trips.test_problems.Deblurring1D import Deblurring1D  # noqa: E402
from trips.test_problems.Deblurring2D import Deblurring2D  # noqa: E402
from trips.utilities import operators as refops  # noqa: E402
from trips.utilities.reg_param.gcv import generalized_crossvalidation  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*a, **k)


def run(out, tag, fn, numeric, delta):
    for rp in ("gcv", "dp", numeric):
        x, p = quiet(fn, rp, **({"delta": delta} if rp == "dp" else {}))
        key = rp if isinstance(rp, str) else "num"
        out[f"{tag}_{key}_x"] = np.asarray(x, dtype=np.float64).reshape(-1)
        out[f"{tag}_{key}_p"] = np.float64(p)
        print(f"  {tag:7s} {str(rp):6s} -> {float(p):.10g}")


def main():
    cases = {
        "deblur1d": dict(kind="blur1d", n=200, sigma=30.0, noise=0.02, xseed=0, eseed=11, k_num=20, lam_num=1e-2),
        "blur2d": dict(kind="blur2d", N=24, dim=np.array([9, 9]), spread=np.array([2.0, 3.0]), noise=0.01, xseed=5, eseed=12,
                       k_num=100, lam_num=1e-3),
        "tall": dict(kind="parallel_beam", N=12, n_angles=19, n_det=17, det_shift=0.29, noise=0.01, xseed=6, eseed=13, k_num=60),
    }
    for name, c in cases.items():
        print(name)
        if c["kind"] == "blur1d":
            D = Deblurring1D(CommitCrime=True)
            A = np.asarray(D.forward_Op_1D(parameter=c["sigma"], nx=c["n"]).todense())
            x_true = D.gen_xtrue(c["n"], "curve0").reshape(-1, 1)
            L = np.asarray(refops.gen_first_derivative_operator(c["n"]).todense())
        elif c["kind"] == "blur2d":
            D = Deblurring2D(CommitCrime=True)
            A = np.asarray(D.forward_Op(tuple(c["dim"]), tuple(c["spread"]), c["N"], c["N"]).todense())
            x_true = dc.test_image(c["N"], c["xseed"])
            L = np.asarray(refops.gen_first_derivative_operator_2D(c["N"], c["N"]).todense())
        else:
            A = dc.build(c)
            x_true = dc.test_image(c["N"], c["xseed"])
            L = None
        b_true = A @ x_true
        e = dc.noise(b_true.shape, c["noise"], np.linalg.norm(b_true), c["eseed"])
        b, delta = b_true + e, float(np.linalg.norm(e))
        out = dict(c, b=b.reshape(-1), delta=delta, shape=np.array(A.shape), sv=np.linalg.svd(A, compute_uv=False))
        run(out, "tsvd", lambda rp, **kw: tSVD_sol(A, b, regparam=rp, **kw), c["k_num"], delta)
        U, S, VT = np.linalg.svd(A)
        out["gcv_tsvd_bhat"] = (U.T @ b).reshape(-1)
        out["gcv_tsvd_k"] = np.int64(generalized_crossvalidation(U, S, VT, b, gcvtype="tsvd"))
        if L is not None:
            n = A.shape[1]
            run(out, "tikh_I", lambda rp, **kw: Tikhonov(A, b, np.eye(n), x_true, regparam=rp, **kw), c["lam_num"], delta)
            run(out, "tikh_L", lambda rp, **kw: Tikhonov(A, b, L, x_true, regparam=rp, **kw), c["lam_num"], delta)
        np.savez_compressed(os.path.join(OUT, f"direct_{name}.npz"), **{k: np.asarray(v) for k, v in out.items()})

    print("gcv tgsvd")
    out = {}
    hand = [np.array([0.1, 0.1, 0.1, 3.0, 3.0, 3.0]), np.array([2.0, 0.3, 1.0, 0.05, 0.5, 0.4, 0.02])]
    shapes = [(6, 6), (5, 7)]                               # (p, n) of R_L: p = n, and p < n (a zero denominator inside)
    rng = np.random.default_rng(100)
    hand.append(rng.standard_normal(40) * np.exp(-0.1 * np.arange(40)))
    shapes.append((30, 30))
    for j, (bh, (p, n)) in enumerate(zip(hand, shapes)):
        bvec = bh.reshape(-1, 1)
        idx = quiet(generalized_crossvalidation, np.eye(bvec.size), None, np.zeros((p, n)), bvec, gcvtype="tgsvd")
        out[f"c{j}_bhat"], out[f"c{j}_pn"], out[f"c{j}_index"] = bh, np.array([p, n]), np.int64(idx)
        print(f"  p={p} n={n} -> {idx}")
    np.savez_compressed(os.path.join(OUT, "direct_gcv_tgsvd.npz"), **out)


if __name__ == "__main__":
    main()
