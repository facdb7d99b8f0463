"""The float64 device SVD (csrc/dense_svd.hip) against LAPACK, and the direct solvers tSVD_sol / Tikhonov against the
reference's answers (tests/golden/direct_*.npz; the problems are rebuilt by tests/direct_cases.py)."""
import numpy as np
import pytest
import scipy.sparse as sps

import direct_cases as dc
from conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _svd(A):
    from trips_py_amd import _dense
    Ut, S, Vt, sweeps = _dense.svd_device(A)
    return Ut.T.cpu().numpy(), S.cpu().numpy(), Vt.cpu().numpy(), sweeps


def _random(m, n, seed):
    return np.random.default_rng(seed).standard_normal((m, n))


def _graded(n, seed, smallest=1e-14):
    rng = np.random.default_rng(seed)
    Q1 = np.linalg.qr(rng.standard_normal((n, n)))[0]
    Q2 = np.linalg.qr(rng.standard_normal((n, n)))[0]
    return (Q1 * np.geomspace(1.0, smallest, n)) @ Q2.T


def _check_against_lapack(A, vectors=True):
    m, n = A.shape
    k = min(m, n)
    U, S, Vh, sweeps = _svd(A)
    assert U.shape == (m, k) and S.shape == (k,) and Vh.shape == (k, n)
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(S)) and np.all(np.isfinite(Vh))
    if vectors:
        Ul, Sl, Vhl = np.linalg.svd(A, full_matrices=False)
    else:
        Sl = np.linalg.svd(A, compute_uv=False)
    assert np.all(np.diff(S) <= 0)
    assert np.max(np.abs(S - Sl)) <= 8 * max(m, n) * EPS * Sl[0]
    nA = np.linalg.norm(A)
    assert np.linalg.norm(A - (U * S) @ Vh) <= 1e-13 * np.sqrt(n) * nA
    V = Vh.T
    assert np.max(np.abs(V.T @ V - np.eye(k))) <= 1e-13 * np.sqrt(n)
    if vectors and k > 1:
        # singular vectors are compared where the singular value is separated from its neighbours by 1e-6 sigma_1: LAPACK's
        # vectors carry angles of order n eps sigma_1 / gap, so a gap relative to sigma_i itself would not make them comparable
        gap = np.full(k, np.inf)
        gap[1:] = np.minimum(gap[1:], Sl[:-1] - Sl[1:])
        gap[:-1] = np.minimum(gap[:-1], Sl[:-1] - Sl[1:])
        sel = gap >= 1e-6 * Sl[0]
        dots = np.abs(np.sum(Vh[sel] * Vhl[sel], axis=1))
        assert np.all(dots >= 1 - 1e-9), dots.min()
    return sweeps


@pytest.mark.parametrize("m,n", [(1, 1), (2, 2), (17, 17), (200, 200), (257, 100), (100, 257)])
def test_svd_shapes(m, n):
    _check_against_lapack(_random(m, n, m * 1000 + n))


def test_svd_graded_1000():
    sweeps = _check_against_lapack(_graded(1000, 4))
    assert sweeps <= 30


def test_svd_blur_2500():
    """The 50^2 blur (Gauss 9 x 9, spread 3): the matrix the large-scale demos densify."""
    _check_against_lapack(dc.blur2d_dense(50, (9, 9), (3.0, 3.0)))


def test_svd_4096():
    _check_against_lapack(_random(4096, 4096, 77), vectors=False)


def test_svd_rank_deficient_and_orthogonal():
    A = _random(60, 40, 5)
    A[:, 3] = 0.0
    A[:, 7] = A[:, 11]
    A[:, 30] = A[:, 11]
    U, S, Vh, _ = _svd(A)
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(S)) and np.all(np.isfinite(Vh))
    Sl = np.linalg.svd(A, compute_uv=False)
    assert np.max(np.abs(S - Sl)) <= 8 * 60 * EPS * Sl[0]
    assert np.count_nonzero(S <= 1e-13 * S[0]) == 3
    assert np.linalg.norm(A - (U * S) @ Vh) <= 1e-13 * np.sqrt(40) * np.linalg.norm(A)
    Q = np.linalg.qr(_random(96, 96, 6))[0]
    Uq, Sq, Vq, sweeps = _svd(Q)
    assert sweeps == 1
    assert np.max(np.abs(Sq - 1.0)) <= 1e-14


def test_svd_bitwise_reproducible():
    A = _graded(300, 9, 1e-10)
    a = _svd(A)
    b = _svd(A)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)


def test_svd_column_limit():
    from trips_py_amd.decompositions import svd
    import torch
    with pytest.raises(ValueError, match="8192"):
        svd(torch.zeros((8193, 8193), dtype=torch.float64, device="cuda"))


def test_decompositions_svd_formats():
    import torch
    from trips_py_amd.decompositions import svd
    A = _random(30, 20, 8)
    U, S, Vh = svd(A)
    Ut, St, Vht = svd(torch.from_numpy(A).cuda())
    assert isinstance(Ut, torch.Tensor) and Ut.device.type == "cuda"
    assert np.array_equal(U, Ut.cpu().numpy()) and np.array_equal(S, St.cpu().numpy())
    assert np.array_equal(svd(np.asmatrix(A))[1], S) and np.array_equal(svd(sps.csr_matrix(A))[1], S)


# ------------------------------------------------------------------------------------------------------------ solvers
def _problem(case):
    g = load_golden("direct_" + case)
    return g, dc.build(g), g["b"].reshape(-1, 1)


@pytest.mark.parametrize("case", ["deblur1d", "blur2d", "tall"])
@pytest.mark.parametrize("rp", ["gcv", "dp", "num"])
def test_tsvd_against_reference(case, rp):
    from trips_py_amd.solvers import tSVD_sol
    g, A, b = _problem(case)
    regparam = int(g["tsvd_num_p"]) if rp == "num" else rp
    x, k = tSVD_sol(A, b, regparam=regparam, **({"delta": float(g["delta"])} if rp == "dp" else {}))
    assert k == int(g[f"tsvd_{rp}_p"])
    xr = g[f"tsvd_{rp}_x"]
    assert x.shape == (A.shape[1], 1)
    assert np.linalg.norm(x.reshape(-1) - xr) <= 1e-10 * np.linalg.norm(xr)


@pytest.mark.parametrize("case,Lkind", [("deblur1d", "I"), ("deblur1d", "L"), ("blur2d", "I"), ("blur2d", "L")])
@pytest.mark.parametrize("rp", ["gcv", "dp", "num"])
def test_tikhonov_against_reference(case, Lkind, rp):
    from trips_py_amd.solvers import Tikhonov
    g, A, b = _problem(case)
    n = A.shape[1]
    L = np.eye(n) if Lkind == "I" else np.asarray(dc.regulariser(g).todense())
    tag = f"tikh_{Lkind}_{rp}"
    lam_ref, xr = float(g[tag + "_p"]), g[tag + "_x"]
    if rp != "num":
        _, lam = Tikhonov(A, b, L, None, regparam=rp, **({"delta": float(g["delta"])} if rp == "dp" else {}))
        if case == "blur2d" and Lkind == "L" and rp == "dp":
            # The reference's lambda is not compared here: its L has a null space (the constants) whose singular value LAPACK
            # returns as ~1e-16 instead of 0, so the reference takes its full-rank branch and scales a column of A by ~1e16 before
            # an SVD (discrepancy_principle.py:38-40); its lambda carries that rounding.  The engine splits the null space off
            # exactly, as the reference does for an L with fewer rows than columns; its lambda must meet the discrepancy.
            x, _ = Tikhonov(A, b, L, None, regparam=lam)
            np.testing.assert_allclose(np.linalg.norm(A @ x - b), 1.01 * float(g["delta"]), rtol=1e-8)
        else:
            np.testing.assert_allclose(lam, lam_ref, rtol=1e-8 if rp == "dp" else 1e-6)
    x, lam = Tikhonov(A, b, L, None, regparam=lam_ref)          # the solve at the reference's lambda
    assert lam == lam_ref and x.shape == (n, 1)
    assert np.linalg.norm(x.reshape(-1) - xr) <= 1e-10 * np.linalg.norm(xr)


def test_input_kinds_give_the_same_answer():
    import torch
    from trips_py_amd.operators import Blur1D, Blur2D
    from trips_py_amd.problems import gauss_psf, gauss_psf_1d
    from trips_py_amd.solvers import Tikhonov, tSVD_sol
    g, A, b = _problem("deblur1d")
    n = A.shape[1]
    L = dc.regulariser(g)
    ref_t = tSVD_sol(A, b, "gcv")
    ref_k = Tikhonov(A, b, np.asarray(L.todense()), None, "gcv")
    assert ref_t[1] == int(g["tsvd_gcv_p"])
    for Ak in (np.asmatrix(A), sps.csr_matrix(A), torch.from_numpy(A).cuda()):
        bk = torch.from_numpy(b).cuda() if isinstance(Ak, torch.Tensor) else b
        xt, kt = tSVD_sol(Ak, bk, "gcv")
        xk, lk = Tikhonov(Ak, bk, L, None, "gcv")
        if isinstance(xt, torch.Tensor):
            xt, xk = xt.cpu().numpy(), xk.cpu().numpy()
        assert kt == ref_t[1] and np.array_equal(xt, ref_t[0])
        assert lk == ref_k[1] and np.array_equal(xk, ref_k[0])
    # engine operators (fp32) are densified through todense(): the same answer as that dense matrix
    op = Blur1D(gauss_psf_1d(n, 30.0), n)
    assert np.array_equal(tSVD_sol(op, b, "gcv")[0], tSVD_sol(op.todense(), b, "gcv")[0])
    g2, A2, b2 = _problem("blur2d")
    op2 = Blur2D(gauss_psf((9, 9), (2.0, 3.0))[0], 24, 24)
    assert np.linalg.norm(op2.todense() - A2) <= 1e-6 * np.linalg.norm(A2)
    assert np.array_equal(Tikhonov(op2, b2, np.eye(576), None, 1e-3)[0], Tikhonov(op2.todense(), b2, np.eye(576), None, 1e-3)[0])


def test_direct_solver_imports():
    import importlib
    from trips_py_amd.solvers import Tikhonov, tSVD_sol
    assert importlib.import_module("trips_py_amd.solvers.tSVD").tSVD_sol is tSVD_sol
    assert importlib.import_module("trips_py_amd.solvers.Tikhonov").Tikhonov is Tikhonov


def test_missing_delta_raises_reference_exception():
    from trips_py_amd.solvers import Tikhonov, tSVD_sol
    A, b = np.eye(3), np.ones((3, 1))
    for call in (lambda: tSVD_sol(A, b, regparam="dp"), lambda: Tikhonov(A, b, np.eye(3), None, regparam="dp")):
        with pytest.raises(Exception) as ei:
            call()
        assert type(ei.value) is Exception and str(ei.value).startswith("A value for the noise level delta was not provided")
