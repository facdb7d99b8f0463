"""The carried Jacobi (trk_dense_svd_carry_f64), the device GSVD built on it and tGSVD_sol: against the plain device SVD, against
the float64 NumPy restatement `gsvd_numpy` (tests/gsvd_cases.py) and against the reference's answers on the 1-D deblurring problem
(tests/golden/direct_tgsvd_deblur1d.npz).  Bounds, per case with M = [A; L], m + p rows, n columns, cond = cond(M):
    c, s and c^2 + s^2 - 1   8 (m + p) eps cond: the device SVD's bound on singular values (sigma_1 = 1 here) times the
                             conditioning through which errors of M's basis reach Q1
    Gram of G = U diag(c)    off-diagonal <= 1e-13 sqrt(n) (what Jacobi guarantees; U^T U itself is not tested at tiny c)
    V^T V - I                1e-13 sqrt(n) cond over the columns with s > n eps; the other columns of V are exactly zero
    residuals of A and L     relative to ||M||_F: max(10 x the reference's own (golden) or gsvd_numpy's, 1e-13 sqrt(n))
    columns of X             up to sign, 1e-9 relative, where c is 1e-6 away from its neighbours (at least a third of them)"""
import numpy as np
import pytest
import scipy.sparse as sps

import gsvd_cases as gc
from conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------------------------------------------- the carry entry point
def _plain(A):
    """trk_dense_svd_f64 unsorted: G^T (n, m), S, V^T (n, n) (row j = column j), sweeps."""
    import torch
    from trips_py_amd import _dense
    m, n = A.shape
    At = torch.from_numpy(np.ascontiguousarray(A.T)).cuda()
    Gt, S, Ct, sweeps = _dense.svd_carry_t(At, m, n, torch.eye(n, dtype=torch.float64, device="cuda"))
    # the identity companion IS the plain SVD: compare with the sorted factors of _svd_tall
    Ut, S2, Vt, sweeps2 = _dense._svd_tall(At, m, n)
    order = torch.sort(S, descending=True, stable=True)[1]
    assert sweeps == sweeps2
    assert torch.equal(S.index_select(0, order), S2) and torch.equal(Ct.index_select(0, order), Vt)
    return Gt.cpu().numpy(), S.cpu().numpy(), Ct.cpu().numpy(), sweeps


def _carry(A, C0):
    import torch
    from trips_py_amd import _dense
    m, n = A.shape
    out = _dense.svd_carry_t(torch.from_numpy(np.ascontiguousarray(A.T)).cuda(), m, n,
                             torch.from_numpy(np.ascontiguousarray(C0.T)).cuda())
    return out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy().T, out[3]


@pytest.fixture(scope="module")
def carry_problem():
    A = np.random.default_rng(257100).standard_normal((257, 100))
    return (A,) + _plain(A)


@pytest.mark.parametrize("nc", [300, 1])
def test_carry_returns_the_companion_times_v(carry_problem, nc):
    """Rows of the companion are rotated independently of one another and of G, by the rotations of the plain SVD.  So a
    companion whose rows are signed powers of two times unit vectors must come back as those multiples of V's rows bit for bit
    (scaling by a power of two commutes with every rounding), which is C0 V exactly; G, S and the sweep count must be the plain
    run's bits.  A Gaussian companion is compared with the float64 product C0 V, which rounds differently from the K = sweeps x
    rounds products by 32 x 32 rotations the kernel applies to a row: each costs at most 32 eps ||row||, hence 2 K 32 eps ||row||."""
    A, Gt, S, Vt, sweeps = carry_problem
    n = A.shape[1]
    V = Vt.T
    rng = np.random.default_rng(nc)
    pick, scale = rng.integers(0, n, nc), rng.choice([-4.0, -1.0, 0.5, 1.0, 8.0], nc)
    E = np.zeros((nc, n))
    E[np.arange(nc), pick] = scale
    Gt1, S1, C1, sw1 = _carry(A, E)
    assert sw1 == sweeps and np.array_equal(Gt1, Gt) and np.array_equal(S1, S)
    assert np.array_equal(C1, V[pick] * scale.reshape(-1, 1))
    C0 = rng.standard_normal((nc, n))
    Gt2, S2, C2, sw2 = _carry(A, C0)
    assert sw2 == sweeps and np.array_equal(Gt2, Gt) and np.array_equal(S2, S)
    rounds = 2 * ((n + 31) // 32) - 1
    bound = 2 * sweeps * rounds * 32 * EPS * np.linalg.norm(C0, axis=1, keepdims=True)
    err = np.abs(C2 - C0 @ V)
    print(f"carry nc={nc}: max err / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    again = _carry(A, C0)
    assert np.array_equal(again[0], Gt2) and np.array_equal(again[1], S2) and np.array_equal(again[2], C2)


def test_colnorm_of_a_row_range():
    import torch
    from trips_py_amd import _dense
    X = np.random.default_rng(3).standard_normal((7, 600))          # 7 columns of 600 rows
    got = _dense.colnorm(torch.from_numpy(X).cuda(), 5, 590).cpu().numpy()
    np.testing.assert_allclose(got, np.linalg.norm(X[:, 5:595], axis=1), rtol=600 * EPS)


# ------------------------------------------------------------------------------------------------------------- the GSVD
_DEVICE = {}


def _device(name):
    """The device's factors of a case, computed once: gsvd's U, V, X, C, S as NumPy, c, s, Y = X^-T and the sweep counts."""
    if name not in _DEVICE:
        from trips_py_amd.decompositions import gsvd_factors
        A, L = gc.case(name)[:2]
        (U, V, X, C, S), f = gsvd_factors(A, L)
        _DEVICE[name] = dict(U=U, V=V, X=X, C=C, S=S, c=np.diag(C).copy(), s=np.diag(S).copy(), Y=f.Yt.cpu().numpy().T,
                             sweeps=f.sweeps)
    return _DEVICE[name]


def _reference_residuals(name):
    if name == "deblur1d":
        g = load_golden("direct_tgsvd_deblur1d")
        return float(g["res_A"]), float(g["res_L"])
    A, L, f, _ = gc.case(name)
    return gc.residuals(A, L, f["G"], f["H"], f["X"])


@pytest.mark.parametrize("name", list(gc.CASES))
def test_gsvd_case(name):
    A, L, f, cond = gc.case(name)
    (m, n), p = A.shape, L.shape[0]
    d = _device(name)
    U, V, X, c, s = d["U"], d["V"], d["X"], d["c"], d["s"]
    assert U.shape == (m, n) and V.shape == (p, n) and X.shape == (n, n) and d["C"].shape == d["S"].shape == (n, n)
    assert np.array_equal(d["C"], np.diag(c)) and np.array_equal(d["S"], np.diag(s))
    for v in (U, V, X, c, s, d["Y"]):
        assert np.all(np.isfinite(v))
    bound = 8 * (m + p) * EPS * cond
    ec, es, e1 = np.max(np.abs(c - f["c"])), np.max(np.abs(s - f["s"])), np.max(np.abs(c * c + s * s - 1.0))
    G = U * c
    gram = G.T @ G
    eg = np.max(np.abs(gram - np.diag(np.diag(gram))))
    live = s > n * EPS
    ev = np.max(np.abs(V[:, live].T @ V[:, live] - np.eye(int(live.sum())))) if live.any() else 0.0
    rA, rL = gc.residuals(A, L, G, V * s, X)
    refA, refL = _reference_residuals(name)
    limA, limL = max(10 * refA, 1e-13 * np.sqrt(n)), max(10 * refL, 1e-13 * np.sqrt(n))
    eI = np.max(np.abs(d["Y"].T @ X - np.eye(n)))
    print(f"gsvd {name}: sweeps {d['sweeps']} J {int(np.sum(c > np.sqrt(0.5)))} | c {ec / bound:.3f} s {es / bound:.3f} "
          f"c2+s2 {e1 / bound:.3f} of bound | gram {eg / (1e-13 * np.sqrt(n)):.3f} | VtV {ev / (1e-13 * np.sqrt(n) * cond):.3f} | "
          f"resA {rA:.2e} ({rA / limA:.3f}) resL {rL:.2e} ({rL / limL:.3f}) | YtX-I {eI:.2e}")
    assert ec <= bound and es <= bound
    assert np.all(np.diff(c) >= 0)
    assert e1 <= bound
    assert eg <= 1e-13 * np.sqrt(n)
    assert ev <= 1e-13 * np.sqrt(n) * cond
    assert int(np.sum(~live)) == gc.CASES[name][2] and not np.any(V[:, ~live])
    assert not np.any(U[:, c <= n * EPS])
    assert rA <= limA and rL <= limL
    # Y = X^-T: ||Y_i|| <= 1 / sigma_min and ||X_j|| <= sigma_max, so the rounding of the two carried blocks meets as cond(M)
    assert eI <= 1e-13 * np.sqrt(n) * cond


@pytest.mark.parametrize("name", list(gc.CASES))
def test_gsvd_x_columns(name):
    f = gc.case(name)[2]
    X = _device(name)["X"]
    n = X.shape[0]
    sel = gc.separated(f["c"])
    if n >= 17:
        assert np.sum(sel) * 3 >= n
    Xd, Xn = X[:, sel], f["X"][:, sel]
    sign = np.sign(np.sum(Xd * Xn, axis=0))
    err = np.linalg.norm(Xd * sign - Xn, axis=0) / np.linalg.norm(Xn, axis=0)
    print(f"gsvd X {name}: {int(np.sum(sel))} of {n} columns, worst {np.max(err):.2e}")
    assert np.max(err) <= 1e-9


def test_gsvd_formats_and_reproducible():
    import torch
    from trips_py_amd.decompositions import gsvd
    A, L = gc.case("g40x40x17")[:2]
    host = gsvd(A, L)
    dev = gsvd(torch.from_numpy(A).cuda(), torch.from_numpy(L).cuda())
    for h, t in zip(host, dev):
        assert isinstance(h, np.ndarray) and isinstance(t, torch.Tensor) and t.device.type == "cuda"
        assert np.array_equal(h, t.cpu().numpy())
    for other in (gsvd(np.asmatrix(A), np.asmatrix(L)), gsvd(sps.csr_matrix(A), sps.csr_matrix(L))):
        for h, o in zip(host, other):
            assert np.array_equal(h, o)
    A, L = gc.case("deblur1d")[:2]
    for h, o in zip(gsvd(A, L), gsvd(A, L)):
        assert np.array_equal(h, o)


def test_rank_deficient_pair_raises():
    from trips_py_amd.decompositions import gsvd
    from trips_py_amd.solvers import tGSVD_sol
    A, L = (v.copy() for v in gc.case("g40x40x17")[:2])
    A[:, 11], L[:, 11] = A[:, 3], L[:, 3]
    with pytest.raises(ValueError, match="full column rank"):
        gsvd(A, L)
    with pytest.raises(ValueError, match="full column rank"):
        tGSVD_sol(A, L, np.ones((40, 1)), regparam=2)


# ------------------------------------------------------------------------------------------------------------ tGSVD_sol
@pytest.mark.parametrize("rp", ["gcv", "dp", "num"])
def test_tgsvd_against_reference(rp):
    from trips_py_amd.solvers import tGSVD_sol
    g = load_golden("direct_tgsvd_deblur1d")
    A, L = gc.case("deblur1d")[:2]
    b = g["b"].reshape(-1, 1)
    regparam = int(g["num_k"]) if rp == "num" else rp
    x, k = tGSVD_sol(A, L, b, regparam=regparam, **({"delta": float(g["delta"])} if rp == "dp" else {}))
    xr = g[rp + "_x"]
    print(f"tgsvd {rp}: k {k} (reference {int(g[rp + '_k'])}), error {np.linalg.norm(x.reshape(-1) - xr) / np.linalg.norm(xr):.2e}")
    assert k == int(g[rp + "_k"])
    assert x.shape == (A.shape[1], 1)
    assert np.linalg.norm(x.reshape(-1) - xr) <= 1e-10 * np.linalg.norm(xr)


def test_tgsvd_slice_semantics_of_k():
    from trips_py_amd.solvers import tGSVD_sol
    A, L, f, _ = gc.case("g40x40x17")
    b = np.random.default_rng(1).standard_normal((40, 1))
    for k in (0, 3, 17, 40, -2):
        x, kk = tGSVD_sol(A, L, b, regparam=k)
        xr = gc.tgsvd_numpy(f, b, k)
        assert kk == k and np.linalg.norm(x.reshape(-1) - xr) <= 1e-10 * max(np.linalg.norm(xr), 1e-300)


def test_tgsvd_input_kinds_give_the_same_answer():
    import torch
    from trips_py_amd.operators import Blur1D
    from trips_py_amd.problems import gauss_psf_1d
    from trips_py_amd.solvers import tGSVD_sol
    g = load_golden("direct_tgsvd_deblur1d")
    A, L = gc.case("deblur1d")[:2]
    b, n = g["b"].reshape(-1, 1), A.shape[1]
    ref = tGSVD_sol(A, L, b, "gcv")
    for Ak, Lk in ((np.asmatrix(A), np.asmatrix(L)), (sps.csr_matrix(A), sps.csr_matrix(L)),
                   (torch.from_numpy(A).cuda(), torch.from_numpy(L).cuda())):
        bk = torch.from_numpy(b).cuda() if isinstance(Ak, torch.Tensor) else b
        x, k = tGSVD_sol(Ak, Lk, bk, "gcv")
        if isinstance(x, torch.Tensor):
            assert x.device.type == "cuda"
            x = x.cpu().numpy()
        assert k == ref[1] and np.array_equal(x, ref[0])
    # engine operators (fp32) are densified through todense(): the same answer as that dense matrix
    op = Blur1D(gauss_psf_1d(n, 30.0), n)
    assert np.array_equal(tGSVD_sol(op, L, b, 150)[0], tGSVD_sol(op.todense(), L, b, 150)[0])
