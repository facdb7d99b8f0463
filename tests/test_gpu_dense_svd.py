"""The device Jacobi SVD (csrc/dense_svd.hip) against its contract, at its block and chunk edges, at every scale and on structured
matrices; the path that does not converge; trk_dense_gemv_f64 entry by entry.  Matrices and checks: tests/dense_svd_cases.py
(tests/test_dense_svd_cases_host.py runs the same checks on LAPACK's factors).  A case that should converge fails if it warns.
Each contract test prints its measured / bound ratios (`pytest -s`)."""
import ctypes
import warnings

import numpy as np
import pytest

import dense_svd_cases as C

pytestmark = pytest.mark.gpu

EPS = C.EPS
_DEVICE = {}


def _svd(A, **kw):
    """(U, S, Vh, sweeps) of _dense.svd_device as NumPy; a warning is an error."""
    from trips_py_amd import _dense
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        Ut, S, Vt, sweeps = _dense.svd_device(A, **kw)
    return Ut.T.cpu().numpy(), S.cpu().numpy(), Vt.cpu().numpy(), sweeps


def _named(name):
    if name not in _DEVICE:
        _DEVICE[name] = _svd(C.named(name))
    return _DEVICE[name]


def _contract(label, A, U, S, Vh, bound_utu):
    r_g, r_diag, r_utu = C.check_contract(A, U, S, Vh, bound_utu)
    print(f"contract {label}: |g_i.g_j| {r_g:.3f}  | |u_j|^2 - 1 | {r_diag:.3f}  U^T U - I "
          f"{'-' if r_utu is None else format(r_utu, '.3f')}  of bound")
    return r_g, r_diag, r_utu


# ------------------------------------------------------------------------------------------- A + B: the contract, the edges
@pytest.mark.parametrize("m,n", C.EDGE_SHAPES + C.WIDE_SHAPES, ids=lambda v: str(v))
def test_edge_shape(m, n):
    A = C.gaussian(m, n)
    U, S, Vh, _ = _svd(A)
    C.check_against_lapack(A, U, S, Vh)
    _contract(f"gauss {m} x {n}", A, U, S, Vh, True)


@pytest.mark.parametrize("name", ["gauss257x100", "gauss100x257", "graded300_1e-6", "graded300_1e-10", "graded300_1e-14", "blur576"])
def test_contract_named(name):
    A = C.named(name)
    U, S, Vh, sweeps = _named(name)
    C.check_against_lapack(A, U, S, Vh, vectors=C.NAMED[name][2])
    _contract(f"{name} ({sweeps} sweeps)", A, U, S, Vh, C.NAMED[name][1])


def _raw_svd(A, pad_a, pad_g, pad_v):
    """trk_dense_svd_f64 through ctypes with lda = m + pad_a, ldg = m + pad_g, ldv = npad + pad_v.  The padding rows of A hold NaN;
    G, V, S and the workspace are followed by one sentinel double.  -> (G^T (n, m), V^T (n, n), S, sweeps, sentinels)."""
    import torch
    from trips_py_amd import _dense, _lib
    eng = _dense._engine()
    m, n = A.shape
    npad, need = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(eng.lib.trk_dense_svd_f64_dims(m, n, ctypes.byref(npad), ctypes.byref(need)), "dims")
    npad, need = npad.value, need.value
    lda, ldg, ldv = m + pad_a, m + pad_g, npad + pad_v
    At = torch.full((n, lda), float("nan"), dtype=torch.float64, device=eng.device)
    At[:, :m] = torch.from_numpy(np.ascontiguousarray(A.T)).to(eng.device)
    sentinel = -12345.678
    G, V, S, work = (torch.full((size + 1,), sentinel, dtype=torch.float64, device=eng.device)
                     for size in (npad * ldg, npad * ldv, n, need))
    sweeps, conv = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(eng.lib.trk_dense_svd_f64(At.data_ptr(), m, n, lda, G.data_ptr(), ldg, V.data_ptr(), ldv, S.data_ptr(), work.data_ptr(),
                                         need, float(max(m, 64) * EPS), 30, ctypes.byref(sweeps), ctypes.byref(conv), eng.stream()),
               "trk_dense_svd_f64")
    torch.cuda.synchronize()
    assert conv.value == 1
    ends = [float(t[-1]) for t in (G, V, S, work)]
    return (G[:-1].view(npad, ldg)[:n, :m].cpu().numpy(), V[:-1].view(npad, ldv)[:n, :n].cpu().numpy(), S[:n].cpu().numpy(),
            sweeps.value, ends, sentinel)


def test_raw_abi_leading_dimensions():
    A = C.gaussian(129, 33)
    Gt0, Vt0, S0, sw0, ends0, sentinel = _raw_svd(A, 0, 0, 0)
    Gt1, Vt1, S1, sw1, ends1, _ = _raw_svd(A, 3, 5, 7)
    assert ends0 == [sentinel] * 4 and ends1 == [sentinel] * 4
    assert np.all(np.isfinite(Gt1)) and np.all(np.isfinite(Vt1)) and np.all(np.isfinite(S1))
    assert sw0 == sw1 and np.array_equal(Gt0, Gt1) and np.array_equal(Vt0, Vt1) and np.array_equal(S0, S1)
    order = np.argsort(-S0, kind="stable")
    C.check_against_lapack(A, (Gt0[order] / S0[order].reshape(-1, 1)).T, S0[order], Vt0[order])


# --------------------------------------------------------------------------------------------------------------- C: scale
@pytest.mark.parametrize("name", C.SCALE_CASES)
@pytest.mark.parametrize("k", [-600, -300, -60, 60, 300, 600])
def test_scale_equivariance_bit_for_bit(name, k):
    """Every threshold of the kernels is relative, the rotation parameters are ratios and a power of two commutes with every
    rounding: the factors of 2^k A are those of A, S times 2^k, in the same number of sweeps."""
    U0, S0, Vh0, sweeps0 = _named(name)
    U, S, Vh, sweeps = _svd(C.scaled(C.named(name), k))
    assert sweeps == sweeps0
    assert np.array_equal(S, np.ldexp(S0, k))
    assert np.array_equal(U, U0) and np.array_equal(Vh, Vh0)


@pytest.mark.parametrize("name", C.SCALE_CASES)
@pytest.mark.parametrize("k", [-600, 600])
def test_out_of_the_squaring_range(name, k):
    """Entries near 2^-600 have an all-zero Gram matrix and entries near 2^600 an infinite one."""
    from trips_py_amd.decompositions import svd
    A = C.scaled(C.named(name), k)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        U, S, Vh = svd(A)
    C.check_against_lapack(A, U, S, Vh)
    _contract(f"{name} x 2^{k}", A, U, S, Vh, C.NAMED[name][1])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_input_is_refused(bad):
    import torch
    from trips_py_amd.decompositions import gsvd, svd
    from trips_py_amd.solvers import Tikhonov, tSVD_sol
    A = C.gaussian(40, 17)
    L = C.gaussian(40, 17, 5)
    b = np.ones((40, 1))
    An, Ln = A.copy(), L.copy()
    An[7, 3] = bad
    Ln[39, 16] = bad
    with pytest.raises(ValueError, match="matrix A has a NaN or Inf"):
        svd(An)
    with pytest.raises(ValueError, match="matrix A has a NaN or Inf"):
        svd(torch.from_numpy(An.T.copy()).cuda())                                     # the wide path
    with pytest.raises(ValueError, match="matrix A has a NaN or Inf"):
        gsvd(An, L)
    with pytest.raises(ValueError, match="matrix L has a NaN or Inf"):
        gsvd(A, Ln)
    with pytest.raises(ValueError, match="matrix A has a NaN or Inf"):
        tSVD_sol(An, b, regparam=3)
    with pytest.raises(ValueError, match="matrix L has a NaN or Inf"):
        Tikhonov(A, b, Ln, None, regparam=0.1)
    svd(A), gsvd(A, L)                                                               # and the finite ones are accepted


# ---------------------------------------------------------------------------------------------------------- D: structure
def test_zero_matrix():
    A = C.zero()
    U, S, Vh, sweeps = _svd(A)
    assert sweeps == 1
    assert not np.any(S) and not np.any(U) and np.array_equal(Vh, np.eye(A.shape[1]))
    U, S, Vh, sweeps = _svd(A.T)
    assert sweeps == 1 and not np.any(S) and not np.any(Vh) and np.array_equal(U, np.eye(A.shape[1]))


def test_rank_one():
    A = C.named("rank_one")
    m, n = A.shape
    U, S, Vh, _ = _svd(A)
    C.check_against_lapack(A, U, S, Vh, vectors=False)
    assert np.all(S[1:] <= 8 * m * EPS * S[0])
    _contract("rank one", A, U, S, Vh, False)
    u, v = A[:, 0] / np.linalg.norm(A[:, 0]), A[0] / np.linalg.norm(A[0])
    assert abs(abs(U[:, 0] @ u) - 1) <= 64 * EPS and abs(abs(Vh[0] @ v) - 1) <= 64 * EPS


def test_diagonal_top_block():
    A = C.named("diag_top")
    U, S, Vh, sweeps = _svd(A)
    assert sweeps == 1
    C.check_diag_top(U, S, Vh)
    C.check_reconstruction(A, U, S, Vh)
    _contract("diag", A, U, S, Vh, False)


def test_repeated_singular_values():
    A = C.named("repeated")
    U, S, Vh, _ = _svd(A)
    C.check_against_lapack(A, U, S, Vh, vectors=False)
    assert np.max(np.abs(S - C.REPEATED_SIGMA)) <= 8 * 64 * EPS * 3
    C.check_rotation_orthogonal(A, U, Vh)
    _contract("repeated", A, U, S, Vh, True)


# ------------------------------------------------------------------------------------------------------ E: no convergence
def test_max_sweeps_reached_warns_and_keeps_the_invariants():
    from trips_py_amd import _dense
    A = C.gaussian(60, 40)
    with pytest.warns(RuntimeWarning, match="not converged after 1 Jacobi sweeps"):
        Ut, S, Vt, sweeps = _dense.svd_device(A, max_sweeps=1)
    assert sweeps == 1
    U, S, Vh = Ut.T.cpu().numpy(), S.cpu().numpy(), Vt.cpu().numpy()
    assert np.all(np.diff(S) <= 0)
    C.check_reconstruction(A, U, S, Vh)
    C.check_rotation_orthogonal(A, U, Vh)
    with pytest.raises(AssertionError):                                               # one sweep is not enough: the contract sees it
        C.check_contract(A, U, S, Vh, True)
    assert _svd(A)[3] > 1


# -------------------------------------------------------------------------------------------------------------- F: gemv
def _gemv_raw(trans, A, lda, x, d, alpha, beta, y0):
    """trk_dense_gemv_f64 through ctypes on a column-major A with leading dimension lda (padding rows NaN); y starts as y0 (NaN
    for beta = 0)."""
    import torch
    from trips_py_amd import _dense, _lib
    eng = _dense._engine()
    m, n = A.shape
    At = torch.full((n, lda), float("nan"), dtype=torch.float64, device=eng.device)
    At[:, :m] = torch.from_numpy(np.ascontiguousarray(A.T)).to(eng.device)
    xd = torch.from_numpy(x).to(eng.device)
    dd = None if d is None else torch.from_numpy(d).to(eng.device)
    y = torch.from_numpy(np.full_like(y0, np.nan) if beta == 0 else y0.copy()).to(eng.device)
    if lda == m:
        _dense.gemv(trans, At, m, n, xd, d=dd, alpha=alpha, beta=beta, y=y)
    else:
        _lib.check(eng.lib.trk_dense_gemv_f64(1 if trans else 0, m, n, At.data_ptr(), lda, xd.data_ptr(),
                                              0 if dd is None else dd.data_ptr(), float(alpha), float(beta), y.data_ptr(), eng.stream()),
                   "trk_dense_gemv_f64")
    return y.cpu().numpy()


@pytest.mark.parametrize("m,n", C.GEMV_SHAPES)
def test_gemv_entrywise(m, n):
    worst = 0.0
    for trans in (False, True):
        A, x, d0, y0 = C.gemv_operands(m, n, trans, m * 7 + n + trans)
        for lda in (m, m + 3):
            for d in (None, d0):
                for alpha, beta in C.GEMV_COEFFS:
                    got = _gemv_raw(trans, A, lda, x, d, alpha, beta, y0)
                    ref, bound = C.gemv_reference(trans, A, x, d, alpha, beta, y0)
                    assert np.all(np.isfinite(got)), (trans, lda, d is None, alpha, beta)
                    err = np.abs(got - ref)
                    assert np.all(err <= bound), (trans, lda, d is None, alpha, beta, float(np.max(err / np.maximum(bound, 1e-300))))
                    worst = max(worst, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))))
    print(f"gemv {m} x {n}: worst error / bound {worst:.3f}")


def test_gemv_refuses_an_aliased_y():
    import torch
    from trips_py_amd import _dense
    A = C.gaussian(17, 17)
    At = torch.from_numpy(np.ascontiguousarray(A.T)).cuda()
    x = torch.from_numpy(C.gaussian(17, 1).reshape(-1)).cuda()
    d = torch.from_numpy(C.gaussian(17, 1, 3).reshape(-1)).cuda()
    x0, d0 = x.clone(), d.clone()
    for trans in (False, True):
        with pytest.raises(ValueError, match="alias"):
            _dense.gemv(trans, At, 17, 17, x, y=x)
        with pytest.raises(ValueError, match="alias"):
            _dense.gemv(trans, At, 17, 17, x, d=d, beta=1.0, y=d)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and torch.equal(d, d0)
