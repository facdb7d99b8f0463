"""The host side of the matrix-free framelet operator (operators.framelet_analysis_matrix, band_tables, Framelet2D's checks) and the
fixtures of tests/framelet_cases.py, on the CPU: the band tables stand for exactly the matrices they were cut from, those matrices
are the reference's, the dyadic operands are exact in float32, and malformed matrices are refused before any device is touched."""
import numpy as np
import pytest
import scipy.sparse as sp

import framelet_cases as C
from conftest import load_golden, relerr
from trips_py_amd import operators as ops


@pytest.mark.parametrize("n,l", C.HOST_TABLE_CASES)
def test_band_tables_rebuild_the_matrix(n, l):
    """(blocks, half, band) of the real W_n puts every entry back where it was, to the bit; half is the level's (or what fits in n)."""
    W = ops.framelet_analysis_matrix(n, l)
    assert sp.issparse(W) and W.shape == ((2 * l + 1) * n, n)
    blocks, half, band = ops.band_tables(W, n)
    assert blocks == 2 * l + 1 and band.shape == (blocks, n, 2 * half + 1) and band.dtype == np.float64
    assert half == min(C.HALF[l], n - 1)
    assert np.array_equal(C.band_dense(blocks, half, band, n), W.toarray())
    # the restated construction of the test helper is the library's
    assert np.array_equal(C.analysis_matrix(n, l).toarray(), W.toarray())
    # a given half-width wider than the matrix needs is honoured (zero columns on both sides)
    b2, h2, band2 = ops.band_tables(W, n, half=half + 2)
    assert (b2, h2) == (blocks, half + 2) and np.array_equal(band2[:, :, 2:-2], band) and not band2[:, :, :2].any() and not band2[:, :, -2:].any()


def test_rebuilt_kronecker_product_is_the_reference_matrix():
    g = load_golden("framelet_ops")
    tn, tm = ops.band_tables(ops.framelet_analysis_matrix(8, 2), 8), ops.band_tables(ops.framelet_analysis_matrix(6, 2), 6)
    K = np.kron(C.band_dense(*tm, 6), C.band_dense(*tn, 8))
    assert K.shape == g["dense_8_6_2"].shape and np.allclose(K, g["dense_8_6_2"], atol=1e-14)


@pytest.mark.parametrize("n,m,l", [(8, 6, 2), (12, 12, 1), (16, 10, 3)])
def test_rebuilt_operators_reproduce_the_recorded_actions(n, m, l):
    """W_n X W_m^T with the matrices rebuilt from the band tables against the reference's own Wx and W^T y."""
    g = load_golden("framelet_ops")
    Wn = sp.csr_matrix(C.band_dense(*ops.band_tables(ops.framelet_analysis_matrix(n, l), n), n))
    Wm = sp.csr_matrix(C.band_dense(*ops.band_tables(ops.framelet_analysis_matrix(m, l), m), m))
    assert relerr(C.forward64(Wn, Wm, g[f"x_{n}_{m}_{l}"], n, m), g[f"Wx_{n}_{m}_{l}"]) < 1e-13
    assert relerr(C.transpose64(Wn, Wm, g[f"y_{n}_{m}_{l}"], n, m), g[f"WTy_{n}_{m}_{l}"]) < 1e-13


@pytest.mark.parametrize("n,m,l", [s for s in C.EXACT_SHAPES if s[0] * s[1] < 100000])
def test_dyadic_operands_are_exact_in_float32(n, m, l):
    """The precondition of the GPU tests' np.array_equal: dyadic taps, integer vectors in [-8, 8], every partial sum below 2^24 units;
    the band tables of the dyadic matrices pass the structure checks (the kernels' interior stencil exists)."""
    Wn, Wm = C.dyadic_matrix(n, l), C.dyadic_matrix(m, l)
    for W, k in ((Wn, n), (Wm, m)):
        assert C.tap_unit(W) >= 1.0 / 128 and np.array_equal(W.data.astype(np.float32).astype(np.float64), W.data)
        blocks, half, band = ops.band_tables(W, k)
        assert half <= C.HALF[l] and np.array_equal(C.band_dense(blocks, half, band, k), W.toarray())
    for tr in (False, True):
        _, _, v, ref = C.exact_case(n, m, l, tr)
        assert v.dtype == np.float32 and np.array_equal(v, np.round(v)) and np.abs(v).max() <= 8
        assert C.exact_margin(Wn, Wm, v, n, m, tr) < 2 ** 24
        assert ref.dtype == np.float32 and np.array_equal(ref.astype(np.float64), (C.transpose64 if tr else C.forward64)(Wn, Wm, v, n, m))


@pytest.mark.parametrize("n,m,l", [s for s in C.EXACT_SHAPES if s[0] * s[1] >= 100000])
def test_large_exact_cases_keep_the_margin(n, m, l):
    """The two large images of the GPU tests: the same precondition (their matrices and references are checked by construction above)."""
    for tr in (False, True):
        Wn, Wm, v, _ = C.exact_case(n, m, l, tr)
        assert np.abs(v).max() <= 8 and C.exact_margin(Wn, Wm, v, n, m, tr) < 2 ** 24


def test_wide_batch_and_nt_store_shapes_reach_their_kernels():
    """The batch cases pass the tile threshold only through their batch, with at least 3 x 3 tiles of 64 x 8 (an interior one among
    them); the non-temporal case has 64 M output floats; their operands keep the margin."""
    for n, m, l in C.WIDE_BATCH_SHAPES:
        H = C.HALF[l]
        assert C.tile_columns(n, m) == C.TJ_SMALL and C.tile_columns(n, m, C.WIDE_BATCH) == C.TJ_LARGE
        assert n > 128 + H and 64 + 63 <= n - 1 - H and m > 16 and 8 >= H and 15 <= m - 1 - H
        Wn, Wm = C.dyadic_matrix(n, l), C.dyadic_matrix(m, l)
        for k in range(3):
            assert C.exact_margin(Wn, Wm, C.int_vector(n * m, 70 + k), n, m, False) < 2 ** 24
    n, m, l = C.NT_STORE_SHAPE
    assert (2 * l + 1) ** 2 * n * m >= C.NT_STORE_FLOATS > (2 * l + 1) ** 2 * (n - 1) * (m - 1)
    Wn, Wm = C.dyadic_matrix(n, l), C.dyadic_matrix(m, l)
    assert C.exact_margin(Wn, Wm, C.int_vector(n * m, 90), n, m, False) < 2 ** 24


@pytest.mark.parametrize("n,m,l", [(16, 10, 3), (33, 17, 1), (40, 24, 4)])
def test_sequential_float32_passes_are_exact_and_within_the_bound(n, m, l):
    """A guard on the fixtures, not on the kernel: two sequential float32 passes give the float64 result to the bit on the dyadic
    operands, and stay inside entry_bound on real taps and standard-normal vectors."""
    Wn, Wm = C.dyadic_matrix(n, l), C.dyadic_matrix(m, l)
    Rn, Rm = C.analysis_matrix(n, l), C.analysis_matrix(m, l)
    for tr in (False, True):
        _, _, v, ref = C.exact_case(n, m, l, tr)
        assert np.array_equal(C.two_pass_float32(Wn, Wm, v, n, m, tr), ref)
        z = C.normal_vector(v.size, 7 + int(tr))
        err = np.abs(C.two_pass_float32(Rn, Rm, z, n, m, tr).astype(np.float64) - (C.transpose64 if tr else C.forward64)(Rn, Rm, z, n, m))
        bound = C.entry_bound(Rn, Rm, z, n, m, tr)
        assert np.all(err <= bound) and err.max() > 0


def test_malformed_matrices_are_rejected():
    W = ops.framelet_analysis_matrix(12, 2).tolil()
    with pytest.raises(ValueError, match="multiple|blocks"):
        ops.band_tables(W[:-1], 12)
    with pytest.raises(ValueError):
        ops.band_tables(W, 11)
    # an entry outside the band of the level's half-width
    bad = W.copy()
    bad[12 + 6, 1] = 0.5
    with pytest.raises(ValueError, match="outside the band"):
        ops.band_tables(bad, 12, half=2)
    # ... and with the half-width taken from the matrix, it makes the interior rows differ
    with pytest.raises(ValueError, match="stencil"):
        ops.band_tables(bad, 12)
    # interior rows that are not one stencil, inside the band
    bad = W.copy()
    bad[24 + 5, 5] *= 1.5
    with pytest.raises(ValueError, match="stencil"):
        ops.band_tables(bad, 12)
    # boundary rows are free
    ok = W.copy()
    ok[24 + 1, 1] *= 1.5
    ok[11, 10] = 0.25
    ops.band_tables(ok, 12)


def test_level_beyond_the_kernels_limit_is_refused_on_the_host(monkeypatch):
    """Level 5 has half-width 11 > 7: ValueError naming the limit and the CSR form, before an engine is asked for."""
    def no_engine():
        raise AssertionError("no device work expected")
    monkeypatch.setattr(ops, "default_engine", no_engine)
    assert ops.band_tables(ops.framelet_analysis_matrix(64, 5), 64)[1] == 11
    for make in (lambda: ops.Framelet2D(64, 48, 5), lambda: ops.create_framelet_operator(64, 48, 5, matrix_free=True)):
        with pytest.raises(ValueError, match=r"limit of 7.*matrix_free=False"):
            make()
