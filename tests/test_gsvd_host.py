"""Host side of gsvd / tGSVD_sol: the reference-shaped import paths, the errors raised before the device is touched, the
comparison instrument `gsvd_numpy` (tests/gsvd_cases.py) against the reference's answers on the 1-D deblurring problem
(tests/golden/direct_tgsvd_deblur1d.npz, tools/make_gsvd_goldens.py), and what each case of the GPU tests states about itself."""
import importlib

import numpy as np
import pytest
import scipy.sparse as sps

import gsvd_cases as gc
from conftest import load_golden


def test_reference_shaped_imports():
    from trips_py_amd.decompositions import gsvd
    from trips_py_amd.solvers import tGSVD_sol
    assert importlib.import_module("trips_py_amd.solvers.tGSVD").tGSVD_sol is tGSVD_sol
    assert callable(gsvd)


@pytest.mark.parametrize("shapes", [((3, 4), (5, 4)), ((5, 4), (3, 4)), ((5, 4), (5, 3)), ((5, 0), (5, 0))])
def test_shape_violations_raise_before_the_device(shapes):
    from trips_py_amd.decompositions import gsvd
    from trips_py_amd.solvers import tGSVD_sol
    (m, n), (p, n2) = shapes
    A, L, b = np.ones((m, n)), np.ones((p, n2)), np.ones((m, 1))
    for kind in (np.asarray, np.asmatrix, sps.csr_matrix):
        with pytest.raises(ValueError, match="gsvd"):
            gsvd(kind(A), kind(L))
        with pytest.raises(ValueError, match="gsvd"):
            tGSVD_sol(kind(A), kind(L), b, regparam=1)


def test_not_a_matrix_raises_before_the_device():
    from trips_py_amd.decompositions import gsvd
    with pytest.raises(ValueError, match="2-D"):
        gsvd(np.ones(4), np.ones((4, 1)))


def test_missing_delta_raises_reference_exception():
    from trips_py_amd.solvers import tGSVD_sol
    with pytest.raises(Exception) as ei:
        tGSVD_sol(np.eye(3), np.eye(3), np.ones((3, 1)), regparam="dp")
    assert type(ei.value) is Exception and str(ei.value).startswith("A value for the noise level delta was not provided")


def test_gsvd_numpy_reproduces_the_reference_c():
    g = load_golden("direct_tgsvd_deblur1d")
    f = gc.case("deblur1d")[2]
    assert np.all(np.diff(g["c"]) >= 0)
    assert np.max(np.abs(f["c"] - g["c"])) <= 1e-12


@pytest.mark.parametrize("rp", ["gcv", "dp", "num"])
def test_gsvd_numpy_reproduces_the_reference_x(rp):
    g = load_golden("direct_tgsvd_deblur1d")
    x = gc.tgsvd_numpy(gc.case("deblur1d")[2], g["b"], int(g[rp + "_k"]))
    assert np.linalg.norm(x - g[rp + "_x"]) <= 1e-10 * np.linalg.norm(g[rp + "_x"])


def test_golden_problem_is_the_direct_fixture():
    g, d = load_golden("direct_tgsvd_deblur1d"), load_golden("direct_deblur1d")
    assert np.array_equal(g["b"], d["b"]) and float(g["delta"]) == float(d["delta"])
    assert int(g["num_k"]) == 150 and g["c"].shape == g["s"].shape == (200,)


@pytest.mark.parametrize("name", list(gc.CASES))
def test_case_is_what_it_states(name):
    A, L, f, cond = gc.case(name)
    (m, n), p = A.shape, L.shape[0]
    assert L.shape[1] == n and m >= n and p >= n
    # full column rank of [A; L], with room: the device refuses a pair at max(m + p, n) eps
    assert cond < 1e3
    assert int(np.sum(f["c"] > np.sqrt(0.5))) == gc.CASES[name][1]
    assert int(np.sum(f["s"] <= n * gc.EPS)) == gc.CASES[name][2]
    assert np.all(np.diff(f["c"]) >= 0)
    rA, rL = gc.residuals(A, L, f["G"], f["H"], f["X"])
    assert max(rA, rL) <= 1e-13 * np.sqrt(n)
    assert np.max(np.abs(f["Y"].T @ f["X"] - np.eye(n))) <= 1e-12 * cond
    if n >= 17:
        assert np.sum(gc.separated(f["c"])) * 3 >= n


def test_deblur1d_case_details():
    """What the issue records of this problem under NumPy: 78 columns with a separated c, a cluster below 1e-6."""
    f = gc.case("deblur1d")[2]
    assert int(np.sum(gc.separated(f["c"]))) == 78
    assert int(np.sum(f["c"] < 1e-6)) > 20


def test_blur2d_case_has_unequal_row_counts_and_a_null_vector():
    A, L, f, _ = gc.case("blur2d")
    assert A.shape == (576, 576) and L.shape == (1104, 576)
    assert np.max(np.abs(L @ np.ones(576))) == 0.0
