"""Host side of the direct solvers: the GCV truncation rules (gcv.py:96-123, gcvtype='tsvd' / 'tgsvd') against the reference's
indices and against hand-computed cases, and the fixtures' problems rebuilt from their parameters (tests/direct_cases.py)
against the singular values of the reference's matrices (tests/golden/direct_*.npz, tools/make_direct_goldens.py)."""
import numpy as np
import pytest

import direct_cases as dc
from conftest import load_golden
from trips_py_amd.reg_param import generalized_crossvalidation
from trips_py_amd.reg_param.gcv import truncation_gcv

CASES = ["deblur1d", "blur2d", "tall"]


@pytest.mark.parametrize("case", CASES)
def test_fixture_problem_rebuilds(case):
    g = load_golden("direct_" + case)
    A = dc.build(g)
    assert A.shape == tuple(int(v) for v in g["shape"])
    sv = np.linalg.svd(A, compute_uv=False)
    assert np.max(np.abs(sv - g["sv"])) <= 1e-12 * g["sv"][0]


@pytest.mark.parametrize("case", CASES)
def test_gcv_tsvd_index_full_u(case):
    g = load_golden("direct_" + case)
    m, n = (int(v) for v in g["shape"])
    bhat = g["gcv_tsvd_bhat"]
    assert bhat.size == m
    k = generalized_crossvalidation(None, np.zeros((n, n)), bhat, gcvtype="tsvd")
    assert k == int(g["gcv_tsvd_k"]) == int(g["tsvd_gcv_p"])     # (the reference's tSVD_sol(regparam='gcv') chose the same)


@pytest.mark.parametrize("case", CASES)
def test_gcv_tsvd_index_thin_u(case):
    """A thin U: the entries of U^T b past column n enter only through their sum of squares and the row count."""
    g = load_golden("direct_" + case)
    m, n = (int(v) for v in g["shape"])
    bhat = g["gcv_tsvd_bhat"]
    k = generalized_crossvalidation(None, np.zeros((n, n)), bhat[:n], gcvtype="tsvd", resid2=float(np.sum(bhat[n:] ** 2)), fullsize=m)
    assert k == int(g["gcv_tsvd_k"])


def test_gcv_tsvd_hand_computed():
    """m = n = 6, bhat^2 = 9, 1, 1, .25, .25, .01: G(k) = sum_{j >= k} bhat_j^2 / (6 - k)^2 = 11.51/36, 2.51/25, 1.51/16,
    .51/9, .26/4, .01/1 -> k = 5.  With (6 - k - 1)^2 the minimum would be k = 3."""
    assert truncation_gcv(np.array([3.0, 1.0, 1.0, 0.5, 0.5, 0.1]), 6, "tsvd") == 5


def test_gcv_tsvd_ties_keep_the_larger_index():
    # equal values of G: the reference's list runs from k = n - 1 down, and min() keeps the first
    assert truncation_gcv(np.array([1.0, 0.0, 0.0, 0.0]), 4, "tsvd", rows=4) == 3


@pytest.mark.parametrize("j", [0, 1, 2])
def test_gcv_tgsvd_index(j):
    g = load_golden("direct_gcv_tgsvd")
    p, n = (int(v) for v in g[f"c{j}_pn"])
    assert generalized_crossvalidation(None, np.zeros((p, n)), g[f"c{j}_bhat"], gcvtype="tgsvd") == int(g[f"c{j}_index"])


def test_gcv_tgsvd_hand_computed():
    # p = n = 6: G(i) = sum_{j < 5-i} bhat_j^2 / (5-i)^2 = 18.03/25, 9.03/16, 0.03/9, 0.02/4, 0.01/1, 0/0 -> i = 2 (an index)
    assert truncation_gcv(np.array([0.1, 0.1, 0.1, 3.0, 3.0, 3.0]), 6, "tgsvd") == 2
    # zero numerators: 0/4, 0/1, 0/0 -> the first
    assert truncation_gcv(np.zeros(3), 3, "tgsvd") == 0
    # p = 2 < n = 4: G(i) = 3/1, 2/0, 1/1, 0/4 -> i = 3; the zero denominator sits inside the range and its inf does not win
    assert truncation_gcv(np.array([1.0, 1.0, 1.0, 1.0]), 4, "tgsvd", p=2) == 3


def test_gcv_rejects_bad_input():
    with pytest.raises(ValueError):
        truncation_gcv(np.ones(3), 4, "tsvd")
    with pytest.raises(ValueError):
        generalized_crossvalidation(None, np.zeros((3, 3)), np.ones(3), gcvtype="tsdv")
