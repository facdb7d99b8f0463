"""The fixtures of the CSR SpMV tests (tests/spmv_cases.py), checked on the CPU: every case sits in the band of mean row lengths
it was built for, in both directions; its exact operands satisfy the precondition under which every summation order is exact in
float32; the ladders hold every row length; the grid-edge cases give the workgroup counts they are named after."""
import numpy as np
import pytest

import spmv_cases as C


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_sits_in_its_band_both_directions(name):
    M = C.case(name)
    _, G, Gt = C.CASES[name]
    assert M.has_canonical_format or name == "empty"                    # distinct, sorted columns per row
    assert C.expected_group(M) == G
    assert C.expected_group(M.T.tocsr()) == Gt


@pytest.mark.parametrize("name", C.EXACT_CASES)
def test_exact_operands_precondition(name):
    """64 * max_i sum_j |a_ij| |x_j| < 2^24 for A and for A^T: values are multiples of 1 / 64 in [-1, 1], vectors integers in
    [-31, 31]."""
    M = C.case(name)
    x, y = C.case_vectors(name)
    assert np.array_equal(M.data * 64, np.round(M.data * 64)) and np.abs(M.data).max(initial=0) <= 1.0
    if not name.startswith("zeros"):
        assert np.all(M.data != 0)
    for v in (x, y):
        assert v.dtype == np.float32 and np.array_equal(v, np.round(v)) and np.abs(v).max() <= 31
    assert C.exact_margin(M, x) < 2 ** 24
    assert C.exact_margin(M.T.tocsr(), y) < 2 ** 24


@pytest.mark.parametrize("G", [2, 4, 8, 16])
def test_ladder_holds_every_row_length_once_among_its_filler(G):
    for name in (f"ladder_g{G}", f"poison_g{G}", f"general_g{G}"):
        M = C.case(name)
        lengths = np.diff(M.indptr)
        nfill, flen = C.FILLER[G]
        assert M.shape == (C.LADDER_TOP + 1 + nfill, 1500)
        counts = np.bincount(lengths, minlength=C.LADDER_TOP + 1)
        want = np.ones(C.LADDER_TOP + 1, dtype=np.int64)
        want[flen] += nfill
        assert np.array_equal(counts, want)
        assert lengths[-1] == C.LADDER_TOP                              # the matrix ends with a ladder row
        # shuffled: ladder rows are spread over the matrix, not one block of it
        where = np.flatnonzero(lengths != flen)
        per_quarter = np.bincount(4 * where // M.shape[0], minlength=4)
        assert per_quarter.min() >= C.LADDER_TOP // 8, per_quarter
    P = C.case(f"poison_g{G}")
    assert not np.isin(P.indices, C.POISON_COLS).any()
    assert np.count_nonzero(np.diff(P.indptr) == 0) >= 1                # the empty row: an unreferenced column of the transpose


@pytest.mark.parametrize("kind", list(C.GRID_ROWS))
@pytest.mark.parametrize("G", [2, 4, 8, 16])
def test_grid_edge_cases_give_their_workgroup_counts(G, kind):
    M = C.case(f"{kind}_g{G}")
    assert C.grid_blocks(M.shape[0], G) == C.GRID_BLOCKS[kind]
    if kind == "ragged8":
        assert M.shape[0] % (C.NT // G) != 0
    if kind == "tiny":
        assert M.shape[0] < C.NT // G


def test_cases_above_the_grid_caps():
    for name, rows, row_len, blocks in (("banded_2", 600_000, 2, 4688), ("banded_64", 70_000, 64, 4375), ("banded_2_mid", 140_000, 2, 1094)):
        M = C.case(name)
        assert M.shape[0] == rows and np.all(np.diff(M.indptr) == row_len)
        assert C.grid_blocks(rows, C.CASES[name][1]) == blocks
    assert C.grid_blocks(600_000, 2) > 4096 and C.grid_blocks(70_000, 16) > 4096 and 1024 < C.grid_blocks(140_000, 2) < 4096
    Z = C.case("zeros_g4")
    assert np.count_nonzero(Z.data == 0) > Z.nnz // 10 and Z.T.tocsr().nnz == Z.nnz     # explicit zeros stay stored
    assert C.case("empty").nnz == 0
    assert C.case("one_row").shape == (1, 5000) and C.case("one_row").nnz == 5000
    assert C.case("one_column").shape == (5000, 1) and C.case("one_column").nnz == 5000


def test_sequential_float32_accumulation_is_exact_on_a_ladder():
    """A guard on the fixture, not on the kernel: row by row, entry by entry in float32, the exact operands give the float64
    product to the bit."""
    M = C.case("ladder_g16")
    x, _ = C.case_vectors("ladder_g16")
    vals = M.data.astype(np.float32)
    assert np.array_equal(vals.astype(np.float64), M.data)
    got = np.zeros(M.shape[0], dtype=np.float32)
    for r in range(M.shape[0]):
        acc = np.float32(0)
        for p in range(M.indptr[r], M.indptr[r + 1]):
            acc = np.float32(acc + np.float32(vals[p] * x[M.indices[p]]))
        got[r] = acc
    want = M @ x.astype(np.float64)
    assert np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(got, want.astype(np.float32))
