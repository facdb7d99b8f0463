"""The CSR SpMV (csrc/spmv.hip, k_csr_group<G, KB, SUMSQ>) entry by entry against scipy in float64 on the same operands, on every
path a row's length, the launch and the batch select.  The matrices are those of tests/spmv_cases.py (checked on the CPU by
tests/test_spmv_cases_host.py).

Exact cases: values k / 64 and integer vectors, for which every summation order is exact in float32 (spmv_cases docstring): the
device result must EQUAL (M64 @ x64).astype(float32), `np.array_equal` — an entry dropped from, or counted twice in, a single row
changes that row's output by a multiple of 1 / 64 and fails, where a norm over the vector would not notice.

Which case reaches what (G lanes per row; "ladder" = rows of every length 0 .. 323, the longest one last):

  entry-per-lane form (G = 2, 4)   pipelined loop, first trip: rows of >= 7 G + 1;  second and later trips (`more`): >= 15 G + 1,
                                   23 G + 1 ...: ladder_g2 (up to 20 trips), ladder_g4 (up to 10); 4-in-flight loop and the
                                   predicated tail: every residue of the length modulo 4 G and 8 G, rows shorter than G, the
                                   empty row: the same ladders.  With KB > 1 columns the pipelined loop is not taken: the batch
                                   test runs the ladder's long rows through the 4-in-flight loop alone.
  quad form (G = 8, 16)            two quads in flight, the odd quad, the tail on lanes 0 .. 2: ladder_g8 (0 .. 80 quads of a
                                   row), ladder_g16, every quad count modulo 2 G and every tail length 0 .. 3
  both handles                     SparseOp(M) forward runs the ladder through the CSR of A, SparseOp(M.T) transposed through the
                                   CSR of A^T the host builds; the opposite direction of each (lengths as the transposition
                                   gives them: G = 8 / 16) is checked as exactly
  row map                          G = 2 grid-stride, G > 2 contiguous spans; grid of 8 and 16 workgroups (XCD permutation of the
                                   block index on, spans of one trip), 9 (off), 8 with a ragged last span, fewer rows than one
                                   trip, a single row of 5000, 5000 rows of one entry, no entry at all
  caps                             banded_2: 4688 workgroups wanted, 4096 run, second grid-stride trip; banded_64: 4375 wanted,
                                   spans of two trips; with sumsq both are capped at 1024 (banded_2_mid: 1094 wanted)
  predication                      poison_g*: x is NaN in column 0 (the index a predicated-off lane substitutes) and in other
                                   columns no row refers to
  batch                            15 columns = passes of 8, 4, 2, 1 with leading dimensions n + pad, m + pad
General operands (standard-normal x, U(-1, 1) values): a bound per entry from the kernel's arithmetic, see test_general_operands.
"""
import functools

import numpy as np
import pytest
import torch

import spmv_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GROUPS = [2, 4, 8, 16]


@functools.lru_cache(maxsize=None)
def op(name, transposed_handle=False):
    """SparseOp of a case (of its transpose: the same matrix through the other CSR of the handle), with the band it was built for."""
    from trips_py_amd.operators import SparseOp
    M = C.case(name)
    _, G, Gt = C.CASES[name]
    assert C.expected_group(M) == G and C.expected_group(M.T.tocsr()) == Gt
    Op = SparseOp(M.T if transposed_handle else M)
    assert Op.matrix.nnz == M.nnz                                       # (stored zeros are kept)
    return Op


@functools.lru_cache(maxsize=None)
def want(name, transpose):
    """(input, expected output) of a case's exact operands: scipy in float64, rounded to float32.  Shared: do not modify."""
    M = C.case(name)
    x, y = C.case_vectors(name)
    v, A = (y, M.T.tocsr()) if transpose else (x, M)
    return v, (A @ v.astype(np.float64)).astype(np.float32)


def run(Op, v, transpose=False, sumsq=None):
    """Op.apply on a host float32 vector ([n] or [batch, n]) into an output pre-filled with a sentinel; host float32 back."""
    dev = Op.engine.device
    nout = Op.shape[1] if transpose else Op.shape[0]
    out = torch.full(v.shape[:-1] + (nout,), SENTINEL, dtype=torch.float32, device=dev)
    Op.apply(torch.from_numpy(np.ascontiguousarray(v)).to(dev), out=out, transpose=transpose, sumsq=sumsq)
    return out.cpu().numpy()


def assert_exact(got, ref, M=None):
    """np.array_equal(got, ref), naming the rows that differ (of M, when given: with their lengths)."""
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32
    if not np.array_equal(got, ref):
        g2, r2 = got.reshape(-1, ref.shape[-1]), ref.reshape(-1, ref.shape[-1])
        col, row = np.nonzero(g2 != r2)
        rows = np.unique(row)
        lens = None if M is None else np.diff(M.indptr)[row[:8]]
        raise AssertionError(f"{rows.size} of {ref.shape[-1]} rows differ; (column, row) {list(zip(col[:8], row[:8]))}, row lengths "
                             f"{lens}, got {g2[col[:8], row[:8]]}, expected {r2[col[:8], row[:8]]}")


def check_both_directions(name, transposed_handle=False):
    """The case's matrix and its transpose applied to the exact operands, through SparseOp(M) or SparseOp(M.T)."""
    M = C.case(name)
    Op = op(name, transposed_handle)
    for tr in (False, True):                                            # tr: the product is with M^T
        v, ref = want(name, tr)
        assert np.all(np.isfinite(ref))
        assert_exact(run(Op, v, transpose=tr != transposed_handle), ref, M.T.tocsr() if tr else M)


# ------------------------------------------------------------------------------------------------------------------ ladders
@pytest.mark.parametrize("handle", ["A", "At"])
@pytest.mark.parametrize("G", GROUPS)
def test_ladder_exact_both_handles(G, handle):
    """Rows of every length 0 .. 323 for the group size G, through the CSR of A (SparseOp(M) forward) and through the CSR of A^T
    (SparseOp(M.T) transposed); the opposite direction of each handle as well."""
    check_both_directions(f"ladder_g{G}", transposed_handle=handle == "At")


@pytest.mark.parametrize("handle", ["A", "At"])
@pytest.mark.parametrize("G", GROUPS)
def test_unreferenced_columns_may_hold_nan(G, handle):
    """Column 0 and a few others occur in no row, and x is NaN there (for A^T: the entries of y at the empty rows of A).  A
    predicated-off lane substitutes index 0 and value 0: a load of x[0] multiplied by that zero would put NaN in every short row."""
    name = f"poison_g{G}"
    M = C.case(name)
    Op = op(name, handle == "At")
    x, y = (v.copy() for v in C.case_vectors(name))
    empty_rows = np.flatnonzero(np.diff(M.indptr) == 0)
    assert empty_rows.size >= 1 and not np.isin(M.indices, C.POISON_COLS).any()
    for tr, v, dead, A in ((False, x, np.array(C.POISON_COLS), M), (True, y, empty_rows, M.T.tocsr())):
        clean = v.astype(np.float64)
        clean[dead] = 0.0
        ref = (A @ clean).astype(np.float32)
        v[dead] = np.nan
        got = run(Op, v, transpose=tr != (handle == "At"))
        assert np.all(np.isfinite(got)), np.flatnonzero(~np.isfinite(got))[:8]
        assert_exact(got, ref, A)


# ------------------------------------------------------------------------------------------------- batch, leading dimensions
@pytest.mark.parametrize("pad", [1, 5])
@pytest.mark.parametrize("G", [2, 16])
def test_batch_of_15_with_padded_leading_dimensions(G, pad):
    """15 columns (passes of 8, 4, 2 and 1) from a [15, n + pad] buffer into a [15, m + pad] buffer, both directions: every column
    exact, the output's pad untouched (the input's pad is NaN: not read)."""
    name = f"ladder_g{G}"
    M = C.case(name)
    Op = op(name)
    dev = Op.engine.device
    rng = np.random.default_rng(G + pad)
    for tr, A in ((False, M), (True, M.T.tocsr())):
        nout, nin = A.shape
        X = rng.integers(-31, 32, (15, nin)).astype(np.float32)
        assert max(C.exact_margin(A, X[j]) for j in range(15)) < 2 ** 24
        ref = np.stack([(A @ X[j].astype(np.float64)).astype(np.float32) for j in range(15)])
        xbuf = torch.full((15, nin + pad), float("nan"), dtype=torch.float32, device=dev)
        xbuf[:, :nin] = torch.from_numpy(X).to(dev)
        ybuf = torch.full((15, nout + pad), SENTINEL, dtype=torch.float32, device=dev)
        res = Op.apply(xbuf[:, :nin], out=ybuf[:, :nout], transpose=tr)
        assert res.data_ptr() == ybuf.data_ptr() and res.stride(0) == nout + pad
        got = ybuf.cpu().numpy()
        assert np.all(got[:, nout:] == SENTINEL)
        assert_exact(got[:, :nout], ref, A)


# ------------------------------------------------------------------------------------------------------------------ sumsq
@pytest.mark.parametrize("batch", [1, 3, 15])
@pytest.mark.parametrize("name", ["ladder_g4", "ladder_g16", "banded_2_mid"])
def test_fused_sumsq_is_the_sum_over_all_columns(name, batch):
    """The fused scalar of an apply of `batch` columns is sum(out^2) over ALL of them (trk.h), both directions: on small grids and on
    one whose uncapped grid (1094 workgroups) exceeds the 1024 partials a reduction may leave."""
    M = C.case(name)
    Op = op(name)
    S = Op.engine.scalars(2)
    rng = np.random.default_rng(batch)
    for tr, A in ((False, M), (True, M.T.tocsr())):
        X = rng.integers(-31, 32, (batch, A.shape[1])).astype(np.float32)
        ref = np.stack([(A @ X[j].astype(np.float64)).astype(np.float32) for j in range(batch)])
        S.set(0, np.array([-1.0, -1.0]))
        got = run(Op, X if batch > 1 else X[0], transpose=tr, sumsq=S.ref(int(tr)))
        assert_exact(got.reshape(batch, -1), ref, A)
        s = S.host()
        expect = float((ref.astype(np.float64) ** 2).sum())
        assert expect > 0 and s[1 - int(tr)] == -1.0
        assert np.isclose(s[int(tr)], expect, rtol=1e-10, atol=0.0), (s[int(tr)], expect)


# ------------------------------------------------------------------------------------------------------------------ grid edges
@pytest.mark.parametrize("kind", list(C.GRID_ROWS))
@pytest.mark.parametrize("G", GROUPS)
def test_grid_edges(G, kind):
    """ceil(rows G / 256) = 8 and 16 (block index permuted over the XCDs, spans of a single trip), 9 (not permuted), 8 with rows no
    multiple of 256 / G (a ragged last span), and fewer rows than one workgroup trip."""
    name = f"{kind}_g{G}"
    assert C.grid_blocks(C.case(name).shape[0], G) == C.GRID_BLOCKS[kind]
    check_both_directions(name)


@pytest.mark.parametrize("name", ["one_row", "one_column", "zeros_g4"])
def test_degenerate_shapes(name):
    """One row of 5000 non-zeros (one group of 16 lanes in a grid of one workgroup), its 5000 x 1 transpose, stored explicit zeros."""
    check_both_directions(name)
    check_both_directions(name, transposed_handle=True)


def test_matrix_without_entries_writes_zeros():
    """nnz = 0: the output is all zeros, not what the buffer held."""
    Op = op("empty")
    m, n = Op.shape
    x, y = C.case_vectors("empty")
    assert_exact(run(Op, x), np.zeros(m, dtype=np.float32))
    assert_exact(run(Op, y, transpose=True), np.zeros(n, dtype=np.float32))
    S = Op.engine.scalars(1)
    S.set(0, np.array([5.0]))
    assert_exact(run(Op, np.stack([x, x, x]), sumsq=S.ref(0)), np.zeros((3, m), dtype=np.float32))
    assert S.host()[0] == 0.0


# ------------------------------------------------------------------------------------------------------------------ above the caps
@pytest.mark.parametrize("name", ["banded_2", "banded_64"])
def test_above_the_grid_caps(name):
    """More groups than 16 workgroups per CU hold: G = 2 grid-strides a second trip, G = 16 runs spans of more than one trip; with
    the fused sumsq the grid is capped at 1024 and every workgroup runs several trips.  Both directions."""
    M = C.case(name)
    G = C.CASES[name][1]
    assert C.grid_blocks(M.shape[0], G) > 4096 and C.grid_blocks(M.shape[1], C.CASES[name][2]) > 4096
    check_both_directions(name)
    Op = op(name)
    S = Op.engine.scalars(2)
    for tr in (False, True):
        v, ref = want(name, tr)
        assert_exact(run(Op, v, transpose=tr, sumsq=S.ref(int(tr))), ref)
        expect = float((ref.astype(np.float64) ** 2).sum())
        assert np.isclose(S.host()[int(tr)], expect, rtol=1e-10, atol=0.0)


# ------------------------------------------------------------------------------------------------------------------ general operands
@pytest.mark.parametrize("handle", ["A", "At"])
@pytest.mark.parametrize("G", GROUPS)
def test_general_operands(G, handle):
    """Standard-normal x, values U(-1, 1), both rounded to float32; against float64 on the rounded operands, per entry:

        |y_i - ref_i| <= (ceil(len_i / 8) + 3) 2^-24 sum_j |a_ij| |x_j|

    A lane's chain holds at most ceil(len / (4 G)) + 1 <= ceil(len / 8) + 1 fused multiply-adds (one rounding each, G >= 2), the sum
    of the chains and of the group's lanes is float64, one rounding takes it to float32; the last unit covers the second-order
    terms and the float64 reference's own rounding.  Arithmetic, not a measurement."""
    name = f"general_g{G}"
    M = C.case(name)
    Op = op(name, handle == "At")
    worst = 0.0
    for tr, A in ((False, M), (True, M.T.tocsr())):
        v = C.normal_vector(A.shape[1], 100 + G + int(tr))
        ref = A @ v.astype(np.float64)
        lens = np.diff(A.indptr)
        bound = (np.ceil(lens / 8) + 3) * 2.0 ** -24 * (abs(A) @ np.abs(v.astype(np.float64)))
        got = run(Op, v, transpose=tr != (handle == "At")).astype(np.float64)
        err = np.abs(got - ref)
        ratio = float(np.max(err[bound > 0] / bound[bound > 0]))
        worst = max(worst, ratio)
        print(f"general_g{G} handle {handle} transpose {tr}: max error / bound {ratio:.3f}")
        over = np.flatnonzero(err > bound)
        assert over.size == 0, (over[:8], lens[over[:8]], err[over[:8]], bound[over[:8]])
        assert np.all(got[lens == 0] == 0.0)
    assert worst > 0.0                                                  # (inexact operands: some rounding has happened)
