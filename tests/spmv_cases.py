"""Matrices and vectors of the CSR SpMV tests (csrc/spmv.hip), built from sizes and seeds alone: tests/test_spmv_cases_host.py
checks the fixtures themselves on the CPU, tests/test_gpu_spmv_accuracy.py runs them through the device kernel.

k_csr_group<G> takes another path with the length of a row relative to its G lanes per row (entry-per-lane form, G = 2 / 4:
an 8-deep pipelined loop with a `more` branch from its second trip on, a 4-in-flight loop, a predicated tail of <= 3 entries per
lane; quad form, G = 8 / 16: two quads in flight, one odd quad, a tail of <= 3 entries on lanes 0 .. 2), and csr_upload picks G from
the MEAN row length.  So a matrix that is to reach every path of one G needs rows of every length next to a mean that stays in
that G's band: ladder().

Exact operands: values k / 64 (k a non-zero integer, |k| <= 64), vectors of integers in [-31, 31].  Every product is a multiple of
1 / 64, and while 64 * sum_j |a_ij| |x_j| < 2^24 (exact_margin) every partial sum of a row, in ANY order, is a multiple of 1 / 64
below 2^24 / 64, a float32: the kernel's fp32 chains, its float64 sum across the group and the rounding of the result are all
exact, and the device result equals the float64 product entry for entry, to the bit.
"""
import functools
import math

import numpy as np
import scipy.sparse as sp

NT = 256                       # threads of a workgroup of k_csr_group
LADDER_TOP = 323               # 20 * 16 + 3: the longest row of a ladder
#: G -> (filler rows, their length): what holds the mean row length of a ladder inside the band of G
FILLER = {2: (4000, 1), 4: (3000, 16), 8: (1200, 32), 16: (0, 0)}


def expected_group(M):
    """The lanes per row csr_upload chooses for the CSR matrix M: the largest power of two not above a quarter of the mean row
    length, 2 .. 16 (restated here; used only to assert that a case sits in the band it was built for)."""
    nrows, nnz = M.shape[0], M.nnz
    group = 2
    while group < 16 and 8 * group * nrows <= nnz:
        group *= 2
    return group


def grid_blocks(nrows, G):
    """Workgroups of an apply before the caps (sp_apply): one group of G lanes per row."""
    return max(1, -(-nrows * G // NT))


def dyadic_values(rng, n):
    """n values k / 64, k a non-zero integer in [-64, 64]."""
    return rng.integers(1, 65, n) * rng.choice(np.array([-1.0, 1.0]), n) / 64.0


def uniform_values(rng, n):
    """n values U(-1, 1), rounded to float32 (held as float64)."""
    return rng.uniform(-1.0, 1.0, n).astype(np.float32).astype(np.float64)


def int_vector(n, seed):
    """n integers in [-31, 31] as float32."""
    return np.random.default_rng(seed).integers(-31, 32, n).astype(np.float32)


def normal_vector(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def exact_margin(M, x):
    """64 * max_i sum_j |a_ij| |x_j|: below 2^24 every order of summation of M x is exact in float32 (module docstring)."""
    if M.nnz == 0:
        return 0.0
    return 64.0 * float((abs(M) @ np.abs(np.asarray(x, dtype=np.float64))).max())


def from_lengths(lengths, ncols, seed, unused=(), values=dyadic_values):
    """CSR matrix whose row r holds lengths[r] entries in distinct, sorted columns drawn from all columns but `unused`."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    allowed = np.setdiff1d(np.arange(ncols, dtype=np.int32), np.asarray(unused, dtype=np.int32))
    assert lengths.max(initial=0) <= allowed.size
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    indices = np.empty(int(indptr[-1]), dtype=np.int32)
    for r, n in enumerate(lengths):
        if n:
            indices[indptr[r]:indptr[r + 1]] = np.sort(rng.choice(allowed, int(n), replace=False, shuffle=False))
    M = sp.csr_matrix((values(rng, indices.size), indices, indptr), shape=(lengths.size, ncols))
    M.has_sorted_indices = True
    return M


def ladder_lengths(G, seed):
    """Every length 0 .. LADDER_TOP once, shuffled among the filler rows of G; the longest row last."""
    nfill, flen = FILLER[G]
    lengths = np.concatenate([np.arange(LADDER_TOP + 1), np.full(nfill, flen)]).astype(np.int64)
    rng = np.random.default_rng(1000 + seed)
    lengths = lengths[rng.permutation(lengths.size)]
    top = int(np.flatnonzero(lengths == LADDER_TOP)[0])                # (the fillers are shorter: one such row)
    lengths[top], lengths[-1] = lengths[-1], lengths[top]
    return lengths


def ladder(G, ncols=1500, seed=0, unused=(), values=dyadic_values):
    """The rows of every length 0 .. 323 among the filler that makes csr_upload choose G lanes per row: an empty row, rows
    shorter than G, every residue of the length modulo 4 G and 8 G, the pipelined loop's entry and its second and third trips,
    odd and even quad counts, every tail length, neighbouring groups of a wave with very different trip counts."""
    return from_lengths(ladder_lengths(G, seed), ncols, seed, unused, values)


def banded(nrows, ncols, row_len, seed):
    """nrows rows of row_len entries each, row r in columns (7 r + 13 t) mod ncols, t < row_len (13 coprime to ncols: distinct),
    values k / 64: structured, for the sizes above the grid caps."""
    assert math.gcd(13, ncols) == 1 and row_len <= ncols
    rng = np.random.default_rng(seed)
    idx = (7 * np.arange(nrows, dtype=np.int64)[:, None] + 13 * np.arange(row_len, dtype=np.int64)[None, :]) % ncols
    M = sp.csr_matrix((dyadic_values(rng, nrows * row_len), idx.astype(np.int32).reshape(-1),
                       np.arange(nrows + 1, dtype=np.int64) * row_len), shape=(nrows, ncols))
    M.sort_indices()
    return M


# ------------------------------------------------------------------------------------------------------------------ the cases
#: columns no row of a "poison" ladder refers to (column 0: the index a predicated-off lane substitutes)
POISON_COLS = (0, 1, 7, 64, 700, 1499)
#: row lengths of the small grid-edge matrices, per G: uniform in [lo, hi], the mean in the middle of the band of G
GRID_LENGTHS = {2: (0, 12), 4: (17, 30), 8: (34, 60), 16: (70, 200)}
#: kind -> G -> rows, such that ceil(rows * G / 256) is 8 and 16 (the XCD permutation of the block index is on, spans of one trip),
#: 9 (permutation off), 8 with a ragged last span (rows no multiple of 256 / G), and fewer rows than one trip of a workgroup
GRID_ROWS = {"grid8": {2: 1024, 4: 512, 8: 256, 16: 128}, "grid16": {2: 2048, 4: 1024, 8: 512, 16: 256},
             "grid9": {2: 1100, 4: 570, 8: 280, 16: 140}, "ragged8": {2: 1001, 4: 489, 8: 243, 16: 121},
             "tiny": {2: 5, 4: 5, 8: 5, 16: 5}}
GRID_BLOCKS = {"grid8": 8, "grid16": 16, "grid9": 9, "ragged8": 8, "tiny": 1}
#: kind -> G -> lanes per row of the transpose (900 rows of whatever lengths the transposition gives)
GRID_GT = {"grid8": {2: 2, 4: 2, 8: 2, 16: 4}, "grid16": {2: 2, 4: 4, 8: 4, 16: 8}, "grid9": {2: 2, 4: 2, 8: 2, 16: 4},
           "ragged8": {2: 2, 4: 2, 8: 2, 16: 4}, "tiny": {2: 2, 4: 2, 8: 2, 16: 2}}


def _grid_case(G, kind):
    nrows = GRID_ROWS[kind][G]
    lo, hi = GRID_LENGTHS[G]
    rng = np.random.default_rng(100 * G + nrows)
    return from_lengths(rng.integers(lo, hi + 1, nrows), 900, 7 * G + nrows)


def _with_explicit_zeros(M, seed):
    M = M.copy()
    M.data[np.random.default_rng(seed).random(M.nnz) < 0.2] = 0.0       # stored entries of value 0: they stay in the structure
    return M


#: name -> (builder, G of the matrix, G of its transpose)
CASES = {}
for _G, _Gt in ((2, 8), (4, 16), (8, 8), (16, 8)):
    CASES[f"ladder_g{_G}"] = (functools.partial(ladder, _G, seed=_G), _G, _Gt)
    CASES[f"poison_g{_G}"] = (functools.partial(ladder, _G, seed=10 + _G, unused=POISON_COLS), _G, _Gt)
    CASES[f"general_g{_G}"] = (functools.partial(ladder, _G, seed=20 + _G, values=uniform_values), _G, _Gt)
for _kind in GRID_ROWS:
    for _G in (2, 4, 8, 16):
        CASES[f"{_kind}_g{_G}"] = (functools.partial(_grid_case, _G, _kind), _G, GRID_GT[_kind][_G])
CASES["zeros_g4"] = (lambda: _with_explicit_zeros(ladder(4, seed=34), 35), 4, 16)
CASES["one_row"] = (lambda: from_lengths([5000], 5000, 41), 16, 2)                    # 1 x 5000, full
CASES["one_column"] = (lambda: from_lengths([5000], 5000, 41).T.tocsr(), 2, 16)       # its 5000 x 1 transpose
CASES["empty"] = (lambda: sp.csr_matrix((37, 53), dtype=np.float64), 2, 2)            # nnz = 0
# above the caps of the grid (16 workgroups per CU: 4096 on 256 CUs; 1024 with a fused sumsq)
CASES["banded_2"] = (lambda: banded(600_000, 600_001, 2, 51), 2, 2)                   # 4688 workgroups uncapped, grid-stride
CASES["banded_64"] = (lambda: banded(70_000, 69_999, 64, 52), 16, 16)                 # 4375 uncapped, spans; 4.5 M non-zeros
CASES["banded_2_mid"] = (lambda: banded(140_000, 140_001, 2, 53), 2, 2)               # 1094: above the sumsq cap only

EXACT_CASES = [n for n in CASES if not n.startswith("general")]


@functools.lru_cache(maxsize=None)
def case(name):
    """The matrix of a case (built once per process; do not modify)."""
    return CASES[name][0]()


def case_vectors(name):
    """Exact input vectors (x for M, y for M^T) of a case."""
    M = case(name)
    seed = sum(name.encode())
    return int_vector(M.shape[1], seed), int_vector(M.shape[0], seed + 1)
