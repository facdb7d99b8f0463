"""Shapes, matrices and vectors of the matrix-free framelet operator's tests (csrc/framelet2d.hip, operators.Framelet2D), built from
sizes and seeds alone: tests/test_framelet_host.py checks them on the CPU, tests/test_gpu_framelet.py runs them through the kernels.

The kernels' tiles (restated here; used only to place shapes): a workgroup is one wave of 64 lanes, lane <-> image row.  Forward: 64
rows x TJ columns; transpose: 64 - 2 H rows x TJ columns (H = 1, 2, 4, 7 for levels 1 .. 4: the half-width the kernel is built
for); TJ = 8 columns, 4 while the apply has fewer than 2048 tiles of 8.  A tile is interior — taps from the block's stencil instead
of the per-row table — when every row (column) it touches is at least H away from both ends.

Dyadic matrices: the reference's construction with sqrt(2)/4 replaced by 3/8.  A tap is then a product of one filter (k/4 or 3k/8)
and at most l - 2 low-pass filters (k/4) — the deepest level comes back without the low-pass product of the level above it — so
a multiple of u = 1/8 for l <= 2, 1/32 for l = 3, 1/128 for l = 4 (tap_unit).  With integer operands every product and partial sum of
the first pass is a multiple of u and of the second pass a multiple of u^2; while max(|W_n| |X| |W_m|^T) / u^2 < 2^24
(exact_margin) all of them, in ANY order, are float32 numbers, and the device result equals the float64 product entry for entry.
"""
import functools

import numpy as np
import scipy.sparse as sp

WAVE = 64
HALF = {1: 1, 2: 2, 3: 4, 4: 7}                 # level -> half-width of the 1-D analysis matrix (and the kernel's H)
TJ_LARGE, TJ_SMALL, SMALL_GRID_TILES = 8, 4, 2048
SQRT2_4 = np.sqrt(2) / 4

# the shapes (n, m, l) the issue fixes
FIXED_SHAPES = [(8, 6, 2), (12, 12, 1), (16, 10, 3), (3, 5, 3), (1, 9, 1), (33, 17, 1), (67, 130, 2), (130, 67, 3)]
# one per level: n and m one short of / one past a multiple of the forward tile (64 rows; 4 columns — 8 for the level-2 shape, whose
# 17 x 129 tiles of 8 are past SMALL_GRID_TILES), >= 3 tiles per axis so that interior, edge and ragged tiles all occur
TILE_SHAPES = [(191, 33, 1), (1025, 1031, 2), (193, 31, 3), (191, 49, 4)]
# the same for the transpose's row tile of 64 - 2 H rows (62, 60, 56, 50)
ADJ_TILE_SHAPES = [(187, 31, 1), (181, 17, 2), (169, 33, 3), (151, 47, 4)]
MULTI_WORKGROUP = (1024, 768, 2)
# the eight-column forward kernel at every level: small images (3 x 3 tiles of 64 x 8: interior, edge and ragged) whose batch of 228
# columns takes the apply past SMALL_GRID_TILES
WIDE_BATCH = 228
WIDE_BATCH_SHAPES = [(131, 17, 1), (133, 19, 2), (137, 23, 3), (143, 23, 4)]
# the non-temporal stores of the forward kernel: the smallest square level-4 image with 64 M output floats
NT_STORE_FLOATS = 64 << 20
NT_STORE_SHAPE = (911, 911, 4)
EXACT_SHAPES = FIXED_SHAPES + TILE_SHAPES + ADJ_TILE_SHAPES + [MULTI_WORKGROUP]
# real taps, per-entry bound: everything but the two large images (their float64 references with |W| cost seconds)
GENERAL_SHAPES = FIXED_SHAPES + [s for s in TILE_SHAPES + ADJ_TILE_SHAPES if s[0] * s[1] < 100000]
HOST_TABLE_CASES = [(8, 2), (6, 2), (12, 1), (16, 3), (10, 3), (3, 3), (1, 1), (40, 4)]      # (n, l)


def tile_columns(n, m, batch=1):
    """The TJ the launcher picks (fr_launch_h)."""
    return TJ_SMALL if -(-n // WAVE) * -(-m // TJ_LARGE) * batch < SMALL_GRID_TILES else TJ_LARGE


@functools.lru_cache(maxsize=None)
def analysis_matrix(n, l, c1=SQRT2_4):
    """The 1-D analysis matrix of level l, (2l+1) n x n CSR, with the high-pass (-1, 0, 1) filter scaled by c1
    (trips/utilities/operators.py:50-103 restated with that one constant as a parameter; c1 = sqrt(2)/4 is the reference)."""
    def construct_H(lev):
        e = np.ones((n,))
        H0 = (sp.spdiags(e, -lev, n, n) + sp.spdiags(2 * e, 0, n, n) + sp.spdiags(e, lev, n, n)).tolil()
        H1 = (sp.spdiags(-e, -lev, n, n) + sp.spdiags(e, lev, n, n)).tolil()
        H2 = (sp.spdiags(-e, -lev, n, n) + sp.spdiags(2 * e, 0, n, n) + sp.spdiags(-e, lev, n, n)).tolil()
        for jj in range(lev):
            H0[jj, lev - jj - 1] += 1
            H0[-jj - 1, -lev + jj] += 1
            H1[jj, lev - jj - 1] -= 1
            H1[-jj - 1, -lev + jj] += 1
            H2[jj, lev - jj - 1] -= 1
            H2[-jj - 1, -lev + jj] -= 1
        return H0.tocsr() / 4, H1.tocsr() * c1, H2.tocsr() / 4

    def analysis(level, w):
        if level == l:
            return sp.vstack(construct_H(level))
        H0, H1, H2 = construct_H(level)
        return sp.vstack((analysis(level + 1, H0), H1, H2)) * w

    W = sp.csr_matrix(analysis(1, 1))
    W.eliminate_zeros()
    return W


def dyadic_matrix(n, l):
    return analysis_matrix(n, l, 3.0 / 8.0)


def tap_unit(W):
    """The largest 2^-k of which every entry of W is a multiple."""
    u = 1.0
    while not np.array_equal(W.data / u, np.round(W.data / u)):
        u /= 2
        assert u >= 2.0 ** -20
    return u


def int_vector(size, seed, top=8):
    """Integers in [-top, top] as float32."""
    return np.random.default_rng(seed).integers(-top, top + 1, size).astype(np.float32)


def normal_vector(size, seed):
    return np.random.default_rng(seed).standard_normal(size).astype(np.float32)


def forward64(Wn, Wm, x, n, m):
    """vec_F(W_n X W_m^T) in float64 (x: [n m] or [batch, n m])."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        return np.stack([forward64(Wn, Wm, v, n, m) for v in x])
    return np.asarray((Wm @ np.asarray(Wn @ x.reshape(n, m, order="F")).T).T).reshape(-1, order="F")


def transpose64(Wn, Wm, y, n, m):
    """vec_F(W_n^T Y W_m) in float64."""
    y = np.asarray(y, dtype=np.float64)
    if y.ndim == 2:
        return np.stack([transpose64(Wn, Wm, v, n, m) for v in y])
    Y = y.reshape(Wn.shape[0], Wm.shape[0], order="F")
    return np.asarray((Wm.T @ np.asarray(Wn.T @ Y).T).T).reshape(-1, order="F")


def exact_margin(Wn, Wm, v, n, m, transpose):
    """max over the entries of (|W_n| |X| |W_m|^T) / (u_n u_m) (transpose: of |W_n|^T |Y| |W_m|): below 2^24 every partial sum of both
    passes, in any order, is a float32 (the first pass's sums are bounded by the same product, in coarser units)."""
    An, Am = abs(Wn), abs(Wm)
    top = (transpose64 if transpose else forward64)(An, Am, np.abs(v), n, m).max()
    return float(top) / (tap_unit(Wn) * tap_unit(Wm))


@functools.lru_cache(maxsize=None)
def exact_case(n, m, l, transpose):
    """(W_n, W_m, input, expected float32 output) of a shape's exact operands.  Shared: do not modify."""
    Wn, Wm = dyadic_matrix(n, l), dyadic_matrix(m, l)
    size = Wn.shape[0] * Wm.shape[0] if transpose else n * m
    v = int_vector(size, 1000 * n + 10 * m + l + int(transpose))
    ref = (transpose64 if transpose else forward64)(Wn, Wm, v, n, m)
    return Wn, Wm, v, ref.astype(np.float32)


def entry_bound(Wn, Wm, v, n, m, transpose):
    """The per-entry error bound of two float32 1-D passes on float32 input v against float64 (real taps):
    forward (T_n + T_m + 4) 2^-24 (|W_n| |X| |W_m|^T), T = the most non-zeros in a row of the 1-D matrix; transpose the same with
    the column counts and |W_n|^T |Y| |W_m|.  One rounding per tap, T fused multiply-adds per pass, one store between the passes."""
    def most(W):
        return int(np.diff((W.tocsc() if transpose else W.tocsr()).indptr).max())
    Tn, Tm = most(Wn), most(Wm)
    mag = (transpose64 if transpose else forward64)(abs(Wn), abs(Wm), np.abs(np.asarray(v, dtype=np.float64)), n, m)
    return (Tn + Tm + 4) * 2.0 ** -24 * mag


def band_dense(blocks, half, band, n):
    """The (blocks n) x n matrix a band table stands for."""
    D = np.zeros((blocks * n, n))
    for t in range(2 * half + 1):
        i = np.arange(n)
        c = i - half + t
        ok = (c >= 0) & (c < n)
        for b in range(blocks):
            D[b * n + i[ok], c[ok]] = band[b, i[ok], t]
    return D


def two_pass_float32(Wn, Wm, v, n, m, transpose):
    """The operator in sequential float32: each 1-D pass an entry-by-entry float32 accumulation over the row's (column's) non-zeros in
    ascending order, a float32 store between the passes — the arithmetic the bound of entry_bound is derived for."""
    def pass32(A, X):                                            # A sparse (r x k) float32 taps, X (k x c) float32 -> (r x c) float32
        A = sp.csr_matrix(A)
        out = np.zeros((A.shape[0], X.shape[1]), dtype=np.float32)
        vals = A.data.astype(np.float32).astype(np.float64)
        X = X.astype(np.float64)
        for r in range(A.shape[0]):
            acc = np.zeros(X.shape[1], dtype=np.float32)
            for p in range(A.indptr[r], A.indptr[r + 1]):
                acc = (acc + vals[p] * X[A.indices[p]]).astype(np.float32)     # (the product is exact in float64: one rounding, as fmaf)
            out[r] = acc
        return out
    v = np.asarray(v, dtype=np.float32)
    if not transpose:
        T = pass32(Wn, v.reshape(n, m, order="F"))
        return pass32(Wm, np.ascontiguousarray(T.T)).T.reshape(-1, order="F")
    Y = v.reshape(Wn.shape[0], Wm.shape[0], order="F")
    Z = pass32(Wm.T, np.ascontiguousarray(Y.T)).T
    return pass32(Wn.T, Z).reshape(-1, order="F")
