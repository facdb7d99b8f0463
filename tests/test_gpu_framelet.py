"""The matrix-free framelet operator (csrc/framelet2d.hip, operators.Framelet2D) on the device, entry by entry.

Exact cases: dyadic analysis matrices and integer vectors in [-8, 8] (tests/framelet_cases.py; the precondition is checked on the
CPU, for every shape used here, by tests/test_framelet_host.py), for which every summation order is exact in float32: the device
result must EQUAL the float64 product rounded to float32, `np.array_equal` — a dropped or doubled tap changes an entry by a multiple of 1/4096 and fails, where a
norm over the vector would not notice.  Outputs go into buffers pre-filled with a sentinel, with a guard on both sides.

Which shape reaches what (forward tile 64 rows x TJ columns, transpose 64 - 2H rows x TJ columns, TJ = 4 below 2048 tiles of 8):
  all boundary          (3, 5, 3), (1, 9, 1): narrower than the band; (8, 6, 2) .. (33, 17, 1): one tile per axis or ragged ones
  interior + edge tiles TILE_SHAPES / ADJ_TILE_SHAPES (>= 3 tiles per axis, n and m one off a multiple of the tile), (67, 130, 2),
                        (130, 67, 3), (1024, 768, 2)
  TJ = 8                (1025, 1031, 2): 17 x 129 tiles of 8; WIDE_BATCH_SHAPES: 3 x 3 tiles x 228 columns, one per level
  non-temporal stores   NT_STORE_SHAPE (911, 911, 4): 64 M output floats (four columns per lane)
  H = 1, 2, 4, 7        one TILE_SHAPE and one ADJ_TILE_SHAPE per level
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import framelet_cases as C
from conftest import bar, load_golden, maxrel, relerr
from test_oracle_golden import lam_close

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 96


@functools.lru_cache(maxsize=None)
def dyadic_op(n, m, l):
    from trips_py_amd.operators import Framelet2D
    Op = Framelet2D.from_analysis(C.dyadic_matrix(n, l), C.dyadic_matrix(m, l), n, m)
    assert Op.shape == ((2 * l + 1) ** 2 * n * m, n * m) and (Op.n, Op.m, Op.l) == (n, m, None) and Op.streaming
    return Op


@functools.lru_cache(maxsize=None)
def real_op(n, m, l):
    from trips_py_amd.operators import Framelet2D
    Op = Framelet2D(n, m, l)
    assert Op.shape == ((2 * l + 1) ** 2 * n * m, n * m) and (Op.n, Op.m, Op.l) == (n, m, l) and not Op.native_axpby
    return Op


def run_guarded(Op, v, transpose):
    """Op.apply on a host float32 vector into the middle of a sentinel-filled buffer; the guards on both sides must survive."""
    dev = Op.engine.device
    nout = Op.shape[1] if transpose else Op.shape[0]
    buf = torch.full((GUARD + nout + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    Op.apply(torch.from_numpy(np.ascontiguousarray(v)).to(dev), out=buf[GUARD:GUARD + nout], transpose=transpose)
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + nout:] == SENTINEL), "a guard region was written"
    return got[GUARD:GUARD + nout]


def assert_exact(got, ref, n, m, l, transpose):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32
    if not np.array_equal(got, ref):
        k = np.flatnonzero(got != ref)
        rows = n if transpose else (2 * l + 1) * n
        where = [(int(i % rows), int(i // rows)) for i in k[:8]]
        raise AssertionError(f"{k.size} of {ref.size} entries differ; (row, column) {where}: got {got[k[:8]]}, expected {ref[k[:8]]}")


# ------------------------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("transpose", [False, True], ids=["fwd", "adj"])
@pytest.mark.parametrize("n,m,l", C.EXACT_SHAPES)
def test_exact_entry_for_entry(n, m, l, transpose):
    Op = dyadic_op(n, m, l)
    _, _, v, ref = C.exact_case(n, m, l, transpose)
    got = run_guarded(Op, v, transpose)
    assert not np.any(got == SENTINEL) or np.any(ref == SENTINEL)          # (every entry written)
    assert_exact(got, ref, n, m, l, transpose)


@pytest.mark.parametrize("n,m,l", [(67, 130, 2), (130, 67, 3)])
def test_batch_of_3_with_padded_leading_dimensions_and_sumsq(n, m, l):
    """3 columns, ldx = n m + 5 and ldy = rows + 3 (forward; the transpose reads rows + 3 apart and writes n m + 5 apart), exact;
    the pads of the output untouched, the pads of the input NaN (not read); sumsq = the float64 sum of squares of the exact output
    over all three columns, to 1e-6 relative."""
    Op = dyadic_op(n, m, l)
    dev = Op.engine.device
    Wn, Wm = C.dyadic_matrix(n, l), C.dyadic_matrix(m, l)
    rows, cols = Op.shape
    S = Op.engine.scalars(2)
    S.set(0, np.array([-1.0, -1.0]))
    for tr in (False, True):
        nin, nout, ldi, ldo = (rows, cols, rows + 3, cols + 5) if tr else (cols, rows, cols + 5, rows + 3)
        V = C.int_vector(3 * nin, 50 + int(tr)).reshape(3, nin)
        assert max(C.exact_margin(Wn, Wm, V[j], n, m, tr) for j in range(3)) < 2 ** 24
        ref = (C.transpose64 if tr else C.forward64)(Wn, Wm, V, n, m).astype(np.float32)
        xbuf = torch.full((3, ldi), float("nan"), dtype=torch.float32, device=dev)
        xbuf[:, :nin] = torch.from_numpy(V).to(dev)
        ybuf = torch.full((3, ldo), SENTINEL, dtype=torch.float32, device=dev)
        res = Op.apply(xbuf[:, :nin], out=ybuf[:, :nout], transpose=tr, sumsq=S.ref(int(tr)))
        assert res.data_ptr() == ybuf.data_ptr() and res.stride(0) == ldo
        got = ybuf.cpu().numpy()
        assert np.all(got[:, nout:] == SENTINEL)
        for j in range(3):
            assert_exact(got[j, :nout], ref[j], n, m, l, tr)
        expect = float((ref.astype(np.float64) ** 2).sum())
        s = S.host()
        assert expect > 0 and abs(s[int(tr)] - expect) <= 1e-6 * expect, (s, expect)
        if not tr:
            assert s[1] == -1.0


@pytest.mark.parametrize("n,m,l", C.WIDE_BATCH_SHAPES)
def test_eight_column_forward_kernel_at_every_level(n, m, l):
    """A batch of 228 columns takes a 3 x 3-tile image past the 2048 tiles from which the forward runs eight columns per lane
    (k_framelet_fwd<H, 8> for H = 1, 2, 4, 7): every column exact (three distinct vectors in rotation), pads untouched."""
    Op = dyadic_op(n, m, l)
    dev = Op.engine.device
    Wn, Wm = C.dyadic_matrix(n, l), C.dyadic_matrix(m, l)
    rows, cols = Op.shape
    assert C.tile_columns(n, m, C.WIDE_BATCH) == C.TJ_LARGE
    V = np.stack([C.int_vector(cols, 70 + k) for k in range(3)])
    ref = C.forward64(Wn, Wm, V, n, m).astype(np.float32)
    xbuf = torch.from_numpy(V).to(dev).repeat(C.WIDE_BATCH // 3, 1)
    ybuf = torch.full((C.WIDE_BATCH, rows + 3), SENTINEL, dtype=torch.float32, device=dev)
    Op.apply(xbuf, out=ybuf[:, :rows])
    got = ybuf.cpu().numpy()
    assert np.all(got[:, rows:] == SENTINEL)
    bad = [j for j in range(C.WIDE_BATCH) if not np.array_equal(got[j, :rows], ref[j % 3])]
    if bad:
        assert_exact(got[bad[0], :rows], ref[bad[0] % 3], n, m, l, False)


def test_non_temporal_stores_at_level_4():
    """From 64 M output floats the forward stores non-temporally (k_framelet_fwd<7, 4, true> here: 15 x 114 tiles of 8 stay below 2048).  Every entry is written (no
    sentinel left, guards intact); 40 output columns q = (c, j) - the first and last three of the image in every third column
    block, and seeded ones - are compared exactly with W_n X W_m[q, :]^T in float64 (the full float64 product would take seconds)."""
    n, m, l = C.NT_STORE_SHAPE
    Op = dyadic_op(n, m, l)
    assert Op.shape[0] >= C.NT_STORE_FLOATS
    Wn, Wm = C.dyadic_matrix(n, l), C.dyadic_matrix(m, l)
    v = C.int_vector(n * m, 90)
    got = run_guarded(Op, v, False)
    assert not np.any(got == SENTINEL)
    Rn = Wn.shape[0]
    edge = [c * m + j for c in range(0, 2 * l + 1, 3) for j in (0, 1, 2, m - 3, m - 2, m - 1)]
    q = np.unique(np.concatenate([edge, np.random.default_rng(91).integers(0, Wm.shape[0], 40 - len(edge))]))
    T = np.asarray(Wn @ v.astype(np.float64).reshape(n, m, order="F"))                 # (R_n x m)
    ref = np.asarray((Wm.tocsr()[q] @ T.T).T).astype(np.float32)                     # (R_n x len(q))
    for k, qq in enumerate(q):
        col = got[qq * Rn:(qq + 1) * Rn]
        assert np.array_equal(col, ref[:, k]), (int(qq), np.flatnonzero(col != ref[:, k])[:8])


# ------------------------------------------------------------------------------------------------------------------ real taps
def check_entry_bound(Op, Wn, Wm, v, ref64, n, m, tr, extra=0.0, tag=""):
    got = run_guarded(Op, v, tr).astype(np.float64)
    bound = C.entry_bound(Wn, Wm, v, n, m, tr) + extra
    err = np.abs(got - ref64)
    ok = bound > 0
    ratio = float(np.max(err[ok] / bound[ok])) if ok.any() else 0.0
    print(f"framelet {tag} {(n, m)} transpose {tr}: max error / bound {ratio:.3f}")
    over = np.flatnonzero(err > bound)
    assert over.size == 0, (over[:8], err[over[:8]], bound[over[:8]])
    return ratio


@pytest.mark.parametrize("n,m,l", C.GENERAL_SHAPES)
def test_real_taps_per_entry_bound(n, m, l):
    """Standard-normal vectors through the reference's own matrices, both directions, against float64 on the float32-rounded input:

        forward    |y - y64|[p, q] <= (T_n + T_m + 4) 2^-24 (|W_n| |X| |W_m|^T)[p, q]     T = most non-zeros in a row of the 1-D matrix
        transpose  |x - x64|[i, j] <= (C_n + C_m + 4) 2^-24 (|W_n|^T |Y| |W_m|)[i, j]     C = most non-zeros in a column

    The kernels' arithmetic is two 1-D passes: one rounding per tap (float64 -> float32), at most T (C) fused multiply-adds per
    pass on one accumulator, one float32 store between the passes; the taps a narrower band is padded with are zeros and add
    nothing.  A sequential float32 emulation on the CPU stays at 0.30 (forward) and 0.07 (transpose) of this bound.  Arithmetic, not a
    measurement."""
    Op = real_op(n, m, l)
    Wn, Wm = C.analysis_matrix(n, l), C.analysis_matrix(m, l)
    worst = 0.0
    for tr in (False, True):
        v = C.normal_vector(Op.shape[0] if tr else Op.shape[1], 300 + l + int(tr))
        ref = (C.transpose64 if tr else C.forward64)(Wn, Wm, v, n, m)
        worst = max(worst, check_entry_bound(Op, Wn, Wm, v, ref, n, m, tr, tag=f"level {l}"))
    assert worst > 0.0                                                  # (inexact operands: some rounding has happened)


@pytest.mark.parametrize("n,m,l", [(8, 6, 2), (12, 12, 1), (16, 10, 3)])
def test_reference_actions(n, m, l):
    """Wx and W^T y as the reference's create_framelet_operator recorded them (framelet_ops.npz), within the bound above plus 1e-12."""
    g = load_golden("framelet_ops")
    Op = real_op(n, m, l)
    Wn, Wm = C.analysis_matrix(n, l), C.analysis_matrix(m, l)
    for tr, vin, vout in ((False, f"x_{n}_{m}_{l}", f"Wx_{n}_{m}_{l}"), (True, f"y_{n}_{m}_{l}", f"WTy_{n}_{m}_{l}")):
        check_entry_bound(Op, Wn, Wm, g[vin].astype(np.float32), g[vout], n, m, tr, extra=1e-12, tag="golden")
    # the PyLops-style surface: float64 in, float64 out
    assert relerr(Op @ g[f"x_{n}_{m}_{l}"], g[f"Wx_{n}_{m}_{l}"]) < 1e-6 and relerr(Op.T @ g[f"y_{n}_{m}_{l}"], g[f"WTy_{n}_{m}_{l}"]) < 1e-6


def test_adjoint_identity_and_repeatability():
    """<W x, y> = <x, W^T y> in float64 to 1e-6 relative at (130, 67, 3); two runs of either direction agree to the bit (a gather in a
    fixed order: no atomics)."""
    n, m, l = 130, 67, 3
    Op = real_op(n, m, l)
    x, y = C.normal_vector(Op.shape[1], 11), C.normal_vector(Op.shape[0], 12)
    Wx, WTy = run_guarded(Op, x, False), run_guarded(Op, y, True)
    lhs, rhs = float(Wx.astype(np.float64) @ y.astype(np.float64)), float(x.astype(np.float64) @ WTy.astype(np.float64))
    print(f"adjoint identity: {lhs!r} {rhs!r} relative {abs(lhs - rhs) / abs(lhs):.2e}")
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs))
    assert np.array_equal(run_guarded(Op, x, False), Wx) and np.array_equal(run_guarded(Op, y, True), WTy)


def test_both_forms_agree():
    """create_framelet_operator(32, 32, 2) as CSR and matrix-free on the same vectors: apart by no more than the sum of the two forms'
    bounds (the CSR kernel's: (ceil(len / 8) + 3) 2^-24 |A| |x| per row, tests/test_gpu_spmv_accuracy.py)."""
    from trips_py_amd.operators import Framelet2D, SparseOp, create_framelet_operator
    n = m = 32
    A, F = create_framelet_operator(n, m, 2), create_framelet_operator(n, m, 2, matrix_free=True)
    assert type(A) is SparseOp and type(F) is Framelet2D and A.shape == F.shape
    Wn = C.analysis_matrix(n, 2)
    for tr in (False, True):
        M = A.matrix.T.tocsr() if tr else A.matrix
        v = C.normal_vector(M.shape[1], 21 + int(tr))
        csr_bound = (np.ceil(np.diff(M.indptr) / 8) + 3) * 2.0 ** -24 * (abs(M) @ np.abs(v.astype(np.float64)))
        bound = csr_bound + C.entry_bound(Wn, Wn, v, n, m, tr)
        diff = np.abs(run_guarded(A, v, tr).astype(np.float64) - run_guarded(F, v, tr).astype(np.float64))
        print(f"forms agree, transpose {tr}: max difference / bound {float(np.max(diff / bound)):.3f}")
        assert np.all(diff <= bound)


def test_vstack_takes_the_generic_path():
    """A VStack with a Framelet2D member applies block by block (it has no .matrix to merge)."""
    from trips_py_amd.operators import SparseOp, VStack, create_framelet_operator
    n, m, l = 8, 6, 2
    F, A = real_op(n, m, l), create_framelet_operator(n, m, l)
    V = VStack([F, A])
    assert type(V) is VStack and not isinstance(V, SparseOp) and V.shape == (2 * F.shape[0], F.shape[1])
    x, y = C.normal_vector(V.shape[1], 31), C.normal_vector(V.shape[0], 32)
    Wn, Wm = C.analysis_matrix(n, l), C.analysis_matrix(m, l)
    ref = C.forward64(Wn, Wm, x, n, m)
    assert relerr(V @ x.astype(np.float64), np.concatenate([ref, ref])) < 1e-6
    refT = C.transpose64(Wn, Wm, y[:F.shape[0]], n, m) + C.transpose64(Wn, Wm, y[F.shape[0]:], n, m)
    assert relerr(V.T @ y.astype(np.float64), refT) < 1e-6


# ------------------------------------------------------------------------------------------------------------------ solvers
def blur(g):
    from trips_py_amd.operators import Blur2D
    N = int(g["N"])
    return Blur2D(g["psf"], N, N)


@pytest.mark.parametrize("tag", ["lam1e-2", "gcv"])
@pytest.mark.parametrize("solver", ["GKS", "MMGKS"])
def test_matrix_free_regulariser_through_the_solvers(solver, tag):
    """GKS / MMGKS with L = create_framelet_operator(32, 32, 2, matrix_free=True) against the reference's own runs: the bars of
    tests/test_gpu_solvers.py::test_framelet_regulariser_through_the_solvers for the CSR form."""
    from trips_py_amd import solvers as S
    from trips_py_amd.operators import Framelet2D, create_framelet_operator
    g = load_golden("gks_blur32_framelet_" + tag if solver == "GKS" else "mmgks_blur32_framelet_p2q1_" + tag)
    N = int(g["N"])
    W = create_framelet_operator(N, N, int(g["level"]), matrix_free=True)
    assert type(W) is Framelet2D
    rp = 1e-2 if tag == "lam1e-2" else "gcv"
    if solver == "GKS":
        x, info = S.GKS(blur(g), g["b"], W, 3, int(g["n_iter"]), rp, g["x_true"])
    else:
        x, info = S.MMGKS(blur(g), g["b"], W, 2, 1, 3, int(g["n_iter"]), rp, g["x_true"])
    assert info["its"] == int(g["its"]) and len(info["xHistory"]) == int(g["n_iter"])
    if tag == "lam1e-2":
        bar(f"framelet_mf[{solver}-lam].x", relerr(x, g["x"]), 1e-5)
        bar(f"framelet_mf[{solver}-lam].x_it1", relerr(info["xHistory"][0], g["x_it1"]), 1e-5)
        bar(f"framelet_mf[{solver}-lam].relError", maxrel(info["relError"], g["relError"]), 1e-5)
        bar(f"framelet_mf[{solver}-lam].Residual", maxrel(info["Residual"], g["Residual"]), 1e-3)
    else:
        assert lam_close(info["regParam_history"], g["regParam_history"], 5e-2)
        bar(f"framelet_mf[{solver}-gcv].relError", maxrel(info["relError"], g["relError"]), 1e-5)
        bar(f"framelet_mf[{solver}-gcv].x", relerr(x, g["x"]), 1e-5)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_device_work():
    """A level beyond the half-width limit: ValueError naming the limit and matrix_free=False.  Straight at the C ABI: a half-width of
    8 is TRK_EUNSUPPORTED, a table whose interior rows differ or with a non-zero outside the matrix is TRK_EINVAL; no handle comes back."""
    from trips_py_amd import operators as ops
    from trips_py_amd.engine import default_engine
    with pytest.raises(ValueError, match=r"limit of 7.*matrix_free=False"):
        ops.create_framelet_operator(64, 48, 5, matrix_free=True)
    lib = default_engine().lib
    n = 24
    blocks, half, band = ops.band_tables(ops.framelet_analysis_matrix(n, 2), n)
    dp = ctypes.POINTER(ctypes.c_double)

    def create(bn, hn, tn, bm, hm, tm):
        h = ctypes.c_void_p()
        tn, tm = np.ascontiguousarray(tn), np.ascontiguousarray(tm)
        rc = lib.trk_framelet2d_create(n, n, bn, hn, tn.ctypes.data_as(dp), bm, hm, tm.ctypes.data_as(dp), ctypes.byref(h))
        return rc, h, lib.trk_last_error().decode()

    rc, h, _ = create(blocks, half, band, blocks, half, band)
    assert rc == 0 and h.value
    assert lib.trk_op_destroy(h) == 0
    bad = band.copy()
    bad[3, 10, 1] += 0.125                                               # an interior row of block 3
    rc, h, msg = create(blocks, half, band, blocks, half, bad)
    assert rc == -1 and not h.value and "stencil" in msg                 # TRK_EINVAL
    bad = band.copy()
    bad[0, 0, 0] = 0.5                                                   # column -2
    rc, h, msg = create(blocks, half, bad, blocks, half, band)
    assert rc == -1 and not h.value and "outside" in msg
    wide = np.zeros((blocks, n, 17))
    wide[:, :, 8 - half:8 + half + 1] = band
    rc, h, msg = create(blocks, 8, wide, blocks, half, band)
    assert rc == -4 and not h.value and "at most 7" in msg               # TRK_EUNSUPPORTED
    rc, h, _ = create(blocks, 7, wide[:, :, 1:-1], blocks, half, band)   # the same band padded to the limit is served
    assert rc == 0 and h.value and lib.trk_op_destroy(h) == 0
