"""The cases of the first-difference tests (tests/tv_cases.py) checked on the CPU: the index-arithmetic references against the
oracle's sparse matrices and the reference project's dense ones (tests/golden/deriv_ops.npz); the slicing against the global
problem; the exact operands for exactness; and the bounds for tightness — NumPy restatements of L^T and tv_grad in the kernels' own
float32 steps pass, the same restatements with one subtle index error each are rejected."""
from fractions import Fraction

import numpy as np
import pytest

import tv_cases as C
from conftest import load_golden

F32, F64 = np.float32, np.float64


def _ops(kind, nt, N, has_next=False, has_prev=False, seed=0):
    """x, y (rows of L), w (rows of L + the previous slice's row), r, dotv of a handle over nt frames."""
    npix, ps, ntemp, rows = C.sizes(N, nt, has_next)
    return dict(X=C.image(kind, nt, N, seed), y=C.vector(kind, rows, seed + 1), w=C.weights(kind, rows + (npix if has_prev else 0), seed),
                r=C.vector(kind, nt * npix, seed + 2, top=31), d=C.vector(kind, nt * npix, seed + 3))


# ------------------------------------------------------------------------------------------------ references against the oracle
@pytest.mark.parametrize("N", [4, 5])
def test_2d_references_equal_the_dense_golden_matrices(N):
    D = load_golden("deriv_ops")[f"D2_{N}"].astype(F64)
    o = _ops("exact", 1, N)
    x64 = o["X"].astype(F64).reshape(-1)
    assert np.array_equal(C.d2_fwd(o["X"]).reshape(-1), D @ x64)
    assert np.array_equal(C.st_fwd(o["X"]), D @ x64)
    assert np.array_equal(C.adj_ref(o["y"], N, 1).val, D.T @ o["y"].astype(F64))
    w64 = o["w"].astype(F64)
    want = o["r"].astype(F64) + 0.25 * (D.T @ (w64 * (D @ x64)))
    assert np.array_equal(C.tv_grad_ref(o["X"], o["w"], o["r"], 0.25).val, want)


@pytest.mark.parametrize("N,nt", [(4, 3), (3, 2)])
def test_spacetime_references_equal_the_dense_golden_matrices(N, nt):
    D = load_golden("deriv_ops")[f"Dst_{N}_{nt}"].astype(F64)
    o = _ops("exact", nt, N)
    x64 = o["X"].astype(F64).reshape(-1)
    assert np.array_equal(C.st_fwd(o["X"]), D @ x64)
    assert np.array_equal(C.adj_ref(o["y"], N, nt).val, D.T @ o["y"].astype(F64))
    want = o["r"].astype(F64) + 0.25 * (D.T @ (o["w"].astype(F64) * (D @ x64)))
    assert np.array_equal(C.tv_grad_ref(o["X"], o["w"], o["r"], 0.25).val, want)
    assert np.array_equal(C.tv_grad_ref(o["X"], None, None, 0.25).val, 0.25 * (D.T @ (D @ x64)))


@pytest.mark.parametrize("N,nt", [(2, 1), (7, 1), (6, 3), (33, 2)])
def test_references_equal_the_oracle_in_float64(N, nt):
    from oracle import cpu_ref as O
    Lm = (O.first_derivative_2d(N, N) if nt == 1 else O.spacetime_derivative(N, N, nt)).astype(F64)
    for kind in ("exact", "normal", "flat"):
        o = _ops("exact" if kind == "exact" else "normal", nt, N)
        X = C.image(kind, nt, N)
        x64, y64, w64, r64 = X.astype(F64).reshape(-1), o["y"].astype(F64), o["w"].astype(F64), o["r"].astype(F64)
        lam = C.lam_of(kind)
        lx, adj = C.st_fwd(X), C.adj_ref(o["y"], N, nt)
        g = C.tv_grad_ref(X, o["w"], o["r"], lam)
        if kind == "exact":
            assert np.array_equal(lx, Lm @ x64) and np.array_equal(adj.val, Lm.T @ y64)
            assert np.array_equal(g.val, r64 + lam * (Lm.T @ (w64 * (Lm @ x64))))
        else:
            assert np.allclose(lx, Lm @ x64, rtol=0, atol=1e-14)
            assert np.all(np.abs(adj.val - Lm.T @ y64) <= 8 * C.U53 * adj.S)
            assert np.all(np.abs(g.val - (r64 + lam * (Lm.T @ (w64 * (Lm @ x64))))) <= 16 * C.U53 * (np.abs(r64) + lam * g.S))
        # the sum of the absolute terms and their count are those of the matrix's rows
        assert np.allclose(adj.S, abs(Lm.T) @ np.abs(y64), rtol=1e-14)
        assert np.array_equal(adj.k, np.asarray((Lm.T != 0).sum(axis=1)).reshape(-1))
        for q, eps in ((1.0, 0.1), (0.7, 1e-3), (2.0, 0.1), (0.5, 0.1)):
            w = C.tv_weights_ref(X, eps, q)
            # (the reference takes the differences, eps^2 and t rounded to float32 as the kernel does: 3 roundings, |e| <= 0.75)
            assert np.allclose(w.val, ((Lm @ x64) ** 2 + eps ** 2) ** (q / 2 - 1), rtol=4e-7)
            assert np.all(w.bound <= (0.75 + C.POWF_CAP + 1) * C.U24 * w.val)


@pytest.mark.parametrize("N,nt", [(1, 1), (2, 3), (3, 1), (16, 3), (5, 2)])
@pytest.mark.parametrize("q", [1.0, 0.5, 2.0, 0.0, 1.3])
def test_isotropic_weights_equal_the_oracle(N, nt, q):
    from oracle import cpu_ref as O
    x = C.vector("normal", N * N * nt, 5)
    tail = C.vector("normal", 7, 6)
    u = np.concatenate((np.zeros(2 * N * N * nt), tail.astype(F64)))
    eps = 0.05
    want = O.iso_tv_weights(x.astype(F64), u, N, N, eps, q).reshape(-1)
    R = C.isotv_weights_ref(x, N, nt, tail, eps, q)
    assert R.val.shape == want.shape and np.allclose(R.val, want, rtol=1e-6)
    ns = N * N * nt
    assert np.array_equal(R.val[:ns], R.val[ns:2 * ns])


def _round_f32(fr):
    """A Fraction rounded to the nearest float32, ties to even (normal range)."""
    if fr == 0:
        return 0.0
    e = 0
    a = abs(fr)
    while a >= 2 ** 24:
        a /= 2
        e += 1
    while a < 2 ** 23:
        a *= 2
        e -= 1
    m = round(a)                                         # Fraction.__round__: half to even
    return float(np.sign(fr)) * float(m) * 2.0 ** e


def test_fma32_rounds_once():
    rng = np.random.default_rng(3)
    a = rng.standard_normal(400).astype(F32)
    c = (rng.standard_normal(400) * 10.0 ** rng.integers(-12, 3, 400)).astype(F32)
    # a^2 = 1 + 2^-11 + 2^-24 is half way between two float32s: the sign of a tiny c decides, which a float64 sum does not see
    a = np.concatenate((a, np.full(4, 1 + 2.0 ** -12, dtype=F32)))
    c = np.concatenate((c, np.array([2.0 ** -60, -2.0 ** -60, 2.0 ** -100, 0.0], dtype=F32)))
    got = C.fma32(a, a, c)
    want = np.array([_round_f32(Fraction(float(x)) ** 2 + Fraction(float(z))) for x, z in zip(a, c)])
    assert got.dtype == F32 and np.array_equal(got.astype(F64), want)
    assert got[-4] != got[-3]


# ------------------------------------------------------------------------------------------------ slicing
@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("ntl", [1, 2])
@pytest.mark.parametrize("N", [3, 5])
def test_slices_reassemble_to_the_global_references(W, ntl, N):
    nt = W * ntl
    npix, ps, ntemp, rows = C.sizes(N, nt)
    for kind in ("exact", "normal"):
        o = _ops(kind, nt, N)
        X, y, r, lam = o["X"], o["y"], o["r"], C.lam_of(kind)
        eps, q = 1e-3, 0.7
        g_lx, g_adj, g_w = C.lx_ref(X), C.adj_ref(y, N, nt), C.tv_weights_ref(X, eps, q)
        g_grad = C.tv_grad_ref(X, o["w"], r, lam)
        seen_rows, seen_pix = np.zeros(rows, dtype=int), np.zeros(nt * npix, dtype=int)
        for s in C.cut(nt, N, W):
            assert s["nt_local"] == ntl
            xs, xprev, xnext = C.frames_of(X, s)
            _, _, _, lrows = C.sizes(N, ntl, s["has_next"])
            assert s["lx_map"].size == lrows and s["w_map"].size == lrows + (npix if s["has_prev"] else 0)
            seen_rows[s["lx_map"]] += 1
            seen_pix[s["out_map"]] += 1
            lx = C.lx_ref(xs, xnext)
            assert np.array_equal(lx.val, g_lx.val[s["lx_map"]]) and np.array_equal(lx.bound, g_lx.bound[s["lx_map"]])
            w = C.tv_weights_ref(xs, eps, q, xprev, xnext)
            assert np.array_equal(w.val, g_w.val[s["w_map"]]) and np.array_equal(w.bound, g_w.bound[s["w_map"]])
            halo = y[s["prev_rows"]] if s["has_prev"] else None
            adj = C.adj_ref(y[s["lx_map"]], N, ntl, s["has_next"], halo)
            assert np.array_equal(adj.val, g_adj.val[s["out_map"]]) and np.array_equal(adj.bound, g_adj.bound[s["out_map"]])
            rs = r[s["out_map"]]
            grad = C.tv_grad_ref(xs, o["w"][s["w_map"]], rs, lam, xprev, xnext)
            assert np.array_equal(grad.val, g_grad.val[s["out_map"]]) and np.array_equal(grad.bound, g_grad.bound[s["out_map"]])
            unit = C.tv_grad_ref(xs, None, None, lam, xprev, xnext)
            assert np.array_equal(unit.val, C.tv_grad_ref(X, None, None, lam).val[s["out_map"]])
        assert np.all(seen_rows == 1) and np.all(seen_pix == 1)


# ------------------------------------------------------------------------------------------------ exact operands
@pytest.mark.parametrize("N,nt", [(2, 1), (5, 3), (257, 2)])
def test_exact_operands_are_exact(N, nt):
    o = _ops("exact", nt, N)
    X, y, w, r, d = o["X"], o["y"], o["w"], o["r"], o["d"]
    lx32, lx64 = C.st_fwd(X, dtype=F32), C.st_fwd(X)
    assert lx32.dtype == F32 and np.array_equal(lx32.astype(F64), lx64) and C.fits_float32(lx64, 1.0)
    a32, a64 = C.adj_ref(y, N, nt, dtype=F32), C.adj_ref(y, N, nt)
    assert np.array_equal(a32.val, a64.val) and C.fits_float32(a64.S, 1.0)
    for ww, rr in ((w, r), (w, None), (None, r), (None, None)):
        g32, g64 = C.tv_grad_ref(X, ww, rr, C.LAM_EXACT, dtype=F32), C.tv_grad_ref(X, ww, rr, C.LAM_EXACT)
        assert np.array_equal(g32.val, g64.val)
        # every partial sum in any order: a multiple of 1/8 no larger than |r| + lam S
        assert C.fits_float32(g64.val, 0.125) and C.fits_float32(np.abs(r.astype(F64)) + C.LAM_EXACT * g64.S, 0.125)
        assert C.sum_is_exact(g64.val, d, 0.125)
    assert C.sum_is_exact(lx64, lx64, 1.0) and C.sum_is_exact(a64.val, a64.val, 1.0) and C.sum_is_exact(X, X, 1.0)


def test_exact_sums_stay_exact_at_the_largest_shape():
    """N = 2049, nt = 2 (the capped grid's case): the absolute sums stay below 2^53 units by the operands' ranges alone."""
    n = 2 * 2049 * 2049
    assert n * (720 * 0.25 + 31) * 15 / 0.125 < 2.0 ** 53          # <out, dotv>
    assert 3 * n * 30.0 ** 2 < 2.0 ** 53 and n * 90.0 ** 2 < 2.0 ** 53      # ||L x||^2, ||L^T y||^2


# ------------------------------------------------------------------------------------------------ mutants
SHAPES = [(5, 2, 2), (257, 2, 2), (5, 4, 1), (6, 2, 1)]              # (N, W, nt_local)


@pytest.mark.parametrize("N,W,ntl", SHAPES)
@pytest.mark.parametrize("kind", ["exact", "normal"])
def test_restatements_pass_and_mutants_are_rejected(N, W, ntl, kind):
    nt = W * ntl
    npix = N * N
    o = _ops(kind, nt, N)
    X, y, lam, exact = o["X"], o["y"], C.lam_of(kind), kind == "exact"
    wg = C.weights(kind, C.sizes(N, nt)[3], 0)
    rejected = {m: 0 for m in C.MUTANTS}
    for s in C.cut(nt, N, W):
        xs, xprev, xnext = C.frames_of(X, s)
        ys, halo = y[s["lx_map"]], (y[s["prev_rows"]] if s["has_prev"] else None)
        ws, rs = wg[s["w_map"]], o["r"][s["out_map"]]
        A = C.adj_ref(ys, N, ntl, s["has_next"], halo)
        bad, ratio = C.compare(C.adj_ref(ys, N, ntl, s["has_next"], halo, dtype=F32).val.astype(F32), A, exact)
        assert bad.size == 0 and ratio <= 1.0
        for ww, rr in ((ws, rs), (None, rs), (ws, None), (None, None)):
            G = C.tv_grad_ref(xs, ww, rr, lam, xprev, xnext)
            model = C.tv_grad_ref(xs, ww, rr, lam, xprev, xnext, dtype=F32).val.astype(F32)
            bad, ratio = C.compare(model, G, exact)
            assert bad.size == 0 and ratio <= 1.0
        G = C.tv_grad_ref(xs, ws, rs, lam, xprev, xnext)
        for m in C.MUTANTS:
            if m == "wrow":
                if not s["has_prev"] or ntl - 1 + s["has_next"] < 1:
                    continue                                   # no previous slice's row, or no row ntemp - 1 to confuse it with
            elif m == "frame0":
                if ntl - 1 + s["has_next"] < 1:
                    continue                                   # frame 0 has no + T[0]
                bad, _ = C.compare(C.adj_ref(ys, N, ntl, s["has_next"], halo, dtype=F32, mutant=m).val.astype(F32), A, exact)
                assert 0 < bad.size <= npix and np.all(bad < npix), (m, "L^T")            # frame 0 alone
            else:
                bad, _ = C.compare(C.adj_ref(ys, N, ntl, s["has_next"], halo, dtype=F32, mutant=m).val.astype(F32), A, exact)
                assert bad.size > 0, (m, "L^T")
            bad, _ = C.compare(C.tv_grad_ref(xs, ws, rs, lam, xprev, xnext, dtype=F32, mutant=m).val.astype(F32), G, exact)
            assert bad.size > 0, (m, "tv_grad")
            if m == "predicate":
                assert np.all((bad % npix) // N == N - 2)      # the one row whose term went missing
            if m == "wrow":
                assert np.all(bad < npix)
            rejected[m] += 1
    # (W = 2 slices of one frame: the slice with a previous one has no temporal row of its own to confuse the boundary row with)
    assert all(v > 0 for m, v in rejected.items() if m != "wrow" or ntl >= 2 or W >= 3), rejected


def test_a_single_wrong_pixel_is_rejected():
    """One entry off by one float32 ulp of the largest term passes no bound; by far less than the norm-wise bars see."""
    N, nt = 257, 2
    o = _ops("normal", nt, N)
    G = C.tv_grad_ref(o["X"], o["w"], o["r"], C.LAM_GENERAL)
    model = C.tv_grad_ref(o["X"], o["w"], o["r"], C.LAM_GENERAL, dtype=F32).val.astype(F32)
    at = 3 * N + N - 1
    model[at] += F32(32 * C.U24 * (abs(o["r"][at]) + C.LAM_GENERAL * G.S[at]))
    bad, _ = C.compare(model, G, False)
    assert list(bad) == [at]
    assert np.linalg.norm(model - G.val) / np.linalg.norm(G.val) < 3e-7


def test_grid_thresholds():
    assert not C.row_batches_strided(2048) and C.row_batches_strided(2049)
    assert not C.temporal_strided(512) and C.temporal_strided(513)
