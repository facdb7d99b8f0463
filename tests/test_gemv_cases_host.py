"""The cases of tests/gemv_cases.py checked on the CPU: the exact operands are what the docstring says and every sum they enter is
exact (multiples of the stated unit below 2^53 units in float64, outputs that fit float32), the general operands keep the dot bound
below the smallest single term, the references' helpers are right.  For every (k, n) tests/test_gpu_gemv_entrywise.py runs."""
import math

import numpy as np
import pytest

import gemv_cases as C

F64 = np.float64
TOP = 2.0 ** 53


def ints(a, scale, top):
    q = np.asarray(a, dtype=F64) * scale
    return bool(np.all(q == np.rint(q)) and np.all(q != 0) and np.all(np.abs(q) <= top))


def check_operands(c):
    assert c.V.dtype == np.float32 and c.V.shape == (c.rows, c.n) and c.w.dtype == np.float32
    vecs = [c.vec(nm) for nm in C.Case.VECTORS]
    assert all(v.dtype == np.float32 and v.shape == (c.n,) for v in vecs)
    if c.exact:
        assert ints(c.V, 64, 64) and all(ints(v, 1, 31) for v in vecs)
        assert np.all(np.isin(c.w, [0.5, 1.0, 2.0, 4.0]))
        assert all(ints(c.coef(nm), 8, 32) for nm in ("y", "c", "h"))
    else:
        for a in [c.V, c.w] + vecs:
            assert np.all(np.abs(a) >= 0.5) and np.all(np.abs(a) <= 2.0)
        assert np.all(c.w > 0)
    assert c.rho2 in (0.25, 4.0) and 1.0 / np.sqrt(c.rho2) in (2.0, 0.5)
    assert not np.array_equal(c.vec("r"), c.vec("r2")) and not np.array_equal(c.vec("r3"), c.vec("r4"))


def check_dots(c, k, names, wpow=0, extra_row=None):
    """The dots of the rows (or of `extra_row`) with every named vector."""
    rows = c.V[:k] if extra_row is None else extra_row[None, :]
    for nm in names:
        t = C.weighted(c.vec(nm), c.w, wpow)
        R = C.dots(rows, t, c.exact)
        assert R.ref.shape == R.bound.shape == (len(rows),)
        if c.exact:
            assert np.array_equal(t.astype(F64), c.vec(nm).astype(F64) * c.w.astype(F64) ** wpow)      # r w, r w^2 exact in float32
            for row in rows:
                assert C.is_multiple(row.astype(F64) * t.astype(F64), 2.0 ** -9)
            assert np.all(R.S * 2.0 ** 9 < TOP) and R.tmin >= 2.0 ** -9       # every partial sum exact; no term is zero
            assert np.all(R.ref.astype(F64) == R.ref)
        else:
            assert np.all(R.bound < R.tmin), (nm, wpow, R.bound.max(), R.tmin)  # one missing element cannot hide inside the bound
            assert R.tmin >= 2.0 ** -13 * 2.0                                   # (so the split sums of `dots` are 2^8 below it)


def check_rounded(c, R, unit):
    """An output rounded once: exact operands — a multiple of `unit` that float32 holds, every partial sum a float64.  Returns
    what a kernel stores."""
    assert np.all(R.bound > 0) and np.all(np.isfinite(R.ref))
    if c.exact:
        assert not R.lo.any() and C.fits_float32(R.ref, unit), float(np.abs(R.ref).max())
        assert float(R.S.max()) / unit < TOP
        return R.ref.astype(np.float32)
    return R.value().astype(np.float32)


def check_squares(c, stored, minus, unit):
    R = C.sum_of_squares(stored, minus)
    if c.exact:
        assert float(R.ref[0]) / unit ** 2 < TOP and C.is_multiple(R.ref, unit ** 2)
    return R


def check_combinations(c, k, forms, base_as=((0.5, -2.0),)):
    """The combinations the device tests form on k rows of the case.  forms: "n" (x = V y), "sumsq" / "err" (the squares of its
    output, of its distance from ref), "base" (a base + s V y for each (a, s), with the squares), "vn" (the new basis vector),
    "chk", "x" (the next iterate, from vn as stored), "xerr", "nt" (trk_gemv_nt's w_out and the dots with it)."""
    y, cc, h = c.coef("y"), c.coef("c")[:k], c.coef("h")[:k]
    V = c.V[:k]
    u = 2.0 ** -9
    if "n" in forms:
        out = check_rounded(c, C.combination(V, y[:k]), u)
        if "sumsq" in forms:
            check_squares(c, out, None, u)
        if "err" in forms:
            check_squares(c, out, c.vec("ref"), u)
    if "base" in forms:
        for a, s in base_as:
            out = check_rounded(c, C.combination(V, y[:k], a, c.vec("base"), s), u)
            check_squares(c, out, None, u)
    if "vn" in forms:
        inv = 1.0 / np.sqrt(c.rho2)
        vn = check_rounded(c, C.combination(V, cc, 1.0, c.vec("w_in"), -1.0, post=inv), u * inv)
        if "chk" in forms:
            R = C.chk_sum(V, cc, c.vec("w_in"))
            assert not c.exact or float(R.ref[0]) / u ** 2 < TOP
        if "x" in forms:
            x = check_rounded(c, C.combination(list(V) + [vn], y[:k + 1]), u * inv / 8)
            if "xerr" in forms:
                check_squares(c, x, c.vec("ref"), u * inv / 8)
    if "nt" in forms:
        w_out = check_rounded(c, C.combination(V, h, 1.0, c.vec("w_in"), -1.0), u)
        G = C.dots(V, w_out, c.exact)
        assert not c.exact or np.all(G.S * 2.0 ** 15 < TOP)


ALL = ("n", "sumsq", "err", "base", "vn", "chk", "x", "xerr", "nt")
DOT_NAMES = ("r", "r2", "r3", "r4")


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
@pytest.mark.parametrize("n", C.LAYOUT_N)
def test_layout_cases(n, exact):
    c = C.case(C.LAYOUT_K, n, exact)
    check_operands(c)
    check_dots(c, c.k, DOT_NAMES)
    check_dots(c, c.k, ("r",), wpow=1)
    check_dots(c, 1, ("r",), extra_row=c.vec("xrow"))
    for k in (c.k, 5):
        check_combinations(c, k, ALL, base_as=((0.5, -2.0), (1.0, -1.0)))


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
def test_weighted_cases(exact):
    for n in (1030, 1031):
        c = C.case(C.WGRAM_K, n, exact, C.WGRAM_K)
        check_operands(c)
        for wpow in (1, 2):
            check_dots(c, c.k, ("r",), wpow=wpow)


def test_weighted_repeats_the_float32_steps():
    r, w = np.float32([3.1, -1.7]), np.float32([1.3, 0.7])
    assert np.array_equal(C.weighted(r, w, 0), r)
    assert np.array_equal(C.weighted(r, w, 1), (r.astype(F64) * w).astype(np.float32))
    assert np.array_equal(C.weighted(r, w, 2), (r.astype(F64) * (w.astype(F64) * w).astype(np.float32)).astype(np.float32))


@pytest.mark.parametrize("k,n,exact", [(C.TILE_KMAX, C.TILE_N, True)] + [(k, n, e) for k, n in C.GRID_CASES for e in (True, False)])
def test_tile_and_grid_cases(k, n, exact):
    """(The row tiles run on exact operands only.)"""
    c = C.case(k, n, exact, k)
    check_operands(c)
    check_dots(c, k, DOT_NAMES)
    check_dots(c, 1, ("r",), extra_row=c.vec("xrow"))


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
def test_ladder_and_split_cases(exact):
    c = C.case(max(C.LADDER_K), C.LADDER_N, exact)
    check_operands(c)
    for k in C.LADDER_K:
        check_combinations(c, k, ("n", "sumsq", "err", "base", "vn", "x"))
    for k, n in [(k, C.SPLIT_N) for k in C.SPLIT_K] + [(12, C.split_edge(256)), (12, C.split_edge(256) + 4)]:
        c = C.case(k, n, exact)
        check_operands(c)
        check_combinations(c, k, ("base", "vn"), base_as=((-1.0, 1.0),))


def test_limit_cases():
    c = C.case(C.KMAX_LDS, C.KMAX_N, True, C.KMAX_LDS + 1)
    check_operands(c)
    check_combinations(c, C.KMAX_LDS, ("n", "err", "base"))
    check_combinations(c, C.KMAX_LDS - 1, ("vn", "x"))
    for k in (8, 9, 16):
        check_combinations(c, k, ("nt",))
    c = C.case(130, C.LADDER_N, True, 130)
    check_combinations(c, 130, ("n", "err"))
    # rounded to float32 after 128 rows (trk_gemv_n_hosty's second launch adds to `out`): exact as well
    check_rounded(c, C.combination(c.V[:128], c.coef("y")[:128]), 2.0 ** -9)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
def test_nontemporal_case(exact):
    """n = 11 x 2^20 + 4: every sum still exact; the dot bound (about 0.06 at most, n^2 2^-53 x 4) still below the smallest term 0.25."""
    c = C.case(C.NT_K, C.NT_N, exact, C.NT_K)
    assert c.n >= C.NT_MIN and c.n % 4 == 0
    check_dots(c, c.k, ("r", "r2", "r4"))
    if not exact:
        assert c.n ** 2 * 4.0 * C.U53 < 0.0625 < 0.25
    check_combinations(c, c.k, ("n", "sumsq", "vn", "x"))


# ------------------------------------------------------------------------------------------------------------ the helpers themselves
def test_dots_against_fsum():
    rng = np.random.default_rng(3)
    V, t = C.band(rng, (3, 5000)), C.band(rng, 5000)
    R = C.dots(V, t)
    for j in range(3):
        p = V[j].astype(F64) * t.astype(F64)
        assert abs(float(R.ref[j]) - math.fsum(p)) <= 2.0 ** -52 * abs(math.fsum(p))
        assert R.bound[j] == 5000 * C.U53 * np.abs(p).sum()
    # terms that cancel to nothing of their size: the split sums are not taken, the reference is still right
    V2 = np.float32([[1.5, -1.5, 2.0 ** -30]])
    assert float(C.dots(V2, np.float32([1, 1, 1])).ref[0]) == 2.0 ** -30
    assert C.dots(np.zeros((2, 0), dtype=np.float32), np.zeros(0, dtype=np.float32)).ref.tolist() == [0, 0]


def test_combination_against_fractions():
    from fractions import Fraction
    rng = np.random.default_rng(4)
    V, base, y = rng.standard_normal((7, 9)).astype(np.float32), rng.standard_normal(9).astype(np.float32), rng.standard_normal(7)
    R = C.combination(V, y, 0.3, base, -1.7, post=0.5)
    for i in range(9):
        want = Fraction(float(np.float64(0.3))) * Fraction(float(base[i]))
        S = abs(want)
        for j in range(7):
            t = Fraction(float(np.float64(-1.7) * y[j])) * Fraction(float(V[j, i]))
            want, S = want + t, S + abs(t)
        want, S = want / 2, S / 2
        assert abs(Fraction(float(R.ref[i])) + Fraction(float(R.lo[i])) - want) <= Fraction(2) ** -100 * S
        assert abs(R.S[i] - float(S)) <= 1e-14 * float(S)
        assert R.bound[i] >= float(abs(want)) * C.U24 * (1 - 1e-9) + 10 * C.U53 * float(S) * (1 - 1e-9)
    near = R.value().astype(np.float32)                                       # the correctly rounded output passes, two units further fails
    far = np.nextafter(np.nextafter(near, np.float32(np.inf)), np.float32(np.inf))
    assert np.all(R.error(near) <= R.bound) and np.all(R.error(far) > R.bound)


def test_lsqr_coefficients_against_the_definition():
    """Two steps of the rotations against the least-squares problem they solve: x_2 = V_2 y_2, y_2 = argmin ||[B_2; damp I] y - beta_1 e_1||."""
    a1, b2, a2, b3, beta1, damp = 1.3, 0.7, 0.9, 1.1, 2.0, 0.4
    (ia1, _, px1), st1 = C.lsqr_coefficients(a1 ** 2, b2 ** 2, beta1 ** 2, damp, None, True)
    (ia2, tw2, px2), st2 = C.lsqr_coefficients(a2 ** 2, b3 ** 2, beta1 ** 2, damp, st1, False)
    # in coordinates of (v_1, v_2): w_1 = v_1, x_1 = px1 w_1; w_2 = v_2 - tw2 w_1, x_2 = x_1 + px2 w_2  (vk = alpha_k v_k, so ia vk = v_k)
    x2 = np.array([px1 - px2 * tw2, px2])
    B = np.array([[a1, 0.0], [b2, a2], [0.0, b3], [damp, 0.0], [0.0, damp]])
    want = np.linalg.lstsq(B, np.array([beta1, 0, 0, 0, 0.0]), rcond=None)[0]
    assert np.allclose(x2, want, rtol=1e-13, atol=0) and ia1 == 1 / a1 and ia2 == 1 / a2
    assert np.isclose(st2[0] ** 2 + st2[1] ** 2, 1.0, rtol=1e-15)


def test_exactness_helpers():
    assert C.fits_float32(np.array([3.5, -2.0 ** 14]), 2.0 ** -9) and not C.fits_float32(np.array([2.0 ** 15]), 2.0 ** -9)
    assert not C.fits_float32(np.array([2.0 ** -10]), 2.0 ** -9) and C.is_multiple(np.array([0.0, 0.375]), 0.125)
    R = C.sum_of_squares(np.float32([3, 4]), np.float32([0, 1]))
    assert R.ref[0] == 18 and R.bound[0] == 2 * C.U53 * 18
    assert C.split_edge(256) == 262144
