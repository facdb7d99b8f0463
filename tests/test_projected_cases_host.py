"""tests/projected_cases.py checked on the CPU: the reference arithmetic against numpy.linalg, the exact operands exact in the NumPy
restatements, every bound on the restatements, the condition cap of every solve case, the measured constants of the bordered
inverse, and the same cases through tests/cpu_engine.py and libtrk's host code (trk_host_bidiag_tikhonov)."""
import decimal

import numpy as np
import pytest

import projected_cases as C


def test_reference_arithmetic_has_at_least_50_digits():
    assert C.decimal is decimal and C.reference_digits() >= 50         # (the stdlib module: it always imports, nothing skips)
    with C.ctx():
        third = decimal.Decimal(1) / decimal.Decimal(3)
        assert abs(third * 3 - 1) < decimal.Decimal(10) ** -55
        assert (decimal.Decimal(2).sqrt() ** 2 - 2).copy_abs() < decimal.Decimal(10) ** -55
    x = np.array([0.1, -1e-300, 3.0 ** 40])
    assert np.array_equal(C.fl(C.dec(x)), x)


@pytest.mark.parametrize("k", [1, 5, 17, 66])
def test_references_agree_with_numpy_on_well_conditioned_cases(k):
    cs = C.random_gram(k)
    M = cs["GA"] + cs["lam"] * cs["GL"]
    ystar = C.fl(C.ref_solve(C.gram_matrix(cs["GA"], cs["GL"], cs["lam"]), C.dec(cs["c"])))
    want = np.linalg.solve(M, cs["c"])
    assert np.linalg.norm(ystar - want) <= 4 * k * np.linalg.cond(M) * C.U * np.linalg.norm(want)
    rng = np.random.default_rng(k)
    G, h = cs["GA"] / np.linalg.norm(cs["GA"], 2) * 0.5, rng.standard_normal(k)
    c, e, v, vb = C.ref_cgs(G, h, 3, rr=float(h @ h) + 1.0)
    cn = np.zeros(k)
    for _ in range(3):
        cn = cn + (h - G @ cn)
    assert np.all(np.abs(C.fl(c) - cn) <= e + 4 * C.U * np.abs(cn))
    assert abs(float(v) - (h @ h + 1.0 - 2 * cn @ h + cn @ G @ cn)) <= vb + 1e-15 * abs(float(v))
    H, beta0 = C.random_hess(k)
    Md, cd = C.hess_system(H, beta0, 1e-2, k)
    rhs = np.zeros(2 * k + 1)
    rhs[0] = beta0
    want = np.linalg.lstsq(np.vstack((H, 0.1 * np.eye(k))), rhs, rcond=None)[0]
    assert np.linalg.norm(C.fl(C.ref_solve(Md, cd)) - want) <= 1e-11 * np.linalg.norm(want)
    a2, b2, b02 = C.random_bidiag(k)
    B = np.zeros((k + 1, k))
    B[np.arange(k), np.arange(k)], B[np.arange(1, k + 1), np.arange(k)] = np.sqrt(a2), np.sqrt(b2)
    for mu in (0.0, 0.5):
        rhs[0] = np.sqrt(b02)
        y = np.linalg.lstsq(np.vstack((B, mu * np.eye(k))), rhs, rcond=None)[0]
        res, _ = C.bidiag_residual(a2, b2, b02, mu, y)
        assert res <= 1e-13 * (np.linalg.norm(y) + 1.0)


@pytest.mark.parametrize("k", C.SIZES + C.BIG_SIZES)
def test_exact_cgs_and_gram_row_operands_are_exact(k):
    cs = C.exact_cgs(k)
    assert C.exact_headroom(cs["G"], cs["h"], 3) < 2.0 ** 53
    if k > 258:
        return
    for passes in (1, 2, 3):
        ci, gci = C.int_cgs(cs["G"], cs["h"], passes)
        want = np.array([float(v) for v in ci])
        c, rho2 = C.np_cgs(cs["G"], cs["h"], passes, cs["rr"])
        assert np.array_equal(c, want)
        assert rho2 == float(int(cs["rr"]) - 2 * int(ci.dot(cs["h"].astype(np.int64).astype(object))) + int(ci.dot(gci)))
        cr, e, v, _ = C.ref_cgs(cs["G"], cs["h"], passes, cs["rr"])
        assert np.array_equal(C.fl(cr), want) and float(v) == rho2
    gr = C.exact_gram_row(k)
    assert C.exact_headroom(gr["G"], gr["c"], 1, a=gr["a"], rhs=gr["rhs"]) < 2.0 ** 51
    row, diag, rk = C.int_gram_row(gr["G"], gr["a"], gr["c"], gr["s"], gr["rho2"], gr["rhs"], gr["tb"])
    r2, d2, k2 = C.np_gram_row(gr["G"], gr["a"], gr["c"], gr["s"], gr["rho2"], gr["rhs"], gr["tb"])
    assert np.array_equal(r2, row) and d2 == diag and k2 == rk
    (rr_, _), (dd_, _), (kk_, _) = C.ref_gram_row(gr["G"], gr["a"], gr["c"], gr["s"], gr["rho2"], gr["rhs"], gr["tb"])
    assert np.array_equal(C.fl(rr_), row) and float(dd_) == diag and float(kk_) == rk


def test_exact_gram_row_headroom_at_the_large_sizes():
    for k in C.BIG_SIZES:
        gr = C.exact_gram_row(k - 1)
        assert C.exact_headroom(gr["G"], gr["c"], 1, a=gr["a"], rhs=gr["rhs"]) < 2.0 ** 51


@pytest.mark.parametrize("k", sorted(set(C.CHOL_SIZES)))
def test_exact_cholesky_operands_are_exact(k):
    cs = C.exact_chol(k)
    M = cs["GA"] + cs["lam"] * cs["GL"]
    assert np.array_equal(M, cs["M"]) and np.all(cs["GL"] % 2 == 0) and np.all(cs["GA"] == np.round(cs["GA"]))
    assert C.cap_value(M) <= C.CAP
    assert np.array_equal(C.np_chol_solve(M, cs["c"]), cs["y"])
    assert np.array_equal(np.linalg.cholesky(M), cs["C"])
    # k_hess_tikhonov mode 0 on H = [C^T; 0], lam = 0: the earlier columns and their Gram block given, the last column by the call
    H = np.vstack((cs["C"].T, np.zeros((1, k))))
    Hd, G = np.full((k + 1, k), np.nan), np.full((k, k), np.nan)
    Hd[:, :k - 1], G[:k - 1, :k - 1] = H[:, :k - 1], cs["M"][:k - 1, :k - 1]
    y = C.np_hess(Hd, G, None, H[:, k - 1], None, 0.0, 3.0, k, 0.0, 0)
    assert np.array_equal(G, cs["M"]) and np.array_equal(y, np.concatenate(([3.0 / cs["C"][0, 0]], np.zeros(k - 1))))


@pytest.mark.parametrize("k", C.SIZES)
def test_exact_bordered_operands_are_exact(k):
    cs = C.exact_border(k)
    assert np.array_equal(cs["GA"] + 0.5 * cs["GL"], cs["M"])
    want_inv = C.exact_border_inverse(cs["p"], k)
    assert np.array_equal(want_inv @ cs["M"], np.eye(k)) and np.abs(want_inv).max() <= k
    for sched in ([(0, k)], [(0, min(3, k))] + [(j - 1, j) for j in range(4, k + 1)], [(0, max(k - 3, 0)), (max(k - 3, 0), k), (k, k)]):
        Minv = np.full((k, k), np.nan)
        for k_from, kk in sched:
            if kk == 0:
                continue
            y = C.np_border(cs["GA"], cs["GL"], 0.5, cs["c"], kk, k_from, Minv)
            assert np.array_equal(Minv[:kk, :kk], C.exact_border_inverse(cs["p"], kk))
        assert np.array_equal(y, want_inv @ cs["c"])


@pytest.mark.parametrize("kmax", [17, 66])
def test_exact_hessenberg_operands_are_exact(kmax):
    cs = C.exact_hess(kmax)
    H = cs["H"]
    assert np.array_equal(np.triu(cs["coef"] + cs["coef2"]), np.triu(H))
    Hd, G, Minv = (np.full((kmax + 1, kmax + 1), np.nan) for _ in range(3))
    for k in range(1, kmax + 1):
        C.np_hess(Hd, G, Minv, cs["coef"][:, k - 1], cs["coef2"][:, k - 1], H[k, k - 1] ** 2, cs["beta0"], k, 0.5, 2 if k <= 2 else 1)
        g, _ = C.ref_hess_row(H, k)
        assert np.array_equal(C.fl(g), G[k - 1, :k])
    assert np.array_equal(np.triu(Hd[:kmax + 1, :kmax], -1), H) and np.array_equal(G[:kmax, :kmax], H.T @ H)


def test_condition_cap_of_every_solve_case():
    for name, cs in C.krylov_cases():
        assert cs["k"] >= 12, "the Krylov case is too shallow to mean anything"
        assert C.cap_value(cs["GA"] + cs["lam"] * cs["GL"]) <= C.CAP, name
        assert np.linalg.cond(cs["GA"]) > 1e6, name                  # the Gram data are conditioned as the solvers' are
        assert "reorth" in name or np.linalg.cond(cs["GA"] + cs["lam"] * cs["GL"]) > 1e8, name
    for k in sorted(set(C.SIZES + C.CHOL_SIZES)):
        cs = C.random_gram(k)
        assert C.cap_value(cs["GA"] + cs["lam"] * cs["GL"]) <= C.CAP, k
        assert C.cap_value(C.exact_border(k)["M"]) <= C.CAP, k
    for name, H, beta0, lam, kmax in C.hess_cases():
        assert kmax >= 12, name
        for k in sorted(k for k in set(C.HESS_CHECK_K) | {87, 88, 139, kmax // 2, kmax} if k <= kmax):     # every k a solve is checked at
            assert C.cap_value(H[:k + 1, :k].T @ H[:k + 1, :k] + lam * np.eye(k)) <= C.CAP, (name, k)
    H = C.exact_hess(C.EXACT_HESS_KMAX)["H"]                        # the integer chain (lam = 0 at k = 1)
    for k in C.HESS_CHECK_K:
        assert C.cap_value(H[:k + 1, :k].T @ H[:k + 1, :k] + (0.0 if k == 1 else C.EXACT_HESS_LAM) * np.eye(k)) <= C.CAP, k
    # (the exact bordered operands at 1024 and 2048 are held to equality with integers: nothing can be lifted or lost there)


@pytest.mark.parametrize("k", [1, 2, 7, 17, 66, 130])
def test_sum_and_product_bounds_hold_for_the_restatements(k):
    rng = np.random.default_rng(k)
    cs = C.random_gram(k)
    G = cs["GA"] / np.linalg.norm(cs["GA"], 2) * 0.9
    h = rng.standard_normal(k)
    rr = float(h @ h) * 10.0
    for passes in (1, 2, 3):
        c, rho2 = C.np_cgs(G, h, passes, rr)
        cr, e, v, vb = C.ref_cgs(G, h, passes, rr)
        assert np.all(np.abs(c - C.fl(cr)) <= e + C.U * np.abs(c))
        assert abs(rho2 - float(v)) <= vb + C.U * abs(rho2)
    a, cc, rhs = rng.standard_normal(k), 1e-3 * rng.standard_normal(k), rng.standard_normal(k)
    row, diag, rk = C.np_gram_row(cs["GA"], a, cc, 3.3, 0.7, rhs, 0.4)
    (rr_, rb), (dd_, db), (kk_, kb) = C.ref_gram_row(cs["GA"], a, cc, 3.3, 0.7, rhs, 0.4)
    assert np.all(np.abs(row - C.fl(rr_)) <= rb) and abs(diag - float(dd_)) <= db and abs(rk - float(kk_)) <= kb


def test_cholesky_bound_holds_for_the_restatement_and_cpu_engine():
    from cpu_engine import CpuEngine, CpuScalars
    eng = CpuEngine()
    cases = [cs for _, cs in C.krylov_cases()] + [C.random_gram(k) for k in (1, 2, 17, 66, 139)]
    for cs in cases:
        k, lam = cs["k"], cs["lam"]
        Md, cd = C.gram_matrix(cs["GA"], cs["GL"], lam), C.dec(cs["c"])
        y = C.np_chol_solve(cs["GA"] + lam * cs["GL"], cs["c"])
        bound = C.chol_bound(cs["GA"], cs["GL"], lam)
        assert C.backward_error(Md, cd, y) <= bound
        S = CpuScalars(2 * k * k + 2 * k)
        S.set(0, np.concatenate((cs["GA"].reshape(-1), cs["GL"].reshape(-1), cs["c"])))
        eng.gram_tikhonov(S.ref(0), k, S.ref(k * k), k, S.ref(2 * k * k), k, lam, S.ref(2 * k * k + k))
        assert C.backward_error(Md, cd, S.host(2 * k * k + k, 2 * k * k + 2 * k)) <= bound


def test_hessenberg_bounds_hold_for_the_restatement():
    for name, H, beta0, lam, kmax in C.hess_cases():
        if kmax > 139:
            continue
        coef, coef2, nrm2, Hs = C.hess_split(H)
        Hd, G = np.full((kmax + 1, kmax), np.nan), np.full((kmax, kmax), np.nan)
        for k in range(1, kmax + 1):
            y = C.np_hess(Hd, G, None, coef[:, k - 1], coef2[:, k - 1], nrm2[k - 1], beta0, k, lam, 0)
            if k in (1, 2, kmax // 2, kmax):
                g, gb = C.ref_hess_row(Hs, k)
                assert np.all(np.abs(G[k - 1, :k] - C.fl(g)) <= gb), (name, k)
                Md, cd = C.hess_system(Hs, beta0, lam, k)
                assert C.backward_error(Md, cd, y) <= C.hess_chol_bound(Hs, lam, k), (name, k)
        assert np.array_equal(np.triu(Hd, -1), Hs)


def test_bordered_inverse_constants_are_what_the_docstring_records():
    worst = C.measure_border_bar()
    for fam, (fwd, inv) in C.BORDER.items():
        got = [v for n, v in worst.items() if C.border_family(n) == fam]
        f, i = max(v[0] for v in got), max(v[1] for v in got)
        assert f <= fwd and i <= inv, (fam, f, i)
        assert f > fwd / 2 and i > inv / 2, ("the recorded constants are stale", fam, f, i)
        assert f"recorded {fwd:g}, {inv:g}" in C.__doc__ and f"{fam} {8 * fwd:g}, {8 * inv:g}" in C.__doc__, fam
        assert C.border_bars({"well": "random-5", "ill": "krylov-plain", "hess": "hess-x"}[fam]) == (8 * fwd, 8 * inv)


def _bidiag_sets():
    out = [("gk", k, C.gk_bidiag(k)) for k in (1, 2, 17, 65, 128)]
    return out + [("random", k, C.random_bidiag(k)) for k in (1, 2, 63, 64, 65, 1000, 2048)]


def test_bidiagonal_bound_holds_for_restatement_cpu_engine_and_host_code():
    from cpu_engine import CpuEngine, CpuScalars
    from trips_py_amd import _lib
    lib = _lib.load()
    eng = CpuEngine()
    for name, k, (a2, b2, b02) in _bidiag_sets():
        for mu in C.MUS:
            y = C.np_bidiag(a2, b2, k, mu, b02)
            res, bound = C.bidiag_residual(a2, b2, b02, mu, y)
            assert res <= bound, (name, k, mu, res / bound)
            yo = C.np_bidiag(a2, b2, k, mu, b02, y_over_alpha=True)
            assert np.all(np.abs(yo * np.sqrt(a2) - y) <= 4 * C.U * np.abs(y))
            # resumed in chunks = restarted, bit for bit
            st = {}
            for kk in sorted({1, max(1, k // 3), max(1, k // 3) + 1, k - 1, k} - {0}):
                yk = C.np_bidiag(a2, b2, min(kk, k), mu, b02, state=st)
            assert np.array_equal(yk, y)
            # libtrk's host code from alpha, beta themselves (its operands are the roots)
            al, be, yh = np.sqrt(a2), np.sqrt(b2), np.empty(k)
            assert lib.trk_host_bidiag_tikhonov(al.ctypes.data, be.ctypes.data, k, float(np.sqrt(b02)), float(mu), 0, yh.ctypes.data) == 0
            res, bound = C.bidiag_residual(al * al, be * be, float(np.sqrt(b02)) ** 2, mu, yh)
            assert res <= bound + 8 * C.U * (float(np.max(al * al + be * be + mu * mu)) * np.linalg.norm(yh) + np.sqrt(b02) * al[0]), (name, k, mu)
            if k <= 65:                                              # (cpu_engine solves the stacked system densely)
                S = CpuScalars(2 * k + 1 + k)
                S.set(0, np.concatenate(([b02], np.stack((a2, b2), axis=1).reshape(-1))))
                eng.bidiag_tikhonov(S.ref(1), 2, S.ref(2), 2, k, mu, S.ref(0), S.ref(2 * k + 1))
                res, bound = C.bidiag_residual(a2, b2, b02, mu, S.host(2 * k + 1, 3 * k + 1))
                assert res <= bound, (name, k, mu, "cpu_engine")


def test_cpu_engine_cgs_coeffs_passes_the_exact_and_general_cases():
    from cpu_engine import CpuEngine, CpuScalars
    eng = CpuEngine()
    for k in (1, 5, 17, 66):
        cs = C.exact_cgs(k)
        S = CpuScalars(k * k + 3 * k)
        S.set(0, np.concatenate((cs["G"].reshape(-1), cs["h"], cs["g_new"])))
        for passes in (0, 1, 2, 3):
            eng.cgs_coeffs(S.ref(0), k, S.ref(k * k), S.ref(k * k + k), k, passes, S.ref(k * k + 2 * k))
            if passes:
                assert np.array_equal(S.host(k * k + 2 * k, k * k + 3 * k), np.array([float(v) for v in C.int_cgs(cs["G"], cs["h"], passes)[0]]))
        rng = np.random.default_rng(k)
        G = C.random_gram(k)["GA"]
        G, h = G / np.linalg.norm(G, 2) * 0.9, rng.standard_normal(k)
        S.set(0, np.concatenate((G.reshape(-1), h)))
        eng.cgs_coeffs(S.ref(0), k, S.ref(k * k), None, k, 3, S.ref(k * k + 2 * k))
        cr, e = C.ref_cgs(G, h, 3)
        assert np.all(np.abs(S.host(k * k + 2 * k, k * k + 3 * k) - C.fl(cr)) <= e + C.U * np.abs(C.fl(cr)))
