"""The projected k x k solves (csrc/projected.hip) entry by entry: bit for bit on exact operands, within derived bounds of a
60-digit reference on general ones.  Operands, references, restatements and bounds: tests/projected_cases.py (checked on the CPU by
tests/test_projected_cases_host.py).  All calls go straight to the C ABI (engine.lib), so a refusal is seen as its return code.

Every device array lives between guard doubles that must be unchanged afterwards; outputs start as NaN; matrices have leading
dimensions larger than k with NaN in the padding and in the rows and columns beyond k, so a read outside the k x k block shows in the
result and a write there shows in the padding.  The worst deviation of every general case is logged as a fraction of its bound
(conftest.bar, limit 1) under projected.entrywise[...].

  entry point                          kernel, mode                                       covering test
  trk_cgs_coeffs, passes 0 .. 3        k_cgs_coeffs (rr = NULL)                           cgs_coeffs_exact, cgs_coeffs_general
  trk_cgs_coeffs_rho                   k_cgs_coeffs (rr, rho2_out; the 1e-300 lift)       cgs_coeffs_exact, cgs_coeffs_general
  trk_arnoldi_step                     k_finalize_cgs                                     finalize_cgs_through_arnoldi_step
  trk_gram_row_from_sweep              k_gram_row_from_sweep, with and without rhs / tb   gram_row_from_sweep_exact, .._general, k_caps
  trk_gks_rows_solve, ga_new           k_gks_rows_solve (install + row + border)          gks_rows_solve_exact, .._general, .._refusals
  trk_gks_rows_solve, a_A / s_A / tb   k_gks_rows_solve (row + row + border)              gks_rows_solve_exact, .._general, .._refusals
  trk_gram_tikhonov, Minv = NULL       k_gram_tikhonov, <= 64 KB of LDS (k <= 89)         gram_tikhonov_cholesky_exact, .._general
                                       k_gram_tikhonov, opt-in LDS (90 <= k <= 139)       gram_tikhonov_cholesky_exact, .._general, .._140
  trk_gram_tikhonov, Minv              k_gram_tikhonov_border: k_from = 0, rows one at    gram_tikhonov_bordered_exact, .._general, k_caps
                                       a time from 3, k - 3, k (y = Minv c alone)
  trk_hess_tikhonov, mode 2            k_hess_tikhonov: k = 1 (lam = 0), k = 2            hess_tikhonov_exact, .._general
  trk_hess_tikhonov, mode 1            k_hess_tikhonov: the chain to 258                  hess_tikhonov_exact, .._general
  trk_hess_tikhonov, mode 0            k_hess_tikhonov: <= 64 KB (k <= 87), opt-in        hess_tikhonov_cholesky_exact, hess_tikhonov_general,
                                       (88 <= k <= 139); coef2 NULL                       hess_tikhonov_refusals
  trk_bidiag_tikhonov, work = NULL     k_bidiag_tikhonov restarted (scratch)              bidiag_tikhonov, .._against_host_code, .._refusals
  trk_bidiag_tikhonov, work            k_bidiag_tikhonov resumed / restarted by the       bidiag_tikhonov_resumed_is_restarted
                                       state (chunks, a changed mu, a smaller k)
"""
import numpy as np
import pytest
import torch

import projected_cases as C
from conftest import bar

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 8
TRK_OK, TRK_EINVAL = 0, -1
NAN = float("nan")


@pytest.fixture(scope="module")
def eng():
    from trips_py_amd.engine import default_engine
    return default_engine()


class Buf:
    """Device doubles between guard doubles, filled from a host array (NaN where the kernel is to write)."""

    def __init__(self, eng, host):
        host = np.ascontiguousarray(np.atleast_1d(np.asarray(host, dtype=np.float64))).reshape(-1)
        self.n = host.size
        self.full = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=eng.device)
        self.v = self.full[GUARD:GUARD + self.n]
        self.v.copy_(torch.from_numpy(host))
        self.ptr = self.v.data_ptr()

    def at(self, i):
        return self.ptr + 8 * i

    def host(self):
        h = self.full.cpu().numpy()
        assert np.all(h[:GUARD] == SENTINEL) and np.all(h[GUARD + self.n:] == SENTINEL), "guard doubles overwritten"
        return h[GUARD:GUARD + self.n].copy()


def nans(n):
    return np.full(int(n), NAN)


def padded(M, rows, ld):
    """M in the top left corner of a rows x ld array of NaN."""
    out = np.full((rows, ld), NAN)
    out[:M.shape[0], :M.shape[1]] = M
    return out


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def block(buf, rows, ld):
    return buf.host().reshape(rows, ld)


def log(name, value):
    bar(f"projected.entrywise[{name}]", value, 1.0)


# ------------------------------------------------------------------------------------------------------------ trk_cgs_coeffs
def _unset_last(G, k):
    out = G.copy()
    out[k - 1, :k] = NAN
    out[:k, k - 1] = NAN
    return out


@pytest.mark.parametrize("k", C.SIZES + C.BIG_SIZES)
def test_cgs_coeffs_exact(eng, k):
    lib, st = eng.lib, eng.stream()
    cs = C.exact_cgs(k)
    G, h = cs["G"], cs["h"]
    assert C.exact_headroom(G, h, 3) < 2.0 ** 53
    ld = k + 3
    full = padded(G, k + 1, ld)
    part = _unset_last(full, k)
    hB, gB, rrB = Buf(eng, h), Buf(eng, cs["g_new"]), Buf(eng, [cs["rr"], 0.0, 0.0])
    Gd = Buf(eng, part)                                             # install only, h and c NULL
    assert lib.trk_cgs_coeffs(Gd.ptr, ld, None, gB.ptr, k, 0, None, st) == TRK_OK
    got = block(Gd, k + 1, ld)
    assert same(got, full) and np.array_equal(got[k - 1, :k], got[:k, k - 1])
    for passes in (1, 2, 3):
        want, gc = C.float_cgs(G, h, passes)
        for with_new in (False, True):
            Gd, cB = Buf(eng, part if with_new else full), Buf(eng, nans(k))
            assert lib.trk_cgs_coeffs(Gd.ptr, ld, hB.ptr, gB.ptr if with_new else None, k, passes, cB.ptr, st) == TRK_OK
            assert np.array_equal(cB.host(), want), (passes, with_new)
            assert same(block(Gd, k + 1, ld), full)
        if passes == 1:
            assert np.array_equal(cB.host(), h)
        ch, cgc = float(want @ h), float(want @ gc)
        rrB.v[1], rrB.v[2] = 2.0 * ch - cgc, 2.0 * ch - cgc - 1.0      # the sum comes out 0, then -1: the documented lift
        for j, rho_want in enumerate((cs["rr"] - 2.0 * ch + cgc, 1e-300, 1e-300)):
            Gd, c2, rho = Buf(eng, part), Buf(eng, nans(k)), Buf(eng, nans(1))
            assert lib.trk_cgs_coeffs_rho(Gd.ptr, ld, hB.ptr, gB.ptr, k, passes, c2.ptr, rrB.at(j), rho.ptr, st) == TRK_OK
            assert np.array_equal(c2.host(), cB.host()) and same(block(Gd, k + 1, ld), full)
            assert rho.host()[0] == rho_want and rho_want > 0.0, (passes, j)
    hB.host(), gB.host()


def _general_gram(k):
    cs = C.random_gram(k)
    return cs["GA"] / np.linalg.norm(cs["GA"], 2) * 0.9


@pytest.mark.parametrize("k", C.SIZES)
def test_cgs_coeffs_general(eng, k):
    lib, st = eng.lib, eng.stream()
    rng = np.random.default_rng(k)
    G, h = _general_gram(k), rng.standard_normal(k)
    rr = 10.0 * float(h @ h)
    ld = k + 1
    full = padded(G, k + 2, ld)
    hB, rrB = Buf(eng, h), Buf(eng, [rr])
    worst_c = worst_rho = 0.0
    for passes in (2, 3):
        cr, e, v, vb = C.ref_cgs(G, h, passes, rr)
        Gd, cB, c2, rho = Buf(eng, full), Buf(eng, nans(k)), Buf(eng, nans(k)), Buf(eng, nans(1))
        assert lib.trk_cgs_coeffs(Gd.ptr, ld, hB.ptr, None, k, passes, cB.ptr, st) == TRK_OK
        assert lib.trk_cgs_coeffs_rho(Gd.ptr, ld, hB.ptr, None, k, passes, c2.ptr, rrB.ptr, rho.ptr, st) == TRK_OK
        assert np.array_equal(c2.host(), cB.host()) and same(block(Gd, k + 2, ld), full)
        Gn, gB, c3 = Buf(eng, _unset_last(full, k)), Buf(eng, G[k - 1]), Buf(eng, nans(k))          # the newest row installed by the call
        assert lib.trk_cgs_coeffs(Gn.ptr, ld, hB.ptr, gB.ptr, k, passes, c3.ptr, st) == TRK_OK
        assert np.array_equal(c3.host(), cB.host()) and same(block(Gn, k + 2, ld), full)
        worst_c = max(worst_c, C.frac(C.diff(cB.host(), cr), e))
        worst_rho = max(worst_rho, C.frac(C.diff(rho.host(), [v]), vb))
    log(f"cgs_coeffs.c,k={k}", worst_c)
    log(f"cgs_coeffs_rho.rho2,k={k}", worst_rho)


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 129])
def test_finalize_cgs_through_arnoldi_step(eng, k):
    """k_finalize_cgs (inside trk_arnoldi_step) against trk_gemv_t2 + trk_cgs_coeffs(passes = 2) + trk_gemv_n + the normalisation:
    G, c, the new basis vector and S, bit for bit; one run."""
    from oracle import cpu_ref as O
    from trips_py_amd.engine import Coef
    from trips_py_amd.operators import Blur2D
    N = 64
    n = N * N
    A = Blur2D(O.gauss_psf((9, 9), (2, 2))[0], N, N, engine=eng)
    rng = np.random.default_rng(k)
    Q, _ = np.linalg.qr(rng.standard_normal((n, k)))
    Vh = np.ascontiguousarray(Q.T).astype(np.float32)
    ldg = k + 2
    G0 = padded((Vh.astype(np.float64) @ Vh.astype(np.float64).T)[:k - 1, :k - 1], k + 1, ldg)     # row k - 1 comes with the step
    res = []
    for one_call in (True, False):
        V = torch.zeros((k + 2, n), dtype=torch.float32, device=eng.device)
        V[:k].copy_(torch.from_numpy(Vh))
        V[k:] = NAN
        w = torch.full((n,), NAN, dtype=torch.float32, device=eng.device)
        Gd, W, S = Buf(eng, G0.reshape(-1)), Buf(eng, nans(2 * k)), Buf(eng, nans(1 + k))
        if one_call:
            eng.arnoldi_step(A._h, V, k, w, Gd.ptr, ldg, W.ptr, S.ptr)
        else:
            A.apply(V[k - 1], out=w)
            eng.gemv_t2(V, k, w, V[k - 1], W.ptr)
            eng.cgs_coeffs(Gd.ptr, ldg, W.ptr, W.at(k), k, 2, S.at(1))
            eng.gemv_n(V, k, S.at(1), V[k], a=1.0, base=w, s=-1.0, sumsq=S.ptr)
            eng.scale(Coef(1.0, den=S.ptr, sqrt_den=True), V[k], V[k])
        res.append((Gd.host(), S.host(), V.cpu().numpy(), W.host()))
    (G1, S1, V1, W1), (G5, S5, V5, W5) = res
    assert same(G1, G5) and same(S1, S5) and same(V1, V5) and same(W1, W5)
    got = G1.reshape(k + 1, ldg)
    assert np.all(np.isfinite(got[:k, :k])) and np.array_equal(got[k - 1, :k], got[:k, k - 1]) and np.all(np.isfinite(S1))
    assert np.all(np.isnan(got[k:])) and np.all(np.isnan(got[:, k:])) and np.all(np.isnan(V1[k + 1])) and np.all(np.isfinite(V1[k]))


# ------------------------------------------------------------------------------------------------------------ trk_gram_row_from_sweep
def _row_expected(G, k, ld, row, diag):
    want = padded(G, k + 2, ld)
    want[k, :k], want[:k, k], want[k, k] = row, row, diag
    return want


@pytest.mark.parametrize("k", C.SIZES + C.BIG_SIZES)
def test_gram_row_from_sweep_exact(eng, k):
    lib, st = eng.lib, eng.stream()
    gr = C.exact_gram_row(k)
    assert C.exact_headroom(gr["G"], gr["c"], 1, a=gr["a"], rhs=gr["rhs"]) < 2.0 ** 51
    row, diag, rk = C.np_gram_row(gr["G"], gr["a"], gr["c"], gr["s"], gr["rho2"], gr["rhs"], gr["tb"])     # exact here: host test
    ld = k + 4
    aB, cB, sc = Buf(eng, gr["a"]), Buf(eng, gr["c"]), Buf(eng, [gr["s"], gr["rho2"], gr["tb"]])
    for with_rhs in (False, True):
        Gd, rhs = Buf(eng, padded(gr["G"], k + 2, ld)), Buf(eng, np.concatenate((gr["rhs"], [NAN, NAN])))
        assert lib.trk_gram_row_from_sweep(Gd.ptr, ld, k, aB.ptr, cB.ptr, sc.at(0), sc.at(1), rhs.ptr if with_rhs else None,
                                           sc.at(2) if with_rhs else None, st) == TRK_OK
        got = block(Gd, k + 2, ld)
        assert same(got, _row_expected(gr["G"], k, ld, row, diag)) and np.array_equal(got[k, :k], got[:k, k])
        assert same(rhs.host(), np.concatenate((gr["rhs"], [rk if with_rhs else NAN, NAN])))
    aB.host(), cB.host(), sc.host()


@pytest.mark.parametrize("k", C.SIZES)
def test_gram_row_from_sweep_general(eng, k):
    lib, st = eng.lib, eng.stream()
    rng = np.random.default_rng(1000 + k)
    G = C.random_gram(k)["GA"]
    a, c, rhs = rng.standard_normal(k) * np.sqrt(k), 1e-3 * rng.standard_normal(k), rng.standard_normal(k)
    s, rho2, tb = 3.3 * k, 0.7, 0.4
    (rr, rb), (dd, db), (kk, kb) = C.ref_gram_row(G, a, c, s, rho2, rhs, tb)
    ld = k + 2
    Gd, rB = Buf(eng, padded(G, k + 1, ld)), Buf(eng, np.concatenate((rhs, [NAN])))
    aB, cB, sc = Buf(eng, a), Buf(eng, c), Buf(eng, [s, rho2, tb])
    assert lib.trk_gram_row_from_sweep(Gd.ptr, ld, k, aB.ptr, cB.ptr, sc.at(0), sc.at(1), rB.ptr, sc.at(2), st) == TRK_OK
    got = block(Gd, k + 1, ld)
    assert np.array_equal(got[k, :k], got[:k, k]) and same(got[:k, :k], G) and np.all(np.isnan(got[:, k + 1:]))
    log(f"gram_row.row,k={k}", C.frac(C.diff(got[k, :k], rr), rb))
    log(f"gram_row.diag,k={k}", C.frac(C.diff(got[k, k], [dd]), db))
    log(f"gram_row.rhs,k={k}", C.frac(C.diff(rB.host()[k], [kk]), kb))
    assert np.array_equal(rB.host()[:k], rhs)


def test_k_caps_are_refusals_without_a_launch(eng):
    """k = 2049 on trk_gram_row_from_sweep and on the bordered trk_gram_tikhonov: TRK_EINVAL, nothing written (the arrays are a few
    doubles: a refusal never reads them)."""
    lib, st = eng.lib, eng.stream()
    bufs = [Buf(eng, nans(16)) for _ in range(6)]
    G, a, c, s, M, y = bufs
    assert lib.trk_gram_row_from_sweep(G.ptr, 4096, 2049, a.ptr, c.ptr, s.at(0), s.at(1), None, None, st) == TRK_EINVAL
    assert lib.trk_gram_tikhonov(G.ptr, 4096, a.ptr, 4096, c.ptr, 2049, 0.5, M.ptr, 4096, 2049, y.ptr, st) == TRK_EINVAL
    assert lib.trk_gram_tikhonov(G.ptr, 4096, a.ptr, 4096, c.ptr, 2049, 0.5, M.ptr, 4096, 0, y.ptr, st) == TRK_EINVAL
    assert lib.trk_cgs_coeffs(G.ptr, 4096, a.ptr, None, 2049, 1, c.ptr, st) == TRK_EINVAL
    assert all(np.all(np.isnan(b.host())) for b in bufs)


# ------------------------------------------------------------------------------------------------------------ trk_gks_rows_solve
def _sweep_products(G, k, row, diag, c, rho2=4.0):
    """a, s with which gram_row_from_sweep yields (row, diag) from the leading k x k block of G and coefficients c, for rho2 = 4
    on integers (exact); in general the products that yield them but for rounding."""
    gc = G[:k, :k] @ c
    a = np.sqrt(rho2) * row + gc
    return a, rho2 * diag + 2.0 * (c @ a) - c @ gc


def _gks_run(eng, fused, sweep_A, GA, GL, n, ldg, ldm, Minv0, k_from, c_sweep, rhs, lam, prod):
    """Row k = n - 1 of both Gram matrices and the bordered solve over n vectors: one launch, or the launches it replaces."""
    lib, st = eng.lib, eng.stream()
    k = n - 1
    GAd, GLd = Buf(eng, padded(GA[:k, :k], n + 1, ldg)), Buf(eng, padded(GL[:k, :k], n + 1, ldg))
    Md, y = Buf(eng, Minv0), Buf(eng, nans(n + 1))
    cB, sc = Buf(eng, c_sweep), Buf(eng, [prod["s_A"], prod["s_L"], prod["tb"], prod["rho2"]])
    aA, aL, gn = Buf(eng, prod["a_A"]), Buf(eng, prod["a_L"]), Buf(eng, GA[k, :n])
    r = Buf(eng, np.concatenate((rhs[:k], [NAN if sweep_A else rhs[k], NAN])))
    if fused:
        rc = lib.trk_gks_rows_solve(GAd.ptr, GLd.ptr, ldg, k, None if sweep_A else gn.ptr, aA.ptr if sweep_A else None,
                                    sc.at(0) if sweep_A else None, sc.at(2) if sweep_A else None, aL.ptr, sc.at(1), cB.ptr, sc.at(3),
                                    r.ptr, lam, Md.ptr, ldm, k_from, y.ptr, st)
        assert rc == TRK_OK
    else:
        if sweep_A:
            assert lib.trk_gram_row_from_sweep(GAd.ptr, ldg, k, aA.ptr, cB.ptr, sc.at(0), sc.at(3), r.ptr, sc.at(2), st) == TRK_OK
        else:
            assert lib.trk_cgs_coeffs(GAd.ptr, ldg, None, gn.ptr, n, 0, None, st) == TRK_OK
        assert lib.trk_gram_row_from_sweep(GLd.ptr, ldg, k, aL.ptr, cB.ptr, sc.at(1), sc.at(3), None, None, st) == TRK_OK
        assert lib.trk_gram_tikhonov(GAd.ptr, ldg, GLd.ptr, ldg, r.ptr, n, lam, Md.ptr, ldm, k_from, y.ptr, st) == TRK_OK
    for b in (cB, sc, aA, aL, gn):
        b.host()
    return GAd.host(), GLd.host(), Md.host(), r.host(), y.host()


def _gks_products(GA, GL, n, c_sweep, rhs, rho2):
    k = n - 1
    a_A, s_A = _sweep_products(GA, k, GA[k, :k], GA[k, k], c_sweep, rho2)
    a_L, s_L = _sweep_products(GL, k, GL[k, :k], GL[k, k], c_sweep, rho2)
    return {"a_A": a_A, "s_A": s_A, "a_L": a_L, "s_L": s_L, "tb": np.sqrt(rho2) * rhs[k] + c_sweep @ rhs[:k], "rho2": rho2}


@pytest.mark.parametrize("n", [n for n in C.SIZES if n >= 2] + C.BIG_SIZES)
def test_gks_rows_solve_exact(eng, n):
    cs = C.exact_border(n)
    GA, GL, rhs = cs["GA"], cs["GL"], cs["c"]
    k = n - 1
    c_sweep = C.small_ints(np.random.default_rng(n), k)
    prod = _gks_products(GA, GL, n, c_sweep, rhs, 4.0)
    ldg, ldm = n + 2, n + 1
    want_inv = C.exact_border_inverse(cs["p"], n)
    for k_from in ((k, 0) if n <= 17 else (k,)):
        Minv0 = padded(C.exact_border_inverse(cs["p"], k_from), n + 1, ldm) if k_from else np.full((n + 1, ldm), NAN)
        for sweep_A in (False, True):
            one = _gks_run(eng, True, sweep_A, GA, GL, n, ldg, ldm, Minv0, k_from, c_sweep, rhs, 0.5, prod)
            three = _gks_run(eng, False, sweep_A, GA, GL, n, ldg, ldm, Minv0, k_from, c_sweep, rhs, 0.5, prod)
            assert all(same(a, b) for a, b in zip(one, three)), (k_from, sweep_A)
            ga, gl, mi, r, y = one
            assert same(ga.reshape(n + 1, ldg), padded(GA, n + 1, ldg)) and same(gl.reshape(n + 1, ldg), padded(GL, n + 1, ldg))
            assert same(mi.reshape(n + 1, ldm), padded(want_inv, n + 1, ldm))
            assert same(r, np.concatenate((rhs, [NAN]))) and same(y, np.concatenate((want_inv @ rhs, [NAN])))


@pytest.mark.parametrize("name", [n for n, _ in C.krylov_cases()])
def test_gks_rows_solve_general(eng, name):
    cs = dict(C.krylov_cases())[name]
    n, lam = cs["k"], cs["lam"]
    GA, GL, rhs = cs["GA"], cs["GL"], cs["c"]
    k = n - 1
    c_sweep = 1e-7 * np.random.default_rng(n).standard_normal(k)
    prod = _gks_products(GA, GL, n, c_sweep, rhs, 0.81)
    ldg, ldm = n + 3, n + 2
    Minv0 = np.full((n + 1, ldm), NAN)                              # (the inverse is built from nothing: k_from = 0)
    for sweep_A in (False, True):
        one = _gks_run(eng, True, sweep_A, GA, GL, n, ldg, ldm, Minv0, 0, c_sweep, rhs, lam, prod)
        three = _gks_run(eng, False, sweep_A, GA, GL, n, ldg, ldm, Minv0, 0, c_sweep, rhs, lam, prod)
        assert all(same(a, b) for a, b in zip(one, three)), sweep_A
        ga, gl, mi, r, y = one
        ga, gl, mi = ga.reshape(n + 1, ldg), gl.reshape(n + 1, ldg), mi.reshape(n + 1, ldm)
        assert np.array_equal(mi[:n, :n], mi[:n, :n].T) and np.array_equal(ga[k, :k], ga[:k, k]) and np.array_equal(gl[k, :k], gl[:k, k])
        assert np.all(np.isnan(ga[:, n:])) and np.all(np.isnan(ga[n:])) and np.all(np.isnan(mi[:, n:])) and np.isnan(y[n])
        # the solve against the reference on the Gram rows the device itself formed (their own bounds: gram_row_from_sweep_general)
        Md = C.gram_matrix(ga[:n, :n], gl[:n, :n], lam)
        cond = np.linalg.cond(ga[:n, :n] + lam * gl[:n, :n])
        fwd, _ = C.border_bars(name)
        log(f"gks_rows_solve.y,{name},{'sweep' if sweep_A else 'ga_new'}", C.forward_ratio(y[:n], C.ref_solve(Md, C.dec(r[:n])), cond) / fwd)


def test_gks_rows_solve_refusals(eng):
    lib, st = eng.lib, eng.stream()
    n = 5
    k = n - 1
    B = {name: Buf(eng, nans((n + 1) * (n + 1))) for name in ("GA", "GL", "Minv")}
    B.update({name: Buf(eng, nans(n + 1)) for name in ("ga_new", "a_A", "a_L", "c", "rhs", "y", "sc")})

    def call(**kw):
        a = dict(GA=B["GA"].ptr, GL=B["GL"].ptr, ldg=n + 1, k=k, ga_new=B["ga_new"].ptr, a_A=None, s_A=None, tb=None, a_L=B["a_L"].ptr,
                 s_L=B["sc"].at(1), c=B["c"].ptr, rho2=B["sc"].at(3), rhs=B["rhs"].ptr, lam=0.5, Minv=B["Minv"].ptr, ldm=n + 1, k_from=k,
                 y=B["y"].ptr)
        a.update(kw)
        return lib.trk_gks_rows_solve(*a.values(), st)

    sweep = dict(ga_new=None, a_A=B["a_A"].ptr, s_A=B["sc"].at(0), tb=B["sc"].at(2))
    bad = [dict(GA=None), dict(GL=None), dict(a_L=None), dict(s_L=None), dict(c=None), dict(rho2=None), dict(rhs=None), dict(Minv=None),
           dict(y=None), dict(k=0), dict(ldg=k), dict(ldm=k), dict(ga_new=None), dict(a_A=B["a_A"].ptr),
           dict(sweep, s_A=None), dict(sweep, tb=None), dict(k_from=-1), dict(k_from=n + 1), dict(k=2048, ldg=4096, ldm=4096, k_from=0)]
    for kw in bad:
        assert call(**kw) == TRK_EINVAL, kw
    assert all(np.all(np.isnan(b.host())) for b in B.values())


# ------------------------------------------------------------------------------------------------------------ trk_gram_tikhonov
@pytest.mark.parametrize("k", sorted(set(C.CHOL_SIZES)))
def test_gram_tikhonov_cholesky_exact(eng, k):
    lib, st = eng.lib, eng.stream()
    cs = C.exact_chol(k)
    lda, ldl = k + 1, k + 5
    GAd, GLd = Buf(eng, padded(cs["GA"], k + 1, lda)), Buf(eng, padded(cs["GL"], k + 1, ldl))
    cB, y = Buf(eng, np.concatenate((cs["c"], [NAN]))), Buf(eng, nans(k + 1))
    assert lib.trk_gram_tikhonov(GAd.ptr, lda, GLd.ptr, ldl, cB.ptr, k, 0.5, None, 0, 0, y.ptr, st) == TRK_OK
    assert same(y.host(), np.concatenate((cs["y"], [NAN])))
    assert same(block(GAd, k + 1, lda), padded(cs["GA"], k + 1, lda)) and same(block(GLd, k + 1, ldl), padded(cs["GL"], k + 1, ldl))
    cB.host()


def _chol_general_cases():
    return C.krylov_cases() + [(f"random-{k}", C.random_gram(k)) for k in sorted(set(C.CHOL_SIZES))]


@pytest.mark.parametrize("name", [n for n, _ in _chol_general_cases()])
def test_gram_tikhonov_cholesky_general(eng, name):
    lib, st = eng.lib, eng.stream()
    cs = dict(_chol_general_cases())[name]
    k, lam = cs["k"], cs["lam"]
    assert C.cap_value(cs["GA"] + lam * cs["GL"]) <= C.CAP
    lda, ldl = k + 3, k + 1
    GAd, GLd = Buf(eng, padded(cs["GA"], k + 1, lda)), Buf(eng, padded(cs["GL"], k + 1, ldl))
    cB, y = Buf(eng, np.concatenate((cs["c"], [NAN]))), Buf(eng, nans(k + 1))
    assert lib.trk_gram_tikhonov(GAd.ptr, lda, GLd.ptr, ldl, cB.ptr, k, lam, None, 0, 0, y.ptr, st) == TRK_OK
    got = y.host()
    assert np.isnan(got[k]) and np.all(np.isfinite(got[:k]))
    eta = C.backward_error(C.gram_matrix(cs["GA"], cs["GL"], lam), C.dec(cs["c"]), got[:k])
    log(f"gram_tikhonov.cholesky,{name}", eta / C.chol_bound(cs["GA"], cs["GL"], lam))
    GAd.host(), GLd.host(), cB.host()


def test_gram_tikhonov_cholesky_140_is_refused(eng):
    lib, st = eng.lib, eng.stream()
    k = 140
    cs = C.random_gram(k)
    GAd, GLd, cB, y = Buf(eng, cs["GA"]), Buf(eng, cs["GL"]), Buf(eng, cs["c"]), Buf(eng, nans(k))
    assert lib.trk_gram_tikhonov(GAd.ptr, k, GLd.ptr, k, cB.ptr, k, 0.5, None, 0, 0, y.ptr, st) == TRK_EINVAL
    assert lib.trk_gram_tikhonov(GAd.ptr, k - 1, GLd.ptr, k, cB.ptr, k, 0.5, None, 0, 0, y.ptr, st) == TRK_EINVAL
    assert lib.trk_gram_tikhonov(GAd.ptr, k, GLd.ptr, k, cB.ptr, k, 0.5, y.ptr, k - 1, 0, y.ptr, st) == TRK_EINVAL       # ldm < k
    assert lib.trk_gram_tikhonov(GAd.ptr, k, GLd.ptr, k, cB.ptr, k, 0.5, y.ptr, k, k + 1, y.ptr, st) == TRK_EINVAL       # k_from > k
    assert np.all(np.isnan(y.host())) and np.array_equal(GAd.host(), cs["GA"].reshape(-1))


def _border_schedules(k):
    out = {"from0": [(0, k)]}
    if k <= 130:
        out["rows"] = [(0, min(3, k))] + [(j - 1, j) for j in range(4, k + 1)]
    out["three"] = ([(0, k - 3)] if k > 3 else []) + [(max(k - 3, 0), k), (k, k)]
    return out


@pytest.mark.parametrize("k", C.SIZES + C.BIG_SIZES)
def test_gram_tikhonov_bordered_exact(eng, k):
    lib, st = eng.lib, eng.stream()
    cs = C.exact_border(k)
    lda, ldl, ldm = k + 1, k + 2, k + 3
    GAd, GLd = Buf(eng, padded(cs["GA"], k + 1, lda)), Buf(eng, padded(cs["GL"], k + 1, ldl))
    cB = Buf(eng, np.concatenate((cs["c"], [NAN])))
    want_inv = C.exact_border_inverse(cs["p"], k)
    if k > 258:                                                      # the inverse of k - 1 rows comes from the host: no O(k^3) launch
        scheds = {"last": [(k - 1, k), (k, k)]}
    else:
        scheds = _border_schedules(k)
    for name, sched in scheds.items():
        start = padded(C.exact_border_inverse(cs["p"], k - 1), k + 1, ldm) if k > 258 else np.full((k + 1, ldm), NAN)
        Md = Buf(eng, start)
        for k_from, kk in sched:
            y = Buf(eng, nans(k + 1))
            assert lib.trk_gram_tikhonov(GAd.ptr, lda, GLd.ptr, ldl, cB.ptr, kk, 0.5, Md.ptr, ldm, k_from, y.ptr, st) == TRK_OK
            if k <= 130 or kk == k:
                inv_kk = C.exact_border_inverse(cs["p"], kk)
                assert same(block(Md, k + 1, ldm), padded(inv_kk, k + 1, ldm)), (name, k_from, kk)
                assert same(y.host(), np.concatenate((inv_kk @ cs["c"][:kk], nans(k + 1 - kk)))), (name, k_from, kk)
    if k <= 139:                                                     # the Cholesky form on the same operands: the same integers
        y0 = Buf(eng, nans(k + 1))
        assert lib.trk_gram_tikhonov(GAd.ptr, lda, GLd.ptr, ldl, cB.ptr, k, 0.5, None, 0, 0, y0.ptr, st) == TRK_OK
        assert same(y0.host(), np.concatenate((want_inv @ cs["c"], [NAN])))
    assert same(block(GAd, k + 1, lda), padded(cs["GA"], k + 1, lda)) and same(block(GLd, k + 1, ldl), padded(cs["GL"], k + 1, ldl))
    cB.host()


def test_bordered_inverse_constants_are_logged():
    """The constants measured on the NumPy restatement (tests/projected_cases.py, recomputed by the host test) next to their bars,
    8 x each, in the record of this run: border.measured[family.quantity] constant bar, in units of cond_2(M) 2^-53."""
    for fam, (fwd, inv) in C.BORDER.items():
        bars = C.border_bars({"well": "random", "ill": "krylov-plain", "hess": "hess"}[fam])
        assert bars == (C.BAR_FACTOR * fwd, C.BAR_FACTOR * inv)
        bar(f"projected.border.measured[{fam}.forward]", fwd, bars[0])
        bar(f"projected.border.measured[{fam}.inverse]", inv, bars[1])


@pytest.mark.parametrize("name", [n for n, _, _ in C.border_cases()])
def test_gram_tikhonov_bordered_general(eng, name):
    lib, st = eng.lib, eng.stream()
    _, cs, sched = next(c for c in C.border_cases() if c[0] == name)
    kmax, lam = cs["k"], cs["lam"]
    lda, ldl, ldm = kmax + 1, kmax + 2, kmax + 3
    GAd, GLd = Buf(eng, padded(cs["GA"], kmax + 1, lda)), Buf(eng, padded(cs["GL"], kmax + 1, ldl))
    cB, Md = Buf(eng, np.concatenate((cs["c"], [NAN]))), Buf(eng, np.full((kmax + 1, ldm), NAN))
    for k_from, k in sched:
        y = Buf(eng, nans(kmax + 1))
        assert lib.trk_gram_tikhonov(GAd.ptr, lda, GLd.ptr, ldl, cB.ptr, k, lam, Md.ptr, ldm, k_from, y.ptr, st) == TRK_OK
        mi = block(Md, kmax + 1, ldm)
        assert np.array_equal(mi[:k, :k], mi[:k, :k].T) and np.all(np.isfinite(mi[:k, :k])), (k_from, k)
        assert np.all(np.isnan(mi[k:])) and np.all(np.isnan(mi[:, k:])), (k_from, k)
    got = y.host()
    assert np.isnan(got[k]) and k == kmax
    GA, GL = cs["GA"], cs["GL"]
    cond = np.linalg.cond(GA + lam * GL)
    Mref, cref = C.gram_matrix(GA, GL, lam), C.dec(cs["c"])
    fwd, inv = C.border_bars(name)
    log(f"gram_tikhonov.border.y,{name}", C.forward_ratio(got[:k], C.ref_solve(Mref, cref), cond) / fwd)
    log(f"gram_tikhonov.border.inverse,{name}", C.inverse_ratio(mi[:k, :k], C.long_matrix(GA, GL, lam), cond) / inv)
    if k <= 139:                                                     # against the Cholesky form: each within its own bound
        y0 = Buf(eng, nans(k))
        assert lib.trk_gram_tikhonov(GAd.ptr, lda, GLd.ptr, ldl, cB.ptr, k, lam, None, 0, 0, y0.ptr, st) == TRK_OK
        assert C.backward_error(Mref, cref, y0.host()) <= C.chol_bound(GA, GL, lam)
        rel = np.linalg.norm(got[:k] - y0.host()) / np.linalg.norm(y0.host())
        assert rel <= (fwd + 4.0 * k) * cond * C.U, rel
    GAd.host(), GLd.host(), cB.host()


# ------------------------------------------------------------------------------------------------------------ trk_hess_tikhonov
class HessDev:
    """H (column-major, ldh = kmax + 3), G and Minv (ldg = kmax + 2) on the device, NaN everywhere a call has not written."""

    def __init__(self, eng, kmax, H0=None, G0=None):
        self.eng, self.kmax, self.ldh, self.ldg = eng, kmax, kmax + 3, kmax + 2
        Hh, Gh = np.full((kmax + 1, self.ldh), NAN), np.full((kmax + 1, self.ldg), NAN)
        if H0 is not None:                                           # columns 0 .. j-1 as an earlier chain left them
            j = H0.shape[1]
            Hh[:j, :j + 1] = np.where(np.triu(np.ones((j + 1, j), dtype=bool), -1), H0, NAN).T     # nothing below the sub-diagonal
            Gh[:j, :j] = G0
        self.H, self.G, self.Minv = Buf(eng, Hh), Buf(eng, Gh), Buf(eng, np.full((kmax + 1, self.ldg), NAN))
        self.y = None

    def call(self, coef, coef2, nrm2_sq, beta0, k, lam, mode, minv=True):
        sc = Buf(self.eng, np.concatenate(([nrm2_sq], coef[:k], [NAN], coef2[:k] if coef2 is not None else [], [NAN])))
        self.y = Buf(self.eng, nans(self.kmax + 1))
        rc = self.eng.lib.trk_hess_tikhonov(self.H.ptr, self.ldh, self.G.ptr, self.Minv.ptr if minv else None, self.ldg, sc.at(1),
                                            sc.at(k + 2) if coef2 is not None else None, sc.at(0), beta0, k, lam, mode, self.y.ptr,
                                            self.eng.stream())
        sc.host()
        return rc

    def Hm(self):
        return block(self.H, self.kmax + 1, self.ldh).T              # (ldh x (kmax + 1)): rows = H's rows

    def Gm(self):
        return block(self.G, self.kmax + 1, self.ldg)

    def Mi(self):
        return block(self.Minv, self.kmax + 1, self.ldg)


def _hess_written(dev, k):
    """Only column k-1's k+1 entries of H, the leading k x k of G and Minv are set; everything else is still NaN."""
    Hm, G, Mi = dev.Hm(), dev.Gm(), dev.Mi()
    mask = np.triu(np.ones_like(Hm, dtype=bool), -1)
    mask[:, k:] = False
    assert np.all(np.isfinite(Hm[mask])) and np.all(np.isnan(Hm[~mask]))
    assert np.all(np.isfinite(G[:k, :k])) and np.all(np.isnan(G[k:])) and np.all(np.isnan(G[:, k:]))
    assert np.array_equal(G[:k, :k], G[:k, :k].T)
    return Hm, G, Mi


CHECK_K = set(C.HESS_CHECK_K)


def test_hess_tikhonov_exact(eng):
    """An integer Hessenberg matrix, column by column to 258: mode 2 (k = 1 with lam = 0, k = 2), then mode 1; every other column
    with coef2 NULL.  The stored columns and G = H^T H are exact; the solves are within the chain's bar of the reference."""
    kmax, lam = C.EXACT_HESS_KMAX, C.EXACT_HESS_LAM
    cs = C.exact_hess(kmax)
    H, beta0 = cs["H"], cs["beta0"]
    dev = HessDev(eng, kmax)
    worst = 0.0
    for k in range(1, kmax + 1):
        two = k % 2 == 0
        coef = cs["coef"][:, k - 1] if two else H[:, k - 1]
        lk = 0.0 if k == 1 else lam
        assert dev.call(coef, cs["coef2"][:, k - 1] if two else None, H[k, k - 1] ** 2, beta0, k, lk, 2 if k <= 2 else 1) == TRK_OK
        if k in CHECK_K:
            Hm, G, Mi = _hess_written(dev, k)
            assert np.array_equal(np.triu(Hm[:k + 1, :k], -1), H[:k + 1, :k]) and np.array_equal(G[:k, :k], H[:k + 1, :k].T @ H[:k + 1, :k])
            assert np.array_equal(Mi[:k, :k], Mi[:k, :k].T) and np.all(np.isnan(Mi[k:])) and np.all(np.isnan(Mi[:, k:]))
            y = dev.y.host()
            assert np.isnan(y[k])
            if k == 1:                                               # 1 / (H00^2 + H10^2) times beta0 H00: see below
                assert y[0] == (1.0 / G[0, 0]) * (beta0 * H[0, 0])
            Md, cd = C.hess_system(H, beta0, lk, k)
            cond = np.linalg.cond(Md.f)
            worst = max(worst, C.forward_ratio(y[:k], C.ref_solve(Md, cd), cond) / C.border_bars("hess")[0])
    log("hess_tikhonov.chain.y,integer-258", worst)
    log("hess_tikhonov.chain.inverse,integer-258", C.inverse_ratio(Mi[:kmax, :kmax], C.long_hess_matrix(H, lam, kmax), cond) / C.border_bars("hess")[1])
    # mode 2 at k = 1, lam = 0, a diagonal entry that is a power of two: exact
    one = HessDev(eng, 1)
    assert one.call(np.array([0.0]), None, 16.0, 3.0, 1, 0.0, 2) == TRK_OK
    assert one.Gm()[0, 0] == 16.0 and one.Mi()[0, 0] == 0.0625 and one.y.host()[0] == 0.0
    assert one.call(np.array([2.0]), np.array([2.0]), 0.0, 3.0, 1, 0.0, 2) == TRK_OK
    assert one.Gm()[0, 0] == 16.0 and one.Mi()[0, 0] == 0.0625 and one.y.host()[0] == 0.75 and same(one.Hm()[:2, 0], np.array([4.0, 0.0]))


@pytest.mark.parametrize("k", sorted(set(C.CHOL_SIZES)))
def test_hess_tikhonov_cholesky_exact(eng, k):
    """Mode 0 on H = [C^T; 0], lam = 0: G = C C^T and y = (beta0 / C00) e_1 exactly; columns 0 .. k-2 and their Gram block are
    uploaded, so one launch per size (87 / 88: the step to the opt-in LDS)."""
    cs = C.exact_chol(k)
    Cm = cs["C"]
    H = np.vstack((Cm.T, np.zeros((1, k))))
    dev = HessDev(eng, k, H[:k, :k - 1], cs["M"][:k - 1, :k - 1])
    assert dev.call(H[:, k - 1], None, 0.0, 3.0, k, 0.0, 0, minv=False) == TRK_OK
    Hm, G, Mi = _hess_written(dev, k)
    assert np.array_equal(np.triu(Hm[:k + 1, :k], -1), H) and np.array_equal(G[:k, :k], cs["M"]) and np.all(np.isnan(Mi))
    assert same(dev.y.host(), np.concatenate(([3.0 / Cm[0, 0]], np.zeros(k - 1), [NAN])))


@pytest.mark.parametrize("name", [c[0] for c in C.hess_cases()])
def test_hess_tikhonov_general(eng, name):
    _, H, beta0, lam, kmax = next(c for c in C.hess_cases() if c[0] == name)
    coef, coef2, nrm2, Hs = C.hess_split(H)
    dev = HessDev(eng, kmax)
    checks = sorted(k for k in CHECK_K | {87, 88, 139, kmax // 2, kmax} if k <= kmax)
    fwd_bar, inv_bar = C.border_bars("hess")
    worst = {"row": 0.0, "mode1": 0.0, "mode2": 0.0, "mode0": 0.0}
    for k in range(1, kmax + 1):
        mode = 2 if k <= 2 else 1
        assert dev.call(coef[:, k - 1], coef2[:, k - 1], nrm2[k - 1], beta0, k, lam, mode) == TRK_OK
        if k not in checks:
            continue
        Hm, G, Mi = _hess_written(dev, k)
        assert np.array_equal(np.triu(Hm[:k + 1, :k], -1), Hs[:k + 1, :k])      # the stored column: fl(coef + coef2), fl(sqrt(nrm2_sq))
        g, gb = C.ref_hess_row(Hs, k)
        worst["row"] = max(worst["row"], C.frac(C.diff(G[k - 1, :k], g), gb))
        Md, cd = C.hess_system(Hs, beta0, lam, k)
        cond = np.linalg.cond(Md.f)
        ystar = C.ref_solve(Md, cd)
        y = dev.y.host()
        assert np.isnan(y[k]) and np.array_equal(Mi[:k, :k], Mi[:k, :k].T)
        worst[f"mode{mode}"] = max(worst[f"mode{mode}"], C.forward_ratio(y[:k], ystar, cond) / fwd_bar)
        if k <= 139:                                                 # mode 0 on a copy of the chain's H and G, this column again
            d0 = HessDev(eng, k, Hm[:k, :k - 1], G[:k - 1, :k - 1])
            assert d0.call(coef[:, k - 1], coef2[:, k - 1], nrm2[k - 1], beta0, k, lam, 0, minv=False) == TRK_OK
            H0, G0, _ = _hess_written(d0, k)
            assert same(H0[:k + 1, :k], Hm[:k + 1, :k]) and np.array_equal(G0[:k, :k], G[:k, :k])
            worst["mode0"] = max(worst["mode0"], C.backward_error(Md, cd, d0.y.host()[:k]) / C.hess_chol_bound(Hs, lam, k))
    for key, v in worst.items():
        log(f"hess_tikhonov.{key},{name}", v)
    log(f"hess_tikhonov.inverse,{name}", C.inverse_ratio(Mi[:kmax, :kmax], C.long_hess_matrix(Hs, lam, kmax), cond) / inv_bar)


def test_hess_tikhonov_refusals(eng):
    lib, st = eng.lib, eng.stream()
    k = 3
    B = {n: Buf(eng, nans(32)) for n in ("H", "G", "Minv", "coef", "nrm", "y")}

    def call(**kw):
        a = dict(H=B["H"].ptr, ldh=k + 1, G=B["G"].ptr, Minv=B["Minv"].ptr, ldg=k, coef=B["coef"].ptr, coef2=None, nrm=B["nrm"].ptr,
                 beta0=1.0, k=k, lam=0.5, mode=1, y=B["y"].ptr)
        a.update(kw)
        return lib.trk_hess_tikhonov(*a.values(), st)

    bad = [dict(H=None), dict(G=None), dict(coef=None), dict(nrm=None), dict(y=None), dict(k=0), dict(ldh=k), dict(ldg=k - 1),
           dict(mode=-1), dict(mode=3), dict(mode=1, Minv=None), dict(mode=2, Minv=None, k=2), dict(mode=2), dict(mode=1, k=1),
           dict(mode=1, lam=0.0), dict(mode=0, k=140, ldh=141, ldg=140), dict(mode=0, lam=-1.0),
           dict(mode=1, k=6000, ldh=6001, ldg=6000)]              # 4 k + 1 doubles of LDS: beyond 160 KB, refused before any launch
    for kw in bad:
        assert call(**kw) == TRK_EINVAL, kw
    assert all(np.all(np.isnan(b.host())) for b in B.values())


# ------------------------------------------------------------------------------------------------------------ trk_bidiag_tikhonov
def _strided(eng, vals, stride):
    host = np.full(len(vals) * stride, NAN)
    host[::stride] = vals
    return Buf(eng, host)


def _bidiag(eng, a2B, sa, b2B, sb, k, mu, b0B, over=0, work=None):
    y = Buf(eng, nans(k + 1))
    rc = eng.lib.trk_bidiag_tikhonov(a2B.ptr, sa, b2B.ptr, sb, k, mu, b0B.ptr, y.ptr, over, None if work is None else work.ptr,
                                     0 if work is None else work.n, eng.stream())
    assert rc == TRK_OK
    got = y.host()
    assert np.isnan(got[k]) and np.all(np.isfinite(got[:k]))
    return got[:k]


BIDIAG_SETS = [("gk", k) for k in (1, 2, 17, 65, 128)] + [("random", k) for k in (1, 2, 63, 64, 65, 1000, 2048)]


@pytest.mark.parametrize("kind,k", BIDIAG_SETS)
def test_bidiag_tikhonov(eng, kind, k):
    """Restarted (work = NULL): the residual of the normal equations in the reference arithmetic within its bound, strides 1, 2, 3,
    mu = 0 among the values, y_over_alpha, and libtrk's host code at the tolerance tests/test_gpu_solvers.py uses."""
    a2, b2, b02 = C.gk_bidiag(k) if kind == "gk" else C.random_bidiag(k)
    b0B = Buf(eng, [b02])
    worst, ys = 0.0, {}
    for sa, sb in ((1, 1), (2, 3), (3, 2)):
        a2B, b2B = _strided(eng, a2, sa), _strided(eng, b2, sb)
        for mu in C.MUS:
            y = _bidiag(eng, a2B, sa, b2B, sb, k, mu, b0B)
            assert np.array_equal(ys.setdefault(mu, y), y)           # the strides change nothing
            res, bound = C.bidiag_residual(a2, b2, b02, mu, y)
            worst = max(worst, res / bound)
            yo = _bidiag(eng, a2B, sa, b2B, sb, k, mu, b0B, over=1)
            assert np.all(np.abs(yo * np.sqrt(a2) - y) <= 4 * C.U * np.abs(y))
        a2B.host(), b2B.host()
    log(f"bidiag_tikhonov.residual,{kind}-{k}", worst)


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 1000, 2048])
def test_bidiag_tikhonov_against_host_code(eng, k):
    """trk_host_bidiag_tikhonov (the same recurrence on the host) on the operands and at the tolerance of tests/test_gpu_solvers.py
    (alpha in [0.5, 1.5), beta in [0.1, 1.1), beta0 = 3.7, mu = 0.21; rtol 1e-12, atol 1e-14): an entry-wise tolerance fits only
    such well-conditioned bidiagonals; the others are held to the residual bound above."""
    rng = np.random.default_rng(k)
    al, be, beta0, mu = 0.5 + rng.random(k), 0.1 + rng.random(k), 3.7, 0.21
    a2B, b2B, b0B = _strided(eng, al ** 2, 2), _strided(eng, be ** 2, 2), Buf(eng, [beta0 ** 2])
    for over in (0, 1):
        y = _bidiag(eng, a2B, 2, b2B, 2, k, mu, b0B, over)
        yh = eng.host_bidiag_tikhonov(np.sqrt(al ** 2), np.sqrt(be ** 2), float(np.sqrt(beta0 ** 2)), mu, y_over_alpha=bool(over))
        assert np.allclose(yh, y, rtol=1e-12, atol=1e-14)


def _chunkings(k):
    one = list(range(1, k + 1)) if k <= 130 else None
    several = sorted(c for c in {1, 2, max(1, k // 3), max(1, k // 3) + 1, max(1, k - 5), max(1, k - 1), k} if c <= k)
    return [c for c in (one, several, [k]) if c]


@pytest.mark.parametrize("k", [1, 2, 17, 63, 64, 65, 1000, 2048])
def test_bidiag_tikhonov_resumed_is_restarted(eng, k):
    """With `work`: any chunking of k — one column at a time, several, all at once — then a changed mu and a smaller k: every call
    returns the bits of a restart (work = NULL) at the same k and mu; the state survives in a buffer of one constant size."""
    a2, b2, b02 = C.random_bidiag(k)
    a2B, b2B, b0B = _strided(eng, a2, 1), _strided(eng, b2, 2), Buf(eng, [b02])
    restart = {}

    def fresh(kk, mu, over=0):
        if (kk, mu, over) not in restart:
            restart[(kk, mu, over)] = _bidiag(eng, a2B, 1, b2B, 2, kk, mu, b0B, over)
        return restart[(kk, mu, over)]

    for mu in (0.0, 1e-2):
        for chunks in _chunkings(k):
            work = Buf(eng, np.zeros(3 * (k + 1) + 4))
            for kk in chunks:
                if len(chunks) <= 8 or kk in (1, 2, k // 2, k - 1, k):
                    assert np.array_equal(_bidiag(eng, a2B, 1, b2B, 2, kk, mu, b0B, 0, work), fresh(kk, mu)), (mu, kk)
                else:
                    _bidiag(eng, a2B, 1, b2B, 2, kk, mu, b0B, 0, work)
            assert np.array_equal(_bidiag(eng, a2B, 1, b2B, 2, k, mu, b0B, 1, work), fresh(k, mu, 1))        # same k: a restart
            assert np.array_equal(_bidiag(eng, a2B, 1, b2B, 2, k, mu + 0.25, b0B, 0, work), fresh(k, mu + 0.25))
            ks = max(1, k - 1)
            assert np.array_equal(_bidiag(eng, a2B, 1, b2B, 2, ks, mu + 0.25, b0B, 0, work), fresh(ks, mu + 0.25))
            assert np.array_equal(_bidiag(eng, a2B, 1, b2B, 2, k, mu + 0.25, b0B, 0, work), fresh(k, mu + 0.25))   # grown again
            work.host()
    a2B.host(), b2B.host(), b0B.host()


def test_bidiag_tikhonov_refusals(eng):
    lib, st = eng.lib, eng.stream()
    k = 4
    a2, b2, b0, y, work = (Buf(eng, nans(16)) for _ in range(5))

    def call(k=k, mu=0.1, a=a2.ptr, b=b2.ptr, b0p=b0.ptr, yp=y.ptr, w=None, wd=0):
        return lib.trk_bidiag_tikhonov(a, 1, b, 1, k, mu, b0p, yp, 0, w, wd, st)

    assert call(k=2049) == TRK_EINVAL and call(k=0) == TRK_EINVAL and call(mu=-1.0) == TRK_EINVAL
    assert call(a=None) == TRK_EINVAL and call(b=None) == TRK_EINVAL and call(b0p=None) == TRK_EINVAL and call(yp=None) == TRK_EINVAL
    assert call(w=work.ptr, wd=3 * (k + 1) + 3) == TRK_EINVAL and call(w=work.ptr, wd=0) == TRK_EINVAL
    assert all(np.all(np.isnan(b.host())) for b in (a2, b2, b0, y, work))
