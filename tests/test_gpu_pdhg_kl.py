"""PDHG with the Kullback-Leibler data term on the GPU (k_pdhg_dual_p_kl and trk_pdhg_iterate_data in csrc/pdhg.hip, solvers/PDHG.py
data='kl') against the NumPy restatement of tests/pdhg_kl_cases.py: one launch of the dual against the storage-faithful entry on
crafted vectors, the fused path against the generic one and the one-call C loop against single steps (bit for bit) for every tv,
and whole solves against the float64 form."""
import numpy as np
import pytest
import torch

import pdhg_cases as C
import pdhg_kl_cases as K
from conftest import bar
from test_gpu_mlem import CAP, PER_BLOCK, SIZES, _dev, _grid, _sum_close, _ulps

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SIGMA, BG = 0.37, 0.75


@pytest.fixture(scope="module")
def eng():
    from trips_py_amd.engine import default_engine
    return default_engine()


# ====================================================================== one launch on crafted vectors
SITUATIONS = ["plain", "d_zero", "large_z", "y_nonpos"]
_base = {}


def _vectors(n):
    """Seeded fp32 vectors, made once per n: w in [0, 8), counts b with exact zeros among them, a dual p in [-2, 1), a background vector
    in [0, 2): z - 1 = p + sigma (w + bg) - 1 falls on both sides of 0."""
    if n not in _base:
        rng = np.random.default_rng(13 * n + 3)
        _base[n] = {"w": (8 * rng.random(n)).astype(F32), "b": rng.poisson(2.0, n).astype(F32), "p": (1 - 3 * rng.random(n)).astype(F32),
                    "bgv": (2 * rng.random(n)).astype(F32)}
        _base[n]["b"][0] = 0.0
        if n > 1:
            _base[n]["b"][n - 1] = 3.0
    return {k: v.copy() for k, v in _base[n].items()}


def _craft(situation, n, bg_vector):
    v = _vectors(n)
    w, b, p = v["w"], v["b"], v["p"]
    bg = v["bgv"] if bg_vector else BG
    bga = np.broadcast_to(np.asarray(bg, dtype=F32), (n,))
    at = sorted({0, n - 1, min(n - 1, (_grid(n) - 1) * PER_BLOCK), n // 2})
    if situation == "d_zero":                                  # z = fmaf(sf, y, p) = 1 exactly: p = 1 - sf y with y a small power of two
        for j, i in enumerate(at):
            w[i] = F32(2.0) - bga[i]
            y = w[i] + bga[i]
            w[i] += F32(2.0) - y                               # y = w + bg lands on 2 exactly (or as close as fp32 allows)
            p[i] = F32(1.0 - np.float64(F32(SIGMA)) * np.float64(w[i] + bga[i]))
            b[i] = float(j % 2) * 3.0                          # with and without a count
    elif situation == "large_z":                               # z near 1e4: the branch the naive form would cancel in
        w[::3] = (F32(2.7e4) + F32(100.0) * w[::3]).astype(F32)
        b[at] = 3.0
        w[at] = 3.0e4
    elif situation == "y_nonpos":                              # A xbar + bg leaves the domain: KL = +inf, the update itself unaffected
        for j, i in enumerate(at):
            b[i] = float(j % 2) * 2.0
            w[i] = -bga[i] - F32(0.5 * (1 + j % 3))
        if n > 7:
            w[5], b[5] = -bga[5], 2.0                          # y == 0 under a count
    return w, b, p, bg


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", SIZES)
def test_one_dual_p_kl_against_the_restatement(eng, n, offset):
    grid = _grid(n)
    for bg_vector in (False, True):
        for situation in SITUATIONS:
            tag = (situation, bg_vector)
            w, b, p, bg = _craft(situation, n, bg_vector)
            want_p, want_kl, want_dp = K.dual_p_kl_f32(SIGMA, bg, w, b, p)
            dw, db, dp = (_dev(eng, a, offset) for a in (w, b, p))
            dbg = _dev(eng, bg, offset) if bg_vector else bg
            NP = eng.scalars(8 * CAP)
            nb = eng.pdhg_dual_p_kl(SIGMA, dbg, dw, db, dp, NP.ref(0), CAP)
            assert nb == grid, tag
            parts = NP.host().reshape(CAP, 8)
            assert not np.any(np.isnan(parts)), tag
            assert not np.any(parts[:, 1]) and not np.any(parts[:, 3:]) and not np.any(parts[nb:]), tag
            got = dp.cpu().numpy()
            assert np.all(np.isfinite(got)) and _ulps(got, want_p) <= 1, tag
            assert np.all(got[b > 0] < 1.0) and np.all(got <= 1.0), tag
            _sum_close(parts[:, 0].sum(), want_kl, tag + ("kl",))
            _sum_close(parts[:, 2].sum(), want_dp, tag + ("dp",))
            assert np.isinf(want_kl) == (situation == "y_nonpos"), tag
            if situation == "d_zero":
                at = sorted({0, n - 1, min(n - 1, (_grid(n) - 1) * PER_BLOCK), n // 2})
                y = w[at] + np.broadcast_to(np.asarray(bg, dtype=F32), (n,))[at]
                assert np.all(C.fma32(F32(SIGMA), np.repeat(y, 2), np.repeat(p[at], 2)) == 1.0), tag       # d is exactly 0 there
            if situation == "large_z":                         # against float64: an ulp of 1, where the naive form is off by 1e-4
                sf = np.float64(F32(SIGMA))
                y = (w + np.broadcast_to(np.asarray(bg, dtype=F32), (n,))).astype(F64)
                ref = K.prox_kl_f64(sf, 0.0, p.astype(F64) + sf * y, b.astype(F64))
                big = y > 1e4
                assert big.any() and np.max(np.abs(got[big].astype(F64) - ref[big])) <= 2.0 ** -23, tag


def test_argument_checks_come_first(eng):
    v = {k: torch.ones(8, dtype=torch.float32, device=eng.device) for k in ("w", "b", "p", "g")}
    Sc = eng.scalars(8 * CAP)
    with pytest.raises(ValueError, match="NULL"):
        eng.pdhg_dual_p_kl(SIGMA, 0.0, v["w"], None, v["p"], Sc.ref(0), CAP)
    for alias in ("w", "b"):
        with pytest.raises(ValueError, match="must not alias"):
            eng.pdhg_dual_p_kl(SIGMA, 0.0, v["w"], v["b"], v[alias], Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="must not alias"):
        eng.pdhg_dual_p_kl(SIGMA, v["g"], v["w"], v["b"], v["g"], Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="too small"):
        eng.pdhg_dual_p_kl(SIGMA, 0.0, v["w"], v["b"], v["p"], Sc.ref(0), 0)
    for sigma in (0.0, -1.0, np.inf):
        with pytest.raises(ValueError, match="sigma"):
            eng.pdhg_dual_p_kl(sigma, 0.0, v["w"], v["b"], v["p"], Sc.ref(0), CAP)
    for bg in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="background"):
            eng.pdhg_dual_p_kl(SIGMA, bg, v["w"], v["b"], v["p"], Sc.ref(0), CAP)
    assert not np.any(Sc.host()) and all(float(t.min()) == 1.0 == float(t.max()) for t in v.values())     # nothing ran
    # the loop's own arguments
    run = _run(eng, "aniso")
    rest = (1, 2, run.sigma, run.tau, run.lam, run.lo, run.hi, run.fused, run.bv, run.p, run.q, run.w, run.u, run.z, run.v, run.X, True,
            run.x_cur, run.xbar, run.xt, run.NP.ref(0), run.cap)
    for groups, data, bg, match in ((3, 1, 0.0, "groups"), (-1, 1, 0.0, "groups"), (0, 2, 0.0, "data is"), (0, 1, -1.0, "background"),
                                    (1, 1, 0.0, "N >= 2")):
        with pytest.raises(ValueError, match=match):
            eng.pdhg_iterate_data(run.A._h, run.L._h, groups, 0, 0, data, bg, *rest)
    assert not np.any(run.NP.host())


# ====================================================================== fused = generic, the loop = steps
ITER_K = 12


def _run(eng, tv, history=True, fused=None, max_iter=ITER_K, background=None):
    from trips_py_amd.solvers import PDHGRun
    P = K.problem(tv)
    return PDHGRun(P.base.device(eng), P.b, P.base.device_L(eng), P.lam, P.sigma, P.tau, P.lo, P.hi, P.x0, max_iter, P.x_true,
                   history=history, fused=fused, tv=tv, data="kl", background=P.bg if background is None else background)


def _bits(run):
    run.rows()
    return [t.clone() for t in (run.x_cur, run.xbar, run.p, run.q)], run.S.host().view(np.int64).copy()


@pytest.mark.parametrize("history", [True, False, 3])
@pytest.mark.parametrize("tv", K.TVS)
def test_run_equals_steps_and_fused_equals_generic(eng, tv, history):
    ref = _run(eng, tv, history)
    assert ref.fused and ref.geo == K.GEOMETRY[tv] and ref.tv == tv and ref.data == "kl"
    for _ in range(ITER_K):
        ref.step()
    want_vecs, want_S = _bits(ref)
    assert np.all(np.isfinite(ref.rows())) and ref.rows()[:, 0].min() > 0
    for calls in ([ITER_K], [1, ITER_K - 1], [3, 5, ITER_K - 8]):
        run = _run(eng, tv, history)
        for c in calls:
            run.run(c)
        assert run.k == ITER_K
        vecs, Sb = _bits(run)
        for key, a, b in zip(("x", "xbar", "p", "q"), vecs, want_vecs):
            assert torch.equal(a, b), (calls, key)
        assert np.array_equal(Sb, want_S), calls
    if history is True:
        assert all(torch.equal(ref.slot(k), run.slot(k)) for k in range(ITER_K))
    # the generic path (u = L xbar and v = L^T q in memory): the same bits, stepped and in one call; the background as a vector too
    for stepped, bg in ((False, None), (True, np.full(K.problem(tv).shape[0], K.problem(tv).bg))):
        gen = _run(eng, tv, history, fused=False, background=bg)
        assert not gen.fused
        if stepped:
            for _ in range(ITER_K):
                gen.step()
        else:
            gen.run(ITER_K)
        for key, a, b in zip(("x", "xbar", "p", "q"), _bits(gen)[0], want_vecs):
            assert torch.equal(a, b), ("generic", stepped, key)
        got, want = gen.rows(), ref.rows()
        assert np.array_equal(got[:, [0, 2]], want[:, [0, 2]])          # the dual of p is one kernel on both paths
        assert np.allclose(got, want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("tv", K.TVS)
def test_l2_through_the_data_loop_is_the_l2_loop(eng, tv):
    """trk_pdhg_iterate_data with data = 0 leaves the bits of the three entries that were there before it."""
    from trips_py_amd.solvers import PDHGRun
    P = K.problem(tv).base

    def make():
        return PDHGRun(P.device(eng), P.b, P.device_L(eng), P.lam, P.sigma, P.tau, P.lo, P.hi, None, ITER_K, P.x_true, tv=tv)
    ref = make()
    ref.run(ITER_K)
    run = make()
    eng.pdhg_iterate_data(run.A._h, run.L._h, K.TVS.index(tv), *(run.geo or (0, 0)), 0, 0.0, 1, ITER_K, run.sigma, run.tau, run.lam, run.lo,
                          run.hi, run.fused, run.bv, run.p, run.q, run.w, run.u, run.z, run.v, run.X, True, run.x_cur, run.xbar, run.xt,
                          run.NP.ref(0), run.cap)
    run.k = ITER_K
    run.x_cur = run.slot(ITER_K - 1)
    for a, b in zip(_bits(run)[0], _bits(ref)[0]):
        assert torch.equal(a, b)
    assert np.array_equal(_bits(run)[1], _bits(ref)[1])


# ====================================================================== whole solves against float64
ITERS = 30
# The worst relative 2-norm distance of the storage-faithful restatement (pdhg_kl_cases.pdhg_kl_f32) from the float64 restatement over
# 30 iterates, measured in NumPy on a CPU on the oracle's operators — what fp32 storage alone costs (tests/test_pdhg_kl_host.py
# recomputes them):
CPU_F32_ITERATES = {"aniso": 8.89e-8, "iso": 8.03e-8, "iso3": 4.75e-8}
# ... and, in the same two runs, the worst relative deviation of KL(b, A xbar + bg) and of the objective KL + lam R:
CPU_F32_KL = {"aniso": 1.82e-8, "iso": 1.57e-8, "iso3": 8.19e-9}
CPU_F32_OBJECTIVE = {"aniso": 1.76e-8, "iso": 1.47e-8, "iso3": 9.81e-9}


def _limit(cpu_figure):
    """8 x the cost of fp32 storage alone, never below 1e-5 (the rule of test_gpu_pdhg.py's bars)."""
    return max(8 * cpu_figure, 1e-5)


@pytest.mark.parametrize("tv", K.TVS)
def test_solve_against_float64(eng, tv):
    from trips_py_amd.solvers import PDHG
    P, geo = K.problem(tv), K.GEOMETRY[tv]
    A, L = P.base.device(eng), P.base.device_L(eng)
    if P.name == "Q5":
        Apair = C.pair(P.base.oracle())
    else:                                                     # the operator's own matrices; the "transpose" is the operator's too
        M, Mt = A.todense(), A.T.todense()
        assert M.shape == P.shape and Mt.shape == P.shape[::-1]
        Apair = ((lambda v: M @ v), (lambda v: Mt @ v))
    ref = P.f64(tv, ITERS, A=Apair, x_true=P.x_true)
    x, info = PDHG(A, P.b, L, P.lam, ITERS, 0, x0=P.x0, x_true=P.x_true, lower=P.lo, upper=P.hi, sigma=P.sigma, tau=P.tau, tv=tv,
                   data="kl", background=P.bg)
    assert info["its"] == ITERS and len(info["xHistory"]) == ITERS and info["data"] == "kl" and "Rnrm" not in info
    H = [h.reshape(-1) for h in info["xHistory"]]
    assert all(float(h.min()) >= P.lo and float(h.max()) <= P.hi for h in H)
    worst = max(np.linalg.norm(h - xr) / np.linalg.norm(xr) for h, xr in zip(H, ref["X"]))
    bar(f"pdhg_kl_{tv}_iterates_vs_float64", worst, _limit(CPU_F32_ITERATES[tv]))
    Sr = ref["S"]
    bar(f"pdhg_kl_{tv}_KL_vs_float64", np.max(np.abs(np.array(info["KL"]) / Sr[:, 0] - 1)), _limit(CPU_F32_KL[tv]))
    bar(f"pdhg_kl_{tv}_objective_vs_float64", np.max(np.abs(np.array(info["objective"]) / (Sr[:, 0] + P.lam * Sr[:, 1]) - 1)),
        _limit(CPU_F32_OBJECTIVE[tv]))
    assert np.allclose(info["relError"], np.sqrt(Sr[:, 6]) / np.linalg.norm(P.x_true), rtol=1e-4)
    want = K.objective_kl(Apair, C.pair(P.base.oracle_L()), P.b, P.bg, P.lam, x, tv, geo)
    assert abs(info["objectiveFinal"] / want - 1) < 1e-5
