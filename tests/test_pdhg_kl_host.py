"""PDHG with the Kullback-Leibler data term without a GPU: the NumPy restatement of tests/pdhg_kl_cases.py checked against the
optimality conditions of the program it solves and against what fp32 storage costs, and PDHG(data='kl')'s host logic (info, argument
errors, the untouched least-squares default) driven through the CPU test engine."""
import numpy as np
import pytest

import pdhg_cases as C
import pdhg_iso_cases as I
import pdhg_kl_cases as K
from cpu_engine import OracleOp
from pdhg_kl_cpu_engine import PdhgKlCpuEngine
from trips_py_amd import solvers as S

EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def eng():
    return PdhgKlCpuEngine()


# ------------------------------------------------------------------ (1) the prox
def test_prox_identity():
    """p = prox_{sigma F*}(z) zeroes b / (1 - p) - bg + (p - z) / sigma, the optimality condition of
    min_p F*(p) + (p - z)^2 / (2 sigma) with F*(p) = -b log(1 - p) - bg p, and p < 1 wherever b > 0.  The residual is judged against
    what evaluating it costs: forming 1 - p from p loses the bits p shares with 1, an error eps / (1 - p) relative in the first term."""
    rng = np.random.default_rng(0)
    n = 20000
    z, b = rng.uniform(-50, 50, n), rng.poisson(3.0, n).astype(np.float64)
    sigma, bg = rng.uniform(0.01, 5.0, n), rng.uniform(0.0, 3.0, n)
    p = K.prox_kl_f64(sigma, bg, z, b)
    pos = b > 0
    assert np.all(p[pos] < 1.0) and np.all(np.isfinite(p))
    res = b[pos] / (1.0 - p[pos]) - bg[pos] + (p[pos] - z[pos]) / sigma[pos]
    scale = b[pos] / (1.0 - p[pos]) ** 2 + bg[pos] + (np.abs(p[pos]) + np.abs(z[pos])) / sigma[pos]
    worst = float(np.max(np.abs(res) / scale))
    print("prox identity: worst scaled residual %.2e" % worst)
    assert worst <= 16 * EPS
    # b == 0: F* = -bg p on p <= 1, the prox is min(z + sigma bg, 1)
    assert np.allclose(p[~pos], np.minimum(z[~pos] + sigma[~pos] * bg[~pos], 1.0), rtol=0, atol=1e-13)
    # the two forms are one number
    d = z + sigma * bg - 1.0
    r = np.sqrt(d * d + 4.0 * sigma * b)
    assert np.allclose(p, 0.5 * (1.0 + z + sigma * bg - r), rtol=0, atol=1e-12)


def test_the_fp32_entry_does_not_cancel_for_large_z():
    """z near 1e4 with a count under it: 1 - p' is 2 sigma b / (d + r), about 1e-4, and the fp32 entry has it to an ulp of 1; the form
    1/2 (1 + z - sqrt(...)) evaluated in fp32 would lose it in the rounding of numbers of size 1e4."""
    sigma, bg = 0.3, 0.5
    w = np.linspace(3.0e4, 3.4e4, 1001).astype(np.float32)
    b = np.full(w.size, 3.0, dtype=np.float32)
    p0 = np.zeros(w.size, dtype=np.float32)
    pn, _kl, _dp = K.dual_p_kl_f32(sigma, bg, w, b, p0)
    z64 = np.float64(np.float32(sigma)) * (w.astype(np.float64) + np.float32(bg))
    want = K.prox_kl_f64(np.float64(np.float32(sigma)), 0.0, z64, b.astype(np.float64))
    assert np.all(z64 > 8e3) and np.max(np.abs(pn.astype(np.float64) - want)) <= 2.0 ** -24
    assert np.all(pn < 1.0)
    z32 = z64.astype(np.float32)
    naive = np.float32(0.5) * (np.float32(1) + z32 - np.sqrt((z32 - np.float32(1)) ** 2 + np.float32(4 * sigma) * b))
    assert np.max(np.abs(naive.astype(np.float64) - want)) > 1e-5
    # b == 0: p' = min(z, 1); d == 0 exactly: p' = 1 - sqrt(sigma b)
    pz, _, _ = K.dual_p_kl_f32(sigma, 0.0, np.float32([-2.0, 0.5, 50.0]), np.zeros(3, dtype=np.float32), np.float32([0.25, 0.25, 0.25]))
    assert np.allclose(pz, [0.25 - 0.6, 0.25 + 0.15, 1.0], rtol=0, atol=1e-6) and pz[2] == 1.0
    pd, _, _ = K.dual_p_kl_f32(0.25, 0.0, np.float32([4.0]), np.float32([4.0]), np.float32([0.0]))
    assert pd[0] == 0.0                                        # z = 1, d = 0, r = sqrt(4 sigma b) = 2: p' = fmaf(0.5, -2, 1)


# ------------------------------------------------------------------ (2) the restatement solves the program
@pytest.mark.parametrize("tv,geo", [("aniso", None), ("iso", (6, 1))])
def test_fixed_point_satisfies_the_kkt_conditions(tv, geo):
    """The 6 x 6 operators of test_pdhg_host.py (3 x 3 Gaussian blur, first differences, step 0.95 / ||K||) with photon counts over a
    background of 0.3, lam = 0.05, box [0, 4]: where the float64 iteration stops moving (relative step <= 1e-14) the point satisfies
    the optimality conditions of min KL(b, A x + bg) + lam R(L x) over the box, stated without reference to the iteration:
    p = 1 - b / (A x + bg) (the gradient of the data term), q in the subdifferential of lam R at L x, and A^T p + L^T q zero on the free
    entries, >= 0 at the lower and <= 0 at the upper bound — under the bound test_pdhg_host.py applies to the least-squares program.
    (Reached in 4956 / 1621 iterations with residuals <= 2.5e-13 when this was written; 17 entries at the lower bound, 9 / 8 at
    the upper, 8 counts of zero.)"""
    from blur_psf_cases import scipy_operator
    from oracle import cpu_ref as O
    M = np.asarray(scipy_operator(O.gauss_psf((3, 3), 1.0)[0], 6, 6, "reflect").todense())
    Lo = O.FirstDerivative2D(6)
    Lm = np.asarray(Lo.todense())
    xt = np.zeros((6, 6))
    xt[1:3, 1:4] = 6.0
    xt[4, 4] = 10.0
    bg = 0.3
    b = np.random.default_rng(6).poisson(M @ xt.reshape(-1) + bg).astype(np.float64)
    assert np.count_nonzero(b == 0) >= 1
    lam, lo, hi = 0.05, 0.0, 4.0
    step = 0.95 / np.sqrt(np.linalg.eigvalsh(M.T @ M + Lm.T @ Lm)[-1])
    run = K.pdhg_kl_f64((lambda v: M @ v, lambda v: M.T @ v), C.pair(Lo), b, bg, lam, step, step, lo, hi, None, 200000, tv, geo,
                        stop_step=1e-14)
    assert len(run["X"]) < 200000, "the iteration did not stop moving: raise the budget"
    x, p, q = run["X"][-1], run["p"], run["q"]
    at_lo, at_hi = x == lo, x == hi
    assert at_lo.sum() >= 1 and at_hi.sum() >= 1 and (~at_lo & ~at_hi).sum() >= 1
    assert np.all((x >= lo) & (x <= hi))
    tol = 1e-10 * max(np.linalg.norm(b), 1.0)
    y = M @ x + bg
    assert np.all(y > 0) and np.all(p < 1.0 + tol)
    worst = [np.abs(p - (1.0 - b / y)).max()]
    assert np.all(p[b == 0] >= 1.0 - tol)                      # a count of zero: its dual sits at 1, the gradient of y
    u = Lm @ x
    if tv == "aniso":
        assert np.abs(q).max() <= lam + tol
        big = np.abs(u) > 1e-8
        assert big.sum() >= 1
        worst.append(np.abs(q[big] - lam * np.sign(u[big])).max())
    else:
        assert I.group_norms(*geo, q).max() <= lam + tol
        ph, pv, sg = I.groups(*geo, u.size)
        un = I.group_norms(*geo, u)
        big_p, big_s = un[:ph.size] > 1e-8, un[ph.size:] > 1e-8
        assert big_p.sum() >= 1 and big_s.sum() >= 1
        for idx in (ph, pv):
            worst.append(np.abs(q[idx][big_p] - lam * u[idx][big_p] / un[:ph.size][big_p]).max())
        worst.append(np.abs(q[sg][big_s] - lam * np.sign(u[sg][big_s])).max())
    g = M.T @ p + Lm.T @ q
    worst.append(np.abs(g[~at_lo & ~at_hi]).max())
    print(tv, "iterations %d, worst residual %.2e (bound %.2e)" % (len(run["X"]), max(worst), tol))
    assert max(worst) <= tol
    assert g[at_lo].min() >= -tol and g[at_hi].max() <= tol


# ------------------------------------------------------------------ (3) what fp32 storage costs
@pytest.fixture(scope="module")
def runs():
    """tv -> (float64 run, storage-faithful run), 30 iterations each on the oracle's operators, computed once."""
    return {tv: (K.problem(tv).f64(tv, 30, x_true=K.problem(tv).x_true), K.problem(tv).f32(tv, 30, x_true=K.problem(tv).x_true))
            for tv in K.TVS}


def figures(P, f64, f32):
    obj = [r["S"][:, 0] + P.lam * r["S"][:, 1] for r in (f32, f64)]
    return (C.worst_distance(f32, f64), float(np.max(np.abs(f32["S"][:, 0] / f64["S"][:, 0] - 1))),
            float(np.max(np.abs(obj[0] / obj[1] - 1))))


@pytest.mark.parametrize("tv", K.TVS)
def test_fp32_storage_cost_is_the_recorded_one(runs, tv):
    """The constants the GPU test's bars are built from (tests/test_gpu_pdhg_kl.py) are these figures, up to the host's BLAS."""
    import test_gpu_pdhg_kl as G
    got = figures(K.problem(tv), *runs[tv])
    print(tv, "iterates %.3e KL %.3e objective %.3e" % got)
    for fig, table in zip(got, (G.CPU_F32_ITERATES, G.CPU_F32_KL, G.CPU_F32_OBJECTIVE)):
        assert 0.5 * table[tv] <= fig <= 2.0 * table[tv], (tv, got)
        assert fig < 5e-7, (tv, got)


@pytest.mark.parametrize("tv", K.TVS)
def test_iterates_stay_in_the_box_and_the_objective_falls(runs, tv):
    P = K.problem(tv)
    for run in runs[tv]:
        assert all(float(x.min()) >= P.lo and float(x.max()) <= P.hi for x in run["X"])
        assert np.all(np.isfinite(run["S"]))
        obj = run["S"][:, 0] + P.lam * run["S"][:, 1]
        assert obj[29] < obj[9] < obj[0]


# ------------------------------------------------------------------ (4) PDHG(data='kl') on the CPU engine
def _ops(eng, P):
    return OracleOp(P.base.oracle(), eng), OracleOp(P.base.oracle_L(), eng)


def _solve(eng, tv, max_iter, **kw):
    P = K.problem(tv)
    A, L = _ops(eng, P)
    kw.setdefault("x_true", P.x_true)
    kw.setdefault("background", P.bg)
    if tv != "aniso":
        kw.setdefault("tv_dims", K.GEOMETRY[tv])
    return S.PDHG(A, P.b.reshape(-1, 1), L, P.lam, max_iter, 0, x0=P.x0, lower=P.lo, upper=P.hi, sigma=P.sigma, tau=P.tau, tv=tv,
                  data="kl", **kw)


def _close(x, ref):
    ref = ref.astype(np.float64).reshape(-1)
    return np.linalg.norm(np.asarray(x).reshape(-1) - ref) <= 1e-6 * np.linalg.norm(ref)


@pytest.mark.parametrize("tv", K.TVS)
def test_info_and_iterates(eng, tv):
    P = K.problem(tv)
    ref = P.f32(tv, 12, x_true=P.x_true)
    x, info = _solve(eng, tv, 12)
    per_iter = ["KL", "active", "dualChange", "objective", "relError", "relResidual", "xHistory"]
    extra = ["its", "sigma", "tau", "normK2", "objectiveFinal", "data"] + ([] if tv == "aniso" else ["tv"])
    assert sorted(info) == sorted(per_iter + extra) and "Rnrm" not in info
    assert info["data"] == "kl" and info["its"] == 12 and all(len(info[k]) == 12 for k in per_iter)
    for k in range(12):
        assert _close(info["xHistory"][k], ref["X"][k])
    Sr = ref["S"][:12]
    assert np.allclose(info["KL"], Sr[:, 0], rtol=1e-5)
    assert np.allclose(info["objective"], Sr[:, 0] + P.lam * Sr[:, 1], rtol=1e-5)          # no factor 1/2
    assert np.allclose(info["dualChange"], np.sqrt(Sr[:, 2] + Sr[:, 3]), rtol=1e-4)
    assert np.allclose(info["relResidual"], np.sqrt(Sr[:, 5] / Sr[:, 4]), rtol=1e-4)
    Ao, Lo = P.pairs()
    want = K.objective_kl(Ao, Lo, P.b, P.bg, P.lam, x, tv, K.GEOMETRY[tv])
    assert abs(info["objectiveFinal"] / want - 1) < 1e-6
    # a background vector is the background number, bit for bit
    xv, iv = _solve(eng, tv, 12, background=np.full(P.shape[0], P.bg))
    assert np.array_equal(x, xv) and iv["KL"] == info["KL"]


@pytest.mark.parametrize("tv", K.TVS)
def test_l2_is_the_call_without_the_argument(eng, tv):
    """data='l2' (the default) is the solver as it was: the same keys, and the bits of the storage-faithful least-squares
    restatements of the three case files, which know nothing of a data argument."""
    import pdhg_iso3_cases as T
    P = K.problem(tv).base
    A, L = OracleOp(P.oracle(), eng), OracleOp(P.oracle_L(), eng)
    kw = dict(lower=P.lo, upper=P.hi, sigma=P.sigma, tau=P.tau, x_true=P.x_true, tv=tv)
    if tv != "aniso":
        kw["tv_dims"] = K.GEOMETRY[tv]
    x0, i0 = S.PDHG(A, P.b, L, P.lam, 8, 0, **kw)
    x1, i1 = S.PDHG(A, P.b, L, P.lam, 8, 0, data="l2", background=123.0, **kw)               # the background belongs to 'kl'
    assert np.array_equal(x0, x1) and sorted(i0) == sorted(i1) and "data" not in i0 and "KL" not in i0 and "Rnrm" in i0
    for key in ("objective", "Rnrm", "dualChange", "relResidual", "active", "relError", "objectiveFinal"):
        assert i0[key] == i1[key], key
    ref = {"aniso": lambda: P.f32(8), "iso": lambda: I.f32(P.name, 8), "iso3": lambda: T.f32(P.name, 8)}[tv]()
    assert np.array_equal(x0.reshape(-1), ref["X"][7].astype(np.float64))
    assert np.allclose(i0["objective"], 0.5 * ref["S"][:, 0] + P.lam * ref["S"][:, 1], rtol=1e-12, atol=0)


def test_argument_errors(eng):
    P = K.problem("aniso")
    A, L = _ops(eng, P)
    m = P.shape[0]
    ok = dict(sigma=P.sigma, tau=P.tau, data="kl")
    with pytest.raises(ValueError, match="counts cannot be negative"):
        S.PDHG(A, np.where(np.arange(m) == 2, -1.0, P.b), L, P.lam, 3, **ok)
    for b in (np.where(np.arange(m) == 2, np.nan, P.b), np.where(np.arange(m) == 2, np.inf, P.b)):
        with pytest.raises(ValueError):
            S.PDHG(A, b, L, P.lam, 3, **ok)
    for bg in (-0.5, np.nan, np.inf, np.full(m, -1.0), np.ones(m + 1)):
        with pytest.raises(ValueError, match="background"):
            S.PDHG(A, P.b, L, P.lam, 3, background=bg, **ok)
    with pytest.raises(ValueError, match="least-squares notion"):
        S.PDHG(A, P.b, L, P.lam, 3, delta=1.0, **ok)
    for data in ("poisson", None, "KL"):
        with pytest.raises(ValueError, match="data must be"):
            S.PDHG(A, P.b, L, P.lam, 3, sigma=P.sigma, tau=P.tau, data=data)
    # negative data is the least-squares solver's business as before
    S.PDHG(A, -P.b, L, P.lam, 2, sigma=P.sigma, tau=P.tau)
    # tol > 0 stops on the step as for 'l2'
    x, info = S.PDHG(A, P.b, L, P.lam, 40, 0.02, x0=P.x0, background=P.bg, **ok)
    assert 1 < info["its"] < 40 and info["relResidual"][-1] <= 0.02 < info["relResidual"][-2]
