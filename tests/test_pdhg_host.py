"""PDHG without a GPU: the NumPy restatement of tests/pdhg_cases.py checked against what the method promises (the optimality
conditions of the program it solves, the norm estimate its default steps rest on, what fp32 storage costs), and PDHG()'s host logic
(info, history sinks, steps, stopping, argument errors) driven through the CPU test engine."""
import numpy as np
import pytest

import pdhg_cases as C
from cpu_engine import OracleOp
from pdhg_cpu_engine import PdhgCpuEngine
from trips_py_amd import solvers as S
from trips_py_amd.operators import Identity, operator_norm_sq

K = 40


@pytest.fixture(scope="module")
def eng():
    return PdhgCpuEngine()


# ------------------------------------------------------------------ (a) the restatement solves the program
def test_fixed_point_satisfies_the_kkt_conditions():
    """6 x 6, 3 x 3 Gaussian blur (sigma 1, reflect; its dense matrix and that matrix's transpose), TV, lam = 0.02, box [0, 0.9]:
    where the float64 iteration stops moving (relative step <= 1e-14) the point satisfies the optimality conditions of
    min 1/2 ||A x - b||^2 + lam ||L x||_1 over the box, stated without reference to the iteration.  (Reached in 2668 iterations with
    residuals <= 6.1e-14 when this was written.)"""
    from blur_psf_cases import scipy_operator
    from oracle import cpu_ref as O
    M = scipy_operator(O.gauss_psf((3, 3), 1.0)[0], 6, 6, "reflect").todense()
    Lo = O.FirstDerivative2D(6)
    Lm = Lo.todense()
    xt = np.zeros((6, 6))
    xt[1:3, 1:4] = 1.5
    xt[4, 4] = 2.5
    bt = M @ xt.reshape(-1)
    e = np.random.default_rng(6).standard_normal(36)
    b = bt + 0.02 * np.linalg.norm(bt) / np.linalg.norm(e) * e
    lam, lo, hi = 0.02, 0.0, 0.9
    step = 0.95 / np.sqrt(np.linalg.eigvalsh(M.T @ M + Lm.T @ Lm)[-1])
    run = C.pdhg_f64((lambda v: M @ v, lambda v: M.T @ v), C.pair(Lo), b, lam, step, step, lo, hi, None, 200000, stop_step=1e-14)
    assert len(run["X"]) < 200000, "the iteration did not stop moving: raise the budget"
    x, p, q = run["X"][-1], run["p"], run["q"]
    at_lo, at_hi = x == lo, x == hi
    assert at_lo.sum() >= 1 and at_hi.sum() >= 1 and (~at_lo & ~at_hi).sum() >= 1
    assert np.all((x >= lo) & (x <= hi))
    tol = 1e-10 * max(np.linalg.norm(b), 1.0)
    assert np.abs(p - (M @ x - b)).max() <= tol
    assert np.abs(q).max() <= lam + tol
    u = Lm @ x
    big = np.abs(u) > 1e-8
    assert big.sum() >= 1 and np.abs(q[big] - lam * np.sign(u[big])).max() <= tol
    g = M.T @ p + Lm.T @ q
    assert np.abs(g[~at_lo & ~at_hi]).max() <= tol
    assert g[at_lo].min() >= -tol and g[at_hi].max() <= tol


# ------------------------------------------------------------------ (b) the norm estimate
@pytest.mark.parametrize("name", C.NAMES)
def test_norm_estimate_is_from_below_and_close(name):
    P = C.problem(name)
    assert 0.95 <= P.est / P.normK2 <= 1.0 + 1e-12, (P.est, P.normK2)
    # the default steps therefore satisfy sigma tau ||K||^2 < 1
    assert P.sigma * P.tau * P.normK2 < 1.0


@pytest.mark.parametrize("name", ["Q1", "Q4"])
def test_operator_norm_sq_on_the_cpu_engine(eng, name):
    """The engine's helper through the CPU engine (fp32 vectors) against the float64 restatement."""
    P = C.problem(name)
    A = OracleOp(P.oracle(), eng)
    L = Identity(120, eng) if name == "Q4" else OracleOp(P.oracle_L(), eng)
    assert abs(operator_norm_sq([A, L], iters=30, seed=0) / P.est - 1) < 1e-5
    assert abs(operator_norm_sq(A, iters=30, seed=0) / P.normA2 - 1) < 0.1
    with pytest.raises(ValueError):
        operator_norm_sq([A, Identity(7, eng)])
    with pytest.raises(ValueError):
        operator_norm_sq([A], iters=0)


# ------------------------------------------------------------------ (d) what fp32 storage costs
@pytest.fixture(scope="module")
def runs():
    """name -> (float64 run, storage-faithful run), 30 iterations each on the oracle's operators, computed once."""
    return {name: (C.problem(name).f64(30, x_true=C.problem(name).x_true),
                   C.problem(name).f32(30, x_true=C.problem(name).x_true, tv_N=C.problem(name).tv_N)) for name in C.NAMES}


def _figures(P, f64, f32):
    obj = [0.5 * r["S"][:, 0] + P.lam * r["S"][:, 1] for r in (f32, f64)]
    return (C.worst_distance(f32, f64), float(np.max(np.abs(np.sqrt(f32["S"][:, 0] / f64["S"][:, 0]) - 1))),
            float(np.max(np.abs(obj[0] / obj[1] - 1))))


@pytest.mark.parametrize("name", C.NAMES)
def test_fp32_storage_cost_is_the_recorded_one(runs, name):
    """The constants the GPU test's bars are built from (tests/test_gpu_pdhg.py) are these figures, up to the host's BLAS."""
    import test_gpu_pdhg as G
    got = _figures(C.problem(name), *runs[name])
    for fig, table in zip(got, (G.CPU_F32_ITERATES, G.CPU_F32_RNRM, G.CPU_F32_OBJECTIVE)):
        assert 0.5 * table[name] <= fig <= 2.0 * table[name], (name, got)
    assert got[0] < 5e-7             # rounding does not grow: the iteration is non-expansive


@pytest.mark.parametrize("name", C.NAMES)
def test_iterates_stay_in_the_box_and_the_objective_falls(runs, name):
    P = C.problem(name)
    for run in runs[name]:
        assert all(float(x.min()) >= P.lo and float(x.max()) <= P.hi for x in run["X"])
        obj = 0.5 * run["S"][:, 0] + P.lam * run["S"][:, 1]
        assert obj[29] < obj[9] < obj[0]
    if name == "Q2":                # the upper bound is active
        assert np.count_nonzero(runs[name][0]["X"][-1] == 3.0) > 10 and np.count_nonzero(runs[name][0]["X"][-1] == 0.0) > 10


# ------------------------------------------------------------------ (c) PDHG() on the CPU engine
def _ops(eng, name):
    P = C.problem(name)
    return P, OracleOp(P.oracle(), eng), (Identity(120, eng) if name == "Q4" else OracleOp(P.oracle_L(), eng))


def _solve(eng, name, max_iter, tol=0, **kw):
    P, A, L = _ops(eng, name)
    kw.setdefault("sigma", P.sigma)
    kw.setdefault("tau", P.tau)
    kw.setdefault("x_true", P.x_true)
    return S.PDHG(A, P.b.reshape(-1, 1), L, P.lam, max_iter, tol, lower=P.lo, upper=P.hi, **kw)


def _close(x, ref):
    ref = ref.astype(np.float64).reshape(-1)
    return np.linalg.norm(np.asarray(x).reshape(-1) - ref) <= 1e-6 * np.linalg.norm(ref)


@pytest.mark.parametrize("name", ["Q1", "Q4"])
def test_info_and_iterates(eng, runs, name):
    P, ref = C.problem(name), runs[name][1]
    x, info = _solve(eng, name, 12)
    per_iter = ["Rnrm", "active", "dualChange", "objective", "relError", "relResidual", "xHistory"]
    assert sorted(info) == sorted(per_iter + ["its", "sigma", "tau", "normK2", "objectiveFinal"])
    assert info["its"] == 12 and all(len(info[k]) == 12 for k in per_iter)
    assert info["sigma"] == P.sigma and info["tau"] == P.tau and info["normK2"] is None
    assert x.shape == (P.shape[1], 1) and np.array_equal(x, info["xHistory"][-1])
    for k in range(12):
        assert _close(info["xHistory"][k], ref["X"][k])
    Sr = ref["S"][:12]
    bn = np.linalg.norm(P.b.astype(np.float32).astype(np.float64))
    assert np.allclose(info["Rnrm"], np.sqrt(Sr[:, 0]) / bn, rtol=1e-5)
    assert np.allclose(info["objective"], 0.5 * Sr[:, 0] + P.lam * Sr[:, 1], rtol=1e-5)
    assert np.allclose(info["dualChange"], np.sqrt(Sr[:, 2] + Sr[:, 3]), rtol=1e-4)
    assert np.allclose(info["relResidual"], np.sqrt(Sr[:, 5] / Sr[:, 4]), rtol=1e-4)
    assert np.allclose(info["relError"], np.sqrt(Sr[:, 6]) / np.linalg.norm(P.x_true), rtol=1e-5)
    assert all(isinstance(a, int) for a in info["active"])
    xs = [h.reshape(-1) for h in info["xHistory"]]
    assert info["active"] == [int(np.count_nonzero((h == P.lo) | (h == P.hi))) for h in xs]
    assert all(h.min() >= P.lo and h.max() <= P.hi for h in xs)
    # the objective at the returned x, recomputed in float64
    want = C.objective(C.pair(P.oracle()), C.pair(P.oracle_L()), P.b.astype(np.float32), P.lam, x)
    assert abs(info["objectiveFinal"] / want - 1) < 1e-6
    _x2, info2 = _solve(eng, name, 12, x_true=None)
    assert "relError" not in info2 and info2["objective"] == info["objective"]


def test_default_steps_come_from_the_norm_estimate(eng):
    P, A, L = _ops(eng, "Q4")
    _x, info = S.PDHG(A, P.b, L, P.lam, 3, lower=-np.inf)
    assert abs(info["normK2"] / P.est - 1) < 1e-5
    assert abs(info["sigma"] * info["tau"] * info["normK2"] - 0.95 ** 2) < 1e-12 and info["sigma"] == info["tau"]
    _x, info = S.PDHG(A, P.b, L, P.lam, 3, lower=-np.inf, normK2=60.0, ratio=4.0)
    assert info["normK2"] == 60.0 and abs(info["sigma"] / info["tau"] - 4.0) < 1e-12
    assert abs(info["sigma"] * info["tau"] * 60.0 - 0.95 ** 2) < 1e-12
    # the defaults of the box: [0, inf)
    x, _info = S.PDHG(A, P.b, L, P.lam, 5)
    assert x.min() == 0.0


@pytest.mark.parametrize("spec", [False, 3, "host", "file"])
def test_history_sinks(eng, spec, tmp_path):
    if spec == "file":
        spec = str(tmp_path / "xhist.npy")
    x0, i0 = _solve(eng, "Q4", 11)
    x1, i1 = _solve(eng, "Q4", 11, history=spec)
    assert np.array_equal(x0, x1) and i0["objective"] == i1["objective"]
    H = i1["xHistory"]
    if spec is False:
        assert H == []
        return
    assert H.iterations == (list(range(11)) if isinstance(spec, str) else [2, 5, 8, 10])
    for j, k in enumerate(H.iterations):
        assert np.array_equal(H[j], i0["xHistory"][k])


def test_x0_is_projected_onto_the_box(eng):
    P, A, L = _ops(eng, "Q1")
    rng = np.random.default_rng(3)
    x0 = rng.standard_normal(P.shape[1]) * 3.0
    xa, ia = S.PDHG(A, P.b, L, P.lam, 4, x0=x0, lower=0.0, upper=1.5, sigma=P.sigma, tau=P.tau)
    xb, ib = S.PDHG(A, P.b, L, P.lam, 4, x0=np.clip(x0, 0.0, 1.5), lower=0.0, upper=1.5, sigma=P.sigma, tau=P.tau)
    assert np.array_equal(xa, xb) and ia["objective"] == ib["objective"]
    assert all(h.min() >= 0.0 and h.max() <= 1.5 for h in ia["xHistory"])
    ref = C.pdhg_f32(C.pair(P.oracle()), C.pair(P.oracle_L()), P.b, P.lam, P.sigma, P.tau, 0.0, 1.5, x0, 4)
    assert _close(xa, ref["X"][3])


def test_tol_stops_where_the_restatement_says(eng):
    P = C.problem("Q4")
    ref = P.f32(K)
    rel = np.sqrt(ref["S"][:, 5] / ref["S"][:, 4])
    tol = float(np.sqrt(rel[14] * rel[15]))
    hit = int(np.nonzero(rel <= tol)[0][0]) + 1
    assert 1 < hit < K
    x, info = _solve(eng, "Q4", K, tol=tol)
    assert info["its"] == hit and len(info["xHistory"]) == hit and len(info["objective"]) == hit
    assert _close(x, ref["X"][hit - 1])


def test_discrepancy_stops_where_the_restatement_says(eng):
    P = C.problem("Q1")
    ref = P.f32(K, tv_N=None)
    res = np.sqrt(ref["S"][:, 0])
    delta = float(np.sqrt(res[11] * res[12])) / 1.01
    hit = int(np.nonzero(res <= 1.01 * delta)[0][0]) + 1
    assert 1 < hit < K
    x, info = _solve(eng, "Q1", K, delta=delta)
    assert info["its"] == hit and _close(x, ref["X"][hit - 1])
    _x, info2 = _solve(eng, "Q1", K, delta=delta, eta=1.5)
    assert info2["its"] < hit


def test_argument_errors(eng):
    P, A, L = _ops(eng, "Q4")
    n = P.shape[1]
    ok = dict(sigma=P.sigma, tau=P.tau)
    for bad in (dict(lam=-1.0), dict(lam=np.nan), dict(lower=1.0, upper=0.5), dict(lower=np.nan), dict(sigma=np.inf), dict(tau=np.nan),
                dict(sigma=0.0), dict(normK2=-1.0, sigma=None), dict(ratio=0.0, sigma=None), dict(x0=np.ones(n + 1)),
                dict(x_true=np.ones(n - 1)), dict(b=np.ones(P.shape[0] + 2)), dict(L=Identity(n + 1, eng)), dict(max_iter=0),
                dict(fused=True)):
        kw = {**ok, **bad}
        lam, b, Lop, its = kw.pop("lam", P.lam), kw.pop("b", P.b), kw.pop("L", L), kw.pop("max_iter", 3)
        with pytest.raises(ValueError):
            S.PDHG(A, b, Lop, lam, its, **kw)


def test_sharded_is_not_built():
    class TwoRanks(PdhgCpuEngine):
        def __init__(self):
            super().__init__()
            self.world = 2
    P = C.problem("Q4")
    e2 = TwoRanks()
    with pytest.raises(NotImplementedError):
        S.PDHG(OracleOp(P.oracle(), e2), P.b, Identity(120, e2), P.lam, 3)
