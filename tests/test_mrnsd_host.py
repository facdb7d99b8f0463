"""MRNSD without a GPU: the NumPy restatement of tests/mrnsd_cases.py checked against what the method promises, and MRNSD()'s
host logic (info, history sinks, x0 rules, stopping, breakdown) driven through the CPU test engine."""
import numpy as np
import pytest

import mrnsd_cases as C
from cpu_engine import OracleOp
from mrnsd_cpu_engine import MrnsdCpuEngine
from trips_py_amd import solvers as S

K = 40


@pytest.fixture(scope="module")
def eng():
    return MrnsdCpuEngine()


@pytest.fixture(scope="module")
def runs():
    """name -> (float64 run, storage-faithful run), K iterations each, computed once."""
    out = {}
    for name in C.NAMES:
        P, o = C.problem(name), C.problem(name).oracle()
        out[name] = (C.mrnsd_f64(o.matvec, o.rmatvec, P.b, P.x0, K), C.mrnsd_f32(o.matvec, o.rmatvec, P.b, P.x0, K, P.x_true))
    return out


# ------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("name", C.NAMES)
def test_iterates_stay_nonnegative(runs, name):
    for run in runs[name]:
        assert all(float(x.min()) >= 0.0 for x in run["X"])


@pytest.mark.parametrize("name", C.EXACT_ADJOINT)
def test_residual_norm_does_not_increase(runs, name):
    for run in runs[name]:
        rr = np.concatenate(([run["rr0"]], run["rr"]))
        assert np.all(np.diff(rr) <= 0.0)


def test_p1_first_step_bounded_one_entry_zero(runs):
    for run in runs["P1"]:
        bounded = [a < t for a, t in zip(run["alpha"], run["theta"])]
        assert bounded == [True] + [False] * (K - 1)
        zeros = [np.nonzero(x == 0)[0] for x in run["X"]]
        assert all(z.size == 1 and z[0] == zeros[0][0] for z in zeros)


def test_unbounded_step_is_steepest_descent_in_the_scaled_metric():
    """alpha = theta forced: x1 = x0 + t d with d = -diag(x0) grad f(x0), f = ||b - A x||^2 / 2, and t the exact line minimum."""
    P, o = C.problem("P1"), C.problem("P1").oracle()
    run = C.mrnsd_f64(o.matvec, o.rmatvec, P.b, P.x0, 1, force_theta=True)
    r0 = P.b - o.matvec(P.x0)
    d = -P.x0 * (-o.rmatvec(r0))
    Ad = o.matvec(d)
    t = float(np.dot(r0, Ad) / np.dot(Ad, Ad))
    assert np.allclose(run["X"][0], P.x0 + t * d, rtol=1e-12, atol=0)
    assert abs(run["alpha"][0] / t - 1) < 1e-12
    f = [np.linalg.norm(r0 - c * t * Ad) for c in (0.99, 1.0, 1.01)]
    assert f[1] < f[0] and f[1] < f[2]


# ------------------------------------------------------------------ MRNSD() on the CPU engine
def _close(x, ref):
    """Equal up to a few fp32 roundings of the step (relative 2-norm)."""
    ref = ref.astype(np.float64).reshape(-1)
    return np.linalg.norm(np.asarray(x).reshape(-1) - ref) <= 1e-6 * np.linalg.norm(ref)


def _solve(eng, name, max_iter, tol=0, x0="problem", **kw):
    P = C.problem(name)
    A = OracleOp(P.oracle(), eng)
    return S.MRNSD(A, P.b.reshape(-1, 1), P.x0 if isinstance(x0, str) else x0, max_iter, tol, x_true=P.x_true, **kw)


@pytest.mark.parametrize("name", C.NAMES)
def test_info_and_iterates(eng, runs, name):
    """The CPU engine rounds an oracle product to fp32 once, as the storage-faithful restatement does; only the order of the
    float64 sum behind ||u||^2 differs (torch's against NumPy's), so the scalars agree to rounding and the iterates to fp32's."""
    P, ref = C.problem(name), runs[name][1]
    x, info = _solve(eng, name, 12)
    assert sorted(info) == ["Rnrm", "bounded", "its", "relError", "relResidual", "stepLength", "xHistory"]
    assert info["its"] == 12 and all(len(info[k]) == 12 for k in info if k != "its")
    assert x.shape == (P.shape[1], 1) and np.array_equal(x, info["xHistory"][-1])
    for k in range(12):
        assert _close(info["xHistory"][k], ref["X"][k])
    assert np.allclose(info["stepLength"], ref["alpha"][:12], rtol=1e-12, atol=0)
    assert info["bounded"] == [a < t for a, t in zip(ref["alpha"][:12], ref["theta"][:12])]
    assert np.allclose(info["Rnrm"], np.sqrt(ref["rr"][:12]) / np.linalg.norm(P.b.astype(np.float32).astype(np.float64)), rtol=1e-12)
    xs = [xk.astype(np.float64) for xk in ref["X"][:12]]
    assert np.allclose(info["relError"], [np.linalg.norm(xk - P.x_true.astype(np.float32)) / np.linalg.norm(P.x_true) for xk in xs],
                       rtol=1e-6)
    # ||alpha s|| is ||x_k - x_{k-1}|| up to the rounding of the update (the clamp moves an entry that alpha s takes to 0 anyway)
    prev = [P.x0.astype(np.float32).astype(np.float64)] + xs[:-1]
    assert np.allclose(info["relResidual"], [np.linalg.norm(a - b) / np.linalg.norm(a) for a, b in zip(xs, prev)], rtol=1e-3)
    _x2, info2 = S.MRNSD(OracleOp(P.oracle(), eng), P.b, P.x0, 12, 0)
    assert "relError" not in info2 and info2["stepLength"] == info["stepLength"]


@pytest.mark.parametrize("spec", [False, 3, "host", "file"])
def test_history_sinks(eng, spec, tmp_path):
    if spec == "file":
        spec = str(tmp_path / "xhist.npy")
    x0, i0 = _solve(eng, "P2", 11)
    x1, i1 = _solve(eng, "P2", 11, history=spec)
    assert np.array_equal(x0, x1) and i0["stepLength"] == i1["stepLength"]
    H = i1["xHistory"]
    if spec is False:
        assert H == []
        return
    assert H.iterations == (list(range(11)) if isinstance(spec, str) else [2, 5, 8, 10])
    for j, k in enumerate(H.iterations):
        assert np.array_equal(H[j], i0["xHistory"][k])
    if isinstance(spec, str) and spec.endswith(".npy"):
        assert np.load(spec, mmap_mode="r").shape == (11, x0.size)


def test_x0_rules(eng):
    P = C.problem("P4")
    A = OracleOp(P.oracle(), eng)
    n = P.shape[1]
    bad = [np.zeros(n), -np.ones(n), np.where(np.arange(n) == 3, -1e-3, 1.0), np.full(n, np.nan), np.ones(n + 1)]
    for x0 in bad:
        with pytest.raises(ValueError):
            S.MRNSD(A, P.b, x0, 3, 0)
    with pytest.raises(ValueError):
        S.MRNSD(A, P.b, P.x0, 0, 0)
    # None: the constant sum(b) / sum(A 1); the problems' x0 is that constant
    xa, ia = S.MRNSD(A, P.b, None, 5, 0)
    xb, ib = S.MRNSD(A, P.b, P.x0, 5, 0)
    assert np.allclose(xa, xb, rtol=1e-5) and np.allclose(ia["stepLength"], ib["stepLength"], rtol=1e-5)
    # ... and 1 when that constant is not positive
    xc, _ic = S.MRNSD(A, -np.abs(P.b), None, 1, 0, history=True)
    xd, _id = S.MRNSD(A, -np.abs(P.b), np.ones(n), 1, 0)
    assert np.array_equal(xc, xd)
    # entries equal to 0 are allowed and stay 0
    x0 = P.x0.copy()
    x0[::7] = 0.0
    x, info = S.MRNSD(A, P.b, x0, 6, 0)
    assert all(np.all(h[::7] == 0) and h.min() >= 0 for h in info["xHistory"])


@pytest.mark.parametrize("name", ["P1", "P3"])
def test_tol_stops_where_the_restatement_says(eng, runs, name):
    ref = runs[name][1]
    tol = 0.05
    hit = [k + 1 for k in range(K) if np.sqrt(ref["gamma"][k]) <= tol * np.sqrt(ref["gamma0"])]
    assert hit and 1 < hit[0] < K
    x, info = _solve(eng, name, K, tol=tol)
    assert info["its"] == hit[0] and len(info["xHistory"]) == hit[0] and len(info["stepLength"]) == hit[0]
    assert _close(x, ref["X"][hit[0] - 1])


@pytest.mark.parametrize("name", ["P1", "P4"])
def test_discrepancy_stops_where_the_restatement_says(eng, runs, name):
    ref = runs[name][1]
    delta = np.sqrt(ref["rr"][11]) / 1.01 * (1 + 1e-9)
    hit = [k + 1 for k in range(K) if np.sqrt(ref["rr"][k]) <= 1.01 * delta]
    assert hit[0] == 12
    x, info = _solve(eng, name, K, delta=delta)
    assert info["its"] == 12
    assert _close(x, ref["X"][11])
    # eta is honoured: a larger one stops earlier
    _x, info2 = _solve(eng, name, K, delta=delta, eta=1.5)
    assert info2["its"] < 12


@pytest.mark.parametrize("history", [True, False])
def test_breakdown_is_truncated(eng, history):
    """b = A x0: r = 0, gamma_0 = 0 — no step can be taken; one iteration is reported and it leaves x0 as it is."""
    P = C.problem("P1")
    A = OracleOp(P.oracle(), eng)
    b = A.apply(eng.to_vec(P.x0)).numpy().astype(np.float64)
    x, info = S.MRNSD(A, b, P.x0, 9, 0, history=history)
    assert info["its"] == 1 and info["stepLength"] == [0.0] and info["bounded"] == [False]
    assert np.array_equal(x.reshape(-1), P.x0.astype(np.float32).astype(np.float64))
    assert np.all(np.isfinite(x))


def test_sharded_is_not_built():
    class TwoRanks(MrnsdCpuEngine):
        def __init__(self):
            super().__init__()
            self.world = 2
    P = C.problem("P4")
    with pytest.raises(NotImplementedError):
        S.MRNSD(OracleOp(P.oracle(), TwoRanks()), P.b, P.x0, 3, 0)
