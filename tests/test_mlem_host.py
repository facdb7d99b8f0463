"""MLEM / Richardson-Lucy without a GPU: the NumPy restatement of tests/mlem_cases.py checked against what the method promises, and
MLEM()'s host logic (input rules, info, history sinks, stopping) driven through the CPU test engine."""
import numpy as np
import pytest

import mlem_cases as C
from cpu_engine import OracleOp
from mlem_cpu_engine import MlemCpuEngine
from trips_py_amd import solvers as S

K = 30


@pytest.fixture(scope="module")
def eng():
    return MlemCpuEngine()


@pytest.fixture(scope="module")
def runs():
    """name -> (float64 run, storage-faithful run), K iterations each, computed once."""
    out = {}
    for name in C.NAMES:
        P, o = C.problem(name), C.problem(name).oracle()
        out[name] = (C.mlem_f64(o.matvec, o.rmatvec, P.b, P.x0, K, P.bg), C.mlem_f32(o.matvec, o.rmatvec, P.b, P.x0, K, P.bg, P.x_true))
    return out


# ------------------------------------------------------------------ the restatement itself
def test_kl_terms_cover_the_domain_without_nan():
    b = np.array([3.0, 0.0, 0.0, 2.0, 2.0, 0.0, -1.0, 2.0, np.inf, 0.0], dtype=np.float32)
    y = np.array([3.0, 0.0, 4.0, 0.0, -1.0, -1.0, 1.0, np.inf, 1.0, np.inf], dtype=np.float32)
    t = C.kl_terms(b, y)
    assert not np.any(np.isnan(t))
    assert t[0] == 0.0 and t[1] == 0.0 and t[2] == 4.0 and np.all(np.isinf(t[3:]))
    assert C.kl_terms(np.float32([2.0]), np.float32([3.0]))[0] == (3.0 - 2.0) + 2.0 * np.log(2.0 / 3.0)


def test_the_problems_are_photon_counts():
    for name in C.NAMES:
        P = C.problem(name)
        assert np.all(P.b >= 0) and np.array_equal(P.b, np.round(P.b)) and P.b.dtype == np.float64
        assert np.all(P.x0 > 0) and P.bg == C.BACKGROUND[name]
    P = C.problem("P1")
    assert np.any(P.b == 0) and np.all(P.oracle().matvec(P.x0) + P.bg > 0)


@pytest.mark.parametrize("name", C.NAMES)
def test_iterates_stay_nonnegative(runs, name):
    for run in runs[name]:
        assert all(float(x.min()) >= 0.0 and np.all(np.isfinite(x)) for x in run["X"])


@pytest.mark.parametrize("name", C.EXACT_ADJOINT)
def test_kl_never_increases_with_an_exact_adjoint(runs, name):
    """The EM property, in float64 (P1: from about 2e4 down by a factor of more than 30 over the 30 iterations)."""
    kl = np.array(runs[name][0]["kl"])
    assert np.all(np.isfinite(kl)) and np.all(np.diff(kl) <= 0.0), kl
    if name == "P1":
        assert kl[-1] < kl[0] / 10


@pytest.mark.parametrize("name", ["P1", "P4"])
def test_flux_is_conserved_without_background(name):
    """bg = 0 and an exact adjoint: sum_i s_i x_k,i = sum_j b_j for every k >= 1, in float64."""
    P, o = C.problem(name), C.problem(name).oracle()
    run = C.mlem_f64(o.matvec, o.rmatvec, P.b, P.x0, K, 0.0)
    worst = max(abs(np.dot(run["s"], x) / P.b.sum() - 1.0) for x in run["X"])
    assert worst <= 1e-12, worst


def test_fixed_point_of_consistent_data():
    """b = A x exactly and bg = 0: rho = 1, t = s, and x stays where it is."""
    P, o = C.problem("P4"), C.problem("P4").oracle()
    x = 1.0 + np.arange(P.shape[1]) / 7.0
    run = C.mlem_f64(o.matvec, o.rmatvec, o.matvec(x), x, 3, 0.0)
    assert all(np.allclose(xk, x, rtol=1e-13, atol=0) for xk in run["X"]) and max(run["kl"]) < 1e-12


# ------------------------------------------------------------------ MLEM() on the CPU engine
def _close(x, ref):
    """Equal up to a few fp32 roundings (relative 2-norm)."""
    ref = ref.astype(np.float64).reshape(-1)
    return np.linalg.norm(np.asarray(x).reshape(-1) - ref) <= 1e-6 * np.linalg.norm(ref)


def _solve(eng, name, max_iter, tol=0, x0="problem", **kw):
    P = C.problem(name)
    A = OracleOp(P.oracle(), eng)
    kw.setdefault("background", P.bg)
    return S.MLEM(A, P.b.reshape(-1, 1), P.x0 if isinstance(x0, str) else x0, max_iter, tol, x_true=P.x_true, **kw)


@pytest.mark.parametrize("name", C.NAMES)
def test_info_and_iterates(eng, runs, name):
    """The CPU engine rounds an oracle product to fp32 once, as the storage-faithful restatement does, and calls the restatement's
    own launches: the iterates and the sums are the restatement's."""
    P, ref = C.problem(name), runs[name][1]
    x, info = _solve(eng, name, 12)
    assert sorted(info) == ["KL", "Rnrm", "its", "objectiveFinal", "relError", "relResidual", "xHistory", "zeros"]
    assert info["its"] == 12 and all(len(info[k]) == 12 for k in info if k not in ("its", "objectiveFinal"))
    assert x.shape == (P.shape[1], 1) and np.array_equal(x, info["xHistory"][-1])
    for k in range(12):
        assert _close(info["xHistory"][k], ref["X"][k])
    b32 = P.b.astype(np.float32).astype(np.float64)
    assert np.allclose(info["KL"], ref["kl"][:12], rtol=1e-12, atol=0)
    assert np.allclose(info["Rnrm"], np.sqrt(ref["rr"][:12]) / np.linalg.norm(b32), rtol=1e-12, atol=0)
    assert np.allclose(info["relResidual"], np.sqrt(np.array(ref["dd"][:12]) / np.array(ref["xx"][:12])), rtol=1e-12, atol=0)
    assert np.allclose(info["relError"], np.sqrt(ref["ee"][:12]) / np.linalg.norm(P.x_true.astype(np.float32).astype(np.float64)),
                       rtol=1e-12, atol=0)
    assert info["zeros"] == ref["zeros"][:12]
    # KL[k - 1] is the value at x_{k-1}; objectiveFinal the one at the returned x, i.e. what a 13th iteration reports
    assert np.isclose(info["objectiveFinal"], ref["kl"][12], rtol=1e-12, atol=0)
    _x2, info2 = S.MLEM(OracleOp(P.oracle(), eng), P.b, P.x0, 12, 0, background=P.bg)
    assert "relError" not in info2 and info2["KL"] == info["KL"]


def test_vector_background_and_alias(eng):
    P = C.problem("P3")
    xa, ia = _solve(eng, "P3", 6)
    xb, ib = _solve(eng, "P3", 6, background=np.full(P.shape[0], P.bg))
    assert np.array_equal(xa, xb) and ia["KL"] == ib["KL"]
    assert S.RichardsonLucy is S.MLEM


@pytest.mark.parametrize("spec", [False, 3, "host", "file"])
def test_history_sinks(eng, spec, tmp_path):
    if spec == "file":
        spec = str(tmp_path / "xhist.npy")
    x0, i0 = _solve(eng, "P2", 11)
    x1, i1 = _solve(eng, "P2", 11, history=spec)
    assert np.array_equal(x0, x1) and i0["KL"] == i1["KL"]
    H = i1["xHistory"]
    if spec is False:
        assert H == []
        return
    assert H.iterations == (list(range(11)) if isinstance(spec, str) else [2, 5, 8, 10])
    for j, k in enumerate(H.iterations):
        assert np.array_equal(H[j], i0["xHistory"][k])
    if isinstance(spec, str) and spec.endswith(".npy"):
        assert np.load(spec, mmap_mode="r").shape == (11, x0.size)


def test_input_rules(eng):
    P = C.problem("P4")
    A = OracleOp(P.oracle(), eng)
    m, n = P.shape
    # a zero (or negative, or non-finite) entry of x0 is refused: it would never move
    for x0 in (np.where(np.arange(n) == 3, 0.0, 1.0), np.zeros(n), -np.ones(n), np.full(n, np.nan), np.full(n, np.inf), np.ones(n + 1)):
        with pytest.raises(ValueError):
            S.MLEM(A, P.b, x0, 3, 0)
    with pytest.raises(ValueError, match="counts cannot be negative"):
        S.MLEM(A, np.where(np.arange(m) == 5, -1.0, P.b), P.x0, 3, 0)
    for b in (np.where(np.arange(m) == 5, np.nan, P.b), np.where(np.arange(m) == 5, np.inf, P.b), P.b[:-1]):
        with pytest.raises(ValueError):
            S.MLEM(A, b, P.x0, 3, 0)
    for bg in (-1.0, np.nan, np.inf, np.full(m, -1.0), np.ones(m - 1)):
        with pytest.raises(ValueError):
            S.MLEM(A, P.b, P.x0, 3, 0, background=bg)
    with pytest.raises(ValueError):
        S.MLEM(A, P.b, P.x0, 0, 0)
    # None: the constant sum(b - bg) / sum(A 1); the problems' x0 is that constant
    P1 = C.problem("P1")
    A1 = OracleOp(P1.oracle(), eng)
    xa, ia = S.MLEM(A1, P1.b, None, 5, 0, background=P1.bg)
    xb, ib = S.MLEM(A1, P1.b, P1.x0, 5, 0, background=P1.bg)
    assert np.allclose(xa, xb, rtol=1e-5) and np.allclose(ia["KL"], ib["KL"], rtol=1e-5)
    # ... and 1 when that constant is not positive
    xc, _ic = S.MLEM(A, np.zeros(m), None, 1, 0)
    xd, _id = S.MLEM(A, np.zeros(m), np.ones(n), 1, 0)
    assert np.array_equal(xc, xd)


def test_an_unseen_unknown_becomes_zero(eng):
    """s_i = (A^T 1)_i = 0 — a column no datum sees: sinv_i = 0, x_i = 0 from the first iteration on, everything else finite."""
    from oracle import cpu_ref as O
    P = C.problem("P4")
    M = C.MC._sparse_matrix().tolil()
    M[:, 17] = 0.0
    A = OracleOp(O.MatrixOp(M.tocsr()), eng)
    x, info = S.MLEM(A, P.b, P.x0, 5, 0)
    assert all(h[17, 0] == 0.0 and np.all(np.isfinite(h)) and h.min() >= 0 for h in info["xHistory"])
    assert all(z >= 1 for z in info["zeros"]) and np.all(np.isfinite(info["KL"]))


@pytest.mark.parametrize("name", ["P1", "P3"])
def test_tol_stops_where_the_restatement_says(eng, runs, name):
    ref = runs[name][1]
    rel = np.sqrt(np.array(ref["dd"]) / np.array(ref["xx"]))
    tol = float(rel[7]) * (1 + 1e-9)
    hit = [k + 1 for k in range(K) if rel[k] <= tol]
    assert hit and 1 < hit[0] < K
    x, info = _solve(eng, name, K, tol=tol)
    assert info["its"] == hit[0] and len(info["xHistory"]) == hit[0] and len(info["KL"]) == hit[0]
    assert _close(x, ref["X"][hit[0] - 1])


@pytest.mark.parametrize("history", [True, False, 3])
@pytest.mark.parametrize("name", ["P1", "P4"])
def test_discrepancy_returns_the_iterate_the_row_describes(eng, runs, name, history):
    """Row k holds ||A x_{k-1} + bg - b||: when it meets eta delta at k >= 2 the solve returns x_{k-1} with its = k - 1."""
    ref = runs[name][1]
    res = np.sqrt(ref["rr"])                                  # res[j] describes x_j (x_0 = the start), read from row j + 1
    delta = res[9] / 1.01 * (1 + 1e-9)
    first = [j for j in range(1, K) if res[j] <= 1.01 * delta][0]
    assert 1 < first <= 9
    x, info = _solve(eng, name, K, delta=delta, history=history)
    assert info["its"] == first and len(info["KL"]) == first and len(info["zeros"]) == first
    assert _close(x, ref["X"][first - 1])
    if history is True:
        assert len(info["xHistory"]) == first and np.array_equal(x, info["xHistory"][-1])
    # the start itself is never returned (k >= 2), and eta is honoured: a larger one stops earlier
    _x, info1 = _solve(eng, name, K, delta=10 * res[0])
    assert info1["its"] == 1
    _x, info2 = _solve(eng, name, K, delta=delta, eta=1.5)
    assert info2["its"] < first


def test_sharded_is_not_built():
    class TwoRanks(MlemCpuEngine):
        def __init__(self):
            super().__init__()
            self.world = 2
    P = C.problem("P4")
    with pytest.raises(NotImplementedError):
        S.MLEM(OracleOp(P.oracle(), TwoRanks()), P.b, P.x0, 3, 0)


def test_poisson_noise():
    from trips_py_amd.problems import poisson_noise
    bt = np.array([[0.0, 1.0], [2.5, 10.0]])
    b = poisson_noise(bt, seed=3)
    assert b.dtype == np.float64 and b.shape == bt.shape and np.array_equal(b, np.round(b)) and b[0, 0] == 0.0
    assert np.array_equal(b, poisson_noise(bt, seed=3)) and np.array_equal(b, np.random.default_rng(3).poisson(bt))
    big = poisson_noise(np.full(20000, 0.5), peak=100.0, background=7.0, seed=1)
    assert abs(big.mean() - 107.0) < 0.5 and not np.array_equal(big, poisson_noise(np.full(20000, 0.5), peak=100.0, background=7.0, seed=2))
    with pytest.raises(ValueError):
        poisson_noise(-bt)
