"""Ordered subsets without a GPU: the bookkeeping of operators.RowSubsets, the NumPy restatements of tests/os_cases.py checked
against what OSEM and SIRT promise, and the host logic of OSEM(), SIRT() and SART() driven through the CPU test engine."""
import numpy as np
import pytest

import mlem_cases as LC
import os_cases as C
from cpu_engine import OracleOp
from os_cpu_engine import OsCpuEngine
from trips_py_amd import solvers as S
from trips_py_amd.operators import RowSubsets, bit_reversed_order


@pytest.fixture(scope="module")
def eng():
    return OsCpuEngine()


def _subsets(eng, name, S_, order="bitrev"):
    rows = C.subset_rows(name, S_)
    return RowSubsets.from_ops([OracleOp(o, eng) for o in C.subset_oracles(name, S_)], rows, sum(len(r) for r in rows), order)


# ------------------------------------------------------------------ subset bookkeeping
@pytest.mark.parametrize("name,S_", [(n, s) for n in C.SUBSETS for s in C.SUBSETS[n]])
def test_rows_partition_and_split_join(eng, name, S_):
    sub = _subsets(eng, name, S_)
    m = C.problem(name, False).shape[0]
    assert sub.shape == C.problem(name, False).shape and len(sub.ops) == len(sub.rows) == S_
    assert np.array_equal(np.sort(np.concatenate(sub.rows)), np.arange(m))
    assert np.array_equal(np.sort(sub.perm), np.arange(m)) and np.array_equal(sub.perm, np.concatenate(sub.rows))
    assert list(sub.offsets) == list(np.cumsum([0] + [len(r) for r in sub.rows])) and sub.offsets[-1] == m
    b = np.random.default_rng(3).standard_normal(m)
    assert np.array_equal(sub.split(b), b[sub.perm]) and np.array_equal(sub.join(sub.split(b)), b)
    assert np.array_equal(sub.split(sub.join(b)), b)


@pytest.mark.parametrize("name,S_", [("P3", 5), ("P3", 12), ("P4", 3), ("F1", 3)])
def test_stacked_subset_oracles_are_the_permuted_operator(name, S_):
    """Each subset's float64 operator is made from its own angles / rows: stacked, they are A[perm] within 1e-12 relative."""
    P = C.problem(name, False)
    o = P.oracle()
    A = np.asarray(o.M.toarray() if hasattr(o, "M") else o.todense())
    perm = np.concatenate(C.subset_rows(name, S_))
    eye = np.eye(P.shape[1])
    stacked = np.vstack([mv(eye) for mv, _ in C.dense_pairs(name, S_)])
    assert stacked.shape == A.shape
    assert np.linalg.norm(stacked - A[perm]) <= 1e-12 * np.linalg.norm(A)


def test_bit_reversal_order():
    for S_, want in C.BITREV.items():
        assert bit_reversed_order(S_) == want == C.bitrev_order(S_), S_
    assert sorted(C.BITREV) == [1, 2, 3, 4, 5, 6, 7, 8, 12]


def test_visiting_orders(eng):
    assert _subsets(eng, "P3", 6).order == [0, 4, 2, 1, 5, 3]
    assert _subsets(eng, "P3", 6, "sequential").order == [0, 1, 2, 3, 4, 5]
    assert _subsets(eng, "P3", 3, [2, 0, 1]).order == [2, 0, 1]
    for bad in ([0, 1, 1], [0, 1], [1, 2, 3], "random"):
        with pytest.raises(ValueError):
            _subsets(eng, "P3", 3, bad)


def test_subset_errors(eng):
    P = C.problem("P4", False)
    ops = [OracleOp(o, eng) for o in C.subset_oracles("P4", 3)]
    rows = C.subset_rows("P4", 3)
    m = P.shape[0]
    for bad in ([rows[0], rows[1], rows[1]], [rows[0], rows[1], rows[2][:-1]], [rows[0], rows[1], np.append(rows[2][:-1], m)]):
        with pytest.raises(ValueError):                        # index lists that do not partition
            RowSubsets.from_ops(ops, bad, m)
    with pytest.raises(ValueError):
        RowSubsets.from_ops(ops[:2], rows, m)
    # an operator without views or rows to deal out: S > 1 says why, S = 1 wraps it
    A = OracleOp(P.oracle(), eng)
    with pytest.raises(ValueError, match="no views or rows"):
        RowSubsets(A, 2)
    one = RowSubsets(A, 1)
    assert one.ops == [A] and one.order == [0] and np.array_equal(one.perm, np.arange(m)) and one.shape == A.shape
    with pytest.raises(ValueError, match="no views"):
        S.SART(A, P.b, None, 3, 0)


# ------------------------------------------------------------------ OSEM in float64
def test_osem_with_one_subset_is_mlem_exactly():
    for name in ("P3", "P4"):
        P, o = C.problem(name, True), C.problem(name, True).oracle()
        a = C.osem_f64([(o.matvec, o.rmatvec)], [np.arange(P.shape[0])], [0], P.b, P.x0, 10, P.bg)
        b = LC.mlem_f64(o.matvec, o.rmatvec, P.b, P.x0, 10, P.bg)
        assert all(np.array_equal(x, y) for x, y in zip(a["X"], b["X"]))
        assert a["kl"] == b["kl"] and a["rr"] == b["rr"] and a["dd"] == b["dd"] and a["zeros"] == b["zeros"]


@pytest.mark.parametrize("name,S_", [(n, s) for n in C.SUBSETS for s in C.SUBSETS[n]])
def test_osem_iterates_stay_nonnegative_and_finite(name, S_):
    P = C.problem(name, True)
    for loop in (C.osem_f64, C.osem_f32):
        run = loop(C.dense_pairs(name, S_), C.subset_rows(name, S_), C.bitrev_order(S_), P.b, P.x0, 10, P.bg)
        assert all(float(x.min()) >= 0.0 and np.all(np.isfinite(x)) for x in run["X"])
        assert np.all(np.isfinite(run["kl"]))


def test_an_unseen_pixel_keeps_its_value():
    """One view per subset on P3: some pixels are seen by no ray of a subset.  That sub-step leaves them as they are — MLEM's update
    would set them to 0 for good — and they are still > 0 after 10 passes."""
    P = C.problem("P3", True)
    run = C.osem_f64(C.dense_pairs("P3", 12), C.subset_rows("P3", 12), C.bitrev_order(12), P.b, P.x0, 10, P.bg)
    unseen = [np.nonzero(si == 0)[0] for si in run["sinv"]]
    assert 1 <= max(len(u) for u in unseen) <= 42              # of 576 pixels (the views at 0 and 90 degrees see every pixel)
    checked = 0
    for _k, s, before, after in run["seen"]:
        assert np.array_equal(after[unseen[s]], before[unseen[s]])
        checked += len(unseen[s])
    assert checked > 0
    ever_unseen = np.unique(np.concatenate(unseen))
    assert np.all(run["X"][-1][ever_unseen] > 0)


def test_ordered_subsets_fit_faster_than_mlem():
    """KL over ALL the data after 5 passes with S = 2, 3, 4, 6 is below KL after 10 MLEM iterations (P3; float64)."""
    P, o = C.problem("P3", True), C.problem("P3", True).oracle()

    def kl_at(x):
        return float(np.sum(LC.kl_terms(P.b, o.matvec(x) + P.bg)))
    mlem = kl_at(C.osem_f64(C.dense_pairs("P3", 1), C.subset_rows("P3", 1), [0], P.b, P.x0, 10, P.bg)["X"][-1])
    for S_ in (2, 3, 4, 6):
        x = C.osem_f64(C.dense_pairs("P3", S_), C.subset_rows("P3", S_), C.bitrev_order(S_), P.b, P.x0, 5, P.bg)["X"][-1]
        assert kl_at(x) < mlem, (S_, kl_at(x), mlem)


# ------------------------------------------------------------------ SIRT in float64
@pytest.mark.parametrize("relax", [1.0, 1.9])
@pytest.mark.parametrize("S_", [1, 3, 12])
def test_sirt_weighted_residual_never_increases(S_, relax):
    P = C.problem("P3", False)
    run = C.sirt_f64(C.dense_pairs("P3", S_), C.subset_rows("P3", S_), C.bitrev_order(S_), P.b, np.zeros(P.shape[1]), 15, relax)
    wr = np.array(run["wr"])
    assert np.all(np.isfinite(wr)) and np.all(np.diff(wr) <= 0.0), wr


@pytest.mark.parametrize("name,S_", [("P3", 1), ("P3", 5), ("P4", 3), ("F1", 3)])
def test_sirt_stays_in_the_box_and_counts_its_bounds(name, S_):
    P = C.problem(name, False)
    hi = 0.2 * float(P.x_true.max())                       # active within the 12 passes on every case
    for loop in (C.sirt_f64, C.sirt_f32):
        run = loop(C.dense_pairs(name, S_), C.subset_rows(name, S_), C.bitrev_order(S_), P.b, np.zeros(P.shape[1]), 12, 1.0, 0.0, hi)
        for x, c in zip(run["X"], run["at_bound"]):
            assert x.min() >= 0.0 and x.max() <= x.dtype.type(hi)              # the bound as the run's precision holds it
            assert c == np.count_nonzero((x == 0.0) | (x == x.dtype.type(hi)))
        assert run["at_bound"][-1] > 0 and np.any(run["X"][-1] == run["X"][-1].dtype.type(hi))


# ------------------------------------------------------------------ OSEM() and SIRT() on the CPU engine
K = 12


def _close(x, ref):
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    return np.linalg.norm(np.asarray(x).reshape(-1) - ref) <= 1e-6 * np.linalg.norm(ref)


def _osem(eng, name, S_, max_iter, tol=0, **kw):
    P = C.problem(name, True)
    kw.setdefault("background", P.bg)
    kw.setdefault("x_true", P.x_true)
    return S.OSEM(OracleOp(P.oracle(), eng), P.b.reshape(-1, 1), P.x0, max_iter, tol, subsets=_subsets(eng, name, S_), **kw)


def _sirt(eng, name, S_, max_iter, tol=0, **kw):
    P = C.problem(name, False)
    kw.setdefault("x_true", P.x_true)
    return S.SIRT(OracleOp(P.oracle(), eng), P.b.reshape(-1, 1), None, max_iter, tol, subsets=_subsets(eng, name, S_), **kw)


@pytest.fixture(scope="module")
def faithful():
    """(kind, name, S) -> the storage-faithful run on the subset oracles, K passes, computed once."""
    cache = {}

    def get(kind, name, S_, **kw):
        key = (kind, name, S_, tuple(sorted(kw.items())))
        if key not in cache:
            P = C.problem(name, kind == "osem")
            pairs = [(o.matvec, o.rmatvec) for o in C.subset_oracles(name, S_)]
            rows, order = C.subset_rows(name, S_), C.bitrev_order(S_)
            if kind == "osem":
                cache[key] = C.osem_f32(pairs, rows, order, P.b, P.x0, K, P.bg, P.x_true)
            else:
                cache[key] = C.sirt_f32(pairs, rows, order, P.b, np.zeros(P.shape[1]), K, x_true=P.x_true, **kw)
        return cache[key]
    return get


@pytest.mark.parametrize("name,S_", [("P3", 1), ("P3", 5), ("P3", 12), ("P4", 3), ("F1", 3)])
def test_osem_info_and_iterates(eng, faithful, name, S_):
    """The CPU engine rounds an oracle product to fp32 once and calls the restatement's own launches: iterates and sums are the
    restatement's.  The vector background takes the subset-major route."""
    P, ref = C.problem(name, True), faithful("osem", name, S_)
    x, info = _osem(eng, name, S_, K)
    assert sorted(info) == ["KL", "Rnrm", "its", "objectiveFinal", "relError", "relResidual", "subsets", "xHistory", "zeros"]
    assert info["its"] == K and info["subsets"] == S_ and np.array_equal(x, info["xHistory"][-1])
    for k in range(K):
        assert _close(info["xHistory"][k], ref["X"][k])
    b32 = P.b.astype(np.float32).astype(np.float64)
    assert np.allclose(info["KL"], ref["kl"], rtol=1e-12, atol=0)
    assert np.allclose(info["Rnrm"], np.sqrt(ref["rr"]) / np.linalg.norm(b32), rtol=1e-12, atol=0)
    assert np.allclose(info["relResidual"], np.sqrt(np.array(ref["dd"]) / np.array(ref["xx"])), rtol=1e-12, atol=0)
    assert np.allclose(info["relError"], np.sqrt(ref["ee"]) / np.linalg.norm(P.x_true.astype(np.float32).astype(np.float64)), rtol=1e-12)
    assert info["zeros"] == ref["zeros"]
    # objectiveFinal: KL over all the data at the returned x, one product per subset
    x32 = np.asarray(x, dtype=np.float32).reshape(-1)
    kl = sum(LC.ratio_f32(o.matvec(x32.astype(np.float64)).astype(np.float32), P.bg, P.b[r])["kl"]
             for o, r in zip(C.subset_oracles(name, S_), C.subset_rows(name, S_)))
    assert np.isclose(info["objectiveFinal"], kl, rtol=1e-12, atol=0)
    xv, iv = _osem(eng, name, S_, K, background=np.full(P.shape[0], P.bg))
    assert np.array_equal(xv, x) and iv["KL"] == info["KL"]


@pytest.mark.parametrize("name,S_,kw", [("P3", 1, {}), ("P3", 5, {"relax": 1.5}), ("P3", 12, {"lower": 0.0, "upper": 1.5}),
                                        ("P4", 3, {"lower": 0.0}), ("F1", 3, {})])
def test_sirt_info_and_iterates(eng, faithful, name, S_, kw):
    P = C.problem(name, False)
    ref = faithful("sirt", name, S_, relax=kw.get("relax", 1.0), lo=kw.get("lower", -np.inf), hi=kw.get("upper", np.inf))
    x, info = _sirt(eng, name, S_, K, **kw)
    assert sorted(info) == ["Rnrm", "atBound", "its", "relError", "relResidual", "subsets", "weightedResidual", "xHistory"]
    assert info["its"] == K and info["subsets"] == S_ and np.array_equal(x, info["xHistory"][-1])
    for k in range(K):
        assert _close(info["xHistory"][k], ref["X"][k])
    b32 = P.b.astype(np.float32).astype(np.float64)
    assert np.allclose(info["Rnrm"], np.sqrt(ref["rr"]) / np.linalg.norm(b32), rtol=1e-12, atol=0)
    assert np.allclose(info["weightedResidual"], ref["wr"], rtol=1e-12, atol=0)
    assert info["atBound"] == ref["at_bound"]
    assert info["atBound"] == [int(np.count_nonzero((h == kw.get("lower", np.inf)) | (h == kw.get("upper", np.inf))))
                               for h in info["xHistory"]]
    if "upper" in kw:
        assert info["atBound"][-1] > 0 and max(float(h.max()) for h in info["xHistory"]) == kw["upper"]


def test_landweber_and_sart(eng):
    """weights=None: x <- x + (relax / normA2) A^T (b - A x), one subset; SART: one view per subset of an operator with views."""
    P = C.problem("P4", False)
    o = P.oracle()
    A = OracleOp(o, eng)
    M = o.M.toarray()
    normA2 = float(np.linalg.norm(M, 2) ** 2)
    x, info = S.SIRT(A, P.b, None, 5, 0, weights=None, normA2=normA2, relax=1.0)
    xr = np.zeros(P.shape[1])
    for _ in range(5):
        xr = xr + (1.0 / normA2) * (M.T @ (P.b - M @ xr))
    assert np.linalg.norm(x.reshape(-1) - xr) <= 1e-5 * np.linalg.norm(xr)
    assert info["subsets"] == 1 and np.all(np.diff(info["Rnrm"]) < 0)
    b32 = P.b.astype(np.float32).astype(np.float64)
    assert np.allclose(np.square(info["Rnrm"]) * np.dot(b32, b32), info["weightedResidual"], rtol=1e-12)      # R = I: slot 1 is slot 0

    class WithViews(OracleOp):                                  # what SART asks of an operator: its views
        angles = np.linspace(0, np.pi, 12, endpoint=False)
    P3 = C.problem("P3", False)
    Av = WithViews(P3.oracle(), eng)
    with pytest.raises(ValueError, match="no views or rows"):   # ... and RowSubsets deals out views of the engine's projectors only
        S.SART(Av, P3.b, None, 2, 0)
    with pytest.raises(ValueError, match="the subsets are the views"):
        S.SART(Av, P3.b, None, 2, 0, subsets=3)


@pytest.mark.parametrize("kind,name,S_", [("osem", "P3", 5), ("sirt", "P3", 5), ("osem", "P4", 3), ("sirt", "F1", 3)])
def test_tol_stops_where_the_rows_say(eng, faithful, kind, name, S_):
    ref = faithful(kind, name, S_, **({} if kind == "osem" else {"relax": 1.0, "lo": -np.inf, "hi": np.inf}))
    rel = np.sqrt(np.array(ref["dd"]) / np.array(ref["xx"]))
    tol = float(rel[5]) * (1 + 1e-9)
    hit = [k + 1 for k in range(K) if rel[k] <= tol][0]
    assert 1 < hit < K
    x, info = (_osem if kind == "osem" else _sirt)(eng, name, S_, K, tol=tol)
    assert info["its"] == hit and len(info["xHistory"]) == hit and len(info["relResidual"]) == hit
    assert _close(x, ref["X"][hit - 1])


@pytest.mark.parametrize("history", [True, False, 3])
@pytest.mark.parametrize("kind", ["osem", "sirt"])
def test_delta_returns_the_current_pass(eng, faithful, kind, history):
    """The running residual of pass k meets eta delta: the solve stops there and returns x_k."""
    ref = faithful(kind, "P3", 5, **({} if kind == "osem" else {"relax": 1.0, "lo": -np.inf, "hi": np.inf}))
    res = np.sqrt(ref["rr"])
    delta = res[6] / 1.01 * (1 + 1e-9)
    first = [k + 1 for k in range(K) if res[k] <= 1.01 * delta][0]
    assert 1 < first <= 7
    solve = _osem if kind == "osem" else _sirt
    x, info = solve(eng, "P3", 5, K, delta=delta, history=history)
    assert info["its"] == first and len(info["Rnrm"]) == first
    assert _close(x, ref["X"][first - 1])
    if history is True:
        assert len(info["xHistory"]) == first and np.array_equal(x, info["xHistory"][-1])
    elif history is False:
        assert info["xHistory"] == []
    else:
        assert info["xHistory"].iterations == sorted(set(list(range(2, first, 3)) + [first - 1]))
    _x, info2 = solve(eng, "P3", 5, K, delta=delta, eta=1.5)
    assert info2["its"] < first


def test_history_sinks(eng):
    x0, i0 = _osem(eng, "P3", 3, 11)
    for spec in (False, 3):
        x1, i1 = _osem(eng, "P3", 3, 11, history=spec)
        assert np.array_equal(x0, x1) and i0["KL"] == i1["KL"]
        if spec is False:
            assert i1["xHistory"] == []
        else:
            assert i1["xHistory"].iterations == [2, 5, 8, 10]
            assert all(np.array_equal(i1["xHistory"][j], i0["xHistory"][k]) for j, k in enumerate([2, 5, 8, 10]))


def test_input_rules(eng):
    P, G = C.problem("P4", True), C.problem("P4", False)
    A = OracleOp(P.oracle(), eng)
    m, n = P.shape
    sub = _subsets(eng, "P4", 3)
    with pytest.raises(ValueError, match="counts cannot be negative"):
        S.OSEM(A, np.where(np.arange(m) == 5, -1.0, P.b), P.x0, 3, 0, subsets=sub)
    for x0 in (np.where(np.arange(n) == 3, 0.0, 1.0), -np.ones(n), np.full(n, np.nan), np.ones(n + 1)):
        with pytest.raises(ValueError):
            S.OSEM(A, P.b, x0, 3, 0, subsets=sub)
    with pytest.raises(ValueError):
        S.OSEM(A, P.b, P.x0, 0, 0, subsets=sub)
    with pytest.raises(ValueError, match="no views or rows"):
        S.OSEM(A, P.b, P.x0, 3, 0, subsets=2)                  # an OracleOp has nothing to deal out
    for relax in (0.0, 2.0, -0.5, 2.5, np.nan):
        with pytest.raises(ValueError, match="relax"):
            S.SIRT(A, G.b, None, 3, 0, subsets=sub, relax=relax)
    with pytest.raises(ValueError, match="subsets=1 only"):
        S.SIRT(A, G.b, None, 3, 0, subsets=sub, weights=None, normA2=1.0)
    with pytest.raises(ValueError):
        S.SIRT(A, G.b, None, 3, 0, lower=1.0, upper=0.0)
    with pytest.raises(ValueError):
        S.SIRT(A, G.b[:-1], None, 3, 0)
    with pytest.raises(ValueError):
        S.SIRT(A, G.b, None, 3, 0, weights="cimmino")
    # subsets made for another operator are refused
    with pytest.raises(ValueError):
        S.OSEM(A, P.b, P.x0, 3, 0, subsets=_subsets(eng, "P3", 3))
    # x0 = None: OSEM starts from the constant sum(b - bg) / sum(A 1), SIRT from zeros clipped into the box
    xa, _ia = S.OSEM(A, P.b, None, 4, 0, subsets=sub)
    xb, _ib = S.OSEM(A, P.b, P.x0, 4, 0, subsets=sub)
    assert np.allclose(xa, xb, rtol=1e-5)
    _x, info = S.SIRT(A, G.b, None, 1, 0, subsets=sub, lower=0.25, relax=1e-6)
    assert float(info["xHistory"][0].min()) >= 0.25


def test_sharded_is_not_built():
    class TwoRanks(OsCpuEngine):
        def __init__(self):
            super().__init__()
            self.world = 2
    P = C.problem("P4", True)
    for solve in (S.OSEM, S.SIRT):
        with pytest.raises(NotImplementedError):
            solve(OracleOp(P.oracle(), TwoRanks()), P.b, P.x0, 3, 0)
