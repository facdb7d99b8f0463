"""PDHG with isotropic space-time TV (tv='iso3') without a GPU: the NumPy restatement of tests/pdhg_iso3_cases.py checked against the
optimality conditions of the program it solves, the bookkeeping of its groups and what fp32 storage costs, and PDHG(tv='iso3')'s
host logic (the geometry, info, argument errors) driven through the CPU test engine."""
import numpy as np
import pytest

import pdhg_cases as C
import pdhg_iso3_cases as T
import pdhg_iso_cases as I
from cpu_engine import OracleOp
from pdhg_iso3_cpu_engine import PdhgIso3CpuEngine
from trips_py_amd import solvers as S
from trips_py_amd.operators import Identity


@pytest.fixture(scope="module")
def eng():
    return PdhgIso3CpuEngine()


# ------------------------------------------------------------------ (0) the groups partition the rows
@pytest.mark.parametrize("N,frames", [(2, 1), (2, 2), (3, 4), (5, 3)])
def test_groups_partition_the_rows(N, frames):
    g = T.groups3(N, frames)
    assert sorted(g) == sorted(T.KINDS)
    assert g["hvt"].shape[0] == 3 and all(g[k].shape[0] == 2 for k in ("hv", "ht", "vt")) and g["single"].ndim == 1
    assert {k: g[k].shape[-1] for k in T.KINDS} == T.group_counts(N, frames)
    every = np.concatenate([g[k].reshape(-1) for k in T.KINDS])
    assert np.array_equal(np.sort(every), np.arange(T.rows_of(N, frames)))            # each row in exactly one group
    # the voxels: every one but the last has exactly one group
    assert sum(T.group_counts(N, frames).values()) == frames * N * N - 1
    # a group is the differences that START at one voxel: the dense operator's rows have their +1 in the same column, and the
    # members come in row order
    from oracle import cpu_ref as O
    Lm = np.asarray(O.SpaceTimeDerivative(N, frames).todense())
    for k in ("hvt", "hv", "ht", "vt"):
        cols = [np.argmax(Lm[r], axis=1) for r in g[k]]
        assert all(np.array_equal(cols[0], c) for c in cols[1:]) and all(np.all(Lm[r].max(axis=1) == 1.0) for r in g[k])
        assert all(np.all(a < b) for a, b in zip(g[k][:-1], g[k][1:]))


# ------------------------------------------------------------------ (0b) one frame: the isotropic dual, bit for bit
@pytest.mark.parametrize("N", [2, 5, 16])
def test_one_frame_is_the_isotropic_dual(N):
    rng = np.random.default_rng(N)
    rows = T.rows_of(N, 1)
    assert rows == 2 * N * (N - 1)
    u, q = (rng.random(rows) - 0.5).astype(np.float32), (0.1 * rng.random(rows) - 0.05).astype(np.float32)
    a, b = T.dual_q_iso3_f32(N, 1, 0.37, 0.1, u, q), I.dual_q_iso_f32(N, 1, 0.37, 0.1, u, q)
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[0], q)
    assert abs(a[1] - b[1]) <= 1e-14 * b[1] and abs(a[2] - b[2]) <= 1e-14 * b[2]


def test_crafted_triple_is_exact():
    """t = (2, 3, 6) has norm 7: kept at lam = 7, halved at lam = 3.5 — every number exact in fp32."""
    g = T.groups3(2, 2)
    rh, rv, rt = (int(r[0]) for r in g["hvt"])
    u, q = np.zeros(T.rows_of(2, 2), dtype=np.float32), np.zeros(T.rows_of(2, 2), dtype=np.float32)
    u[[rh, rv, rt]], q[[rh, rv, rt]] = (2.0, 4.0, 8.0), (1.0, 1.0, 2.0)
    for lam, want in ((7.0, (2.0, 3.0, 6.0)), (3.5, (1.0, 1.5, 3.0))):
        qn, s1, _s3 = T.dual_q_iso3_f32(2, 2, 0.5, lam, u, q)
        assert tuple(qn[[rh, rv, rt]]) == want and abs(s1 - np.sqrt(84.0)) < 1e-14


# ------------------------------------------------------------------ (1) the restatement solves the program
def test_fixed_point_satisfies_the_kkt_conditions():
    """(N, nt) = (4, 3), a dense seeded 60 x 48 matrix, lam = 0.02, box [0, 0.9], step 0.95 / ||K||: where the float64 iteration
    stops moving (relative step <= 1e-14) the point satisfies the optimality conditions of
    min 1/2 ||A x - b||^2 + lam sum_g ||(L x)_g||_2 over the box with the groups (h, v, t), stated without reference to the
    iteration: q in the subdifferential of the group norms at L x (every group inside the ball; on the sphere, along u_g, where
    u_g != 0), p = A x - b, and A^T p + L^T q zero on the free entries, >= 0 at the lower and <= 0 at the upper bound.  The bar is
    the one of tests/test_pdhg_iso_host.py.  (Reached in 458 iterations with residuals <= 5.7e-14; 5 entries at the lower bound, 11
    at the upper, 32 free; 17 of 18 triples non-zero, all 17 with three non-zero members, and every pair and single non-zero.  A
    wrong group shows at the size of lam = 0.02.)"""
    from oracle import cpu_ref as O
    N, nt, m = 4, 3, 60
    n = N * N * nt
    rng = np.random.default_rng(3)
    M = rng.standard_normal((m, n)) / np.sqrt(n)
    xt = np.clip(rng.random(n) * 1.6 - 0.3, 0, None).reshape(nt, N, N)
    xt[1, 1:3, 1:3] += 0.8
    xt = xt.reshape(-1)
    bt = M @ xt
    e = rng.standard_normal(m)
    b = bt + 0.02 * np.linalg.norm(bt) / np.linalg.norm(e) * e
    Lo = O.SpaceTimeDerivative(N, nt)
    Lm = np.asarray(Lo.todense())
    lam, lo, hi = 0.02, 0.0, 0.9
    step = 0.95 / np.sqrt(np.linalg.eigvalsh(M.T @ M + Lm.T @ Lm)[-1])
    run = T.pdhg_iso3_f64((lambda v: M @ v, lambda v: M.T @ v), C.pair(Lo), b, lam, step, step, lo, hi, None, 200000, (N, nt),
                          stop_step=1e-14)
    assert len(run["X"]) < 200000, "the iteration did not stop moving: raise the budget"
    x, p, q = run["X"][-1], run["p"], run["q"]
    at_lo, at_hi = x == lo, x == hi
    assert at_lo.sum() >= 1 and at_hi.sum() >= 1 and (~at_lo & ~at_hi).sum() >= 1
    assert np.all((x >= lo) & (x <= hi))
    tol = 1e-10 * max(np.linalg.norm(b), 1.0)
    worst = np.abs(p - (M @ x - b)).max()
    assert worst <= tol
    qn = T.group_norms(N, nt, q)
    assert max(v.max() for v in qn.values()) <= lam + tol
    u = Lm @ x
    g, un = T.groups3(N, nt), T.group_norms(N, nt, u)
    for kind in T.KINDS:
        rows = g[kind] if kind != "single" else g[kind][None]
        big = un[kind] > 1e-8
        assert big.sum() >= 1, kind                                                   # a non-zero group of every kind
        for r in rows:
            worst = max(worst, np.abs(q[r][big] - lam * u[r][big] / un[kind][big]).max())
    assert np.count_nonzero((un["hvt"] > 1e-8) & np.all(u[g["hvt"]] != 0, axis=0)) >= 1   # triples with three non-zero members
    gr = M.T @ p + Lm.T @ q
    worst = max(worst, np.abs(gr[~at_lo & ~at_hi]).max(), -gr[at_lo].min(), gr[at_hi].max())
    print("KKT residual %.3e (bar %.3e)" % (worst, tol))
    assert worst <= tol


# ------------------------------------------------------------------ (2) what fp32 storage costs
@pytest.fixture(scope="module")
def runs():
    """name -> (float64 run, storage-faithful run in the fused kernels' order), 30 iterations each, computed once."""
    return {name: (T.f64(name, 30, x_true=T.problem(name).x_true), T.f32(name, 30, x_true=T.problem(name).x_true, fused=True))
            for name in T.NAMES}


def _figures(P, f64, f32):
    obj = [0.5 * r["S"][:, 0] + P.lam * r["S"][:, 1] for r in (f32, f64)]
    return (C.worst_distance(f32, f64), float(np.max(np.abs(np.sqrt(f32["S"][:, 0] / f64["S"][:, 0]) - 1))),
            float(np.max(np.abs(obj[0] / obj[1] - 1))))


@pytest.mark.parametrize("name", T.NAMES)
def test_fp32_storage_cost_is_the_recorded_one(runs, name):
    """The constants the GPU test's bars are built from (tests/test_gpu_pdhg_iso3.py) are these figures, up to the host's BLAS."""
    import test_gpu_pdhg_iso3 as G
    got = _figures(T.problem(name), *runs[name])
    print(name, "iterates %.3e Rnrm %.3e objective %.3e" % got)
    for fig, table in zip(got, (G.CPU_F32_ITERATES, G.CPU_F32_RNRM, G.CPU_F32_OBJECTIVE)):
        assert 0.5 * table[name] <= fig <= 2.0 * table[name], (name, got)
        assert fig < 5e-7, (name, got)


def test_q5u_has_its_upper_bound_active(runs):
    P = T.problem("Q5u")
    assert np.isfinite(P.hi) and P.hi == float(np.float32(P.hi)) and P.lo == 0.0
    x64, x32 = runs["Q5u"][0]["X"][-1], runs["Q5u"][1]["X"][-1]
    assert np.count_nonzero(x64 == P.hi) > T.Q5U_MIN_AT_UPPER and np.count_nonzero(x32 == np.float32(P.hi)) > T.Q5U_MIN_AT_UPPER
    assert np.count_nonzero(x64 == 0.0) >= 1
    assert runs["Q5"][0]["X"][-1].max() > P.hi                    # and the bound binds: Q5's own solve goes above it


# ------------------------------------------------------------------ (3) the iterates
@pytest.mark.parametrize("name", T.NAMES)
def test_iterates_stay_in_the_box_and_the_objective_falls(runs, name):
    P = T.problem(name)
    for run in runs[name]:
        assert all(float(x.min()) >= P.lo and float(x.max()) <= P.hi for x in run["X"])
        obj = 0.5 * run["S"][:, 0] + P.lam * run["S"][:, 1]
        assert obj[29] < obj[9] < obj[0]


def test_it_is_not_the_isotropic_solve(runs):
    """On Q5 the 'iso3' iterate after 30 iterations is another point than the 'iso' one (spatially isotropic, temporally l1): no
    test of this term passes on the kernels of that one.  Slot 1 is the sum of three-member norms: never above 'iso''s."""
    iso = I.f64("Q5", 30)
    x3, xi = runs["Q5"][0]["X"][-1], iso["X"][-1]
    dist = np.linalg.norm(x3 - xi) / np.linalg.norm(xi)
    print("iso3 against iso after 30 iterations: %.3e" % dist)
    assert dist > 1e-3
    assert runs["Q5"][0]["S"][0, 0] == iso["S"][0, 0]
    assert np.all(runs["Q5"][0]["S"][1:, 1] != iso["S"][1:, 1])
    u = C.problem("Q5").oracle_L().matvec(xi)
    assert T.norm_sum(16, 3, u) < float(I.group_norms(16, 3, u).sum())


# ------------------------------------------------------------------ (4) PDHG(tv='iso3') on the CPU engine
def _ops(eng, name):
    P = T.problem(name)
    return P, OracleOp(P.oracle(), eng), OracleOp(P.oracle_L(), eng)


def _solve(eng, name, max_iter, **kw):
    P, A, L = _ops(eng, name)
    kw.setdefault("x_true", P.x_true)
    return S.PDHG(A, P.b.reshape(-1, 1), L, P.lam, max_iter, 0, lower=P.lo, upper=P.hi, sigma=P.sigma, tau=P.tau, **kw)


def _close(x, ref):
    ref = ref.astype(np.float64).reshape(-1)
    return np.linalg.norm(np.asarray(x).reshape(-1) - ref) <= 1e-6 * np.linalg.norm(ref)


@pytest.mark.parametrize("name", T.NAMES)
def test_info_and_iterates(eng, name):
    P, geo = T.problem(name), T.GEOMETRY[name]
    ref = T.f32(name, 12, x_true=P.x_true)                     # the unfused forms: what the CPU engine has
    x, info = _solve(eng, name, 12, tv="iso3", tv_dims=geo)
    per_iter = ["Rnrm", "active", "dualChange", "objective", "relError", "relResidual", "xHistory"]
    assert sorted(info) == sorted(per_iter + ["its", "sigma", "tau", "normK2", "objectiveFinal", "tv"])
    assert info["tv"] == "iso3" and info["its"] == 12 and all(len(info[k]) == 12 for k in per_iter)
    assert x.shape == (P.shape[1], 1) and np.array_equal(x, info["xHistory"][-1])
    for k in range(12):
        assert _close(info["xHistory"][k], ref["X"][k])
    Sr = ref["S"][:12]
    bn = np.linalg.norm(P.b.astype(np.float32).astype(np.float64))
    assert np.allclose(info["Rnrm"], np.sqrt(Sr[:, 0]) / bn, rtol=1e-5)
    assert np.allclose(info["objective"], 0.5 * Sr[:, 0] + P.lam * Sr[:, 1], rtol=1e-5)
    assert np.allclose(info["dualChange"], np.sqrt(Sr[:, 2] + Sr[:, 3]), rtol=1e-4)
    xs = [h.reshape(-1) for h in info["xHistory"]]
    assert info["active"] == [int(np.count_nonzero((h == P.lo) | (h == np.float32(P.hi)))) for h in xs]
    # the objective carries the three-member norms: recomputed in float64 at the returned x, and not 'iso''s value
    pairs = (C.pair(P.oracle()), C.pair(P.oracle_L()))
    want = T.objective_iso3(*pairs, P.b.astype(np.float32), P.lam, x, geo)
    assert abs(info["objectiveFinal"] / want - 1) < 1e-6
    assert abs(I.objective_iso(*pairs, P.b.astype(np.float32), P.lam, x, geo) / want - 1) > 1e-3
    # 'iso' on the same call is another solve
    xi, ii = _solve(eng, name, 12, tv="iso", tv_dims=geo)
    assert ii["tv"] == "iso" and np.linalg.norm(x - xi) > 1e-4 * np.linalg.norm(xi)


def test_geometry_of_the_first_difference_classes():
    """FirstDerivative2D carries (N, 1), SpaceTimeDerivative (N, nt); tv_dims overrides and is checked against the shape, which for
    'iso3' has no room for further rows.  (Built without handles: the constructors need the HIP library.)"""
    from trips_py_amd.operators import FirstDerivative2D, SpaceTimeDerivative
    from trips_py_amd.solvers.PDHG import _iso_geometry
    L2 = FirstDerivative2D.__new__(FirstDerivative2D)
    L2.N, L2.shape = 5, (40, 25)
    Ls = SpaceTimeDerivative.__new__(SpaceTimeDerivative)
    Ls.N, Ls.nt_global, Ls.shape = 4, 3, (3 * 24 + 2 * 16, 48)
    assert _iso_geometry(L2, "iso3", None) == (5, 1) and _iso_geometry(Ls, "iso3", None) == (4, 3)
    assert _iso_geometry(Ls, "iso3", (4, 3)) == (4, 3)
    for L, dims in ((L2, (4, 1)), (Ls, (4, 4)), (Ls, (4, 2)), (Ls, (4, 1)), (L2, (5, 2))):
        with pytest.raises(ValueError):
            _iso_geometry(L, "iso3", dims)


def test_argument_errors(eng):
    import scipy.sparse as sp
    from oracle import cpu_ref as O
    P, A, L = _ops(eng, "Q5")
    n = P.shape[1]
    ok = dict(sigma=P.sigma, tau=P.tau)
    Lm = O.spacetime_derivative(16, 16, 3)
    surplus = OracleOp(O.MatrixOp(sp.vstack((Lm, Lm[:5])).tocsr()), eng)
    for Lop, bad in ((Identity(n, eng), dict(tv="iso3")),                      # no geometry on this operator
                     (OracleOp(O.MatrixOp(Lm), eng), dict(tv="iso3")),         # a CSR matrix without tv_dims
                     (surplus, dict(tv="iso3", tv_dims=(16, 3))),              # a surplus tail of 5 rows
                     (L, dict(tv="iso3", tv_dims=(15, 3))),                    # a wrong N
                     (L, dict(tv="iso3", tv_dims=(16, 2))),                    # wrong frames
                     (L, dict(tv="iso3", tv_dims=(16, 4))),
                     (L, dict(tv="iso3", tv_dims=(1, 768))),
                     (L, dict(tv="iso3", tv_dims=(16, 0))),
                     (L, dict(tv="iso3", tv_dims=16)),
                     (L, dict(tv="iso2")),
                     (L, dict(tv="aniso", tv_dims=(16, 3))),
                     (L, dict(tv="iso3", tv_dims=(16, 3), fused=True))):       # no fused form on this engine
        with pytest.raises(ValueError):
            S.PDHG(A, P.b, Lop, P.lam, 3, **ok, **bad)
    # the operator with the surplus rows is a fine 'iso' problem: only 'iso3' refuses the tail
    _x, info = S.PDHG(A, P.b, surplus, P.lam, 2, tv="iso", tv_dims=(16, 3), **ok)
    assert info["tv"] == "iso"
