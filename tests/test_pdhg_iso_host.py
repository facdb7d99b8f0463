"""PDHG with isotropic TV without a GPU: the NumPy restatement of tests/pdhg_iso_cases.py checked against the optimality conditions
of the program it solves and against what fp32 storage costs, and PDHG(tv='iso')'s host logic (the geometry of the groups, info,
argument errors) driven through the CPU test engine."""
import numpy as np
import pytest

import pdhg_cases as C
import pdhg_iso_cases as I
from cpu_engine import OracleOp
from pdhg_iso_cpu_engine import PdhgIsoCpuEngine
from trips_py_amd import solvers as S
from trips_py_amd.operators import Identity


@pytest.fixture(scope="module")
def eng():
    return PdhgIsoCpuEngine()


# ------------------------------------------------------------------ (0) the groups partition the rows
@pytest.mark.parametrize("N,frames,tail", [(2, 1, 0), (5, 2, 25), (16, 3, 512)])
def test_groups_partition_the_rows(N, frames, tail):
    rows = frames * 2 * N * (N - 1) + tail
    ph, pv, sg = I.groups(N, frames, rows)
    assert ph.size == pv.size == frames * (N - 1) ** 2 and sg.size == frames * 2 * (N - 1) + tail
    assert np.array_equal(np.sort(np.concatenate((ph, pv, sg))), np.arange(rows))
    # a pair is the two differences that start at one pixel: the dense operator's rows have their +1 in the same column
    if N == 5:
        from oracle import cpu_ref as O
        Lm = np.asarray(O.FirstDerivative2D(N).todense())
        k = (N - 1) ** 2
        assert np.array_equal(np.argmax(Lm[ph[:k]], axis=1), np.argmax(Lm[pv[:k]], axis=1))
        assert np.all(Lm[ph[:k]].max(axis=1) == 1.0)


# ------------------------------------------------------------------ (1) the restatement solves the program
def test_fixed_point_satisfies_the_kkt_conditions():
    """The 6 x 6 problem of test_pdhg_host.py (3 x 3 Gaussian blur, lam = 0.02, box [0, 0.9], step 0.95 / ||K||) with the isotropic
    term: where the float64 iteration stops moving (relative step <= 1e-14) the point satisfies the optimality conditions of
    min 1/2 ||A x - b||^2 + lam sum_g ||(L x)_g||_2 over the box, stated without reference to the iteration: q in the subdifferential
    of the group norms at L x (every group inside the ball; on the sphere, along u_g, where u_g != 0), p = A x - b, and
    A^T p + L^T q zero on the free entries, >= 0 at the lower and <= 0 at the upper bound.  (Reached in 935 iterations with residuals
    <= 5.4e-14; 9 entries at the lower bound, 6 at the upper, 21 free; 21 of 25 pairs and 3 singles non-zero.)"""
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
    run = I.pdhg_iso_f64((lambda v: M @ v, lambda v: M.T @ v), C.pair(Lo), b, lam, step, step, lo, hi, None, 200000, (6, 1),
                         stop_step=1e-14)
    assert len(run["X"]) < 200000, "the iteration did not stop moving: raise the budget"
    x, p, q = run["X"][-1], run["p"], run["q"]
    at_lo, at_hi = x == lo, x == hi
    assert at_lo.sum() >= 1 and at_hi.sum() >= 1 and (~at_lo & ~at_hi).sum() >= 1
    assert np.all((x >= lo) & (x <= hi))
    tol = 1e-10 * max(np.linalg.norm(b), 1.0)
    assert np.abs(p - (M @ x - b)).max() <= tol
    assert I.group_norms(6, 1, q).max() <= lam + tol
    u = Lm @ x
    ph, pv, sg = I.groups(6, 1, u.size)
    un = I.group_norms(6, 1, u)
    big_p, big_s = un[:ph.size] > 1e-8, un[ph.size:] > 1e-8
    assert np.count_nonzero(big_p & (u[ph] != 0) & (u[pv] != 0)) >= 1 and big_s.sum() >= 1
    for idx in (ph, pv):
        assert np.abs(q[idx][big_p] - lam * u[idx][big_p] / un[:ph.size][big_p]).max() <= tol
    assert np.abs(q[sg][big_s] - lam * np.sign(u[sg][big_s])).max() <= tol
    g = M.T @ p + Lm.T @ q
    assert np.abs(g[~at_lo & ~at_hi]).max() <= tol
    assert g[at_lo].min() >= -tol and g[at_hi].max() <= tol


# ------------------------------------------------------------------ (2) what fp32 storage costs
@pytest.fixture(scope="module")
def runs():
    """name -> (float64 run, storage-faithful run), 30 iterations each on the oracle's operators, computed once."""
    return {name: (I.f64(name, 30, x_true=C.problem(name).x_true),
                   I.f32(name, 30, x_true=C.problem(name).x_true, tv_N=C.problem(name).tv_N)) for name in I.NAMES}


def _figures(P, f64, f32):
    obj = [0.5 * r["S"][:, 0] + P.lam * r["S"][:, 1] for r in (f32, f64)]
    return (C.worst_distance(f32, f64), float(np.max(np.abs(np.sqrt(f32["S"][:, 0] / f64["S"][:, 0]) - 1))),
            float(np.max(np.abs(obj[0] / obj[1] - 1))))


@pytest.mark.parametrize("name", I.NAMES)
def test_fp32_storage_cost_is_the_recorded_one(runs, name):
    """The constants the GPU test's bars are built from (tests/test_gpu_pdhg_iso.py) are these figures, up to the host's BLAS."""
    import test_gpu_pdhg_iso as G
    got = _figures(C.problem(name), *runs[name])
    print(name, "iterates %.3e Rnrm %.3e objective %.3e" % got)
    for fig, table in zip(got, (G.CPU_F32_ITERATES, G.CPU_F32_RNRM, G.CPU_F32_OBJECTIVE)):
        assert 0.5 * table[name] <= fig <= 2.0 * table[name], (name, got)
        assert fig < 5e-7, (name, got)


# ------------------------------------------------------------------ (3) the iterates
@pytest.mark.parametrize("name", I.NAMES)
def test_iterates_stay_in_the_box_the_objective_falls_and_it_is_not_the_anisotropic_solve(runs, name):
    P = C.problem(name)
    for run in runs[name]:
        assert all(float(x.min()) >= P.lo and float(x.max()) <= P.hi for x in run["X"])
        obj = 0.5 * run["S"][:, 0] + P.lam * run["S"][:, 1]
        assert obj[29] < obj[9] < obj[0]
    # slot 1 is the sum of the group norms: never above the l1 norm of the same vector, which the anisotropic run reports
    aniso = P.f64(30)
    assert runs[name][0]["S"][0, 1] <= aniso["S"][0, 1] and runs[name][0]["S"][0, 0] == aniso["S"][0, 0]
    xi, xa = runs[name][0]["X"][-1], aniso["X"][-1]
    dist = np.linalg.norm(xi - xa) / np.linalg.norm(xa)
    print(name, "isotropic against anisotropic after 30 iterations: %.3e" % dist)
    assert dist > 1e-3


# ------------------------------------------------------------------ (4) PDHG(tv='iso') on the CPU engine
def _ops(eng, name):
    P = C.problem(name)
    return P, OracleOp(P.oracle(), eng), OracleOp(P.oracle_L(), eng)


def _solve(eng, name, max_iter, **kw):
    P, A, L = _ops(eng, name)
    kw.setdefault("x_true", P.x_true)
    return S.PDHG(A, P.b.reshape(-1, 1), L, P.lam, max_iter, 0, lower=P.lo, upper=P.hi, sigma=P.sigma, tau=P.tau, **kw)


def _close(x, ref):
    ref = ref.astype(np.float64).reshape(-1)
    return np.linalg.norm(np.asarray(x).reshape(-1) - ref) <= 1e-6 * np.linalg.norm(ref)


@pytest.mark.parametrize("name", ["Q1", "Q5"])
def test_info_and_iterates(eng, name):
    """An operator that is neither first-difference class takes its geometry from tv_dims; Q5's carries a tail of temporal rows."""
    P, geo = C.problem(name), I.GEOMETRY[name]
    ref = I.f32(name, 12, x_true=P.x_true)                     # the unfused forms: what the CPU engine has
    x, info = _solve(eng, name, 12, tv="iso", tv_dims=geo)
    per_iter = ["Rnrm", "active", "dualChange", "objective", "relError", "relResidual", "xHistory"]
    assert sorted(info) == sorted(per_iter + ["its", "sigma", "tau", "normK2", "objectiveFinal", "tv"])
    assert info["tv"] == "iso" and info["its"] == 12 and all(len(info[k]) == 12 for k in per_iter)
    assert x.shape == (P.shape[1], 1) and np.array_equal(x, info["xHistory"][-1])
    for k in range(12):
        assert _close(info["xHistory"][k], ref["X"][k])
    Sr = ref["S"][:12]
    bn = np.linalg.norm(P.b.astype(np.float32).astype(np.float64))
    assert np.allclose(info["Rnrm"], np.sqrt(Sr[:, 0]) / bn, rtol=1e-5)
    assert np.allclose(info["objective"], 0.5 * Sr[:, 0] + P.lam * Sr[:, 1], rtol=1e-5)
    assert np.allclose(info["dualChange"], np.sqrt(Sr[:, 2] + Sr[:, 3]), rtol=1e-4)
    assert np.allclose(info["relResidual"], np.sqrt(Sr[:, 5] / Sr[:, 4]), rtol=1e-4)
    xs = [h.reshape(-1) for h in info["xHistory"]]
    assert info["active"] == [int(np.count_nonzero((h == P.lo) | (h == P.hi))) for h in xs]
    # the objective carries the group norms: recomputed in float64 at the returned x, and not the l1 value
    want = I.objective_iso(C.pair(P.oracle()), C.pair(P.oracle_L()), P.b.astype(np.float32), P.lam, x, geo)
    assert abs(info["objectiveFinal"] / want - 1) < 1e-6
    assert abs(C.objective(C.pair(P.oracle()), C.pair(P.oracle_L()), P.b.astype(np.float32), P.lam, x) / want - 1) > 1e-3
    # the anisotropic solve of the same call is another solve
    xa, _ia = _solve(eng, name, 12)
    assert np.linalg.norm(x - xa) > 1e-3 * np.linalg.norm(xa)


def test_aniso_is_the_call_without_the_argument(eng):
    x0, i0 = _solve(eng, "Q1", 8)
    x1, i1 = _solve(eng, "Q1", 8, tv="aniso")
    assert np.array_equal(x0, x1) and sorted(i0) == sorted(i1) and "tv" not in i0
    for key in ("objective", "Rnrm", "dualChange", "relResidual", "active", "relError", "objectiveFinal"):
        assert i0[key] == i1[key], key
    ref = C.problem("Q1").f32(8)
    assert _close(x0, ref["X"][7])


def test_geometry_of_the_first_difference_classes():
    """FirstDerivative2D carries (N, 1), SpaceTimeDerivative (N, nt); tv_dims overrides and is checked against the shape.  (Built
    without handles: the constructors need the HIP library.)"""
    from trips_py_amd.operators import FirstDerivative2D, SpaceTimeDerivative
    from trips_py_amd.solvers.PDHG import _iso_geometry
    L2 = FirstDerivative2D.__new__(FirstDerivative2D)
    L2.N, L2.shape = 5, (40, 25)
    Ls = SpaceTimeDerivative.__new__(SpaceTimeDerivative)
    Ls.N, Ls.nt_global, Ls.shape = 4, 3, (3 * 24 + 2 * 16, 48)
    assert _iso_geometry(L2, "iso", None) == (5, 1) and _iso_geometry(Ls, "iso", None) == (4, 3)
    assert _iso_geometry(L2, "aniso", None) is None
    assert _iso_geometry(Ls, "iso", (4, 3)) == (4, 3)
    with pytest.raises(ValueError):
        _iso_geometry(L2, "iso", (4, 1))
    with pytest.raises(ValueError):
        _iso_geometry(Ls, "iso", (4, 4))


def test_argument_errors(eng):
    P, A, L = _ops(eng, "Q1")
    n = P.shape[1]
    ok = dict(sigma=P.sigma, tau=P.tau)
    for Lop, bad in ((L, dict(tv="iso")),                                     # no geometry on this operator
                     (Identity(n, eng), dict(tv="iso")),
                     (L, dict(tv="iso", tv_dims=(33, 1))),                    # rows < frames 2 N (N - 1), cols != frames N^2
                     (L, dict(tv="iso", tv_dims=(31, 1))),                  # rows suffice, cols != N^2
                     (L, dict(tv="iso", tv_dims=(1, 1024))),                  # N < 2
                     (L, dict(tv="iso", tv_dims=(32, 0))),
                     (L, dict(tv="iso", tv_dims=32)),
                     (L, dict(tv="isotropic")), (L, dict(tv=None)),
                     (L, dict(tv="aniso", tv_dims=(32, 1))),
                     (L, dict(tv="iso", tv_dims=(32, 1), fused=True))):       # no fused form on this engine
        with pytest.raises(ValueError):
            S.PDHG(A, P.b, Lop, P.lam, 3, **ok, **bad)
    # rows < frames 2 N (N - 1) with the columns right: a 2-D operator one row short
    from oracle import cpu_ref as O
    short = OracleOp(O.MatrixOp(O.first_derivative_2d(32, 32)[:-1]), eng)
    with pytest.raises(ValueError):
        S.PDHG(A, P.b, short, P.lam, 3, tv="iso", tv_dims=(32, 1), **ok)
