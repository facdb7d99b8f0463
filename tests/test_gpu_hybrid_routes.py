"""A default Hybrid_GMRES / Hybrid_LSQR call takes the route its plan names (tests/test_hybrid_routes.py has the plans): the planned
route's entry point is called, the other routes' entry points are not, and the result equals the same call with that route switched off
at the tolerances tests/test_gpu_solvers.py has for that pair of routes.  The smallest sizes at which every route engages: Hybrid_GMRES
posts to the workers from k = 12 of n_iter = 14 > 12, Hybrid_LSQR's worker wants n_iter > 2."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N = 32
COUNTED = ("trk_hgmres_iter", "hess_tikhonov", "post_hess_gcv", "post_hess_dp", "trk_hlsqr_select", "gk_step_lsqr", "bidiag_tikhonov")


def _count_entry_points(monkeypatch, eng):
    """Call counters on the entry points of the routes."""
    from trips_py_amd.solvers._worker import _Searcher
    calls = dict.fromkeys(COUNTED, 0)

    def counted(name, fn):
        def g(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return g
    for name in COUNTED:
        owner = eng.lib if name.startswith("trk_") else _Searcher if name.startswith("post_") else eng
        monkeypatch.setattr(owner, name, counted(name, getattr(owner, name)))
    return calls


def _problem(A, seed):
    dev = A.engine.device
    g = torch.Generator(device=dev).manual_seed(seed)
    xt = torch.rand(A.shape[1], device=dev, generator=g)
    b = A.apply(xt)
    e = torch.randn(b.numel(), device=dev, generator=g)
    delta = 0.01 * float(b.norm())                       # 1 % noise
    return xt, b + e * (delta / e.norm()), delta


def _close(a, c, tol):
    return float(torch.linalg.norm(a.reshape(-1) - c.reshape(-1)) / torch.linalg.norm(c.reshape(-1))) < tol


@pytest.mark.parametrize("reg", [1e-2, "gcv", "dp"])
def test_hybrid_gmres_default_call_takes_the_library_route(reg, monkeypatch):
    from trips_py_amd.operators import Blur2D
    from trips_py_amd.problems import gauss_psf
    from trips_py_amd.solvers import Hybrid_GMRES
    A, its = Blur2D(gauss_psf((9, 9), (2, 2))[0], N, N), 14
    xt, b, delta = _problem(A, 11)
    kw = {"delta": delta} if reg == "dp" else {}
    calls = _count_entry_points(monkeypatch, A.engine)
    x1, i1 = Hybrid_GMRES(A, b, its, reg, xt, **kw)
    # one call per Arnoldi step and one per iterate still posted at the end (the two workers' jobs), nothing from the other routes
    assert its <= calls["trk_hgmres_iter"] <= its + 2, calls
    assert calls["hess_tikhonov"] == calls["post_hess_gcv"] == calls["post_hess_dp"] == 0, calls
    before = dict(calls)
    x0, i0 = Hybrid_GMRES(A, b, its, reg, xt, c_loop=False, **kw)
    assert calls["trk_hgmres_iter"] == before["trk_hgmres_iter"]
    # c_loop=False: a number stays on the device, gcv / dp post iterates k = 12, 13, 14 from the interpreter's loop
    assert (calls["hess_tikhonov"], calls["post_hess_gcv"], calls["post_hess_dp"]) == {1e-2: (its, 0, 0), "gcv": (0, 3, 0), "dp": (0, 0, 3)}[reg]
    assert len(i1["regParam_history"]) == len(i0["regParam_history"]) == its and i1["its"] == i0["its"]
    # the bars of test_hybrid_gmres_device_projected_solve_equals_the_host_one, ..._gcv_one_library_call_per_iteration_equals_the_python_loop
    # and ..._discrepancy_principle_one_library_call_per_iteration
    if reg == 1e-2:
        assert i1["regParam_history"] == i0["regParam_history"]
    else:
        assert np.allclose(i1["regParam_history"], i0["regParam_history"], rtol={"gcv": 1e-10, "dp": 1e-8}[reg], atol=1e-300 if reg == "dp" else 0)
    x_tol, err_tol, res_tol = {1e-2: (1e-5, 1e-5, 1e-6), "gcv": (1e-6, 1e-6, 1e-10), "dp": (1e-6, 1e-6, 1e-7)}[reg]
    assert np.allclose(i1["relResidual"], i0["relResidual"], rtol=res_tol)
    assert np.allclose(i1["relError"], i0["relError"], rtol=err_tol)
    assert _close(x1, x0, x_tol)
    for k in (0, 11, its - 1):
        assert _close(i1["xHistory"][k], i0["xHistory"][k], x_tol), k


@pytest.mark.parametrize("reg", [1e-2, "gcv", "dp"])
def test_hybrid_lsqr_default_call_takes_the_planned_route(reg, monkeypatch):
    from trips_py_amd.operators import Radon2DParallel
    from trips_py_amd.solvers import Hybrid_LSQR
    A, its = Radon2DParallel(N, np.linspace(0, np.pi, 12, endpoint=False)), 6
    xt, b, delta = _problem(A, 12)
    kw = {"delta": delta} if reg == "dp" else {}
    calls = _count_entry_points(monkeypatch, A.engine)
    x1, i1 = Hybrid_LSQR(A, b, its, reg, xt, **kw)
    if reg == 1e-2:
        # the recurrence, each update on the next Golub-Kahan step (steps 2 .. its carry the updates of x_1 .. x_{its-1}); against the
        # combination x = V y (x_by_recurrence=False), bars of test_hybrid_lsqr_recurrence_equals_the_combination
        assert calls["gk_step_lsqr"] == its - 1 and calls["bidiag_tikhonov"] == calls["trk_hlsqr_select"] == 0, calls
        x0, i0 = Hybrid_LSQR(A, b, its, reg, xt, x_by_recurrence=False)
        assert calls["gk_step_lsqr"] == its - 1 and calls["bidiag_tikhonov"] == its - 1 and calls["trk_hlsqr_select"] == 0, calls
        assert i1["regParam_history"] == i0["regParam_history"] and len(i1["xHistory"]) == len(i0["xHistory"]) == its - 1
        assert _close(x1, x0, 1e-5) and np.allclose(i1["relError"], i0["relError"], rtol=1e-5)
        for k in (0, its // 2, its - 2):
            assert _close(i1["xHistory"][k], i0["xHistory"][k], 1e-5), k
    else:
        # the host's turn in one library call, for the iterates of steps 2 .. its; against the four calls of the interpreter's loop
        # (one_call=False), bars of test_hybrid_lsqr_automatic_lambda_host_turn_in_one_library_call
        assert calls["trk_hlsqr_select"] == its - 1 and calls["bidiag_tikhonov"] == calls["gk_step_lsqr"] == 0, calls
        x0, i0 = Hybrid_LSQR(A, b, its, reg, xt, one_call=False, **kw)
        assert calls["trk_hlsqr_select"] == its - 1 and calls["bidiag_tikhonov"] == calls["gk_step_lsqr"] == 0, calls
        assert i1["regParam_history"] == i0["regParam_history"] and len(i1["regParam_history"]) == its - 1
        assert _close(x1, x0, 1e-6) and np.allclose(i1["relError"], i0["relError"], rtol=1e-6)
        for k in (0, its // 2, its - 2):
            assert _close(i1["xHistory"][k], i0["xHistory"][k], 1e-6), k
    assert calls["trk_hgmres_iter"] == calls["hess_tikhonov"] == 0
