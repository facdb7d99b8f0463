"""Which route a Hybrid_GMRES / Hybrid_LSQR call takes: the two `_plan` functions against a table.  The expected plans were worked out by
hand from the boolean expressions the solvers had before the plan functions existed (c_ok, c_fixed, on_dev, async_gcv, dp_async, c_dp;
recur, fuse_update, host_y, searcher, one_call) and are literals: nothing here is computed by the code under test.  No GPU."""
import sys

import numpy as np
import pytest

from conftest import load_golden, relerr
from cpu_engine import CpuEngine, OracleOp
from oracle import cpu_ref as O
from test_oracle_golden import lam_close
from trips_py_amd import solvers as S

# (the package exports the two functions under the names of their modules)
HG, HL = sys.modules["trips_py_amd.solvers.Hybrid_GMRES"], sys.modules["trips_py_amd.solvers.Hybrid_LSQR"]

# one rank, a plain library handle, every kernel and entry point, LAPACK capsules, no x_true without the fused error: the MI355X engine
G_CAPABLE = dict(world=1, handle=True, one_call=True, device_solve=True, err_ok=True, lapack=True, gram_max_k=139)
DP = {"delta": 0.1}

GMRES_ROWS = [
    # regparam, n_iter, kwargs, capabilities that differ      -> route, selector, worker, from_k, bidiag
    (1e-2, 20, {}, {},                                         ("library", "number", True, 2, False)),
    (1e-2, 20, {"c_loop": False}, {},                          ("device", "number", False, None, False)),
    (1e-2, 20, {"device_solve": False}, {},                    ("host", "number", False, None, False)),
    (1e-2, 20, {"c_loop": False}, {"device_solve": False},     ("host", "number", False, None, False)),
    (1e-2, 1, {}, {},                                          ("device", "number", False, None, False)),   # the one-call loop wants n_iter >= 2
    (1e-2, 0, {}, {},                                          ("host", "number", False, None, False)),     # (and raises: no iterate)
    (0.0, 139, {}, {},                                         ("host", "number", False, None, False)),     # GRAM_TIKHONOV_MAX_K
    (0.0, 138, {}, {},                                         ("library", "number", True, 2, False)),
    (0.0, 138, {"c_loop": False}, {},                          ("device", "number", False, None, False)),
    ("gcv", 12, {}, {},                                        ("host", "gcv", False, None, True)),         # BIDIAG_FROM_K: n_iter > 12
    ("gcv", 13, {}, {},                                        ("library", "gcv", True, 12, True)),
    ("gcv", 20, {"c_loop": False}, {},                         ("host", "gcv", True, 12, True)),
    ("gcv", 20, {"async_search": False}, {},                   ("host", "gcv", False, None, True)),
    ("gcv", 20, {"gcv_by_bidiag": False}, {},                  ("host", "gcv", False, None, False)),
    ("dp", 20, DP, {},                                         ("library", "dp", True, 12, True)),
    ("dp", 12, DP, {},                                         ("host", "dp", False, None, True)),
    ("dp", 20, {**DP, "c_loop": False}, {},                    ("host", "dp", True, 12, True)),
    ("dp", 20, {**DP, "explicitProj": True}, {},               ("host", "dp", False, None, False)),
    ("dp", 20, {**DP, "dp_by_bidiag": False}, {},              ("host", "dp", False, None, False)),
    ("dp", 20, {**DP, "async_search": False}, {},              ("host", "dp", False, None, True)),
    ("l_curve", 20, {}, {},                                    ("host", "l_curve", False, None, False)),
    # no library route on two ranks, without an operator handle, with x_true but no fused error, without LAPACK capsules
    (1e-2, 20, {}, {"world": 2},                               ("device", "number", False, None, False)),
    (1e-2, 20, {}, {"handle": False},                          ("device", "number", False, None, False)),
    (1e-2, 20, {}, {"err_ok": False},                          ("device", "number", False, None, False)),
    (1e-2, 20, {}, {"lapack": False},                          ("device", "number", False, None, False)),
    (1e-2, 20, {}, {"one_call": False},                        ("device", "number", False, None, False)),
    ("gcv", 20, {}, {"world": 2},                              ("host", "gcv", True, 12, True)),
    ("gcv", 20, {}, {"handle": False},                         ("host", "gcv", True, 12, True)),
    ("gcv", 20, {}, {"err_ok": False},                         ("host", "gcv", True, 12, True)),
    ("gcv", 20, {}, {"lapack": False},                         ("host", "gcv", False, None, False)),
    ("dp", 20, DP, {"world": 2},                               ("host", "dp", True, 12, True)),
    ("dp", 20, DP, {"handle": False},                          ("host", "dp", True, 12, True)),
    ("dp", 20, DP, {"err_ok": False},                          ("host", "dp", True, 12, True)),
    ("dp", 20, DP, {"lapack": False},                          ("host", "dp", False, None, False)),
]


@pytest.mark.parametrize("regparam,n_iter,kwargs,caps,expected", GMRES_ROWS)
def test_hybrid_gmres_plan(regparam, n_iter, kwargs, caps, expected):
    assert HG.BIDIAG_FROM_K == HG.WORKER_FROM_K == 12
    plan = HG._plan(regparam, n_iter, kwargs, HG.Caps(**{**G_CAPABLE, **caps}))
    assert tuple(plan) == expected and plan._fields == ("route", "selector", "worker", "from_k", "bidiag")


L_CAPABLE = dict(damped_update=True, step_update=True, hosty=True, err_ok=True, lib=True, select=True)

LSQR_ROWS = [
    # regparam, n_iter, kwargs, keep, have_xt, capabilities that differ  -> recur, fuse_update, host_y, worker, one_call
    (1e-2, 20, {}, True, True, {},                                 (True, True, False, False, False)),
    (0.0, 20, {}, True, False, {},                                 (True, True, False, False, False)),
    (1e-2, 20, {"x_by_recurrence": False}, True, True, {},         (False, False, False, False, False)),
    (1e-2, 20, {"update_on_the_step": False}, True, True, {},      (True, False, False, False, False)),
    (1e-2, 20, {}, False, False, {},                               (False, False, False, False, False)),    # history=False, no x_true
    (1e-2, 20, {}, False, True, {},                                (True, True, False, False, False)),
    (1e-2, 1, {}, True, True, {},                                  (False, False, False, False, False)),
    (-1.0, 20, {}, True, True, {},                                 (False, False, False, False, False)),
    (1e-2, 20, {}, True, True, {"step_update": False},             (True, False, False, False, False)),     # an operator without the rider
    (1e-2, 20, {}, True, True, {"damped_update": False},           (False, False, False, False, False)),
    ("gcv", 20, {}, True, True, {},                                (False, False, True, True, True)),
    ("dp", 20, DP, True, True, {},                                 (False, False, True, True, True)),
    ("gcv", 20, {"one_call": False}, True, True, {},               (False, False, True, True, False)),
    ("dp", 20, {**DP, "one_call": False}, True, True, {},          (False, False, True, True, False)),
    ("gcv", 20, {"async_search": False}, True, True, {},           (False, False, True, False, False)),
    ("dp", 20, {**DP, "async_search": False}, True, True, {},      (False, False, True, False, False)),
    ("gcv", 2, {}, True, True, {},                                 (False, False, True, False, False)),     # the worker wants n_iter > 2
    ("gcv", 3, {}, True, True, {},                                 (False, False, True, True, True)),
    ("gcv", 20, {"host_projected_solve": False}, True, True, {},   (False, False, False, True, False)),
    ("gcv", 20, {}, True, True, {"err_ok": False},                 (False, False, False, True, False)),
    ("gcv", 20, {}, True, True, {"select": False},                 (False, False, True, True, False)),
    ("gcv", 20, {}, True, True, {"lib": False, "select": False},   (False, False, True, False, False)),
    # l_curve: always searched in this thread; the projected solve on the host where the engine can take y in a launch's arguments
    ("l_curve", 20, {}, True, True, {},                            (False, False, True, False, False)),
    ("l_curve", 20, {}, True, True, {"hosty": False},              (False, False, False, False, False)),
    ("l_curve", 20, {"host_projected_solve": False}, True, True, {}, (False, False, False, False, False)),
]


@pytest.mark.parametrize("regparam,n_iter,kwargs,keep,have_xt,caps,expected", LSQR_ROWS)
def test_hybrid_lsqr_plan(regparam, n_iter, kwargs, keep, have_xt, caps, expected):
    plan = HL._plan(regparam, n_iter, kwargs, keep, have_xt, HL.Caps(**{**L_CAPABLE, **caps}))
    assert tuple(plan) == expected and plan._fields == ("recur", "fuse_update", "host_y", "worker", "one_call")


@pytest.fixture(scope="module")
def eng():
    return CpuEngine()


@pytest.mark.parametrize("solver", ["Hybrid_LSQR", "Hybrid_GMRES"])
def test_dp_without_delta_raises_before_any_route_is_chosen(eng, solver, monkeypatch):
    g = load_golden("hybrid_lsqr_blur32_dp")
    N = int(g["N"])
    planned = []
    mod = sys.modules[f"trips_py_amd.solvers.{solver}"]
    monkeypatch.setattr(mod, "_plan", lambda *a, **k: planned.append(a) or pytest.fail("a route was planned"))
    with pytest.raises(Exception, match="A value for the noise level delta was not provided and the discrepancy principle cannot be applied"):
        getattr(S, solver)(OracleOp(O.Blur2D(g["psf"], N, N), eng), g["b"], 5, "dp")
    assert planned == []


def test_hybrid_lsqr_l_curve_without_host_y_still_works(eng, monkeypatch):
    """The test engine has no trk_gemv_n_hosty: the plan says inline searches and the projected solve on the device (the table's row
    with hosty off), and the solve agrees with the reference's run at the bars of test_host_solvers.test_hybrid."""
    g = load_golden("hybrid_lsqr_blur32_lcurve")
    N = int(g["N"])
    seen = []
    plan = HL._plan
    monkeypatch.setattr(HL, "_plan", lambda *a: seen.append(plan(*a)) or seen[-1])
    x, info = S.Hybrid_LSQR(OracleOp(O.Blur2D(g["psf"], N, N), eng), g["b"], int(g["n_iter"]), "l_curve", g["x_true"])
    assert [tuple(p) for p in seen] == [(False, False, False, False, False)]
    assert info["its"] == int(g["its"]) and len(info["xHistory"]) == int(g["n_hist"]) and info["relResidual"] == []
    assert lam_close(info["regParam_history"], g["regParam_history"], 2e-3)
    assert np.allclose(info["relError"], g["relError"], rtol=2e-4)
    assert relerr(x, g["x"]) < 1e-4
