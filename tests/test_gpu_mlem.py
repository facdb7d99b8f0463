"""MLEM / Richardson-Lucy on the GPU (csrc/mlem.hip, solvers/MLEM.py) against the NumPy restatement of tests/mlem_cases.py:
one launch of each kernel on crafted vectors against the storage-faithful form, the one-call C loop against single steps (bit for
bit), and whole solves against the float64 form."""
import numpy as np
import pytest
import torch

import mlem_cases as C
from conftest import bar

pytestmark = pytest.mark.gpu

CAP = 1024                 # blocks of a streaming kernel at most (stream_grid)
PER_BLOCK = 1024           # floats per block before the grid stops growing
F32 = np.float32


@pytest.fixture(scope="module")
def eng():
    from trips_py_amd.engine import default_engine
    return default_engine()


def _grid(n):
    return min((n + PER_BLOCK - 1) // PER_BLOCK, CAP)


def _ulps(a, b):
    """Largest distance in units in the last place between two fp32 arrays (equal values, -0 and 0 included, count 0)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    d = np.abs(ia - ib)
    d[a == b] = 0
    return int(d.max()) if d.size else 0


def _dev(eng, a, offset):
    """A device copy that starts `offset` floats behind a 16-byte boundary."""
    t = torch.empty(a.size + 4, dtype=torch.float32, device=eng.device)
    assert t.data_ptr() % 16 == 0
    w = t[offset:offset + a.size]
    w.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=F32)))
    return w


def _sum_close(got, want, tag):
    if np.isinf(want):
        assert got == want, tag                                # inf must be exactly inf
    else:
        assert abs(got - want) <= 1e-12 * abs(want), (tag, got, want)


# ====================================================================== one launch on crafted vectors
SIZES = [1, 3, 1024, 1027, 66561, 614402, 1300003]
RATIO_SITUATIONS = ["plain", "y_nonpos_under_a_count", "y_zero_b_zero", "y_negative_b_zero"]
UPDATE_SITUATIONS = ["plain", "t_negative", "sinv_zero"]

_base = {}


def _vectors(n):
    """Seeded fp32 vectors, made once per n.  Data side: w in [0.5, 50.5), counts b with exact zeros among them, a background vector
    in [0, 2).  Unknowns: x in [0.5, 1.5), t in [0, 2), sinv in [0.1, 1.1), x_true."""
    if n not in _base:
        rng = np.random.default_rng(11 * n + 5)
        _base[n] = {"w": (0.5 + 50 * rng.random(n)).astype(F32), "b": rng.poisson(3.0, n).astype(F32), "bgv": (2 * rng.random(n)).astype(F32),
                    "x": (0.5 + rng.random(n)).astype(F32), "t": (2 * rng.random(n)).astype(F32), "sinv": (0.1 + rng.random(n)).astype(F32),
                    "xt": rng.random(n).astype(F32)}
        _base[n]["b"][0] = 0.0                                 # an exact zero also where n is 1 or 3 ...
        if n > 1:
            _base[n]["b"][n - 1] = 4.0                         # ... and a count in the tail
    return {k: v.copy() for k, v in _base[n].items()}


BG = 0.75


def _craft_ratio(situation, n, bg_vector):
    """(w, b, bg): the crafted entries sit at the start, the end (the scalar tail) and at the first float4 of the last block."""
    v = _vectors(n)
    w, b = v["w"], v["b"]
    bg = v["bgv"] if bg_vector else BG
    at = sorted({0, n - 1, min(n - 1, (_grid(n) - 1) * PER_BLOCK), n // 2})
    bga = np.broadcast_to(np.asarray(bg, dtype=F32), (n,))
    if situation == "y_nonpos_under_a_count":                  # y == 0 and y < 0 with b > 0: rho = 0, KL = +inf
        for j, i in enumerate(at):
            b[i] = 2.0 + j
            w[i] = -bga[i] if j % 2 == 0 else -bga[i] - F32(1.5)
    elif situation == "y_zero_b_zero":                         # y == 0 with b == 0: rho = 0, the term is 0, KL stays finite
        for i in at:
            b[i], w[i] = 0.0, -bga[i]
    elif situation == "y_negative_b_zero":                     # y < 0 with b == 0: rho = 0, KL = +inf
        for i in at:
            b[i], w[i] = 0.0, -bga[i] - F32(0.5)
    return w, b, bg


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", SIZES)
def test_one_ratio_against_the_restatement(eng, n, offset):
    grid = _grid(n)
    for bg_vector in (False, True):
        for situation in RATIO_SITUATIONS:
            for alias in ((True, False) if situation == "plain" else (True,)):
                tag = (situation, bg_vector, alias)
                w, b, bg = _craft_ratio(situation, n, bg_vector)
                want = C.ratio_f32(w, bg, b)
                dw, db = _dev(eng, w, offset), _dev(eng, b, offset)
                dbg = _dev(eng, bg, offset) if bg_vector else bg
                rho = dw if alias else _dev(eng, np.full(n, 7.0, dtype=F32), offset)
                NP = eng.scalars(8 * CAP)
                nb = eng.mlem_ratio(dbg, dw, db, rho, NP.ref(0), CAP)
                assert nb == grid, tag
                parts = NP.host().reshape(CAP, 8)
                assert not np.any(np.isnan(parts)), tag
                assert not np.any(parts[:, 2:]) and not np.any(parts[nb:]), tag      # its slots of its blocks' rows only
                assert _ulps(rho.cpu().numpy(), want["rho"]) <= 1, tag
                if not alias:
                    assert np.array_equal(dw.cpu().numpy().view(np.int32), w.view(np.int32)), tag
                _sum_close(parts[:, 0].sum(), want["kl"], tag + ("kl",))
                _sum_close(parts[:, 1].sum(), want["rr"], tag + ("rr",))
                if situation in ("y_nonpos_under_a_count", "y_negative_b_zero"):
                    assert want["kl"] == np.inf and np.isfinite(want["rr"]), tag
                    y = w + np.broadcast_to(np.asarray(bg, dtype=F32), (n,))
                    assert np.all(rho.cpu().numpy()[y <= 0] == 0.0), tag
                else:
                    assert np.isfinite(want["kl"]) and want["kl"] >= 0, tag


def _craft_update(situation, n):
    v = _vectors(n)
    at = sorted({0, n - 1, min(n - 1, (_grid(n) - 1) * PER_BLOCK), n // 2})
    if situation == "t_negative":                              # an operator with negative entries: the clamp holds x' at 0
        v["t"][at] = -0.5
        v["t"][::7] = -np.abs(v["t"][::7])
    elif situation == "sinv_zero":                             # an unknown no datum sees
        v["sinv"][at] = 0.0
        v["sinv"][::5] = 0.0
    return v, at


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", SIZES)
def test_one_update_against_the_restatement(eng, n, offset):
    grid = _grid(n)
    for situation in UPDATE_SITUATIONS:
        for with_xt in (True, False):
            for alias in ((True, False) if situation == "plain" else (False,)):
                tag = (situation, with_xt, alias)
                v, at = _craft_update(situation, n)
                want = C.update_f32(v["x"], v["t"], v["sinv"], v["xt"] if with_xt else None)
                d = {k: _dev(eng, v[k], offset) for k in ("x", "t", "sinv", "xt")}
                x_new = d["x"] if alias else _dev(eng, np.full(n, 7.0, dtype=F32), offset)
                NP = eng.scalars(8 * CAP)
                nb = eng.mlem_update(d["x"], d["t"], d["sinv"], d["xt"] if with_xt else None, x_new, NP.ref(0), CAP)
                assert nb == grid, tag
                parts = NP.host().reshape(CAP, 8)
                assert not np.any(np.isnan(parts)), tag
                assert not np.any(parts[:, :4]) and not np.any(parts[nb:]), tag
                got = x_new.cpu().numpy()
                assert _ulps(got, want["x"]) <= 1 and got.min() >= 0.0, tag
                for slot, key in ((4, "xx"), (5, "dd"), (6, "ee")):
                    _sum_close(parts[:, slot].sum(), want[key], tag + (key,))
                assert parts[:, 7].sum() == want["zeros"], tag
                if situation == "plain":
                    assert want["zeros"] == 0
                else:
                    assert want["zeros"] >= len(at) and np.all(got[at] == 0.0), tag
                if not with_xt:
                    assert want["ee"] == 0.0 and not np.any(parts[:, 6])


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
def test_sinv(eng, offset):
    for n in (1, 3, 1027, 66561):
        s = _vectors(n)["t"] - F32(0.25)                       # of either sign
        s[0] = 0.0
        want = C.sinv_f32(s)
        ds = _dev(eng, s, offset)
        out = _dev(eng, np.full(n, 7.0, dtype=F32), offset)
        eng.mlem_sinv(ds, out)
        assert _ulps(out.cpu().numpy(), want) == 0 and out.cpu().numpy()[0] == 0.0
        eng.mlem_sinv(ds, ds)                                  # in place
        assert _ulps(ds.cpu().numpy(), want) == 0


def test_argument_checks_come_first(eng):
    """Bad arguments are refused with trk_last_error's text before anything is launched."""
    v = {k: torch.ones(8, dtype=torch.float32, device=eng.device) for k in ("w", "b", "g", "x", "t", "s", "o")}
    Sc = eng.scalars(8 * CAP)
    with pytest.raises(ValueError, match="NULL"):
        eng.mlem_ratio(0.0, v["w"], None, v["w"], Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="alias w only"):
        eng.mlem_ratio(0.0, v["w"], v["b"], v["b"], Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="alias w only"):
        eng.mlem_ratio(v["g"], v["w"], v["b"], v["g"], Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="too small"):
        eng.mlem_ratio(0.0, v["w"], v["b"], v["w"], Sc.ref(0), 0)
    for bg in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="background"):
            eng.mlem_ratio(bg, v["w"], v["b"], v["w"], Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="m >= 1"):
        eng._pdhg("trk_mlem_ratio", 0, 0.0, None, v["w"], v["b"], v["o"], Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="n >= 1"):
        eng._pdhg("trk_mlem_update", 0, v["x"], v["t"], v["s"], None, v["o"], Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="NULL"):
        eng.mlem_update(v["x"], v["t"], None, None, v["o"], Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="alias x only"):
        eng.mlem_update(v["x"], v["t"], v["s"], None, v["t"], Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="alias x only"):
        eng.mlem_update(v["x"], v["t"], v["s"], v["o"], v["o"], Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="too small"):
        eng.mlem_update(v["x"], v["t"], v["s"], None, v["o"], Sc.ref(0), 0)
    assert eng.lib.trk_mlem_sinv(8, None, v["o"].data_ptr(), eng.stream()) == -1 and b"NULL" in eng.lib.trk_last_error()
    assert eng.lib.trk_mlem_sinv(0, v["s"].data_ptr(), v["o"].data_ptr(), eng.stream()) == -1
    assert not np.any(Sc.host()) and all(float(t.min()) == 1.0 == float(t.max()) for t in v.values())     # nothing ran
    # the loop: its own checks before the first launch
    P = C.problem("P4")
    A = P.device(eng)
    m, n = P.shape
    w, t, b, sinv, x = eng.empty(m), eng.empty(n), eng.to_vec(P.b), eng.to_vec(np.ones(n)), eng.to_vec(P.x0)
    X = eng.empty_basis(2, n)
    with pytest.raises(ValueError, match="too small"):
        eng.mlem_iterate(A._h, 1, 2, 0.0, b, sinv, w, t, X, False, x, None, Sc.ref(0), 0)
    with pytest.raises(ValueError, match="k_first"):
        eng.mlem_iterate(A._h, 0, 2, 0.0, b, sinv, w, t, X, False, x, None, Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="background"):
        eng.mlem_iterate(A._h, 1, 2, -2.0, b, sinv, w, t, X, False, x, None, Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="NULL"):
        eng.mlem_iterate(A._h, 1, 2, 0.0, b, None, w, t, X, False, x, None, Sc.ref(0), CAP)
    assert not np.any(Sc.host())


# ====================================================================== the one-call loop against single steps
K = 12


def _bits(run):
    run.rows()
    vecs = [v.clone() for v in (run.x_cur, run.w, run.t)]
    return vecs, run.S.host().view(np.int64).copy(), run.NP.host().view(np.int64).copy()


@pytest.mark.parametrize("history", [True, False, 3])
@pytest.mark.parametrize("with_xt", [True, False])
@pytest.mark.parametrize("name", C.NAMES)
def test_run_equals_steps(eng, name, with_xt, history):
    from trips_py_amd.solvers import MLEMRun
    P = C.problem(name)
    A = P.device(eng)
    xt = P.x_true if with_xt else None
    bg = np.full(P.shape[0], P.bg) if name == "P3" else P.bg            # one problem through the background vector
    ref = MLEMRun(A, P.b, P.x0, K, xt, history=history, background=bg)
    for _ in range(K):
        ref.step()
    want_vecs, want_S, want_NP = _bits(ref)
    assert np.all(np.isfinite(ref.rows()))
    for calls in ([K], [1, K - 1], [3, 5, K - 8]):
        run = MLEMRun(A, P.b, P.x0, K, xt, history=history, background=bg)
        for c in calls:
            run.run(c)
        assert run.k == K
        vecs, S, NP = _bits(run)
        for key, a, b in zip("xwt", vecs, want_vecs):
            assert torch.equal(a, b), (calls, key)
        assert np.array_equal(S, want_S) and np.array_equal(NP, want_NP), calls
    if history is True:
        assert all(torch.equal(ref.slot(k), run.slot(k)) for k in range(K))


# ====================================================================== whole solves against float64
ITERS = 30
# The worst relative 2-norm distance of the storage-faithful restatement (mlem_cases.mlem_f32) from the float64 restatement over 30
# iterates, measured in NumPy on a CPU for these four problems on the oracle's operators — what fp32 storage alone costs:
CPU_F32_ITERATES = {"P1": 2.05e-7, "P2": 1.02e-7, "P3": 3.51e-7, "P4": 3.31e-7}
# ... and, in the same two runs, the worst relative deviation of KL(b, A x_{k-1} + bg) and of ||A x_{k-1} + bg - b||:
CPU_F32_KL = {"P1": 1.49e-8, "P2": 5.67e-8, "P3": 5.37e-8, "P4": 3.17e-7}
CPU_F32_RNRM = {"P1": 3.57e-8, "P2": 9.41e-8, "P3": 8.80e-8, "P4": 1.53e-7}


def _limit(cpu_figure):
    """8 x the cost of fp32 storage alone, never below 1e-5 (the rule of the MRNSD and PDHG bars)."""
    return max(8 * cpu_figure, 1e-5)


def _float64_operator(P, A):
    """(matvec, rmatvec) in float64: the operator's own dense matrices — the "transpose" is the operator's too — or the oracle's Radon."""
    if P.name == "P3":
        o = P.oracle()
        return o.matvec, o.rmatvec
    M, Mt = A.todense(), A.T.todense()
    assert M.shape == P.shape and Mt.shape == P.shape[::-1]
    return (lambda v: M @ v), (lambda v: Mt @ v)


@pytest.mark.parametrize("name", C.NAMES)
def test_solve_against_float64(eng, name):
    from trips_py_amd.solvers import MLEM
    P = C.problem(name)
    A = P.device(eng)
    matvec, rmatvec = _float64_operator(P, A)
    ref = C.mlem_f64(matvec, rmatvec, P.b, P.x0, ITERS, P.bg)
    faithful = C.mlem_f32(matvec, rmatvec, P.b, P.x0, ITERS, P.bg)
    x, info = MLEM(A, P.b, P.x0, ITERS, 0, x_true=P.x_true, background=P.bg)
    assert info["its"] == ITERS and len(info["xHistory"]) == ITERS
    H = [h.reshape(-1) for h in info["xHistory"]]
    assert all(float(h.min()) >= 0.0 and np.all(np.isfinite(h)) for h in H)
    worst = max(np.linalg.norm(h - xr) / np.linalg.norm(xr) for h, xr in zip(H, ref["X"]))
    bar(f"mlem_{name}_iterates_vs_float64", worst, _limit(CPU_F32_ITERATES[name]))
    bar(f"mlem_{name}_KL_vs_float64", C.worst_scalar(info["KL"], ref["kl"]), _limit(CPU_F32_KL[name]))
    bar(f"mlem_{name}_Rnrm_vs_float64", C.worst_scalar(info["Rnrm"], np.sqrt(ref["rr"]) / np.linalg.norm(P.b)), _limit(CPU_F32_RNRM[name]))
    assert np.allclose(info["relError"], [np.linalg.norm(xr - P.x_true) / np.linalg.norm(P.x_true) for xr in ref["X"]], rtol=1e-4)
    assert np.allclose(info["relResidual"], np.sqrt(np.array(ref["dd"]) / np.array(ref["xx"])), rtol=1e-3)
    # the count of exact zeros: the kernel's is the iterates' own, and the storage-faithful restatement's
    assert info["zeros"] == [int(np.count_nonzero(h == 0)) for h in H]
    assert info["zeros"] == faithful["zeros"]
    # objectiveFinal is KL at the returned x: what iteration 31 would report
    more = C.mlem_f64(matvec, rmatvec, P.b, ref["X"][-1], 1, P.bg)
    bar(f"mlem_{name}_objectiveFinal_vs_float64", abs(info["objectiveFinal"] / more["kl"][0] - 1), _limit(CPU_F32_KL[name]))


def test_flux_is_conserved_without_background(eng):
    """P1 (an exact adjoint) with bg = 0: sum_i s_i x_k,i = sum_j b_j for every iterate, within the bar of the iterates."""
    from trips_py_amd.solvers import MLEM
    P = C.problem("P1")
    A = P.device(eng)
    s = A.T.todense() @ np.ones(P.shape[0])
    _x, info = MLEM(A, P.b, P.x0, ITERS, 0)
    worst = max(abs(np.dot(s, h.reshape(-1)) / P.b.sum() - 1.0) for h in info["xHistory"])
    bar("mlem_P1_flux_bg0", worst, _limit(CPU_F32_ITERATES["P1"]))


def test_tol_delta_and_history_off_on_the_device(eng):
    """tol > 0 and delta read a row back every iteration and stop where the tol = 0 run's rows say; delta returns x_{k-1}."""
    from trips_py_amd.solvers import MLEM, MLEMRun
    P = C.problem("P1")
    A = P.device(eng)
    run = MLEMRun(A, P.b, P.x0, ITERS, background=P.bg)
    run.run(ITERS)
    rows = run.rows()
    rel = np.sqrt(rows[:, 5] / rows[:, 4])
    tol = float(rel[7]) * (1 + 1e-9)
    hit = int(np.nonzero(rel <= tol)[0][0]) + 1
    assert 1 < hit < ITERS
    x, info = MLEM(A, P.b, P.x0, ITERS, tol, history=False, background=P.bg)
    assert info["its"] == hit and info["xHistory"] == []
    assert np.array_equal(x.reshape(-1), run.slot(hit - 1).cpu().numpy().astype(np.float64))
    res = np.sqrt(rows[:, 1])                                    # row k (index k - 1) describes x_{k-1}
    delta = res[9] / 1.01 * (1 + 1e-9)
    k = int(np.nonzero(res[1:] <= 1.01 * delta)[0][0]) + 2       # the first row k >= 2 that meets it
    for history in (True, False):
        x, info = MLEM(A, P.b, P.x0, ITERS, 0, history=history, background=P.bg, delta=delta)
        assert info["its"] == k - 1 and len(info["KL"]) == k - 1
        assert np.array_equal(x.reshape(-1), run.slot(k - 2).cpu().numpy().astype(np.float64))
    assert info["objectiveFinal"] == rows[k - 1, 0]              # KL at x_{k-1}: the same kernel on the same product
