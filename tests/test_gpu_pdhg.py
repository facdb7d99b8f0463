"""PDHG on the GPU (csrc/pdhg.hip, the fused forms in csrc/pdhg_tv.hip, solvers/PDHG.py) against the NumPy restatement of
tests/pdhg_cases.py: one launch of each kernel on crafted vectors against the storage-faithful form, the fused first-difference
kernels against the generic path (bit for bit), the one-call C loop against single steps (bit for bit), and whole solves against the
float64 form."""
import numpy as np
import pytest
import torch

import pdhg_cases as C
from conftest import bar

pytestmark = pytest.mark.gpu

CAP = 4096                 # rows of 8 partials: the fused kernels' grid is capped there, a streaming kernel's at 1024
PER_BLOCK = 1024           # floats per block of a streaming kernel before its grid stops growing


@pytest.fixture(scope="module")
def eng():
    from trips_py_amd.engine import default_engine
    return default_engine()


def _ulps(a, b):
    """Largest distance in units in the last place between two fp32 arrays (equal values, -0 and 0 included, count 0)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    d = np.abs(ia - ib)
    d[a == b] = 0
    return int(d.max()) if d.size else 0


def _dev(eng, a, offset=0):
    """A device copy that starts `offset` floats behind a 16-byte boundary."""
    t = torch.empty(a.size + 4, dtype=torch.float32, device=eng.device)
    assert t.data_ptr() % 16 == 0
    w = t[offset:offset + a.size]
    w.copy_(torch.from_numpy(a))
    return w


def _sums_match(cols, want, tag):
    for j, (val, ref) in enumerate(zip(cols, want)):
        assert abs(val - ref) <= 1e-12 * abs(ref), (tag, j, val, ref)


# ====================================================================== (1) one launch of each streaming kernel
SIZES = [1, 3, 1024, 1027, 66561, 1300003]
# (sigma, lam, tau, lo, hi); 0.5, 1 and 0.25 are exact in fp32, the others round
SITUATIONS = {"random": (0.37, 0.013, 0.21, 0.1, 0.9), "q_at_lam_pushed_outward": (0.5, 1.0, 0.25, 0.0, 2.0),
              "q_lands_on_lam": (0.5, 1.0, 0.25, 0.0, 2.0), "x_at_bound_pushed_outward": (0.37, 0.013, 0.25, 0.0, 2.0),
              "x_at_bound_pushed_inward": (0.37, 0.013, 0.25, 0.0, 2.0), "no_box": (0.37, 0.013, 0.21, -np.inf, np.inf),
              "lower_equals_upper": (0.37, 0.013, 0.21, 0.3, 0.3), "lam_zero": (0.37, 0.0, 0.21, 0.0, np.inf)}

_base, _want = {}, {}


def _vectors(n, m):
    if (n, m) not in _base:
        rng = np.random.default_rng(11 * n + m)
        f = np.float32
        _base[(n, m)] = {"x": rng.random(n).astype(f), "z": (rng.random(n) - 0.5).astype(f), "v": (rng.random(n) - 0.5).astype(f),
                         "xt": rng.random(n).astype(f), "u": rng.standard_normal(n).astype(f),
                         "q": (0.02 * rng.random(n) - 0.01).astype(f), "w": rng.standard_normal(m).astype(f),
                         "b": rng.standard_normal(m).astype(f), "p": rng.standard_normal(m).astype(f)}
    return {k: a.copy() for k, a in _base[(n, m)].items()}


def _craft(situation, n, m):
    v = _vectors(n, m)
    sigma, lam, tau, lo, hi = SITUATIONS[situation]
    half = np.arange(n) % 2 == 0
    if situation == "q_at_lam_pushed_outward":
        v["q"] = np.where(half, 1.0, -1.0).astype(np.float32)
        v["u"] = (np.abs(v["u"]) * np.where(half, 1.0, -1.0)).astype(np.float32)
    elif situation == "q_lands_on_lam":                       # fmaf(0.5, +-1, +-0.5) = +-1 = +-lam exactly
        v["q"] = np.where(half, 0.5, -0.5).astype(np.float32)
        v["u"] = np.where(half, 1.0, -1.0).astype(np.float32)
    elif situation.startswith("x_at_bound"):
        out = 1.0 if situation.endswith("outward") else -1.0
        v["x"] = np.where(half, 0.0, 2.0).astype(np.float32)
        v["z"] = (np.abs(v["z"]) * np.where(half, out, -out)).astype(np.float32)     # g > 0 moves x down
        v["v"] = (np.abs(v["v"]) * np.where(half, out, -out)).astype(np.float32)
    return v, (sigma, lam, tau, lo, hi)


def _expected(situation, with_xt, with_v, n, m):
    key = (situation, with_xt, with_v, n, m)
    if key not in _want:
        v, (sigma, lam, tau, lo, hi) = _craft(situation, n, m)
        _want[key] = (C.dual_p_f32(sigma, v["w"], v["b"], v["p"]), C.dual_q_f32(sigma, lam, v["u"], v["q"]),
                      C.primal_f32(tau, lo, hi, v["x"], v["z"], v["v"] if with_v else None, v["xt"] if with_xt else None))
    return _want[key]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("m_kind", ["m_eq_n", "m_515"])
@pytest.mark.parametrize("n", SIZES)
def test_one_launch_against_the_restatement(eng, n, m_kind, offset):
    m = n if m_kind == "m_eq_n" else 515
    grid = lambda k: min((k + PER_BLOCK - 1) // PER_BLOCK, 1024)   # noqa: E731
    for situation in SITUATIONS:
        for with_xt, with_v in (((True, True), (False, True), (True, False)) if situation == "random" else ((True, True),)):
            tag = (situation, with_xt, with_v)
            v, (sigma, lam, tau, lo, hi) = _craft(situation, n, m)
            (pn, s0, s2), (qn, s1, s3), (xn, xb, tail) = _expected(situation, with_xt, with_v, n, m)
            d = {k: _dev(eng, a, offset) for k, a in v.items()}
            x_new, xbar = _dev(eng, np.zeros(n, dtype=np.float32), offset), _dev(eng, np.zeros(n, dtype=np.float32), offset)
            NP = eng.scalars(8 * CAP)
            assert eng.pdhg_dual_p(sigma, d["w"], d["b"], d["p"], NP.ref(0), CAP) == grid(m), tag
            assert eng.pdhg_dual_q(sigma, lam, d["u"], d["q"], NP.ref(0), CAP) == grid(n), tag
            assert eng.pdhg_primal(tau, lo, hi, d["x"], d["z"], d["v"] if with_v else None, x_new, xbar,
                                   d["xt"] if with_xt else None, NP.ref(0), CAP) == grid(n), tag
            got = {"p": d["p"], "q": d["q"], "x": x_new, "xbar": xbar}
            for key, want in (("p", pn), ("q", qn), ("x", xn), ("xbar", xb)):
                assert _ulps(got[key].cpu().numpy(), want) <= 1, (tag, key)
            lf, lof, hif = np.float32(lam), np.float32(lo), np.float32(hi)
            qh, xh = d["q"].cpu().numpy(), x_new.cpu().numpy()
            assert np.all((qh >= -lf) & (qh <= lf)) and np.all((xh >= lof) & (xh <= hif)), tag
            parts = NP.host().reshape(CAP, 8)
            assert not parts[max(grid(n), grid(m)):].any(), tag       # a kernel writes its blocks' rows only
            cols = parts.sum(axis=0)
            _sums_match(cols[:7], [s0, s1, s2, s3] + tail[:3], tag)
            assert cols[7] == tail[3] == np.count_nonzero((xh == lof) | (xh == hif)), tag
            if situation == "q_at_lam_pushed_outward":
                assert np.array_equal(qh, v["q"]) and s3 == 0.0
            if situation == "q_lands_on_lam":
                assert np.array_equal(np.abs(qh), np.ones(n, dtype=np.float32))
            if situation == "x_at_bound_pushed_outward":
                assert np.array_equal(xh, v["x"]) and cols[7] == n and cols[5] == 0.0
            if situation == "x_at_bound_pushed_inward":
                assert np.all((xh > 0.0) & (xh < 2.0)) and cols[7] == 0
            if situation == "no_box":
                assert cols[7] == 0
            if situation == "lower_equals_upper":
                assert np.all(xh == lof) and cols[7] == n
            if situation == "lam_zero":
                assert not qh.any()
            if not with_xt:
                assert cols[6] == 0.0
    # x_new may be x
    v, (sigma, lam, tau, lo, hi) = _craft("random", n, m)
    xn, xb, _tail = _expected("random", True, True, n, m)[2]
    x, xbar = _dev(eng, v["x"], offset), _dev(eng, np.zeros(n, dtype=np.float32), offset)
    eng.pdhg_primal(tau, lo, hi, x, _dev(eng, v["z"], offset), _dev(eng, v["v"], offset), x, xbar, _dev(eng, v["xt"], offset),
                    eng.scalars(8 * CAP).ref(0), CAP)
    assert _ulps(x.cpu().numpy(), xn) <= 1 and _ulps(xbar.cpu().numpy(), xb) <= 1


def test_argument_checks_come_first(eng):
    """Bad arguments are refused with trk_last_error's text before anything is launched."""
    from trips_py_amd.operators import SparseOp
    v = {k: torch.zeros(8, dtype=torch.float32, device=eng.device) for k in "xzvqupwbnr"}
    NP = eng.scalars(8 * CAP)
    with pytest.raises(ValueError, match="too small"):
        eng.pdhg_dual_p(0.5, v["w"], v["b"], v["p"], NP.ref(0), 0)
    with pytest.raises(ValueError, match="alias"):
        eng.pdhg_dual_p(0.5, v["w"], v["b"], v["w"], NP.ref(0), CAP)
    with pytest.raises(ValueError, match="sigma"):
        eng.pdhg_dual_q(float("inf"), 0.1, v["u"], v["q"], NP.ref(0), CAP)
    with pytest.raises(ValueError, match="lam"):
        eng.pdhg_dual_q(0.5, -0.1, v["u"], v["q"], NP.ref(0), CAP)
    with pytest.raises(ValueError, match="lo <= hi"):
        eng.pdhg_primal(0.5, 1.0, 0.0, v["x"], v["z"], v["v"], v["n"], v["r"], None, NP.ref(0), CAP)
    with pytest.raises(ValueError, match="xbar must not alias"):
        eng.pdhg_primal(0.5, 0.0, 1.0, v["x"], v["z"], v["v"], v["n"], v["x"], None, NP.ref(0), CAP)
    assert not NP.host().any()
    import scipy.sparse as sp
    Ls = SparseOp(sp.identity(8, format="csr"), engine=eng)
    assert eng.pdhg_fused_caps(Ls._h) == 0
    with pytest.raises(NotImplementedError):
        eng.pdhg_tv_dual(Ls._h, 0.5, 0.1, v["x"], v["q"], NP.ref(0), CAP)
    with pytest.raises(NotImplementedError):
        eng.pdhg_tv_primal(Ls._h, 0.5, 0.0, 1.0, v["x"], v["z"], v["q"], v["n"], v["r"], None, NP.ref(0), CAP)


# ====================================================================== (2) the fused first-difference kernels
def _tv_inputs(N, seed):
    rng = np.random.default_rng(seed)
    f, n, r = np.float32, N * N, 2 * N * (N - 1)
    return {"xbar": rng.random(n).astype(f), "q": (0.02 * rng.random(r) - 0.01).astype(f), "x": rng.random(n).astype(f),
            "z": (0.2 * rng.random(n) - 0.1).astype(f), "xt": rng.random(n).astype(f)}


def _generic(eng, L, par, d, with_xt):
    """trk_op_apply on the same handle, then the streaming kernels: (q', x', xbar', the eight column sums)."""
    sigma, lam, tau, lo, hi = par
    q, NP = d["q"].clone(), eng.scalars(8 * CAP)
    eng.pdhg_dual_q(sigma, lam, L.apply(d["xbar"]), q, NP.ref(0), CAP)
    x_new, xbar = torch.empty_like(d["x"]), torch.empty_like(d["x"])
    eng.pdhg_primal(tau, lo, hi, d["x"], d["z"], L.apply(q, transpose=True), x_new, xbar, d["xt"] if with_xt else None, NP.ref(0), CAP)
    return q, x_new, xbar, NP.host().reshape(CAP, 8).sum(axis=0)


def _fused(eng, L, par, d, with_xt):
    sigma, lam, tau, lo, hi = par
    q, NP = d["q"].clone(), eng.scalars(8 * CAP)
    nb = eng.pdhg_tv_dual(L._h, sigma, lam, d["xbar"], q, NP.ref(0), CAP)
    x_new, xbar = torch.empty_like(d["x"]), torch.empty_like(d["x"])
    assert eng.pdhg_tv_primal(L._h, tau, lo, hi, d["x"], d["z"], q, x_new, xbar, d["xt"] if with_xt else None, NP.ref(0), CAP) == nb
    parts = NP.host().reshape(CAP, 8)
    assert not parts[nb:].any()
    return q, x_new, xbar, parts.sum(axis=0), nb


@pytest.mark.parametrize("with_xt", [True, False])
@pytest.mark.parametrize("N", [2, 5, 33, 257, 260, 2052])
def test_fused_tv_kernels(eng, N, with_xt):
    """One column, a ragged row batch, the 256-thread column block crossed, and N = 2052, the first size whose 9 x 513 blocks exceed
    the cap of 4096 (455 row batches: a block strides over two): against the restatement (1 ulp, sums 1e-12) and against the generic
    path on the same handle (bit for bit, sums aside)."""
    from trips_py_amd.operators import FirstDerivative2D
    L = FirstDerivative2D(N, engine=eng)
    assert eng.pdhg_fused_caps(L._h) == 1
    par = (0.37, 0.004, 0.21, 0.2, 0.8)
    sigma, lam, tau, lo, hi = par
    v = _tv_inputs(N, N)
    d = {k: eng.to_vec(a) for k, a in v.items()}
    qf, xf, bf, cols, nb = _fused(eng, L, par, d, with_xt)
    gx = (N + 255) // 256
    assert nb == gx * min((N + 3) // 4, 4096 // gx) == eng.pdhg_blocks(1, 1, 1, L._h) and (N != 2052 or nb == 4095)
    qn, s1, s3 = C.tv_dual_f32(N, sigma, lam, v["xbar"], v["q"])
    qh, xh = qf.cpu().numpy(), xf.cpu().numpy()
    assert _ulps(qh, qn) <= 1
    xn, xb, tail = C.tv_primal_f32(N, tau, lo, hi, v["x"], v["z"], qh, v["xt"] if with_xt else None)    # (gathers the device's q')
    assert _ulps(xh, xn) <= 1 and _ulps(bf.cpu().numpy(), xb) <= 1
    _sums_match(cols[[1, 3, 4, 5, 6]], [s1, s3] + tail[:3], N)
    assert cols[7] == tail[3]
    assert np.all(np.abs(qh) <= np.float32(lam)) and np.all((xh >= np.float32(lo)) & (xh <= np.float32(hi)))
    assert cols[7] == np.count_nonzero((xh == np.float32(lo)) | (xh == np.float32(hi)))
    if N >= 33:
        assert np.count_nonzero(np.abs(qh) == np.float32(lam)) > 0 and 0 < cols[7] < N * N
    assert cols[0] == 0.0 and cols[2] == 0.0
    qg, xg, bg, gcols = _generic(eng, L, par, d, with_xt)
    assert torch.equal(qf, qg) and torch.equal(xf, xg) and torch.equal(bf, bg)
    _sums_match(cols[[1, 3, 4, 5, 6]], gcols[[1, 3, 4, 5, 6]], N)
    assert cols[7] == gcols[7]


# ====================================================================== (3) the one-call loop against single steps
K = 12


def _run(eng, P, history=True, fused=None, with_xt=True, max_iter=K):
    from trips_py_amd.solvers import PDHGRun
    return PDHGRun(P.device(eng), P.b, P.device_L(eng), P.lam, P.sigma, P.tau, P.lo, P.hi, None, max_iter,
                   P.x_true if with_xt else None, history=history, fused=fused)


def _bits(run):
    run.rows()
    return [t.clone() for t in (run.x_cur, run.xbar, run.p, run.q)], run.S.host().view(np.int64).copy()


@pytest.mark.parametrize("history", [True, False, 3])
@pytest.mark.parametrize("name", C.NAMES)
def test_run_equals_steps(eng, name, history):
    P = C.problem(name)
    ref = _run(eng, P, history)
    assert ref.fused == (name in C.FUSED)
    for _ in range(K):
        ref.step()
    want_vecs, want_S = _bits(ref)
    assert np.all(np.isfinite(ref.rows())) and ref.rows()[:, 4].min() > 0
    for calls in ([K], [1, K - 1], [3, 5, K - 8]):
        run = _run(eng, P, history)
        for c in calls:
            run.run(c)
        assert run.k == K
        vecs, Sb = _bits(run)
        for key, a, b in zip(("x", "xbar", "p", "q"), vecs, want_vecs):
            assert torch.equal(a, b), (calls, key)
        assert np.array_equal(Sb, want_S), calls
    if history is True:
        assert all(torch.equal(ref.slot(k), run.slot(k)) for k in range(K))
    if name in C.FUSED:
        gen = _run(eng, P, history, fused=False)
        assert not gen.fused
        gen.run(K)
        for key, a, b in zip(("x", "xbar", "p", "q"), _bits(gen)[0], want_vecs):
            assert torch.equal(a, b), ("generic", key)
        assert np.allclose(gen.rows(), ref.rows(), rtol=1e-12, atol=0)
    else:
        with pytest.raises(ValueError):
            _run(eng, P, history, fused=True)


# ====================================================================== (4) whole solves against float64
ITERS = 30
# The worst relative 2-norm distance of the storage-faithful restatement (pdhg_cases.pdhg_f32) from the float64 restatement over 30
# iterates, measured in NumPy on a CPU for these five problems on the oracle's operators — what fp32 storage alone costs
# (tests/test_pdhg_host.py recomputes them):
CPU_F32_ITERATES = {"Q1": 7.45e-8, "Q2": 1.21e-7, "Q3": 9.32e-8, "Q4": 9.15e-8, "Q5": 1.15e-7}
# ... and, in the same two runs, the worst relative deviation of ||A xbar - b|| / ||b|| and of the objective:
CPU_F32_RNRM = {"Q1": 6.19e-8, "Q2": 1.54e-7, "Q3": 5.18e-8, "Q4": 1.70e-7, "Q5": 6.33e-8}
CPU_F32_OBJECTIVE = {"Q1": 9.58e-8, "Q2": 2.92e-7, "Q3": 6.60e-8, "Q4": 1.29e-7, "Q5": 7.48e-8}


def _limit(cpu_figure):
    """8 x the cost of fp32 storage alone, never below 1e-5 (the rule of the automatic-lambda bars)."""
    return max(8 * cpu_figure, 1e-5)


@pytest.mark.parametrize("name", C.NAMES)
def test_solve_against_float64(eng, name):
    from trips_py_amd.solvers import PDHG
    P = C.problem(name)
    A, L = P.device(eng), P.device_L(eng)
    if name in ("Q3", "Q5"):
        Apair = C.pair(P.oracle())
    else:                                                     # the operator's own matrices; the "transpose" is the operator's too
        M, Mt = A.todense(), A.T.todense()
        assert M.shape == P.shape and Mt.shape == P.shape[::-1]
        Apair = ((lambda v: M @ v), (lambda v: Mt @ v))
    ref = P.f64(ITERS, A=Apair, x_true=P.x_true)
    x, info = PDHG(A, P.b, L, P.lam, ITERS, 0, x_true=P.x_true, lower=P.lo, upper=P.hi, sigma=P.sigma, tau=P.tau)
    assert info["its"] == ITERS and len(info["xHistory"]) == ITERS
    H = [h.reshape(-1) for h in info["xHistory"]]
    assert all(float(h.min()) >= P.lo and float(h.max()) <= P.hi for h in H)
    worst = max(np.linalg.norm(h - xr) / np.linalg.norm(xr) for h, xr in zip(H, ref["X"]))
    bar(f"pdhg_{name}_iterates_vs_float64", worst, _limit(CPU_F32_ITERATES[name]))
    Sr = ref["S"]
    bar(f"pdhg_{name}_Rnrm_vs_float64", np.max(np.abs(np.array(info["Rnrm"]) / (np.sqrt(Sr[:, 0]) / np.linalg.norm(P.b)) - 1)),
        _limit(CPU_F32_RNRM[name]))
    bar(f"pdhg_{name}_objective_vs_float64", np.max(np.abs(np.array(info["objective"]) / (0.5 * Sr[:, 0] + P.lam * Sr[:, 1]) - 1)),
        _limit(CPU_F32_OBJECTIVE[name]))
    assert np.allclose(info["relError"], np.sqrt(Sr[:, 6]) / np.linalg.norm(P.x_true), rtol=1e-4)
    want = C.objective(Apair, C.pair(P.oracle_L()), P.b, P.lam, x)
    assert abs(info["objectiveFinal"] / want - 1) < 1e-5
    if name == "Q2":
        assert np.count_nonzero(H[-1] == 3.0) > 10 and info["active"][-1] == np.count_nonzero((H[-1] == 0.0) | (H[-1] == 3.0))


# ====================================================================== (5) the norm estimate and the objective
@pytest.mark.parametrize("name", C.NAMES)
def test_operator_norm_sq_on_the_device(eng, name):
    from trips_py_amd.operators import operator_norm_sq
    P = C.problem(name)
    assert abs(operator_norm_sq([P.device(eng), P.device_L(eng)], iters=30, seed=0) / P.est - 1) < 1e-4


def test_objective_decreases_and_default_steps(eng):
    from trips_py_amd.solvers import PDHG
    P = C.problem("Q1")
    _x, info = PDHG(P.device(eng), P.b, P.device_L(eng), P.lam, 300, history=False)
    assert info["its"] == 300 and info["xHistory"] == []
    assert info["objective"][299] < info["objective"][29]
    assert abs(info["normK2"] / P.est - 1) < 1e-4 and abs(info["sigma"] * info["tau"] * info["normK2"] - 0.9025) < 1e-12
    assert info["objectiveFinal"] < info["objective"][29]


# ====================================================================== (6) stopping on the device
def test_tol_stops_where_the_rows_say(eng):
    """tol > 0 reads a row back every iteration and stops where the tol = 0 run's rows say, with that iterate's bits."""
    from trips_py_amd.solvers import PDHG
    P = C.problem("Q1")
    run = _run(eng, P, True, with_xt=False, max_iter=ITERS)
    run.run(ITERS)
    rows = run.rows()
    rel = np.sqrt(rows[:, 5]) / np.sqrt(rows[:, 4])
    tol = float(np.sqrt(rel[14] * rel[15]))
    hit = int(np.nonzero(rel <= tol)[0][0]) + 1
    assert 1 < hit < ITERS
    x, info = PDHG(P.device(eng), P.b, P.device_L(eng), P.lam, ITERS, tol, lower=P.lo, upper=P.hi, sigma=P.sigma, tau=P.tau,
                   history=False)
    assert info["its"] == hit and info["xHistory"] == []
    assert np.array_equal(x.reshape(-1), run.slot(hit - 1).cpu().numpy().astype(np.float64))
    assert info["relResidual"] == list(rel[:hit])
