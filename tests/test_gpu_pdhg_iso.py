"""PDHG with isotropic TV on the GPU (k_pdhg_tv_dual<kPairs, true> and k_pdhg_tv_dual<kPairs, false> in csrc/pdhg_tv.hip, the entry points in
csrc/pdhg.hip, solvers/PDHG.py tv='iso') against the NumPy restatement of tests/pdhg_iso_cases.py: one launch of each dual form
against the storage-faithful form, crafted pairs, the fused form against the unfused one (bit for bit), the one-call C loop against
single steps (bit for bit), and whole solves against the float64 form."""
import numpy as np
import pytest
import torch

import pdhg_cases as C
import pdhg_iso_cases as I
from conftest import bar
from test_gpu_pdhg import CAP, PER_BLOCK, _dev, _sums_match, _ulps

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SIGMA, LAM, TAU, LO, HI = 0.37, 0.1, 0.21, 0.2, 0.8      # |q + sigma u| falls on both sides of lam on random images


@pytest.fixture(scope="module")
def eng():
    from trips_py_amd.engine import default_engine
    return default_engine()


def _stream_grid(k):
    return min((k + PER_BLOCK - 1) // PER_BLOCK, 1024)


def _column_grid(N):
    gx = (N + 255) // 256
    return gx * min((N + 3) // 4, 4096 // gx)


_inputs = {}


def _tv_inputs(N):
    """Seeded image vectors and a dual inside the ball (|q_h|, |q_v| <= 0.05 < lam / sqrt 2), computed once per size."""
    if N not in _inputs:
        rng = np.random.default_rng(7 * N + 1)
        n, r = N * N, 2 * N * (N - 1)
        _inputs[N] = {"xbar": rng.random(n).astype(F32), "q": (0.1 * rng.random(r) - 0.05).astype(F32), "x": rng.random(n).astype(F32),
                      "z": (0.2 * rng.random(n) - 0.1).astype(F32), "xt": rng.random(n).astype(F32)}
    return _inputs[N]


def _check_projection(N, frames, lam, u, q, qh):
    """What the projection promises of q' = qh whatever the rounding: singles inside [-lf, lf] exactly, every pair's float64 norm
    <= lf (1 + 8 * 2^-24) — the stated operations give 1 + 4 * 2^-24 (two roundings in m2, one in m, one in s, one in the product)
    and the 8 leaves one further unit each to sqrt and divide.  Returns the mask of the pairs the restatement keeps (m <= lf)."""
    lf = F32(lam)
    ph, pv, sg = I.groups(N, frames, u.size)
    assert np.all((qh[sg] >= -lf) & (qh[sg] <= lf))
    norms = np.sqrt(qh[ph].astype(F64) ** 2 + qh[pv].astype(F64) ** 2)
    assert norms.max(initial=0.0) <= F64(lf) * (1 + 8 * 2.0 ** -24)
    assert np.all(np.isfinite(qh))
    th, tv = C.fma32(F32(SIGMA), u[ph], q[ph]), C.fma32(F32(SIGMA), u[pv], q[pv])
    keep = np.sqrt(I.fma32_arrays(th, th, tv * tv)) <= lf
    assert np.array_equal(qh[ph][keep], th[keep]) and np.array_equal(qh[pv][keep], tv[keep])      # a kept pair is t itself
    return keep


# ====================================================================== (1) the fused dual, one launch
@pytest.mark.parametrize("N", [2, 5, 33, 257, 260, 2052])
def test_fused_dual_against_the_restatement(eng, N):
    """The sizes of test_gpu_pdhg.py's fused test: one pair and two singles, one column block with a ragged row batch, the 256-thread
    column block crossed, and N = 2052 where the grid cap makes a block stride over two row batches."""
    from trips_py_amd.operators import FirstDerivative2D
    L = FirstDerivative2D(N, engine=eng)
    v = _tv_inputs(N)
    q, NP = eng.to_vec(v["q"]), eng.scalars(8 * CAP)
    nb = eng.pdhg_tv_dual_iso(L._h, SIGMA, LAM, eng.to_vec(v["xbar"]), q, NP.ref(0), CAP)
    assert nb == _column_grid(N) == eng.pdhg_blocks_iso(1, 1, 2 * N * (N - 1), N, 1, L._h) == eng.pdhg_blocks(1, 1, 1, L._h)
    assert N != 2052 or nb == 4095
    qn, s1, s3 = I.tv_dual_iso_f32(N, SIGMA, LAM, v["xbar"], v["q"])
    qh = q.cpu().numpy()
    print(N, "ulps", _ulps(qh, qn))
    assert _ulps(qh, qn) <= 1
    parts = NP.host().reshape(CAP, 8)
    assert not parts[nb:].any() and not parts[:, [0, 2, 4, 5, 6, 7]].any()
    _sums_match(parts.sum(axis=0)[[1, 3]], [s1, s3], N)
    keep = _check_projection(N, 1, LAM, C.d2_fwd_f32(N, v["xbar"]), v["q"], qh)
    if N >= 33:
        assert 0 < np.count_nonzero(keep) < keep.size


# ====================================================================== (2) crafted pairs through both dual forms
# sigma = 0.5; (lam, q_h, q_v, u_h, u_v) -> (q_h', q_v'), every number exact in fp32
CRAFTED = {"kept": (5.0, 2.0, 2.0, 2.0, 4.0, 3.0, 4.0),                         # t = (3, 4), m = 5 <= 5
           "scaled": (2.5, 2.0, 2.0, 2.0, 4.0, 1.5, 2.0),                       # t = (3, 4), s = 0.5
           "on_the_ball_pushed_outward": (5.0, 3.0, 4.0, 6.0, 8.0, 3.0, 4.0),   # t = (6, 8), s = 0.5: q' = q
           "one_member_zero": (2.0, 0.0, 2.0, 0.0, 4.0, 0.0, 2.0),              # t = (0, 4), s = 0.5
           "lam_zero_t_zero": (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),              # m = 0 <= 0: kept, no 0 / 0
           "lam_zero_t_nonzero": (0.0, 0.0, 0.0, 2.0, 4.0, 0.0, 0.0),           # s = 0 / m = 0
           "lands_on_the_ball": (5.0, 1.5, 2.0, 3.0, 4.0, 3.0, 4.0)}            # q inside, t = (3, 4) of norm lam exactly


@pytest.mark.parametrize("case", list(CRAFTED))
def test_crafted_pairs(eng, case):
    """N = 2: rows [H00, H10, V00, V01], the pair is (H00, V00).  The fused form gets an image with those differences."""
    from trips_py_amd.operators import FirstDerivative2D
    lam, qh0, qv0, uh, uv, wh, wv = CRAFTED[case]
    a = 8.0
    img = np.array([a, a - uh, a - uv, a - 1.0], dtype=F32)          # [[a, b], [c, d]]: H00 = a - b, V00 = a - c
    u = C.d2_fwd_f32(2, img)
    assert u[0] == uh and u[2] == uv
    q0 = np.array([qh0, 0.25, qv0, -0.25], dtype=F32)
    qn, s1, s3 = I.dual_q_iso_f32(2, 1, 0.5, lam, u, q0)
    assert qn[0] == wh and qn[2] == wv                               # the restatement gives the exact values
    L = FirstDerivative2D(2, engine=eng)
    for form in ("unfused", "fused"):
        q, NP = eng.to_vec(q0), eng.scalars(8 * CAP)
        if form == "fused":
            nb = eng.pdhg_tv_dual_iso(L._h, 0.5, lam, eng.to_vec(img), q, NP.ref(0), CAP)
        else:
            nb = eng.pdhg_dual_q_iso(2, 1, 0.5, lam, eng.to_vec(u), q, NP.ref(0), CAP)
        got = q.cpu().numpy()
        assert nb == 1 and np.array_equal(got, qn) and np.all(np.isfinite(got)), (form, got, qn)
        cols = NP.host().reshape(CAP, 8).sum(axis=0)
        _sums_match(cols[[1, 3]], [s1, s3], (case, form))
        assert np.isfinite(cols).all()


# ====================================================================== (3) the unfused dual
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("N,frames,tail", [(2, 1, 0), (5, 2, 25), (16, 3, 512), (33, 1, 7), (260, 2, 0)])
def test_unfused_dual_against_the_restatement(eng, N, frames, tail, offset):
    """Several frames, with and without a tail; (33, 1, 7): the tail starts 2112 floats in and ends ragged; (16, 3, 512): the rows of
    SpaceTimeDerivative(16, 3).  offset1 moves both operands one float off a 16-byte boundary."""
    off = frames * 2 * N * (N - 1)
    rows = off + tail
    rng = np.random.default_rng(1000 * N + 10 * frames + tail)
    u, q0 = (rng.random(rows) - 0.5).astype(F32), (0.1 * rng.random(rows) - 0.05).astype(F32)
    ud, q, NP = _dev(eng, u, offset), _dev(eng, q0, offset), eng.scalars(8 * CAP)
    nb = eng.pdhg_dual_q_iso(N, frames, SIGMA, LAM, ud, q, NP.ref(0), CAP)
    grouped, tail_blocks = _column_grid(N) * frames, (_stream_grid(tail) if tail else 0)
    assert nb == grouped + tail_blocks == eng.pdhg_blocks_iso(1, 1, rows, N, frames)
    qn, s1, s3 = I.dual_q_iso_f32(N, frames, SIGMA, LAM, u, q0)
    qh = q.cpu().numpy()
    assert _ulps(qh, qn) <= 1
    parts = NP.host().reshape(CAP, 8)
    assert not parts[nb:].any() and not parts[:, [0, 2, 4, 5, 6, 7]].any()
    _sums_match(parts.sum(axis=0)[[1, 3]], [s1, s3], (N, frames, tail))
    keep = _check_projection(N, frames, LAM, u, q0, qh)
    if N >= 16:
        assert 0 < np.count_nonzero(keep) < keep.size
    # the tail is the streaming kernel on the slices: the bits of pdhg_dual_q alone, and its blocks' rows of partials lie behind
    # the grouped kernel's — no row is written by both
    if tail:
        ut, qt, NT = _dev(eng, u[off:], (offset + off) % 4), _dev(eng, q0[off:], (offset + off) % 4), eng.scalars(8 * CAP)
        assert eng.pdhg_dual_q(SIGMA, LAM, ut, qt, NT.ref(0), CAP) == tail_blocks
        assert torch.equal(q[off:], qt)
        assert np.array_equal(parts[grouped:nb], NT.host().reshape(CAP, 8)[:tail_blocks])
    _q, g1, g3 = I.dual_q_iso_f32(N, frames, SIGMA, LAM, u[:off], q0[:off])
    _sums_match(parts[:grouped].sum(axis=0)[[1, 3]], [g1, g3], ("grouped rows", N, frames, tail))


# ====================================================================== (4) fused = unfused on the 2-D handle
@pytest.mark.parametrize("N", [2, 5, 33, 257, 260, 2052])
def test_fused_equals_unfused(eng, N):
    from trips_py_amd.operators import FirstDerivative2D
    L = FirstDerivative2D(N, engine=eng)
    d = {k: eng.to_vec(a) for k, a in _tv_inputs(N).items()}
    qf, qg, NPf, NPg = d["q"].clone(), d["q"].clone(), eng.scalars(8 * CAP), eng.scalars(8 * CAP)
    eng.pdhg_tv_dual_iso(L._h, SIGMA, LAM, d["xbar"], qf, NPf.ref(0), CAP)
    eng.pdhg_dual_q_iso(N, 1, SIGMA, LAM, L.apply(d["xbar"]), qg, NPg.ref(0), CAP)
    assert torch.equal(qf, qg) and not torch.equal(qf, d["q"])
    xf, bf, xg, bg = (torch.empty_like(d["x"]) for _ in range(4))
    eng.pdhg_tv_primal(L._h, TAU, LO, HI, d["x"], d["z"], qf, xf, bf, d["xt"], NPf.ref(0), CAP)
    eng.pdhg_primal(TAU, LO, HI, d["x"], d["z"], L.apply(qg, transpose=True), xg, bg, d["xt"], NPg.ref(0), CAP)
    assert torch.equal(xf, xg) and torch.equal(bf, bg)
    cf, cg = NPf.host().reshape(CAP, 8).sum(axis=0), NPg.host().reshape(CAP, 8).sum(axis=0)
    _sums_match(cf[[1, 3, 4, 5, 6]], cg[[1, 3, 4, 5, 6]], N)
    assert cf[7] == cg[7]
    # ... and it is not the anisotropic dual
    qa = d["q"].clone()
    eng.pdhg_tv_dual(L._h, SIGMA, LAM, d["xbar"], qa, eng.scalars(8 * CAP).ref(0), CAP)
    assert not torch.equal(qa, qf)


# ====================================================================== (5) the one-call loop against single steps
K = 12


def _run(eng, name, history=True, fused=None, max_iter=K):
    from trips_py_amd.solvers import PDHGRun
    P = C.problem(name)
    return PDHGRun(P.device(eng), P.b, P.device_L(eng), P.lam, P.sigma, P.tau, P.lo, P.hi, None, max_iter, P.x_true, history=history,
                   fused=fused, tv="iso", tv_dims=(24, 1) if name == "Q3" else None)


def _bits(run):
    run.rows()
    return [t.clone() for t in (run.x_cur, run.xbar, run.p, run.q)], run.S.host().view(np.int64).copy()


@pytest.mark.parametrize("history", [True, False, 3])
@pytest.mark.parametrize("name", I.NAMES)
def test_run_equals_steps(eng, name, history):
    ref = _run(eng, name, history)
    assert ref.fused == (name in I.FUSED) and ref.geo == I.GEOMETRY[name] and ref.tv == "iso"
    for _ in range(K):
        ref.step()
    want_vecs, want_S = _bits(ref)
    assert np.all(np.isfinite(ref.rows())) and ref.rows()[:, 4].min() > 0
    for calls in ([K], [1, K - 1], [3, 5, K - 8]):
        run = _run(eng, name, history)
        for c in calls:
            run.run(c)
        assert run.k == K
        vecs, Sb = _bits(run)
        for key, a, b in zip(("x", "xbar", "p", "q"), vecs, want_vecs):
            assert torch.equal(a, b), (calls, key)
        assert np.array_equal(Sb, want_S), calls
    if history is True:
        assert all(torch.equal(ref.slot(k), run.slot(k)) for k in range(K))
    if name in I.FUSED:
        gen = _run(eng, name, history, fused=False)
        assert not gen.fused
        gen.run(K)
        for key, a, b in zip(("x", "xbar", "p", "q"), _bits(gen)[0], want_vecs):
            assert torch.equal(a, b), ("unfused", key)
        assert np.allclose(gen.rows(), ref.rows(), rtol=1e-12, atol=0)
    else:
        with pytest.raises(ValueError):
            _run(eng, name, history, fused=True)


# ====================================================================== (6) whole solves against float64
ITERS = 30
# The worst relative 2-norm distance of the storage-faithful restatement (pdhg_iso_cases.pdhg_iso_f32) from the float64 restatement
# over 30 iterates, measured in NumPy on a CPU on the oracle's operators — what fp32 storage alone costs
# (tests/test_pdhg_iso_host.py recomputes them):
CPU_F32_ITERATES = {"Q1": 8.83e-8, "Q2": 1.15e-7, "Q3": 9.74e-8, "Q5": 1.11e-7}
# ... and, in the same two runs, the worst relative deviation of ||A xbar - b|| / ||b|| and of the objective:
CPU_F32_RNRM = {"Q1": 8.90e-8, "Q2": 1.39e-7, "Q3": 6.08e-8, "Q5": 6.19e-8}
CPU_F32_OBJECTIVE = {"Q1": 1.23e-7, "Q2": 2.66e-7, "Q3": 8.64e-8, "Q5": 8.15e-8}


def _limit(cpu_figure):
    """8 x the cost of fp32 storage alone, never below 1e-5 (the rule of test_gpu_pdhg.py's bars)."""
    return max(8 * cpu_figure, 1e-5)


@pytest.mark.parametrize("name", I.NAMES)
def test_solve_against_float64(eng, name):
    from trips_py_amd.solvers import PDHG
    P, geo = C.problem(name), I.GEOMETRY[name]
    A, L = P.device(eng), P.device_L(eng)
    if name in ("Q3", "Q5"):
        Apair = C.pair(P.oracle())
    else:                                                     # the operator's own matrices; the "transpose" is the operator's too
        M, Mt = A.todense(), A.T.todense()
        assert M.shape == P.shape and Mt.shape == P.shape[::-1]
        Apair = ((lambda v: M @ v), (lambda v: Mt @ v))
    ref = I.f64(name, ITERS, A=Apair, x_true=P.x_true)
    x, info = PDHG(A, P.b, L, P.lam, ITERS, 0, x_true=P.x_true, lower=P.lo, upper=P.hi, sigma=P.sigma, tau=P.tau, tv="iso",
                   tv_dims=geo if name == "Q3" else None)
    assert info["its"] == ITERS and len(info["xHistory"]) == ITERS and info["tv"] == "iso"
    H = [h.reshape(-1) for h in info["xHistory"]]
    assert all(float(h.min()) >= P.lo and float(h.max()) <= P.hi for h in H)
    worst = max(np.linalg.norm(h - xr) / np.linalg.norm(xr) for h, xr in zip(H, ref["X"]))
    bar(f"pdhg_iso_{name}_iterates_vs_float64", worst, _limit(CPU_F32_ITERATES[name]))
    Sr = ref["S"]
    bar(f"pdhg_iso_{name}_Rnrm_vs_float64", np.max(np.abs(np.array(info["Rnrm"]) / (np.sqrt(Sr[:, 0]) / np.linalg.norm(P.b)) - 1)),
        _limit(CPU_F32_RNRM[name]))
    bar(f"pdhg_iso_{name}_objective_vs_float64", np.max(np.abs(np.array(info["objective"]) / (0.5 * Sr[:, 0] + P.lam * Sr[:, 1]) - 1)),
        _limit(CPU_F32_OBJECTIVE[name]))
    assert np.allclose(info["relError"], np.sqrt(Sr[:, 6]) / np.linalg.norm(P.x_true), rtol=1e-4)
    want = I.objective_iso(Apair, C.pair(P.oracle_L()), P.b, P.lam, x, geo)
    assert abs(info["objectiveFinal"] / want - 1) < 1e-5
    if name == "Q2":
        assert np.count_nonzero(H[-1] == 3.0) > 10 and info["active"][-1] == np.count_nonzero((H[-1] == 0.0) | (H[-1] == 3.0))


# ====================================================================== (7) argument checks
def test_argument_checks_come_first(eng):
    """Bad arguments are refused with trk_last_error's text before anything is launched."""
    import scipy.sparse as sp
    from trips_py_amd.operators import FirstDerivative2D, SparseOp
    u, q, x = (torch.zeros(n, dtype=torch.float32, device=eng.device) for n in (40, 40, 25))
    NP = eng.scalars(8 * CAP)
    L = FirstDerivative2D(5, engine=eng)
    with pytest.raises(ValueError, match="rows"):
        eng.pdhg_dual_q_iso(5, 2, 0.5, 0.1, u, q, NP.ref(0), CAP)                # 40 rows < 2 * 40
    with pytest.raises(ValueError, match="N >= 2"):
        eng.pdhg_dual_q_iso(1, 1, 0.5, 0.1, u, q, NP.ref(0), CAP)
    with pytest.raises(ValueError, match="frames"):
        eng.pdhg_dual_q_iso(5, 0, 0.5, 0.1, u, q, NP.ref(0), CAP)
    with pytest.raises(ValueError, match="sigma"):
        eng.pdhg_dual_q_iso(5, 1, float("inf"), 0.1, u, q, NP.ref(0), CAP)
    with pytest.raises(ValueError, match="lam"):
        eng.pdhg_dual_q_iso(5, 1, 0.5, float("nan"), u, q, NP.ref(0), CAP)
    with pytest.raises(ValueError, match="alias"):
        eng.pdhg_dual_q_iso(5, 1, 0.5, 0.1, q, q, NP.ref(0), CAP)
    with pytest.raises(ValueError, match="too small"):
        eng.pdhg_dual_q_iso(5, 1, 0.5, 0.1, u, q, NP.ref(0), 1)                  # two row batches: two blocks
    with pytest.raises(ValueError, match="too small"):
        eng.pdhg_dual_q_iso(4, 1, 0.5, 0.1, u, q, NP.ref(0), 1)                  # one grouped block and one for the 16 tail rows
    with pytest.raises(ValueError, match="sigma"):
        eng.pdhg_tv_dual_iso(L._h, 0.0, 0.1, x, q, NP.ref(0), CAP)
    with pytest.raises(ValueError, match="lam"):
        eng.pdhg_tv_dual_iso(L._h, 0.5, -0.1, x, q, NP.ref(0), CAP)
    with pytest.raises(ValueError, match="too small"):
        eng.pdhg_tv_dual_iso(L._h, 0.5, 0.1, x, q, NP.ref(0), 1)
    with pytest.raises(ValueError, match="rows"):
        eng.pdhg_blocks_iso(25, 25, 39, 5, 1)
    assert not NP.host().any() and not q.any()
    Ls = SparseOp(sp.identity(25, format="csr"), engine=eng)
    with pytest.raises(NotImplementedError):
        eng.pdhg_tv_dual_iso(Ls._h, 0.5, 0.1, x, q, NP.ref(0), CAP)
    with pytest.raises(NotImplementedError):
        eng.pdhg_blocks_iso(25, 25, 40, 5, 1, Ls._h)
    # the loop refuses a geometry that is not L's, and a fused call whose geometry is not the handle's
    from trips_py_amd.solvers import PDHGRun
    P = C.problem("Q1")
    run = PDHGRun(P.device(eng), P.b, P.device_L(eng), P.lam, P.sigma, P.tau, P.lo, P.hi, None, 2, tv="iso")
    for geo in ((31, 1), (16, 4)):
        run.geo = geo
        with pytest.raises(ValueError):
            run.run(1)
    assert not run.q.any() and not run.p.any()
    P = C.problem("Q3")
    run = PDHGRun(P.device(eng), P.b, P.device_L(eng), P.lam, P.sigma, P.tau, P.lo, P.hi, None, 2, tv="iso", tv_dims=(24, 1))
    run.fused = True                                             # a CSR handle has no fused form
    with pytest.raises(NotImplementedError):
        run.run(1)
    assert not run.q.any() and not run.p.any()
