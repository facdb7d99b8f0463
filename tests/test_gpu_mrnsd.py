"""MRNSD on the GPU (csrc/mrnsd.hip, solvers/MRNSD.py) against the NumPy restatement of tests/mrnsd_cases.py:
one trk_mrnsd_update launch on crafted vectors against the storage-faithful form, the one-call C loop against single steps
(bit for bit), and whole solves against the float64 form."""
import numpy as np
import pytest
import torch

import mrnsd_cases as C
from conftest import bar

pytestmark = pytest.mark.gpu

CAP = 1024                 # blocks of a streaming kernel at most (stream_grid), and the gb capacity used here
PER_BLOCK = 1024           # floats per block before the grid stops growing


@pytest.fixture(scope="module")
def eng():
    from trips_py_amd.engine import default_engine
    return default_engine()


def _grid(n, m):
    return min((max(n, m) + PER_BLOCK - 1) // PER_BLOCK, CAP)


# ====================================================================== one launch on crafted vectors
SIZES = [1, 3, 1024, 1027, 66561, 614402, 1300003]
SITUATIONS = ["min_first", "min_last", "min_last_block", "no_negative_s", "zeros_in_x", "bound_above_theta", "unorm_zero"]

_base = {}


def _vectors(n, m):
    """Seeded fp32 vectors, made once per (n, m): x in [0.5, 1.5], the others of either sign."""
    if (n, m) not in _base:
        rng = np.random.default_rng(7 * n + m)
        f = np.float32
        _base[(n, m)] = {"x": (0.5 + rng.random(n)).astype(f), "g": (3 * rng.random(n) - 1.5).astype(f),
                         "s": (0.5 * rng.random(n) - 0.25).astype(f), "z": (rng.random(n) - 0.5).astype(f),
                         "xt": rng.random(n).astype(f), "r": rng.standard_normal(m).astype(f), "u": rng.standard_normal(m).astype(f)}
    return {k: v.copy() for k, v in _base[(n, m)].items()}


def _craft(situation, n, m):
    """Vectors and the scalars (gamma, bound, ||u||^2) of a situation; theta = gamma / ||u||^2 = 1 (both 0.75) except unorm_zero.
    x / -s >= 2 on the base vectors, so a bound of 0.3 cuts the step and one of 2.5 does not; afterwards the ratio of an entry is
    x' / (x' g') ~ 1 / g' >= 0.4 with g' <= 2.5, so an entry with g' = 50 (z = 0 there) holds the next minimum."""
    v = _vectors(n, m)
    gamma, bound, uu = 0.75, 0.3, 0.75
    # (the first float4 of the last block, where n reaches that far)
    at = {"min_first": 0, "min_last": n - 1, "min_last_block": min(n - 1, (_grid(n, m) - 1) * PER_BLOCK)}.get(situation)
    if at is not None:
        v["g"][at], v["z"][at] = 50.0, 0.0
    elif situation == "no_negative_s":
        v["g"], v["z"], v["s"] = -np.abs(v["g"]), -np.abs(v["z"]), np.abs(v["s"])
        bound = np.inf
    elif situation == "zeros_in_x":
        v["x"][::5] = 0.0
        v["s"][::5] = -np.abs(v["s"][::5])                # would go negative: the clamp holds them at 0
        v["s"][::10] = 0.0
    elif situation == "bound_above_theta":
        bound = 2.5
    elif situation == "unorm_zero":
        uu = 0.0
        v["s"] = -(v["x"] * v["g"])                        # what the kernel recomputes: s must come back bit for bit
    return v, gamma, bound, uu


_want = {}


def _expected(situation, with_xt, n, m):
    """The restatement's update of a situation, computed once and shared by the scalar-source and alignment cases."""
    key = (situation, with_xt, n, m)
    if key not in _want:
        v, gamma, bound, uu = _craft(situation, n, m)
        _want[key] = C.update_f32(gamma, bound, uu, v["x"], v["g"], v["s"], v["z"], v["r"], v["u"], v["xt"] if with_xt else None)
    return _want[key]


def _ulps(a, b):
    """Largest distance in units in the last place between two fp32 arrays (equal values, -0 and 0 included, count 0)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    d = np.abs(ia - ib)
    d[a == b] = 0
    return int(d.max()) if d.size else 0


def _partials(total, count, rng, minimum=False):
    """`count` doubles whose sum (minimum) is `total` in ANY order: multiples of 2^-10 that add up exactly (+inf and larger values
    around the one minimum, which sits in the last entry)."""
    if minimum:
        p = np.full(count, np.inf)
        p[::3] = total + 1.0 + rng.integers(0, 1000, size=p[::3].size) / 1024.0 if np.isfinite(total) else np.inf
        p[-1] = total
        return p
    p = rng.integers(0, 64, size=count) / 1024.0
    p[0] += total - p.sum()
    assert p.sum() == total and p[::-1].sum() == total
    return p


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("src", ["finished", "partials"])
@pytest.mark.parametrize("m_kind", ["m_eq_n", "m_515"])
@pytest.mark.parametrize("n", SIZES)
def test_one_update_against_the_restatement(eng, n, m_kind, src, offset):
    m = n if m_kind == "m_eq_n" else 515
    grid = _grid(n, m)
    rng = np.random.default_rng(n + m)

    def dev(a):
        """A device copy that starts `offset` floats behind a 16-byte boundary."""
        t = torch.empty(a.size + 4, dtype=torch.float32, device=eng.device)
        assert t.data_ptr() % 16 == 0
        w = t[offset:offset + a.size]
        w.copy_(torch.from_numpy(a))
        return w

    for situation in SITUATIONS:
        for with_xt in ((True, False) if situation in ("min_last", "zeros_in_x") else (True,)):
            v, gamma, bound, uu = _craft(situation, n, m)
            want = _expected(situation, with_xt, n, m)
            d = {k: dev(a) for k, a in v.items()}
            x_new = dev(np.zeros(n, dtype=np.float32))
            count = max(grid, 3) if src == "partials" else 1
            IN = eng.scalars(3 * CAP)                       # gamma | bound | ||u||^2 sources
            IN.set(0, _partials(gamma, count, rng))
            IN.set(CAP, _partials(bound, count, rng, minimum=True))
            IN.set(2 * CAP, _partials(uu, count, rng))
            OUT, ROW, NP = eng.scalars(2 * CAP), eng.scalars(4), eng.scalars(4 * CAP)
            nb = eng.mrnsd_update(IN.ref(0), count, IN.ref(CAP), count, IN.ref(2 * CAP), count, d["x"], x_new, d["g"], d["s"], d["z"],
                                  d["r"], d["u"], d["xt"] if with_xt else None, OUT.ref(0), CAP, ROW.ref(0), ROW.ref(2), NP.ref(0), CAP)
            tag = (situation, with_xt)
            assert nb == grid, tag
            row, out, parts = ROW.host(), OUT.host(), NP.host()[:4 * nb].reshape(nb, 4)
            # the published scalars: exact operations on exactly converted inputs
            assert row[0] == uu and row[1] == want["alpha"] and row[2] == gamma and row[3] == bound, (tag, row, want["alpha"])
            got = {"x": x_new, "g": d["g"], "s": d["s"], "r": d["r"]}
            for key, t in got.items():
                assert _ulps(t.cpu().numpy(), want[key]) <= 1, (tag, key)
            assert float(x_new.min()) >= 0.0, tag
            assert float(np.min(out[CAP:CAP + nb])) == want["bound"], (tag, np.min(out[CAP:CAP + nb]), want["bound"])
            sums = {"gamma": out[:nb].sum(), "xx": parts[:, 0].sum(), "dd": parts[:, 1].sum(), "ee": parts[:, 2].sum(),
                    "rr": parts[:, 3].sum()}
            for key, val in sums.items():
                assert abs(val - want[key]) <= 1e-12 * abs(want[key]), (tag, key, val, want[key])
            if situation == "unorm_zero":                   # alpha = 0: the state is what it was, bit for bit
                assert row[1] == 0.0
                for key, t in got.items():
                    assert np.array_equal(t.cpu().numpy().view(np.int32), v[key].view(np.int32)), (tag, key)
            if situation == "no_negative_s":
                assert want["bound"] == np.inf and row[1] == 1.0
            if situation == "bound_above_theta":
                assert row[1] == 1.0
            if situation.startswith("min_"):
                assert row[1] == 0.3 and want["bound"] < 0.021


def test_argument_checks_come_first(eng):
    """Bad arguments are refused with trk_last_error's text before anything is launched."""
    v = {k: torch.zeros(8, dtype=torch.float32, device=eng.device) for k in "xgszru"}
    Sc = eng.scalars(4 * CAP)
    with pytest.raises(ValueError, match="ping-pong"):       # the partials written where they are read
        eng.mrnsd_update(Sc.ref(0), 2, Sc.ref(CAP), 2, Sc.ref(8), 1, v["x"], v["x"], v["g"], v["s"], v["z"], v["r"], v["u"], None,
                         Sc.ref(0), CAP, Sc.ref(3 * CAP), None, Sc.ref(3 * CAP + 8), CAP)
    with pytest.raises(ValueError, match="too small"):
        eng.mrnsd_update(Sc.ref(0), 1, Sc.ref(1), 1, Sc.ref(2), 1, v["x"], v["x"], v["g"], v["s"], v["z"], v["r"], v["u"], None,
                         Sc.ref(2 * CAP), 0, Sc.ref(3 * CAP), None, Sc.ref(3 * CAP + 8), CAP)
    with pytest.raises(ValueError, match="bad argument"):
        eng.mrnsd_finish(None, 1, Sc.ref(0), 1, Sc.ref(8))


# ====================================================================== the one-call loop against single steps
K = 12


def _bits(run):
    _s0, _rows = run.rows()
    vecs = [v.clone() for v in (run.x_cur, run.g, run.s, run.r)]
    return vecs, run.S.host().view(np.int64).copy()


@pytest.mark.parametrize("history", [True, False, 3])
@pytest.mark.parametrize("with_xt", [True, False])
@pytest.mark.parametrize("name", C.NAMES)
def test_run_equals_steps(eng, name, with_xt, history):
    from trips_py_amd.solvers import MRNSDRun
    P = C.problem(name)
    A = P.device(eng)
    xt = P.x_true if with_xt else None
    ref = MRNSDRun(A, P.b, P.x0, K, xt, history=history)
    for _ in range(K):
        ref.step()
    want_vecs, want_S = _bits(ref)
    for calls in ([K], [1, K - 1], [3, 5, K - 8]):
        run = MRNSDRun(A, P.b, P.x0, K, xt, history=history)
        for c in calls:
            run.run(c)
        assert run.k == K
        vecs, S = _bits(run)
        for key, a, b in zip("xgsr", vecs, want_vecs):
            assert torch.equal(a, b), (calls, key)
        assert np.array_equal(S, want_S), calls
    if history is True:
        assert all(torch.equal(ref.slot(k), run.slot(k)) for k in range(K))


# ====================================================================== whole solves against float64
ITERS = 30
# The worst relative 2-norm distance of the storage-faithful restatement (mrnsd_cases.mrnsd_f32) from the float64 restatement over 30
# iterates, measured in NumPy on a CPU for these four problems on the oracle's operators — what fp32 storage alone costs:
CPU_F32_ITERATES = {"P1": 2.42e-6, "P2": 6.83e-7, "P3": 4.57e-7, "P4": 1.15e-6}
# ... and, in the same two runs, the worst relative deviation of the step lengths alpha_k and of ||r_k|| / ||b||:
CPU_F32_STEP = {"P1": 6.95e-7, "P2": 3.89e-7, "P3": 4.46e-7, "P4": 7.07e-6}
CPU_F32_RNRM = {"P1": 9.53e-8, "P2": 8.21e-8, "P3": 2.28e-7, "P4": 3.14e-6}


def _limit(cpu_figure):
    """8 x the cost of fp32 storage alone, never below 1e-5 (the rule of the automatic-lambda bars)."""
    return max(8 * cpu_figure, 1e-5)


@pytest.mark.parametrize("name", C.NAMES)
def test_solve_against_float64(eng, name):
    from trips_py_amd.solvers import MRNSD
    P = C.problem(name)
    A = P.device(eng)
    if name == "P3":
        o = P.oracle()
        matvec, rmatvec = o.matvec, o.rmatvec
    else:                                                     # the operator's own matrices; the "transpose" is the operator's too
        M, Mt = A.todense(), A.T.todense()
        assert M.shape == P.shape and Mt.shape == P.shape[::-1]
        matvec, rmatvec = (lambda v: M @ v), (lambda v: Mt @ v)
    ref = C.mrnsd_f64(matvec, rmatvec, P.b, P.x0, ITERS)
    x, info = MRNSD(A, P.b, P.x0, ITERS, 0, x_true=P.x_true)
    assert info["its"] == ITERS and len(info["xHistory"]) == ITERS
    H = [h.reshape(-1) for h in info["xHistory"]]
    assert all(float(h.min()) >= 0.0 for h in H)
    worst = max(np.linalg.norm(h - xr) / np.linalg.norm(xr) for h, xr in zip(H, ref["X"]))
    bar(f"mrnsd_{name}_iterates_vs_float64", worst, _limit(CPU_F32_ITERATES[name]))
    assert info["bounded"] == [a < t for a, t in zip(ref["alpha"], ref["theta"])]
    bar(f"mrnsd_{name}_stepLength_vs_float64", np.max(np.abs(np.array(info["stepLength"]) / np.array(ref["alpha"]) - 1)),
        _limit(CPU_F32_STEP[name]))
    bar(f"mrnsd_{name}_Rnrm_vs_float64", np.max(np.abs(np.array(info["Rnrm"]) / (np.sqrt(ref["rr"]) / np.linalg.norm(P.b)) - 1)),
        _limit(CPU_F32_RNRM[name]))
    assert np.allclose(info["relError"], [np.linalg.norm(xr - P.x_true) / np.linalg.norm(P.x_true) for xr in ref["X"]], rtol=1e-4)
    if name == "P1":
        zeroed = np.nonzero(ref["X"][0] == 0)[0]
        assert zeroed.size == 1
        assert H[0][zeroed[0]] == 0.0 and H[ITERS - 1][zeroed[0]] == 0.0


def test_tol_and_history_off_on_the_device(eng):
    """tol > 0 reads a row back every iteration (trk_mrnsd_finish on the way) and stops where the tol = 0 run's gammas say."""
    from trips_py_amd.solvers import MRNSD, MRNSDRun
    P = C.problem("P1")
    A = P.device(eng)
    run = MRNSDRun(A, P.b, P.x0, ITERS)
    run.run(ITERS)
    s0, rows = run.rows()
    tol = 0.05
    hit = int(np.nonzero(np.sqrt(rows[:, 2]) <= tol * np.sqrt(s0[0]))[0][0]) + 1
    assert 1 < hit < ITERS
    x, info = MRNSD(A, P.b, P.x0, ITERS, tol, history=False)
    assert info["its"] == hit and info["xHistory"] == []
    assert np.array_equal(x.reshape(-1), run.slot(hit - 1).cpu().numpy().astype(np.float64))
