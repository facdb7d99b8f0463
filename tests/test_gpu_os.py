"""Ordered subsets on the GPU (csrc/subsets.hip, solvers/OSEM.py, solvers/SIRT.py) against the NumPy restatements of
tests/os_cases.py: one launch of each new kernel on crafted vectors against the storage-faithful form, the one-call C loops against
single steps (bit for bit), OSEM with one subset against MLEM (bit for bit), and whole solves against the float64 form on the
float64 operator of every subset."""
import numpy as np
import pytest
import torch

import mlem_cases as LC
import os_cases as C
from conftest import bar

pytestmark = pytest.mark.gpu

CAP = 1024                 # blocks of a streaming kernel at most (stream_grid)
PER_BLOCK = 1024           # floats per block before the grid stops growing
F32 = np.float32
INF = float("inf")


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
    assert abs(got - want) <= 1e-12 * abs(want), (tag, got, want)


# ====================================================================== one launch on crafted vectors
SIZES = [1, 3, 1024, 1027, 66561, 1300003]       # the tail alone, a second block, a block past the float4 body, the grid cap
_base = {}


def _vectors(n):
    """Seeded fp32 vectors, made once per n: x in [0.5, 1.5), t in [0, 2), reciprocals in [0.1, 1.1), x_ref, x_true; data w, b."""
    if n not in _base:
        rng = np.random.default_rng(13 * n + 7)
        _base[n] = {"x": (0.5 + rng.random(n)).astype(F32), "t": (2 * rng.random(n)).astype(F32), "inv": (0.1 + rng.random(n)).astype(F32),
                    "xr": (0.5 + rng.random(n)).astype(F32), "xt": rng.random(n).astype(F32),
                    "w": (0.5 + 50 * rng.random(n)).astype(F32), "b": (50 * rng.random(n)).astype(F32)}
    return {k: v.copy() for k, v in _base[n].items()}


def _crafted(n):
    """The start, the middle, the first float4 of the last block, the end (the scalar tail)."""
    return sorted({0, n - 1, min(n - 1, (_grid(n) - 1) * PER_BLOCK), n // 2})


def _check_x_launch(tag, parts, nb, n, got, want, with_xt):
    """What the two update kernels share: their vector within 1 ulp, slots 4..7 of their own blocks' rows, nothing else, no NaN."""
    assert nb == _grid(n), tag
    assert not np.any(np.isnan(parts)) and not np.any(np.isnan(got)), tag
    assert not np.any(parts[:, :4]) and not np.any(parts[nb:]), tag
    assert _ulps(got, want["x"]) <= 1, tag
    for slot, key in ((4, "xx"), (5, "dd"), (6, "ee")):
        _sum_close(parts[:, slot].sum(), want[key], tag + (key,))
    assert parts[:, 7].sum() == want["count"], tag
    if not with_xt:
        assert want["ee"] == 0.0 and not np.any(parts[:, 6]), tag


OPTIONALS = [(True, True), (True, False), (False, True), (False, False)]      # (x_ref, x_true) present


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", SIZES)
def test_one_osem_update_against_the_restatement(eng, n, offset):
    at = _crafted(n)
    worst = 0
    for situation in ("plain", "t_negative", "sinv_zero"):
        for with_ref, with_xt in (OPTIONALS if situation == "plain" else OPTIONALS[::3]):
            for alias in ((True, False) if situation == "plain" else (False,)):
                tag = (situation, with_ref, with_xt, alias)
                v = _vectors(n)
                if situation == "t_negative":                  # an operator with negative entries: the clamp holds x' at 0
                    v["t"][at] = -0.5
                    v["t"][::7] = -np.abs(v["t"][::7])
                elif situation == "sinv_zero":                 # the subset does not see these unknowns
                    v["inv"][at] = 0.0
                    v["inv"][::5] = 0.0
                want = C.osem_update_f32(v["x"], v["t"], v["inv"], v["xr"] if with_ref else None, v["xt"] if with_xt else None)
                d = {k: _dev(eng, v[k], offset) for k in ("x", "t", "inv", "xr", "xt")}
                x_new = d["x"] if alias else _dev(eng, np.full(n, 7.0, dtype=F32), offset)
                NP = eng.scalars(8 * CAP)
                nb = eng.osem_update(d["x"], d["t"], d["inv"], d["xr"] if with_ref else None, d["xt"] if with_xt else None, x_new,
                                     NP.ref(0), CAP)
                got = x_new.cpu().numpy()
                _check_x_launch(tag, NP.host().reshape(CAP, 8), nb, n, got, want, with_xt)
                worst = max(worst, _ulps(got, want["x"]))
                assert got.min() >= 0.0, tag
                if situation == "sinv_zero":                   # the keep rule: bit for bit the value that came in
                    kept = v["inv"] == 0
                    assert np.array_equal(got[kept].view(np.int32), v["x"][kept].view(np.int32)) and np.all(got[at] == v["x"][at]), tag
                    assert want["count"] == 0
                elif situation == "t_negative":
                    assert want["count"] >= len(at) and np.all(got[at] == 0.0), tag
                if with_ref:                                   # d is measured from x_ref, not from x
                    assert want["dd"] != C.osem_update_f32(v["x"], v["t"], v["inv"])["dd"], tag
    bar(f"osem_update_n{n}_off{offset}_ulps", worst, 1.5)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", SIZES)
def test_one_sirt_residual_against_the_restatement(eng, n, offset):
    at = _crafted(n)
    worst = 0
    for situation in ("plain", "rinv_zero", "no_rinv"):
        for alias in (True, False):
            tag = (situation, alias)
            v = _vectors(n)
            if situation == "rinv_zero":                       # a ray that meets no pixel
                v["inv"][at] = 0.0
                v["inv"][::5] = 0.0
            rinv = None if situation == "no_rinv" else v["inv"]
            want = C.sirt_residual_f32(v["w"], v["b"], rinv)
            dw, db = _dev(eng, v["w"], offset), _dev(eng, v["b"], offset)
            dr = None if rinv is None else _dev(eng, rinv, offset)
            rho = dw if alias else _dev(eng, np.full(n, 7.0, dtype=F32), offset)
            NP = eng.scalars(8 * CAP)
            nb = eng.sirt_residual(dr, dw, db, rho, NP.ref(0), CAP)
            parts, got = NP.host().reshape(CAP, 8), rho.cpu().numpy()
            assert nb == _grid(n), tag
            assert not np.any(np.isnan(parts)) and not np.any(np.isnan(got)), tag
            assert not np.any(parts[:, 2:]) and not np.any(parts[nb:]), tag      # its slots of its blocks' rows only
            assert _ulps(got, want["rho"]) <= 1, tag
            worst = max(worst, _ulps(got, want["rho"]))
            if not alias:
                assert np.array_equal(dw.cpu().numpy().view(np.int32), v["w"].view(np.int32)), tag
            _sum_close(parts[:, 0].sum(), want["dd"], tag + ("dd",))
            _sum_close(parts[:, 1].sum(), want["wd"], tag + ("wd",))
            if situation == "rinv_zero":
                assert np.all(got[v["inv"] == 0] == 0.0) and np.all(got[at] == 0.0), tag
            if situation == "no_rinv":
                assert want["wd"] == want["dd"], tag
    bar(f"sirt_residual_n{n}_off{offset}_ulps", worst, 1.5)


BOXES = {"both_infinite": (-INF, INF), "lower": (0.75, INF), "upper": (-INF, 1.25), "both": (0.75, 1.25)}


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", SIZES)
def test_one_sirt_update_against_the_restatement(eng, n, offset):
    at = _crafted(n)
    worst = 0
    omega = 0.7
    for situation in ("both_infinite", "lower", "upper", "both", "cinv_zero", "no_cinv"):
        lo, hi = BOXES.get(situation, (-INF, INF))
        plain = situation == "both_infinite"
        for with_ref, with_xt in (OPTIONALS if plain else OPTIONALS[::3]):
            for alias in ((True, False) if plain else (False,)):
                tag = (situation, with_ref, with_xt, alias)
                v = _vectors(n)
                v["t"] -= F32(1.0)                             # of either sign: the step goes up and down
                if situation in ("lower", "both"):
                    v["t"][at], v["inv"][at] = -5.0, 1.0       # x - 3.5: far below the lower bound
                if situation == "upper":
                    v["t"][at], v["inv"][at] = 5.0, 1.0        # x + 3.5: far above the upper one
                if situation == "cinv_zero":                   # the subset does not see these unknowns: they do not move
                    v["inv"][at] = 0.0
                    v["inv"][::5] = 0.0
                cinv = None if situation == "no_cinv" else v["inv"]
                want = C.sirt_update_f32(omega, lo, hi, v["x"], v["t"], cinv, v["xr"] if with_ref else None, v["xt"] if with_xt else None)
                d = {k: _dev(eng, v[k], offset) for k in ("x", "t", "inv", "xr", "xt")}
                x_new = d["x"] if alias else _dev(eng, np.full(n, 7.0, dtype=F32), offset)
                NP = eng.scalars(8 * CAP)
                nb = eng.sirt_update(omega, lo, hi, d["x"], d["t"], None if cinv is None else d["inv"], d["xr"] if with_ref else None,
                                     d["xt"] if with_xt else None, x_new, NP.ref(0), CAP)
                got = x_new.cpu().numpy()
                _check_x_launch(tag, NP.host().reshape(CAP, 8), nb, n, got, want, with_xt)
                worst = max(worst, _ulps(got, want["x"]))
                assert got.min() >= F32(lo) and got.max() <= F32(hi), tag
                if situation in ("lower", "both"):
                    assert np.all(got[at] == F32(lo)) and want["count"] >= len(at), tag
                elif situation == "upper":
                    assert np.all(got[at] == F32(hi)) and want["count"] >= len(at), tag
                elif situation == "cinv_zero":
                    kept = v["inv"] == 0
                    assert np.array_equal(got[kept].view(np.int32), v["x"][kept].view(np.int32)) and want["count"] == 0, tag
                else:
                    assert want["count"] == 0, tag             # an infinite bound is never counted
    bar(f"sirt_update_n{n}_off{offset}_ulps", worst, 1.5)


def test_argument_checks_come_first(eng):
    """Bad arguments are refused with trk_last_error's text before anything is launched."""
    v = {k: torch.ones(8, dtype=torch.float32, device=eng.device) for k in ("x", "t", "s", "r", "e", "o", "w", "b")}
    Sc = eng.scalars(8 * CAP)
    # trk_osem_update
    with pytest.raises(ValueError, match="NULL"):
        eng.osem_update(v["x"], v["t"], None, None, None, v["o"], Sc.ref(0), CAP)
    for slot in ("t", "s", "r", "e"):
        with pytest.raises(ValueError, match="alias x only"):
            eng.osem_update(v["x"], v["t"], v["s"], v["r"], v["e"], v[slot], Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="too small"):
        eng.osem_update(v["x"], v["t"], v["s"], None, None, v["o"], Sc.ref(0), 0)
    with pytest.raises(ValueError, match="n >= 1"):
        eng._pdhg("trk_osem_update", 0, v["x"], v["t"], v["s"], None, None, v["o"], Sc.ref(0), CAP)
    # trk_sirt_residual
    with pytest.raises(ValueError, match="NULL"):
        eng.sirt_residual(v["r"], v["w"], None, v["w"], Sc.ref(0), CAP)
    for slot in ("b", "r"):
        with pytest.raises(ValueError, match="alias w only"):
            eng.sirt_residual(v["r"], v["w"], v["b"], v[slot], Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="too small"):
        eng.sirt_residual(None, v["w"], v["b"], v["w"], Sc.ref(0), 0)
    with pytest.raises(ValueError, match="m >= 1"):
        eng._pdhg("trk_sirt_residual", 0, None, v["w"], v["b"], v["o"], Sc.ref(0), CAP)
    # trk_sirt_update
    with pytest.raises(ValueError, match="NULL"):
        eng.sirt_update(1.0, -INF, INF, v["x"], None, v["s"], None, None, v["o"], Sc.ref(0), CAP)
    for slot in ("t", "s", "r", "e"):
        with pytest.raises(ValueError, match="alias x only"):
            eng.sirt_update(1.0, -INF, INF, v["x"], v["t"], v["s"], v["r"], v["e"], v[slot], Sc.ref(0), CAP)
    with pytest.raises(ValueError, match="too small"):
        eng.sirt_update(1.0, -INF, INF, v["x"], v["t"], v["s"], None, None, v["o"], Sc.ref(0), 0)
    with pytest.raises(ValueError, match="n >= 1"):
        eng._pdhg("trk_sirt_update", 0, 1.0, -INF, INF, v["x"], v["t"], v["s"], None, None, v["o"], Sc.ref(0), CAP)
    for omega in (0.0, -1.0, INF, float("nan")):
        with pytest.raises(ValueError, match="omega"):
            eng.sirt_update(omega, -INF, INF, v["x"], v["t"], v["s"], None, None, v["o"], Sc.ref(0), CAP)
    for lo, hi in ((1.0, 0.0), (float("nan"), 1.0), (0.0, float("nan"))):
        with pytest.raises(ValueError, match="lo <= hi"):
            eng.sirt_update(1.0, lo, hi, v["x"], v["t"], v["s"], None, None, v["o"], Sc.ref(0), CAP)
    with pytest.raises(ValueError, match=">= 1"):
        eng.subsets_blocks(0, 8)
    assert not np.any(Sc.host()) and all(float(t.min()) == 1.0 == float(t.max()) for t in v.values())     # nothing ran
    # the loops: their own checks before the first launch
    P = C.problem("P4", True)
    sub = _subsets(eng, "P4", 3)
    m, n = P.shape
    H = [o._h for o in sub.ops]
    w, t, xw, b, x = eng.empty(m), eng.empty(n), eng.empty(n), eng.to_vec(sub.split(P.b)), eng.to_vec(P.x0)
    SINV, X = torch.ones((3, n), dtype=torch.float32, device=eng.device), eng.empty_basis(2, n)
    before = [u.clone() for u in (w, t, xw, X)]

    def osem(handles=H, order=sub.order, row_off=sub.offsets, k_first=1, bg=0.0, x_prev=x, xw=xw, cap=CAP):
        eng.osem_iterate(handles, order, row_off, k_first, 2, bg, b, SINV, w, t, xw, X, False, x_prev, None, Sc.ref(0), cap)

    def sirt(handles=H, order=sub.order, row_off=sub.offsets, k_first=1, omega=1.0, lo=-INF, hi=INF, x_prev=x, xw=xw, cap=CAP):
        eng.sirt_iterate(handles, order, row_off, k_first, 2, b, None, None, omega, lo, hi, w, t, xw, X, False, x_prev, None, Sc.ref(0),
                         cap)
    for loop in (osem, sirt):
        with pytest.raises(ValueError, match="S >= 1"):
            loop(handles=[], order=[], row_off=[0])
        for order in ([0, 1, 1], [0, 1, 3], [-1, 0, 1]):
            with pytest.raises(ValueError, match="not a permutation"):
                loop(order=order)
        with pytest.raises(ValueError, match="increasing"):
            loop(row_off=[0, 50, 50, 150])
        with pytest.raises(ValueError, match="row_off"):
            loop(row_off=[0, 40, 100, 150])                    # increasing, but not the rows of the subsets
        with pytest.raises(ValueError, match="start at 0"):
            loop(row_off=[1, 51, 101, 151])
        with pytest.raises(ValueError, match="NULL operator"):
            loop(handles=[H[0], None, H[2]])
        with pytest.raises(ValueError, match="too small"):
            loop(cap=0)
        with pytest.raises(ValueError, match="k_first"):
            loop(k_first=0)
        with pytest.raises(ValueError, match="scratch iterate"):
            loop(xw=None)
        with pytest.raises(ValueError, match="scratch iterate"):
            loop(xw=x)
        with pytest.raises(ValueError, match="NULL argument"):
            loop(x_prev=None)
    with pytest.raises(ValueError, match="background"):
        osem(bg=-2.0)
    with pytest.raises(ValueError, match="omega"):
        sirt(omega=0.0)
    with pytest.raises(ValueError, match="lo <= hi"):
        sirt(lo=1.0, hi=0.0)
    assert not np.any(Sc.host()) and all(torch.equal(a, c) for a, c in zip(before, (w, t, xw, X)))


# ====================================================================== the one-call loops against single steps
K = 12
_subs = {}


def _subsets(eng, name, S_):
    """The RowSubsets of a problem's device operator, made once (the handles are shared by the tests of this module)."""
    from trips_py_amd.operators import RowSubsets
    if (name, S_) not in _subs:
        _subs[(name, S_)] = RowSubsets(C.problem(name, False).device(eng), S_)
    return _subs[(name, S_)]


def _make_run(eng, kind, name, S_, iters, x_true, history):
    from trips_py_amd.solvers import OSEMRun, SIRTRun
    P = C.problem(name, kind == "osem")
    sub = _subsets(eng, name, S_)
    xt = P.x_true if x_true else None
    if kind == "osem":
        bg = np.full(P.shape[0], P.bg) if S_ == 5 else P.bg                 # one case through the (subset-major) background vector
        return OSEMRun(None, P.b, P.x0, iters, xt, history, bg, sub)
    lo, hi = (0.0, 0.2 * float(P.x_true.max())) if S_ in (5, 3) else (-INF, INF)
    return SIRTRun(None, P.b, None, iters, xt, history, sub, relax=1.5, lower=lo, upper=hi)


def _bits(run):
    run.rows()
    vecs = [v.clone() for v in (run.x_cur, run.w, run.t)]
    return vecs, run.SS.host().view(np.int64).copy(), run.NP.host().view(np.int64).copy()


@pytest.mark.parametrize("history", [True, False, 3])
@pytest.mark.parametrize("name,S_", [("P3", 1), ("P3", 5), ("P3", 12), ("P4", 3), ("F1", 3)])
@pytest.mark.parametrize("kind", ["osem", "sirt"])
def test_run_equals_steps(eng, kind, name, S_, history):
    ref = _make_run(eng, kind, name, S_, K, True, history)
    for _ in range(K):
        ref.step()
    want_vecs, want_S, want_NP = _bits(ref)
    assert np.all(np.isfinite(ref.rows())) and ref.substep_rows().shape == (K, S_, 8)
    for calls in ([K], [1, K - 1], [3, 5, K - 8]):
        run = _make_run(eng, kind, name, S_, K, True, history)
        assert run._c_loop() is not None
        for c in calls:
            run.run(c)
        assert run.k == K
        vecs, S, NP = _bits(run)
        for key, a, b in zip("xwt", vecs, want_vecs):
            assert torch.equal(a, b), (calls, key)
        assert np.array_equal(S, want_S) and np.array_equal(NP, want_NP), calls
    if history is True:
        assert all(torch.equal(ref.slot(k), run.slot(k)) for k in range(K))


@pytest.mark.parametrize("name", ["P3", "P4"])
def test_osem_with_one_subset_is_mlem_bit_for_bit(eng, name):
    """Ties the new loop to the pinned one: every pixel is seen there, so the keep rule never acts and OSEMRun with S = 1 issues
    MLEM's arithmetic — the iterates and the rows are MLEMRun's, bit for bit, stepping and in one call."""
    from trips_py_amd.solvers import MLEMRun, OSEMRun
    P = C.problem(name, True)
    o = P.oracle()
    assert np.all(o.rmatvec(np.ones(P.shape[0])) > 0)                       # every pixel is seen
    A = P.device(eng)
    ref = MLEMRun(A, P.b, P.x0, K, P.x_true, background=P.bg)
    ref.run(K)
    for stepping in (False, True):
        run = OSEMRun(A, P.b, P.x0, K, P.x_true, True, P.bg, 1)
        if stepping:
            for _ in range(K):
                run.step()
        else:
            run.run(K)
        assert float(run.SINV.min()) > 0
        assert all(torch.equal(ref.slot(k), run.slot(k)) for k in range(K))
        assert np.array_equal(ref.rows().view(np.int64), run.rows().view(np.int64))
        assert torch.equal(ref.w, run.w) and torch.equal(ref.t, run.t)


# ====================================================================== whole solves against float64
ITERS = 30
CASES = [(n, s) for n in C.SUBSETS for s in C.SUBSETS[n]]
# The worst relative 2-norm distance of the storage-faithful restatement (os_cases.osem_f32 / sirt_f32) from the float64 one over 30
# passes, measured in NumPy on a CPU on the float64 operator of every subset — what fp32 storage alone costs — and, in the same two
# runs, the worst relative deviation of the running KL and of the running residual.  OSEM from the problem's x0:
CPU_F32_OSEM_X = {("P3", 1): 3.51e-07, ("P3", 2): 2.76e-07, ("P3", 3): 3.73e-07, ("P3", 5): 2.99e-07, ("P3", 12): 1.78e-07,
                  ("P4", 1): 3.31e-07, ("P4", 3): 2.63e-07, ("F1", 1): 2.58e-07, ("F1", 3): 2.01e-07}
CPU_F32_OSEM_KL = {("P3", 1): 5.37e-08, ("P3", 2): 8.11e-08, ("P3", 3): 6.34e-08, ("P3", 5): 5.42e-08, ("P3", 12): 5.86e-08,
                   ("P4", 1): 3.17e-07, ("P4", 3): 8.77e-07, ("F1", 1): 4.18e-07, ("F1", 3): 3.41e-07}
CPU_F32_OSEM_R = {("P3", 1): 8.80e-08, ("P3", 2): 5.90e-08, ("P3", 3): 6.31e-08, ("P3", 5): 6.06e-08, ("P3", 12): 7.14e-08,
                  ("P4", 1): 1.53e-07, ("P4", 3): 4.72e-07, ("F1", 1): 6.69e-07, ("F1", 3): 5.39e-07}
# SIRT with relax = 1 from zeros, no box: iterates, running residual, running weighted residual ...
CPU_F32_SIRT_X = {("P3", 1): 1.05e-07, ("P3", 2): 1.62e-07, ("P3", 3): 1.53e-07, ("P3", 5): 2.46e-07, ("P3", 12): 3.18e-07,
                  ("P4", 1): 9.86e-08, ("P4", 3): 1.35e-07, ("F1", 1): 9.53e-08, ("F1", 3): 1.80e-07}
CPU_F32_SIRT_R = {("P3", 1): 5.89e-08, ("P3", 2): 3.99e-07, ("P3", 3): 2.45e-07, ("P3", 5): 2.02e-07, ("P3", 12): 5.00e-07,
                  ("P4", 1): 9.62e-08, ("P4", 3): 1.80e-07, ("F1", 1): 1.06e-07, ("F1", 3): 2.85e-07}
CPU_F32_SIRT_W = {("P3", 1): 1.21e-07, ("P3", 2): 8.51e-07, ("P3", 3): 5.23e-07, ("P3", 5): 4.86e-07, ("P3", 12): 9.06e-07,
                  ("P4", 1): 1.44e-07, ("P4", 3): 2.03e-07, ("F1", 1): 1.93e-07, ("F1", 3): 3.67e-07}
# ... and in the box 0 <= x <= 0.2 max(x_true), whose upper bound is active:
CPU_F32_BOX_X = {("P3", 1): 7.15e-08, ("P3", 2): 7.27e-08, ("P3", 3): 8.44e-08, ("P3", 5): 9.88e-08, ("P3", 12): 7.89e-08,
                 ("P4", 1): 5.63e-08, ("P4", 3): 4.40e-08, ("F1", 1): 6.79e-08, ("F1", 3): 9.46e-08}
CPU_F32_BOX_R = {("P3", 1): 4.43e-08, ("P3", 2): 5.83e-08, ("P3", 3): 6.95e-08, ("P3", 5): 6.45e-08, ("P3", 12): 6.32e-08,
                 ("P4", 1): 3.97e-08, ("P4", 3): 3.90e-08, ("F1", 1): 4.17e-08, ("F1", 3): 3.62e-08}
CPU_F32_BOX_W = {("P3", 1): 9.69e-08, ("P3", 2): 1.30e-07, ("P3", 3): 1.32e-07, ("P3", 5): 1.28e-07, ("P3", 12): 1.19e-07,
                 ("P4", 1): 7.54e-08, ("P4", 3): 7.12e-08, ("F1", 1): 7.29e-08, ("F1", 3): 6.57e-08}


def _limit(cpu_figure):
    """8 x the cost of fp32 storage alone, never below 1e-5 (the rule of the MRNSD, PDHG and MLEM bars)."""
    return max(8 * cpu_figure, 1e-5)


def _float64_pairs(eng, name, S_):
    """Per subset (matvec, rmatvec) in float64: the oracle's operator of the subset's own angles (Radon, fan-beam), or the subset
    handle's own dense matrices (sparse; the "transpose" is the handle's too)."""
    if name != "P4":
        return C.dense_pairs(name, S_)
    out = []
    for op in _subsets(eng, name, S_).ops:
        M, Mt = op.todense(), op.T.todense()
        out.append(((lambda v, M=M: M @ v), (lambda v, Mt=Mt: Mt @ v)))
    return out


def _worst(H, X):
    return max(np.linalg.norm(h - xr) / np.linalg.norm(xr) for h, xr in zip(H, X))


@pytest.mark.parametrize("name,S_", CASES)
def test_osem_solve_against_float64(eng, name, S_):
    from trips_py_amd.solvers import OSEM
    P, key, tag = C.problem(name, True), (name, S_), f"osem_{name}_S{S_}"
    sub = _subsets(eng, name, S_)
    pairs, rows, order = _float64_pairs(eng, name, S_), C.subset_rows(name, S_), C.bitrev_order(S_)
    assert sub.order == order and all(np.array_equal(a, b) for a, b in zip(sub.rows, rows))
    ref = C.osem_f64(pairs, rows, order, P.b, P.x0, ITERS, P.bg)
    faithful = C.osem_f32(pairs, rows, order, P.b, P.x0, ITERS, P.bg)
    x, info = OSEM(sub.A, P.b, P.x0, ITERS, 0, x_true=P.x_true, subsets=sub, background=P.bg)
    assert info["its"] == ITERS and info["subsets"] == S_ and len(info["xHistory"]) == ITERS
    H = [h.reshape(-1) for h in info["xHistory"]]
    assert all(float(h.min()) >= 0.0 and np.all(np.isfinite(h)) for h in H)
    bar(f"{tag}_iterates_vs_float64", _worst(H, ref["X"]), _limit(CPU_F32_OSEM_X[key]))
    bar(f"{tag}_KL_vs_float64", C.worst_scalar(info["KL"], ref["kl"]), _limit(CPU_F32_OSEM_KL[key]))
    bar(f"{tag}_Rnrm_vs_float64", C.worst_scalar(info["Rnrm"], np.sqrt(ref["rr"]) / np.linalg.norm(P.b)), _limit(CPU_F32_OSEM_R[key]))
    assert np.allclose(info["relError"], [np.linalg.norm(xr - P.x_true) / np.linalg.norm(P.x_true) for xr in ref["X"]], rtol=1e-4)
    assert np.allclose(info["relResidual"], np.sqrt(np.array(ref["dd"]) / np.array(ref["xx"])), rtol=1e-3)
    assert info["zeros"] == [int(np.count_nonzero(h == 0)) for h in H]
    assert info["zeros"] == faithful["zeros"]
    # objectiveFinal: KL over all the data at the returned x
    xl = ref["X"][-1]
    kl = sum(float(np.sum(LC.kl_terms(P.b[r], mv(xl) + P.bg))) for (mv, _), r in zip(pairs, rows))
    bar(f"{tag}_objectiveFinal_vs_float64", abs(info["objectiveFinal"] / kl - 1), _limit(CPU_F32_OSEM_KL[key]))


@pytest.mark.parametrize("box", [False, True], ids=["plain", "box"])
@pytest.mark.parametrize("name,S_", CASES)
def test_sirt_solve_against_float64(eng, name, S_, box):
    from trips_py_amd.solvers import SIRT
    P, key = C.problem(name, False), (name, S_)
    tag = f"sirt_{'box_' if box else ''}{name}_S{S_}"
    lo, hi = (0.0, 0.2 * float(P.x_true.max())) if box else (-INF, INF)
    TX, TR, TW = (CPU_F32_BOX_X, CPU_F32_BOX_R, CPU_F32_BOX_W) if box else (CPU_F32_SIRT_X, CPU_F32_SIRT_R, CPU_F32_SIRT_W)
    sub = _subsets(eng, name, S_)
    pairs, rows, order = _float64_pairs(eng, name, S_), C.subset_rows(name, S_), C.bitrev_order(S_)
    z = np.zeros(P.shape[1])
    ref = C.sirt_f64(pairs, rows, order, P.b, z, ITERS, 1.0, lo, hi)
    faithful = C.sirt_f32(pairs, rows, order, P.b, z, ITERS, 1.0, lo, hi)
    x, info = SIRT(sub.A, P.b, None, ITERS, 0, x_true=P.x_true, subsets=sub, lower=lo, upper=hi)
    assert info["its"] == ITERS and info["subsets"] == S_ and len(info["xHistory"]) == ITERS
    H = [h.reshape(-1) for h in info["xHistory"]]
    assert all(np.all(np.isfinite(h)) and h.min() >= lo and h.max() <= float(F32(hi)) for h in H)
    bar(f"{tag}_iterates_vs_float64", _worst(H, ref["X"]), _limit(TX[key]))
    bar(f"{tag}_Rnrm_vs_float64", C.worst_scalar(info["Rnrm"], np.sqrt(ref["rr"]) / np.linalg.norm(P.b)), _limit(TR[key]))
    bar(f"{tag}_weightedResidual_vs_float64", C.worst_scalar(info["weightedResidual"], ref["wr"]), _limit(TW[key]))
    assert np.allclose(info["relError"], [np.linalg.norm(xr - P.x_true) / np.linalg.norm(P.x_true) for xr in ref["X"]], rtol=1e-4)
    hi32 = float(F32(hi))
    assert info["atBound"] == [int(np.count_nonzero((h == lo) | (h == hi32))) for h in H]       # (no iterate is infinite)
    assert info["atBound"] == faithful["at_bound"]
    if box:
        assert info["atBound"][-1] > 0 and any(float(h.max()) == hi32 for h in H)           # the upper bound is active


def test_sart_is_sirt_with_one_view_per_subset(eng):
    from trips_py_amd.solvers import SART, SIRT
    P = C.problem("P3", False)
    A = P.device(eng)
    xa, ia = SART(A, P.b, None, 4, 0, relax=0.8)
    xb, ib = SIRT(A, P.b, None, 4, 0, subsets=12, relax=0.8)
    assert np.array_equal(xa, xb) and ia["subsets"] == 12 and ia["Rnrm"] == ib["Rnrm"]
    from trips_py_amd.operators import Blur2D, RowSubsets
    B = Blur2D(np.ones((3, 3)) / 9.0, 8, 8, engine=eng)
    with pytest.raises(ValueError, match="no views"):
        SART(B, np.ones(64), None, 2, 0)
    with pytest.raises(ValueError, match="no views or rows"):
        RowSubsets(B, 2)
    with pytest.raises(ValueError, match="views of the operator"):
        RowSubsets(A, 13)
    assert RowSubsets(B, 1).ops == [B]


def test_landweber_on_the_device(eng):
    """weights=None: the step relax / ||A||^2 with the engine's own norm estimate; the residual falls monotonically."""
    from trips_py_amd.solvers import SIRT
    P = C.problem("P4", False)
    A = P.device(eng)
    M = A.todense()
    x, info = SIRT(A, P.b, None, 10, 0, weights=None)
    from trips_py_amd.operators import operator_norm_sq
    step = float(F32(1.0 / operator_norm_sq(A)))
    xr = np.zeros(P.shape[1])
    for _ in range(10):
        xr = xr + step * (M.T @ (P.b - M @ xr))
    bar("landweber_P4_vs_float64", np.linalg.norm(x.reshape(-1) - xr) / np.linalg.norm(xr), 1e-5)
    assert np.all(np.diff(info["Rnrm"]) < 0) and info["atBound"] == [0] * 10


def test_tol_delta_and_history_off_on_the_device(eng):
    """tol > 0 and delta read a row back every pass and stop where the tol = 0 run's rows say; delta returns that pass's iterate."""
    from trips_py_amd.solvers import OSEM, SIRT
    for kind in ("osem", "sirt"):
        P = C.problem("P3", kind == "osem")
        sub = _subsets(eng, "P3", 5)
        run = _make_run(eng, kind, "P3", 5, ITERS, False, True)
        run.run(ITERS)
        rows = run.rows()

        def solve(tol, **kw):
            if kind == "osem":
                return OSEM(sub.A, P.b, P.x0, ITERS, tol, subsets=sub, background=np.full(P.shape[0], P.bg), **kw)
            return SIRT(sub.A, P.b, None, ITERS, tol, subsets=sub, relax=1.5, lower=0.0, upper=0.2 * float(P.x_true.max()), **kw)
        rel = np.sqrt(rows[:, 5] / rows[:, 4])
        tol = float(rel[7]) * (1 + 1e-9)
        hit = int(np.nonzero(rel <= tol)[0][0]) + 1
        assert 1 < hit < ITERS
        x, info = solve(tol, history=False)
        assert info["its"] == hit and info["xHistory"] == []
        assert np.array_equal(x.reshape(-1), run.slot(hit - 1).cpu().numpy().astype(np.float64))
        res = np.sqrt(rows[:, 1 if kind == "osem" else 0])
        delta = res[9] / 1.01 * (1 + 1e-9)
        k = int(np.nonzero(res <= 1.01 * delta)[0][0]) + 1
        assert 1 < k <= 10
        for history in (True, False):
            x, info = solve(0, history=history, delta=delta)
            assert info["its"] == k and len(info["Rnrm"]) == k
            assert np.array_equal(x.reshape(-1), run.slot(k - 1).cpu().numpy().astype(np.float64))


def test_stacked_subsets_apply_as_the_permuted_operator(eng):
    """RowSubsets as an operator is the subset-major stack: A[perm] of the float64 operator, to the projector's own accuracy."""
    P = C.problem("P3", False)
    sub = _subsets(eng, "P3", 5)
    M = np.asarray(P.oracle().todense())[sub.perm]
    x = np.random.default_rng(5).random(P.shape[1])
    y = np.random.default_rng(6).random(P.shape[0])
    assert np.linalg.norm(sub.matvec(x) - M @ x) <= 1e-5 * np.linalg.norm(M @ x)
    assert np.linalg.norm(sub.rmatvec(y) - M.T @ y) <= 1e-5 * np.linalg.norm(M.T @ y)
