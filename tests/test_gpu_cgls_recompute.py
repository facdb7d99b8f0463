"""The large-image CGLS loop that recomputes A p and A^T r instead of storing them (trk_cgls_iterate_recompute) and its parts:
the blur's norm-only pass (trk_op_apply_sumsq_raw), its epilogue with a coefficient taken from raw block partials
(trk_op_apply_ratio), the x-only batched update — against the launches they replace.  The new kernels do the same fp32 operations
in the same order on every entry, so every comparison here is exact."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 21
X_BATCH_MIN_N = 8 << 20          # trk_cgls_x_batch: off below this many unknowns
PCAP = 4096
MODES = ["reflect", "constant", "nearest", "mirror", "wrap"]
# 16x16; the narrowest ny the sliding kernel takes; a second, mostly empty span and a partial last band; fifteen 10-row bands (9x9),
# the odd ones marching upward, two spans
IMAGES = [(16, 16), (10, 8), (37, 264), (150, 512)]


def _sep_psf(k, seed):
    """A separable k x k PSF without any symmetry: forward and "transpose" weights differ, rows and columns differ."""
    rng = np.random.default_rng(seed)
    c, r = rng.uniform(0.2, 1.0, k), rng.uniform(0.2, 1.0, k)
    return np.outer(c / c.sum(), r / r.sum())


def _blur(k, nx, ny, mode):
    from trips_py_amd.operators import Blur2D
    A = Blur2D(_sep_psf(k, 3 * k + nx), nx, ny, boundary=mode)
    assert A.engine.op_can_fuse(A._h) == 1 and A.engine.op_can_recompute(A._h) == 1
    return A


def _randn(eng, n, seed):
    return torch.randn(n, device=eng.device, generator=torch.Generator(device=eng.device).manual_seed(seed))


def _apply_raw(A, tr, x, P):
    """y = Op(x) by the storing kernel, ||y||^2 left as raw block partials in P; returns (y, count)."""
    eng = A.engine
    y = eng.empty(x.numel())
    n = eng.op_apply_fused(A._h, tr, x, None, 0.0, None, 0, None, 0, None, y, P.ref(0), PCAP)
    return y, n


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [3, 5, 7, 9])
def test_norm_only_partials_equal_the_storing_kernels(k, mode):
    for nx, ny in IMAGES:
        A = _blur(k, nx, ny, mode)
        eng = A.engine
        x = _randn(eng, nx * ny, 5 + nx)
        for tr in (False, True):
            P1, P2 = eng.scalars(PCAP), eng.scalars(PCAP)
            P2.t.fill_(-1.0)
            _y, n1 = _apply_raw(A, tr, x, P1)
            n2 = eng.op_apply_sumsq_raw(A._h, tr, x, P2.ref(0), PCAP)
            assert n1 == n2 and n1 >= 1, (nx, ny, tr)
            assert torch.equal(P1.t[:n1], P2.t[:n2]), (nx, ny, tr)
            assert torch.all(P2.t[n2:] == -1.0), (nx, ny, tr)              # nothing beyond the counted partials is written
            assert float(P2.t[:n2].sum()) > 0.0


def _p_update_to(eng, t, p, p_out, gnew, gnew_n, gold, pub):
    rc = eng.lib.trk_cgls_p_update_to(p.numel(), t.data_ptr(), p.data_ptr(), p_out.data_ptr(), gnew, int(gnew_n), gold, pub,
                                      eng.stream())
    assert rc == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [3, 5, 7, 9])
def test_ratio_epilogue_equals_apply_then_update(k, mode):
    """r <- r - (gamma_old / S(delta)) (A p) against apply + trk_cgls_r_update, p' <- (A^T r) + (S(gamma) / gamma_old) p against
    apply + trk_cgls_p_update_to: in place and out of place, the partials-fed operand raw (the norm-only pass's own partials) and as
    one finished scalar, both directions; the published scalar is the update kernel's."""
    for nx, ny in IMAGES:
        A = _blur(k, nx, ny, mode)
        eng = A.engine
        n = nx * ny
        x, z0 = _randn(eng, n, 7 + nx), _randn(eng, n, 8 + nx)
        for tr in (False, True):
            P, Pn = eng.scalars(PCAP), eng.scalars(PCAP)
            y, n_p = _apply_raw(A, tr, x, P)
            assert eng.op_apply_sumsq_raw(A._h, tr, x, Pn.ref(0), PCAP) == n_p
            S = eng.scalars(8)                      # 0: gamma_old, 1: the finished sum, 2 / 3: published by reference / by the new kernel
            S.set(0, [0.37])
            S.set(1, [float(P.t[:n_p].sum())])
            for src, src_n in ((Pn.ref(0), n_p), (S.ref(1), 1)):
                # ---- the residual's form: coefficient on the product, negative, the partials in the denominator
                r_ref = z0.clone()
                eng.cgls_r_update(S.ref(0), src, src_n, r_ref, y, S.ref(2))
                for in_place in (True, False):
                    S.set(3, [-1.0])
                    z = z0.clone()
                    out = z if in_place else eng.empty(n)
                    eng.op_apply_ratio(A._h, tr, x, False, -1.0, S.ref(0), 1, src, src_n, z, out, S.ref(3), True)
                    assert torch.equal(out, r_ref), (nx, ny, tr, src_n, in_place, "r")
                    if not in_place:
                        assert torch.equal(z, z0)
                    h = S.host(2, 4)
                    assert h[0] == h[1], (nx, ny, tr, src_n, in_place, "delta")
                # ---- the direction's form: coefficient on z, the partials in the numerator
                p_ref = eng.empty(n)
                _p_update_to(eng, y, z0, p_ref, src, src_n, S.ref(0), S.ref(2))
                p_ref2 = z0.clone()
                eng.cgls_p_update(y, p_ref2, src, src_n, S.ref(0), S.ref(2))
                assert torch.equal(p_ref, p_ref2)
                for in_place in (True, False):
                    S.set(3, [-1.0])
                    z = z0.clone()
                    out = z if in_place else eng.empty(n)
                    eng.op_apply_ratio(A._h, tr, x, True, 1.0, src, src_n, S.ref(0), 1, z, out, S.ref(3), False)
                    assert torch.equal(out, p_ref), (nx, ny, tr, src_n, in_place, "p")
                    if not in_place:
                        assert torch.equal(z, z0)
                    h = S.host(2, 4)
                    assert h[0] == h[1], (nx, ny, tr, src_n, in_place, "gamma")


def test_ratio_refuses_aliasing_the_operand():
    A = _blur(9, 16, 16, "reflect")
    eng = A.engine
    x, z = _randn(eng, 256, 1), _randn(eng, 256, 2)
    S = eng.scalars(2)
    S.set(0, [1.0, 2.0])
    with pytest.raises(ValueError):
        eng.op_apply_ratio(A._h, False, x, False, -1.0, S.ref(0), 1, S.ref(1), 1, z, x)
    with pytest.raises(ValueError):
        eng.op_apply_ratio(A._h, False, x, True, 1.0, S.ref(0), 1, S.ref(1), 1, x, z)


# ------------------------------------------------------------------------------------------------------------ the loop
def _problem(shape, with_xt, x0_kind, seed=11):
    from trips_py_amd.operators import Blur2D
    from trips_py_amd.problems import gauss_psf
    nx, ny = shape
    A = Blur2D(gauss_psf((9, 9), (3, 3))[0], nx, ny)
    rng = np.random.default_rng(seed + nx)
    b = rng.standard_normal(nx * ny)
    xt = rng.standard_normal(nx * ny) if with_xt else None
    x0 = np.zeros(nx * ny) if x0_kind == "zero" else np.asarray(A.T @ b.reshape(-1, 1)).reshape(-1)
    return A, b, x0, xt


def _state(run):
    return [v.clone() for v in (run.x_cur, run.p, run.r)]


@functools.lru_cache(maxsize=1)
def _reference(shape, with_xt, x0_kind):
    """Stepwise, one x update per iteration (the reference of tests/test_gpu_cgls_xbatch.py): the problem, the state after every
    iteration, gamma_0 and the rows.  Computed once per problem and shared by the values of s; never modified."""
    from trips_py_amd.solvers import CGLSRun
    A, b, x0, xt = _problem(shape, with_xt, x0_kind)
    ref = CGLSRun(A, b, x0, K, xt, history=False, defer_norms=True, grouping=1, x_batch=1, recompute=False)
    assert ref.raw and ref.grouping == 1 and ref.x_batch == 1 and not ref.recompute
    states = []
    for _ in range(K):
        ref.step()
        states.append(_state(ref))
    g0, rows = ref.rows()
    return (A, b, x0, xt), states, g0, rows.copy()


def _partitions(s):
    """Calls of run() that add up to K; 'step' = single step() calls."""
    return [[K], [1, K - 1], [s, s + 1, K - 2 * s - 1], [3, 5, 13], [5] + ["step"] * (K - 5)]


@pytest.mark.parametrize("s", [1, 3, 8])
@pytest.mark.parametrize("x0_kind", ["zero", "ATb"])
@pytest.mark.parametrize("with_xt", [True, False])
@pytest.mark.parametrize("shape", [(64, 64), (520, 520), (1000, 1000), (100, 264)])
def test_recompute_loop_equals_stepwise(shape, with_xt, x0_kind, s):
    from trips_py_amd.solvers import CGLSRun
    (A, b, x0, xt), states, g0, rows = _reference(shape, with_xt, x0_kind)
    for calls in _partitions(s):
        run = CGLSRun(A, b, x0, K, xt, history=False, defer_norms=True, grouping=1, x_batch=s, recompute=True)
        assert run.recompute and run.x_batch == s
        for c in calls:
            if c == "step":
                run.step()
            else:
                run.run(c)
            for name, got, want in zip(("x_cur", "p", "r"), _state(run), states[run.k - 1]):
                assert torch.equal(got, want), (calls, run.k, name)
        assert run.k == K
        g0_b, rows_b = run.rows()
        assert g0_b == g0, calls
        assert np.array_equal(rows_b, rows), calls
        if not with_xt:
            assert np.all(rows_b[:, 4] == 0.0)


# ------------------------------------------------------------------------------------------------------------ rule and fall-backs
def test_rule():
    from trips_py_amd.engine import default_engine
    eng = default_engine()
    for n in (1, 64 * 64, 1 << 20, 2048 * 2048, X_BATCH_MIN_N - 1):
        assert eng.cgls_recompute(n) == 0, n
    for e in range(0, 34):
        for n in ((1 << e) - 1, 1 << e, 3 << e):
            on = eng.cgls_recompute(max(1, n))
            assert on in (0, 1), n
            if on:
                assert eng.cgls_x_batch(n) > 1, n        # never on where the x-batch form is off


def _run_all(run):
    run.run(K)
    g0, rows = run.rows()
    return run.x_cur.clone(), run.p.clone(), run.r.clone(), run.t.clone(), run.w.clone(), g0, rows.copy()


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a[:5], b[:5])) and a[5] == b[5] and np.array_equal(a[6], b[6])


def test_fallbacks_keep_todays_path():
    """history=True, grouping=0, finished scalars: asking for the recompute loop changes nothing — the form stays off and run() leaves
    the bits (w and t included) it leaves without the request."""
    from trips_py_amd.solvers import CGLSRun
    A, b, x0, xt = _problem((64, 64), True, "zero")
    for kw in (dict(history=True, defer_norms=True, grouping=1), dict(history=False, defer_norms=True, grouping=0),
               dict(history=False, defer_norms=False)):
        r1 = CGLSRun(A, b, x0, K, xt, x_batch=8, **kw)
        r2 = CGLSRun(A, b, x0, K, xt, x_batch=8, recompute=True, **kw)
        assert not r1.recompute and not r2.recompute and r2.x_batch == 1, kw
        assert _same(_run_all(r1), _run_all(r2)), kw
        if kw["history"] is True:
            assert torch.equal(r1.X, r2.X)
    # an explicit x_batch below the rule's threshold without recompute=True: the x-batch loop as it was (t and w are its own)
    r3 = CGLSRun(A, b, x0, K, xt, history=False, defer_norms=True, grouping=1, x_batch=3)
    r4 = CGLSRun(A, b, x0, K, xt, history=False, defer_norms=True, grouping=1, x_batch=3, recompute=False)
    assert not r3.recompute and not r4.recompute and r3.x_batch == 3
    assert _same(_run_all(r3), _run_all(r4))


def test_operator_without_the_capability_keeps_todays_path():
    from trips_py_amd.operators import Radon2DParallel
    from trips_py_amd.solvers import CGLSRun
    A = Radon2DParallel(64, np.linspace(0, np.pi, 30, endpoint=False))
    eng = A.engine
    assert eng.op_can_fuse(A._h) == 2 and eng.op_can_recompute(A._h) == 0
    m, n = A.shape
    rng = np.random.default_rng(3)
    b, x0 = rng.standard_normal(m), np.zeros(n)
    r1 = CGLSRun(A, b, x0, K, None, history=False, defer_norms=True, grouping=1, x_batch=3)
    r2 = CGLSRun(A, b, x0, K, None, history=False, defer_norms=True, grouping=1, x_batch=3, recompute=True)
    assert r1.raw and r1.x_batch == 3 and not r1.recompute and not r2.recompute
    assert _same(_run_all(r1), _run_all(r2))
    P = eng.scalars(PCAP)
    with pytest.raises(NotImplementedError):
        eng.op_apply_sumsq_raw(A._h, False, r1.p, P.ref(0), PCAP)


def test_full_size_rule_selected():
    """The benchmark's shape: 4096^2, no x_true, run(10) then run(100); the rule's choice against the one-update loop that stores
    w and t."""
    from trips_py_amd.operators import Blur2D
    from trips_py_amd.problems import gauss_psf
    from trips_py_amd.solvers import CGLSRun
    N = 4096
    A = Blur2D(gauss_psf((9, 9), (3, 3))[0], N, N)
    eng = A.engine
    dev = eng.device
    b = torch.randn(N * N, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    x0 = torch.zeros(N * N, device=dev)
    out = []
    for kw in (dict(recompute=False, x_batch=1), dict()):
        run = CGLSRun(A, b, x0, 110, None, history=False, defer_norms=True, **kw)
        assert run.grouping == 1
        if not kw:
            assert run.x_batch == eng.cgls_x_batch(N * N) and run.recompute == bool(eng.cgls_recompute(N * N))
        run.run(10)
        run.run(100)
        g0, rows = run.rows()
        out.append((run.x_cur.clone(), run.p.clone(), g0, rows.copy()))
        del run
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and np.array_equal(out[0][3], out[1][3])
    assert np.all(np.isfinite(out[0][3])) and bool(torch.all(torch.isfinite(out[1][0])))
