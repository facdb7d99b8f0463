"""The history-less CGLS iteration with its x updates made s at a time (trk_cgls_iterate_xbatch: trk_cgls_p_update_to into a ring of
directions, trk_cgls_xs_update every s-th iteration and at the end of a call) against the one-update launches of `step()`.
The batched kernel does the same fp32 operations in the same order, so every comparison here is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 21
X_BATCH_MIN_N = 8 << 20          # trk_cgls_x_batch: off below this many unknowns
X_BATCH_MAX = 8


def _problem(N, with_xt, x0_kind, seed=11):
    from trips_py_amd.operators import Blur2D
    from trips_py_amd.problems import gauss_psf
    A = Blur2D(gauss_psf((9, 9), (3, 3))[0], N, N)
    rng = np.random.default_rng(seed + N)
    b = rng.standard_normal(N * N)
    xt = rng.standard_normal(N * N) if with_xt else None
    x0 = np.zeros(N * N) if x0_kind == "zero" else np.asarray(A.T @ b.reshape(-1, 1)).reshape(-1)
    return A, b, x0, xt


def _state(run):
    return [v.clone() for v in (run.x_cur, run.p, run.r, run.t, run.w)]


def _reference(A, b, x0, xt, iters=K):
    """Stepwise, one x update per iteration: the state after every iteration, the rows and gamma_0."""
    from trips_py_amd.solvers import CGLSRun
    ref = CGLSRun(A, b, x0, iters, xt, history=False, defer_norms=True, grouping=1, x_batch=1)
    assert ref.raw and ref.grouping == 1 and ref.x_batch == 1
    states = []
    for _ in range(iters):
        ref.step()
        states.append(_state(ref))
    g0, rows = ref.rows()
    return states, g0, rows.copy()


def _partitions(s):
    """Calls of run() that add up to K; 'step' = single step() calls."""
    return [[K], [1, K - 1], [s, s + 1, K - 2 * s - 1], [3, 5, 13], [5] + ["step"] * (K - 5)]


@pytest.mark.parametrize("x0_kind", ["zero", "ATb"])
@pytest.mark.parametrize("with_xt", [True, False])
@pytest.mark.parametrize("s", [2, 3, 4, 8])
@pytest.mark.parametrize("N", [64, 520, 1000])
def test_xbatch_equals_stepwise(N, s, with_xt, x0_kind):
    from trips_py_amd.solvers import CGLSRun
    A, b, x0, xt = _problem(N, with_xt, x0_kind)
    states, g0, rows = _reference(A, b, x0, xt)
    for calls in _partitions(s):
        run = CGLSRun(A, b, x0, K, xt, history=False, defer_norms=True, grouping=1, x_batch=s)
        assert run.x_batch == s and run.P_ring.shape[0] == s - 1
        for c in calls:
            if c == "step":
                run.step()
            else:
                run.run(c)
            for name, got, want in zip(("x_cur", "p", "r", "t", "w"), _state(run), states[run.k - 1]):
                assert torch.equal(got, want), (calls, run.k, name)
        assert run.k == K
        g0_b, rows_b = run.rows()
        assert g0_b == g0, calls
        assert np.array_equal(rows_b, rows), calls
        if not with_xt:
            assert np.all(rows_b[:, 4] == 0.0)


def test_history_keeps_the_form_off():
    from trips_py_amd.solvers import CGLSRun
    A, b, x0, xt = _problem(64, True, "zero")
    r1 = CGLSRun(A, b, x0, K, xt, history=True, defer_norms=True, grouping=1)
    r2 = CGLSRun(A, b, x0, K, xt, history=True, defer_norms=True, grouping=1, x_batch=8)
    assert r2.x_batch == 1 and r2.P_ring is None
    r1.run(K)
    r2.run(K)
    assert torch.equal(r1.X, r2.X)
    (g1, rows1), (g2, rows2) = r1.rows(), r2.rows()
    assert g1 == g2 and np.array_equal(rows1, rows2)
    # other groupings and finished scalars: off as well
    r3 = CGLSRun(A, b, x0, K, xt, history=False, defer_norms=True, grouping=0, x_batch=8)
    r4 = CGLSRun(A, b, x0, K, xt, history=False, defer_norms=False, x_batch=8)
    assert r3.x_batch == 1 and r4.x_batch == 1


def test_full_size_rule_selected():
    """The benchmark's shape: 4096^2, no x_true, run(10) then run(100); the rule's s against s = 1."""
    from trips_py_amd.operators import Blur2D
    from trips_py_amd.problems import gauss_psf
    from trips_py_amd.solvers import CGLSRun
    N = 4096
    A = Blur2D(gauss_psf((9, 9), (3, 3))[0], N, N)
    dev = A.engine.device
    b = torch.randn(N * N, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    x0 = torch.zeros(N * N, device=dev)
    out = []
    for xb in (1, None):
        run = CGLSRun(A, b, x0, 110, None, history=False, defer_norms=True, x_batch=xb)
        assert run.grouping == 1
        if xb is None:
            assert run.x_batch == A.engine.cgls_x_batch(N * N)
        run.run(10)
        run.run(100)
        g0, rows = run.rows()
        out.append((run.x_cur.clone(), run.p.clone(), g0, rows.copy()))
        del run
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and np.array_equal(out[0][3], out[1][3])
    assert np.all(np.isfinite(out[0][3]))


def test_rule():
    from trips_py_amd.engine import default_engine
    eng = default_engine()
    for n in (1, 64 * 64, 1 << 20, 2048 * 2048, X_BATCH_MIN_N - 1):
        assert eng.cgls_x_batch(n) == 1, n
    for e in range(0, 34):
        for n in ((1 << e) - 1, 1 << e, 3 << e):
            assert 1 <= eng.cgls_x_batch(max(1, n)) <= X_BATCH_MAX, n
