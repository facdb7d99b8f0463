"""The norm-only blur pass (trk_op_apply_sumsq_raw, k_blur_slide<…RC_NORM>) on images WITH interior spans.

A wave of the sliding kernel owns a 256-column span.  At 9x9 (every mode but constant) the norm-only pass marches a span that touches
neither the left nor the right border of the image through a form of the row block without any border rule, and forms the column
pairs of its horizontal taps once per row; the first and the last span keep the border rule.  The images of
tests/test_gpu_cgls_recompute.py are at most 512 columns wide — two spans, both at a border — so none of them reaches the interior
form.  These do.  The pass does the fp32 operations of the storing kernel in their order on every entry, so every comparison is
exact."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PCAP = 4096
MODES = ["reflect", "constant", "nearest", "mirror", "wrap"]
# (10, 776): one short band; four spans, two interior; the last span partial and mostly inactive (8 of its 256 columns)
# (37, 1024): four 10-row bands for 9x9, the odd ones marching upward; two interior spans, the last span exactly full
# (150, 768): an exactly full last span, many bands, a partial last band; one interior span
# (8, 520): fewer rows than K = 9 (every staged row above and below the image is extended); one interior span
# (2600, 776): tall enough for 19-row bands at 9x9 (four spans x 260 ten-row bands would be more waves than SIMDs): 27 staged rows per
#              band, so the march runs its UNGUARDED steady-state block between the guarded first and last one — the shorter images
#              above get ten-row bands, 18 staged rows, and never reach it.  Top and bottom bands extend rows, the others do not.
IMAGES = [(10, 776), (37, 1024), (150, 768), (8, 520), (2600, 776)]


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


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [3, 5, 7, 9])
def test_norm_only_partials_equal_the_storing_kernels_on_interior_spans(k, mode):
    for nx, ny in IMAGES:
        assert -(-ny // 256) >= 3, "an image of this file has a span that touches no border"
        A = _blur(k, nx, ny, mode)
        eng = A.engine
        x = _randn(eng, nx * ny, 5 + nx)
        for tr in (False, True):
            P1, P2 = eng.scalars(PCAP), eng.scalars(PCAP)
            P2.t.fill_(-1.0)
            y = eng.empty(nx * ny)
            n1 = eng.op_apply_fused(A._h, tr, x, None, 0.0, None, 0, None, 0, None, y, P1.ref(0), PCAP)
            n2 = eng.op_apply_sumsq_raw(A._h, tr, x, P2.ref(0), PCAP)
            assert n1 == n2 and n1 >= 3, (nx, ny, tr)
            assert n1 % (-(-ny // 256)) == 0, (nx, ny, tr)                  # one partial per (band, span)
            assert torch.equal(P1.t[:n1], P2.t[:n2]), (nx, ny, tr)
            assert torch.all(P2.t[n2:] == -1.0), (nx, ny, tr)              # nothing beyond the counted partials is written
            assert float(P2.t[:n2].sum()) > 0.0


def test_tall_image_reaches_the_steady_state_block():
    """(2600, 776) at 9x9: four spans, 19-row bands (one partial per wave: 4 x ceil(2600 / 19) = 548), i.e. 27 staged rows per band =
    three blocks of nine, the middle one unguarded.  If the band rule ever changes, this says so instead of the tests above going
    quietly back to guarded blocks only."""
    nx, ny = 2600, 776
    A = _blur(9, nx, ny, "reflect")
    eng = A.engine
    P = eng.scalars(PCAP)
    n = eng.op_apply_sumsq_raw(A._h, False, _randn(eng, nx * ny, 1), P.ref(0), PCAP)
    assert n == 4 * -(-nx // 19), n


def test_interior_partials_see_every_column():
    """A single non-zero entry in an interior span moves the partials of that span (and of its neighbours within the PSF's reach)
    exactly as it moves the storing kernel's: the interior form reads its left and right neighbour groups from the image."""
    nx, ny, k = 37, 1024, 9
    A = _blur(k, nx, ny, "reflect")
    eng = A.engine
    for col in (256, 259, 511, 512, 767):                                  # first / last columns of the interior spans
        x = torch.zeros(nx * ny, device=eng.device)
        x[17 * ny + col] = 1.5
        for tr in (False, True):
            P1, P2 = eng.scalars(PCAP), eng.scalars(PCAP)
            y = eng.empty(nx * ny)
            n1 = eng.op_apply_fused(A._h, tr, x, None, 0.0, None, 0, None, 0, None, y, P1.ref(0), PCAP)
            n2 = eng.op_apply_sumsq_raw(A._h, tr, x, P2.ref(0), PCAP)
            assert n1 == n2
            assert torch.equal(P1.t[:n1], P2.t[:n2]), (col, tr)
            assert int((P2.t[:n2] != 0).sum()) >= 2, (col, tr)              # the PSF reaches across the span's border


# ------------------------------------------------------------------------------------------------------------ the loop
K = 20
SHAPES = [(100, 776), (2600, 776)]           # ten-row bands (guarded blocks only) / 19-row bands (with the steady-state block)


@functools.lru_cache(maxsize=None)
def _xbatch_reference(mode, s, shape):
    """The x-batch loop that stores w and t, K iterations: the problem, its final state and rows.  Computed once per (mode, s)."""
    from trips_py_amd.operators import Blur2D
    from trips_py_amd.problems import gauss_psf
    from trips_py_amd.solvers import CGLSRun
    nx, ny = shape
    A = Blur2D(gauss_psf((9, 9), (3, 3))[0], nx, ny, boundary=mode)
    rng = np.random.default_rng(11 + nx)
    b, xt, x0 = rng.standard_normal(nx * ny), rng.standard_normal(nx * ny), np.zeros(nx * ny)
    ref = CGLSRun(A, b, x0, K, xt, history=False, defer_norms=True, grouping=1, x_batch=s, recompute=False)
    assert ref.raw and ref.x_batch == s and not ref.recompute
    ref.run(K)
    g0, rows = ref.rows()
    return (A, b, x0, xt), [v.clone() for v in (ref.x_cur, ref.p, ref.r)], g0, rows.copy()


@pytest.mark.parametrize("s", [1, 3])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_recompute_loop_equals_xbatch_loop_with_interior_spans(shape, mode, s):
    from trips_py_amd.solvers import CGLSRun
    (A, b, x0, xt), state, g0, rows = _xbatch_reference(mode, s, shape)
    run = CGLSRun(A, b, x0, K, xt, history=False, defer_norms=True, grouping=1, x_batch=s, recompute=True)
    assert run.recompute and run.x_batch == s
    run.run(K)
    assert run.k == K
    for name, got, want in zip(("x_cur", "p", "r"), (run.x_cur, run.p, run.r), state):
        assert torch.equal(got, want), name
    g0_b, rows_b = run.rows()
    assert g0_b == g0
    assert np.array_equal(rows_b, rows)
    assert np.all(np.isfinite(rows_b))
