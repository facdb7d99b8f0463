"""GPU parity of the blur's boundary modes (Blur2D(..., boundary=m), trk_blur2d_create_bc) with float64 scipy.ndimage.convolve:
every mode on every kernel path of csrc/blur2d.hip (sliding, LDS strip, generic; batched with a leading dimension; the fused
CGLS apply; the axpby epilogue), the 4096^2 9x9 blur's borders, reflect unchanged, and the solvers on non-reflect blurs.
Bar: 1e-5 relative in fp32, as tests/test_gpu_blur.py."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.ndimage import convolve, convolve1d

from conftest import bar, load_golden, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-5
MODES = ["reflect", "constant", "nearest", "mirror", "wrap"]
NEW_MODES = MODES[1:]


def ext_index(i, n, mode):
    """Image index of (integer array) sample positions i of a length-n line extended by `mode`, -1 where constant mode reads 0:
    scipy.ndimage's extension rules, restated at any distance."""
    i = np.asarray(i)
    if mode == "reflect":
        p = 2 * n
        r = np.mod(i, p)
        return np.where(r >= n, p - 1 - r, r)
    if mode == "mirror":
        if n == 1:
            return np.zeros_like(i)
        p = 2 * n - 2
        r = np.mod(i, p)
        return np.where(r >= n, p - r, r)
    if mode == "wrap":
        return np.mod(i, n)
    if mode == "nearest":
        return np.clip(i, 0, n - 1)
    return np.where((i >= 0) & (i < n), i, -1)


def window_ref(img, psf, mode, r0, r1, c0, c1):
    """scipy.ndimage.convolve(img, psf, mode)[r0:r1, c0:c1] in float64 from the window and its halo only."""
    kh, kw = psf.shape
    T, L = kh - 1 - kh // 2, kw - 1 - kw // 2
    ri = ext_index(np.arange(r0 - T, r1 + kh // 2), img.shape[0], mode)
    ci = ext_index(np.arange(c0 - L, c1 + kw // 2), img.shape[1], mode)
    sub = img[np.ix_(np.maximum(ri, 0), np.maximum(ci, 0))].astype(np.float64)
    sub[ri < 0, :] = 0.0
    sub[:, ci < 0] = 0.0
    full = convolve(sub, psf, mode="constant")          # only the window's interior part is used: it never sees the padding
    return full[T:T + r1 - r0, L:L + c1 - c0]


class BlurBC64:
    """float64 restatement of the operator: convolve(X, psf, mode) and the flipped-PSF "transpose" (oracle protocol)."""

    def __init__(self, psf, nx, ny, mode):
        from oracle import cpu_ref as O

        class _Op(O._Op):
            def _fwd(s, x):
                return convolve(x.reshape(nx, ny), psf, mode=mode).reshape(-1)

            def _adj(s, y):
                return convolve(y.reshape(nx, ny), psf[::-1, ::-1], mode=mode).reshape(-1)
        self.op = _Op()
        self.op.shape = (nx * ny, nx * ny)


def gauss(K, s1, s2=None):
    from trips_py_amd.problems import gauss_psf
    return gauss_psf((K, K), (s1, s2 if s2 is not None else s1))[0]


def check_both(A, psf, nx, ny, mode, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(nx * ny).astype(np.float32).astype(np.float64)
    X = x.reshape(nx, ny)
    e_f = relerr(A @ x, convolve(X, psf, mode=mode))
    e_t = relerr(A.T @ x, convolve(X, psf[::-1, ::-1], mode=mode))
    assert e_f < TOL and e_t < TOL, (mode, e_f, e_t)


# ------------------------------------------------------------------------------------------------ scipy restatement sanity
@pytest.mark.parametrize("mode", MODES)
def test_window_restatement_is_scipy(mode):
    """The index restatement the large-image checks use equals scipy on a small image, windows touching every border,
    and a PSF longer than the image (extension beyond one period)."""
    rng = np.random.default_rng(1)
    img = rng.standard_normal((11, 7))
    for psf in (rng.random((5, 5)), rng.random((4, 6)), rng.random((27, 19))):
        ref = convolve(img, psf, mode=mode)
        assert np.allclose(window_ref(img, psf, mode, 0, 11, 0, 7), ref, rtol=0, atol=1e-12)
        assert np.allclose(window_ref(img, psf, mode, 3, 9, 2, 5), ref[3:9, 2:5], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ every mode x every path
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", [3, 5, 7, 9])
@pytest.mark.parametrize("shape", [(130, 520), (37, 64), (300, 8)])
def test_slide_path(mode, K, shape):
    """Separable odd PSFs <= 9x9 with ny % 4 == 0: k_blur_slide (several spans, bands marching up and down, 8-column images
    whose two edge lanes are neighbours)."""
    from trips_py_amd.operators import Blur2D
    nx, ny = shape
    psf = gauss(K, K / 3.0, K / 2.5)
    A = Blur2D(psf, nx, ny, boundary=mode)
    assert A.boundary == mode
    check_both(A, psf, nx, ny, mode, K * nx + ny)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,sep", [(11, True), (13, True), (15, True), (3, False), (5, False), (9, False), (13, False)])
@pytest.mark.parametrize("shape", [(130, 260), (37, 53)])
def test_strip_path(mode, K, sep, shape):
    """k_blur_strip: separable 11..15, and non-separable odd PSFs (any odd size up to 15); ny % 4 != 0 included."""
    from trips_py_amd.operators import Blur2D
    nx, ny = shape
    rng = np.random.default_rng(K + 100 * sep)
    if sep:
        psf = gauss(K, K / 3.0, K / 4.0)
    else:
        psf = rng.random((K, K))
        psf /= psf.sum()
    check_both(Blur2D(psf, nx, ny, boundary=mode), psf, nx, ny, mode, K)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("psf_shape,shape", [((4, 4), (33, 17)), ((10, 10), (16, 16)), ((5, 7), (24, 40)), ((4, 6), (20, 28)),
                                             ((25, 31), (9, 14)), ((17, 17), (5, 8))])
def test_generic_path(mode, psf_shape, shape):
    """k_blur_generic: even, rectangular and longer-than-the-image PSFs (the extension repeats beyond one period)."""
    from trips_py_amd.operators import Blur2D
    nx, ny = shape
    rng = np.random.default_rng(psf_shape[0] * 7 + psf_shape[1])
    psf = rng.random(psf_shape)
    psf /= psf.sum()
    check_both(Blur2D(psf, nx, ny, boundary=mode), psf, nx, ny, mode, nx)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 2, 5, 64, 256])
def test_blur1d_length_n_psf(mode, n):
    """The 1-D operator of Deblurring1D: a length-n PSF reaches a whole image length past each edge (k_blur_generic)."""
    from trips_py_amd.operators import Blur1D
    from trips_py_amd.problems import gauss_psf_1d
    psf = gauss_psf_1d(n, 3)
    A = Blur1D(psf, boundary=mode)
    x = np.random.default_rng(n).standard_normal(n).astype(np.float32).astype(np.float64)
    assert relerr(A @ x, convolve1d(x, psf, mode=mode)) < TOL
    assert relerr(A.T @ x, convolve1d(x, psf[::-1], mode=mode)) < TOL


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,shape,pad", [(9, (64, 128), 4), (5, (40, 96), 8), (9, (64, 128), 1), (11, (37, 53), 3), (4, (20, 24), 5)])
def test_batched_apply_with_leading_dimension(mode, K, shape, pad):
    """k columns at a leading dimension > n (the GKS / MMGKS k-column apply): pad % 4 == 0 takes the sliding kernel, otherwise
    the strip / generic kernels."""
    from trips_py_amd.operators import Blur2D
    nx, ny = shape
    n = nx * ny
    rng = np.random.default_rng(K * pad)
    psf = gauss(K, 2.0) if K % 2 else rng.random((K, K))
    A = Blur2D(psf, nx, ny, boundary=mode)
    dev = A.engine.device
    k = 3
    big = torch.from_numpy(rng.standard_normal((k, n + pad)).astype(np.float32)).to(dev)
    X = big[:, :n]
    outb = torch.full((k, n + pad), 7.0, device=dev)
    for tr in (False, True):
        Y = A.apply(X, out=outb[:, :n], transpose=tr)
        assert torch.all(outb[:, n:] == 7.0)                  # the leading dimension's gap is never written
        p = psf[::-1, ::-1] if tr else psf
        for j in range(k):
            xj = X[j].cpu().numpy().astype(np.float64).reshape(nx, ny)
            assert relerr(Y[j].cpu().numpy(), convolve(xj, p, mode=mode)) < TOL, (tr, j)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,shape", [(9, (256, 256)), (7, (100, 520)), (3, (64, 8)), (5, (37, 64))])
def test_fused_apply(mode, K, shape):
    """trk_op_apply_fused (CGLS's combine-on-load): y = A (x1 + cb x2), comb = x1 + cb x2 written out, ||y||^2 as raw
    partials; and its one-operand form (x2 = NULL)."""
    from trips_py_amd.operators import Blur2D
    nx, ny = shape
    n = nx * ny
    psf = gauss(K, K / 3.0, K / 2.5)
    A = Blur2D(psf, nx, ny, boundary=mode)
    eng = A.engine
    rng = np.random.default_rng(K + n)
    x1 = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(eng.device)
    x2 = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(eng.device)
    S = eng.scalars(2)
    S[0], S[1] = 3.0, 4.0                                    # cb = -1 * 3 / 4
    cap = 4096
    part = torch.zeros(cap, dtype=torch.float64, device=eng.device)
    for tr in (False, True):
        p = psf[::-1, ::-1] if tr else psf
        comb, y = eng.empty(n), eng.empty(n)
        nb = eng.op_apply_fused(A._h, tr, x1, x2, -1.0, S[0:1], 1, S[1:2], 1, comb, y, part, cap)
        want_comb = x1.double() - 0.75 * x2.double()
        assert float((comb.double() - want_comb).abs().max()) < 1e-6 * float(want_comb.abs().max())
        ref = convolve(want_comb.cpu().numpy().reshape(nx, ny), p, mode=mode)
        assert relerr(y.cpu().numpy(), ref) < TOL, tr
        assert np.isclose(float(part[:nb].sum()), float((y.double() ** 2).sum()), rtol=1e-7)
        nb = eng.op_apply_fused(A._h, tr, x1, None, 0.0, None, 0, None, 0, None, y, part, cap)
        assert relerr(y.cpu().numpy(), convolve(x1.double().cpu().numpy().reshape(nx, ny), p, mode=mode)) < TOL
        # fp32 sums of <= 16 squares per lane go into the fp64 total: on the smallest images few groups average the rounding out
        # (1.1e-8 measured at 64 x 8, in reflect as in the other modes)
        assert np.isclose(float(part[:nb].sum()), float((y.double() ** 2).sum()), rtol=1e-7)


@pytest.mark.parametrize("mode", NEW_MODES)
@pytest.mark.parametrize("K,shape", [(9, (256, 256)), (7, (100, 520)), (3, (300, 8)), (11, (64, 64)), (9, (50, 50))])
def test_axpby_epilogue_equals_apply_then_axpby(mode, K, shape):
    """trk_op_apply_axpby on a non-reflect blur: the epilogue kernel (or, where the sliding kernel does not serve the shape,
    apply + trk_axpby) gives the same bits as apply followed by trk_axpby."""
    from trips_py_amd.engine import Coef
    from trips_py_amd.operators import Blur2D
    nx, ny = shape
    psf = gauss(K, K / 3.0, K / 2.5)
    A = Blur2D(psf, nx, ny, boundary=mode)
    eng = A.engine
    rng = np.random.default_rng(K * nx + ny)
    x = torch.from_numpy(rng.standard_normal(nx * ny).astype(np.float32)).to(eng.device)
    z = torch.from_numpy(rng.standard_normal(nx * ny).astype(np.float32)).to(eng.device)
    S = eng.scalars(4)
    S[0], S[1] = 9.0, 4.0
    for tr in (False, True):
        for with_z in (True, False):
            a, b = Coef(2.0, num=S[0:1], den=S[1:2], sqrt_num=True), Coef(-1.0, den=S[1:2], sqrt_den=True)
            want = A.apply(x, transpose=tr)
            eng.axpby(a, want, b, z if with_z else None, want, sumsq=S[2:3])
            got = eng.empty(nx * ny)
            A.apply_axpby(x, a, b, z if with_z else None, got, transpose=tr, sumsq=S[3:4])
            assert torch.equal(got, want), (tr, with_z)
            h = eng.to_host(S)
            assert np.isclose(h[3], h[2], rtol=1e-8)
    got = eng.empty(nx * ny)
    A.apply_axpby(x, 1.0, -1.0, z, got)
    assert torch.equal(got, A.apply(x) - z)


# ------------------------------------------------------------------------------------------------ 4096^2
@pytest.mark.parametrize("mode", NEW_MODES)
def test_4096_borders_and_properties(mode):
    """The headline size with a 9x9 Gaussian: every corner and edge window against scipy (from the window's extended halo),
    the adjoint identity where the flipped PSF is the adjoint, constants preserved (or not, for 'constant')."""
    from trips_py_amd.operators import Blur2D
    N, h = 4096, 96
    psf = gauss(9, 3.0)
    A = Blur2D(psf, N, N, boundary=mode)
    eng = A.engine
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(N * N, generator=g, dtype=torch.float32).to(eng.device)
    Ax = A.apply(x)
    ATx = A.apply(x, transpose=True)
    ximg = x.reshape(N, N).cpu().numpy()
    out, outT = Ax.reshape(N, N).cpu().numpy(), ATx.reshape(N, N).cpu().numpy()
    lo, mid, hi = 0, N // 2 - h // 2, N - h
    for r0 in (lo, mid, hi):
        for c0 in (lo, mid, hi):
            ref = window_ref(ximg, psf, mode, r0, r0 + h, c0, c0 + h)
            refT = window_ref(ximg, psf[::-1, ::-1], mode, r0, r0 + h, c0, c0 + h)
            assert relerr(out[r0:r0 + h, c0:c0 + h], ref) < TOL, (r0, c0)
            assert relerr(outT[r0:r0 + h, c0:c0 + h], refT) < TOL, (r0, c0)
    ones = torch.ones(N * N, dtype=torch.float32, device=eng.device)
    A1 = A.apply(ones).reshape(N, N)
    if mode == "constant":
        assert float(A1[0, 0]) < 1.0 and float(A1[0, -1]) < 1.0 and float(A1[-1, 0]) < 1.0 and float(A1[-1, -1]) < 1.0
        assert abs(float(A1[N // 2, N // 2]) - 1.0) < 1e-6
    else:
        assert float((A1 - 1).abs().max()) < 1e-6
    if mode in ("constant", "wrap"):
        y = torch.randn(N * N, generator=g, dtype=torch.float32).to(eng.device)
        ATy = A.apply(y, transpose=True)
        S = eng.scalars(2)
        eng.dot(Ax, y, S[0:1])
        eng.dot(x, ATy, S[1:2])
        d = eng.to_host(S)
        assert abs(d[0] - d[1]) < 1e-6 * float(torch.linalg.norm(Ax.double()) * torch.linalg.norm(y.double()))


# ------------------------------------------------------------------------------------------------ reflect unchanged
@pytest.mark.parametrize("psf_kind,shape", [("g9", (130, 520)), ("g3", (300, 8)), ("g13", (64, 64)), ("ns7", (37, 53)),
                                            ("e4", (33, 17)), ("g9", (64, 130))])
def test_reflect_is_unchanged(psf_kind, shape):
    """boundary='reflect' and its alias 'grid-mirror' are the handle trk_blur2d_create makes, bit for bit, on every path
    (plain, batched, transposed, epilogue, fused)."""
    from trips_py_amd.operators import Blur2D, _HandleOperator
    nx, ny = shape
    rng = np.random.default_rng(nx)
    if psf_kind[0] == "g":
        psf = gauss(int(psf_kind[1:]), 2.5)
    else:
        psf = rng.random((int(psf_kind[-1]),) * 2)
        psf /= psf.sum()
    A0 = Blur2D(psf, nx, ny)
    eng = A0.engine
    arr = np.ascontiguousarray(psf, dtype=np.float64)
    h = ctypes.c_void_p()
    assert eng.lib.trk_blur2d_create(arr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), psf.shape[0], psf.shape[1], nx, ny,
                                     ctypes.byref(h)) == 0
    Aold = _HandleOperator(h, eng)
    ops = [Aold, Blur2D(psf, nx, ny, boundary="reflect"), Blur2D(psf, nx, ny, boundary="grid-mirror")]
    assert A0.boundary == ops[1].boundary == ops[2].boundary == "reflect"
    X = torch.from_numpy(rng.standard_normal((2, nx * ny)).astype(np.float32)).to(eng.device)
    z = torch.from_numpy(rng.standard_normal(nx * ny).astype(np.float32)).to(eng.device)
    for tr in (False, True):
        ref1, refb = A0.apply(X[0], transpose=tr), A0.apply(X, transpose=tr)
        refe = eng.empty(nx * ny)
        A0.apply_axpby(X[0], 2.0, -0.5, z, refe, transpose=tr)
        for A in ops:
            assert torch.equal(A.apply(X[0], transpose=tr), ref1)
            assert torch.equal(A.apply(X, transpose=tr), refb)
            got = eng.empty(nx * ny)
            A.apply_axpby(X[0], 2.0, -0.5, z, got, transpose=tr)
            assert torch.equal(got, refe)
        if eng.op_can_fuse(A0._h) == 1:
            S = eng.scalars(2)
            S[0], S[1] = 1.0, 3.0
            part = torch.zeros(4096, dtype=torch.float64, device=eng.device)
            res = []
            for A in [A0] + ops:
                comb, y = eng.empty(nx * ny), eng.empty(nx * ny)
                eng.op_apply_fused(A._h, tr, X[0], X[1], 1.0, S[0:1], 1, S[1:2], 1, comb, y, part, 4096)
                res.append((comb, y))
            for comb, y in res[1:]:
                assert torch.equal(comb, res[0][0]) and torch.equal(y, res[0][1])


# ------------------------------------------------------------------------------------------------ solvers
@pytest.mark.parametrize("mode", NEW_MODES)
def test_deblur1d_goldens_cgls_and_hybrid_lsqr(mode):
    """The reference's Deblurring1D.forward_Op_1D(3, 256, boundary_condition=mode) with its CGLS and Hybrid_LSQR
    (tools/make_boundary_goldens.py), at the bounds of tests/test_gpu_cgls.py's deblur1d_cgls_n256."""
    from trips_py_amd.problems import Deblurring1D
    from trips_py_amd.solvers import CGLS, Hybrid_LSQR
    g = load_golden("deblur1d_bc_" + mode)
    n = int(g["n"])
    D1 = Deblurring1D(CommitCrime=True)
    A = D1.forward_Op_1D(3, n, boundary_condition=mode)
    assert D1.boundary_condition == mode and A.boundary == mode
    assert np.allclose(D1.PSF, g["psf"], rtol=1e-15, atol=0)
    assert relerr(A @ g["x"], g["Ax"]) < TOL and relerr(A.T @ g["x"], g["ATx"]) < TOL
    x, info = CGLS(A, g["b"], np.zeros((n, 1)), int(g["cgls_max_iter"]), 0.0, x_true=g["x_true"])
    assert info["its"] == int(g["cgls_its"])
    assert np.allclose(info["relError"][:15], g["cgls_relError"][:15], rtol=1e-3)
    assert info["relError"][-1] < 2 * g["cgls_relError"][-1] + 1e-3
    x, info = Hybrid_LSQR(A, g["b"], int(g["hlsqr_n_iter"]), float(g["hlsqr_lam"]), g["x_true"])
    assert np.allclose(info["relError"][:15], g["hlsqr_relError"][:15], rtol=1e-3)
    assert info["relError"][-1] < 2 * g["hlsqr_relError"][-1] + 1e-3
    bar(f"bc.deblur1d_{mode}.hlsqr_x", relerr(x, g["hlsqr_x"]), 1e-3)


def test_deblur1d_aliases_store_the_name_given():
    from trips_py_amd.problems import Deblurring1D
    D1 = Deblurring1D()
    A = D1.forward_Op_1D(3, 64, boundary_condition="grid-wrap")
    assert D1.boundary_condition == "grid-wrap" and A.boundary == "wrap"


@pytest.mark.parametrize("mode", ["constant", "wrap"])
def test_cgls_512_streaming_fused_loop(mode, monkeypatch):
    """BASELINE C2's problem (512^2, 9x9, 100 iterations) on a non-reflect blur: the tiled small-image loop reports the mode
    unsupported (trk_cgls_tiled_caps), the streaming fused loop runs it, and it matches a float64 CGLS on scipy."""
    from oracle import cpu_ref as O
    from trips_py_amd.problems import Deblurring2D, add_noise, synthetic_image
    from trips_py_amd.solvers import CGLS
    from trips_py_amd.solvers.CGLS import CGLSRunFused
    N, its = 512, 100
    A = Deblurring2D().forward_Op((9, 9), (3, 3), N, N, boundary_condition=mode)
    Aref = Deblurring2D().forward_Op((9, 9), (3, 3), N, N)
    eng = A.engine
    assert CGLSRunFused.tiled_usable(Aref, eng) and not CGLSRunFused.tiled_usable(A, eng)
    assert CGLSRunFused.usable(A, eng)
    psf = A.psf
    Ao = BlurBC64(psf, N, N, mode).op
    xt = synthetic_image(N, 0).reshape(-1, 1)
    b, _ = add_noise(Ao @ xt, 0.01, 1)
    xo, io = O.cgls(Ao, b, np.zeros((N * N, 1)), its, 0, x_true=xt)
    runs = []
    init = CGLSRunFused.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        runs.append(self.tiled)
    monkeypatch.setattr(CGLSRunFused, "__init__", spy)
    x, info = CGLS(A, b, np.zeros((N * N, 1)), its, 0, x_true=xt, history=False, fused=True)
    assert runs == [0], runs                                  # the streaming fused loop, not a tiled form
    assert info["its"] == its
    assert relerr(x, xo) < TOL, relerr(x, xo)
    assert np.allclose(info["relError"], io["relError"], rtol=1e-4)
    assert np.allclose(info["relResidual"], io["relResidual"], rtol=1e-3)


@pytest.mark.parametrize("mode", ["wrap", "constant"])
def test_projection_solvers_on_a_non_reflect_blur(mode):
    """Hybrid-LSQR, Hybrid-GMRES, GKS and MMGKS (L = 2-D first derivative, fixed lambda; GKS / MMGKS apply A to k columns at
    a leading dimension) on a 64^2 non-reflect blur against the oracle's float64 restatements on the same operator."""
    from oracle import cpu_ref as O
    from trips_py_amd import solvers as S
    from trips_py_amd.operators import Blur2D, FirstDerivative2D
    from trips_py_amd.problems import synthetic_image
    N = 64
    psf = gauss(9, 2.0)
    A, Ao = Blur2D(psf, N, N, boundary=mode), BlurBC64(psf, N, N, mode).op
    xt = synthetic_image(N, 3).reshape(-1)
    rng = np.random.default_rng(5)
    b = Ao @ xt
    e = rng.standard_normal(b.size)
    b = (b + 0.01 * np.linalg.norm(b) / np.linalg.norm(e) * e).astype(np.float32).astype(np.float64)
    L, Lo = FirstDerivative2D(N), O.FirstDerivative2D(N)
    x, _ = S.Hybrid_LSQR(A, b, 20, 1e-2)
    xo, _ = O.hybrid_lsqr(Ao, b.reshape(-1, 1), 20, 1e-2)
    bar(f"bc.{mode}.hybrid_lsqr", relerr(x, xo), 1e-4)
    x, _ = S.Hybrid_GMRES(A, b, 15, 1e-2)
    xo, _ = O.hybrid_gmres(Ao, b.reshape(-1, 1), 15, 1e-2)
    bar(f"bc.{mode}.hybrid_gmres", relerr(x, xo), 1e-4)
    x, info = S.GKS(A, b, L, 3, 10, 1e-2, xt)
    xo, io = O.gks(Ao, b.reshape(-1, 1), Lo, 3, 10, 1e-2, xt.reshape(-1, 1))
    bar(f"bc.{mode}.gks", relerr(x, xo), 1e-4)
    x, info = S.MMGKS(A, b, L, 2, 1, 3, 8, 1e-2, xt, epsilon=0.1)
    xo, io = O.mmgks(Ao, b.reshape(-1, 1), Lo, 2, 1, 3, 8, 1e-2, xt.reshape(-1, 1), epsilon=0.1)
    assert info["its"] == io["its"]
    bar(f"bc.{mode}.mmgks", relerr(x, xo), 1e-4)
