"""GPU checks of the blur's LDS tile kernel (csrc/blur_tile.hip: any PSF up to 64x64) on the cases of tests/blur_psf_cases.py:
the general form against the generic kernel bit for bit and against float64 scipy, the separable form against scipy, batched
applies at a leading dimension, the fused sum of squares, the path rule, forward_Op(psf_type=...) and CGLS / GKS on a defocus
blur.  Bar: 1e-5 relative in fp32, as tests/test_gpu_blur.py."""
import numpy as np
import pytest
import torch
from scipy.ndimage import convolve

import blur_psf_cases as C
from conftest import bar, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-5
GENERAL = [p for p in C.PSFS if C.expected_form(p) == "general"]
SEPARABLE = [p for p in C.PSFS if C.expected_form(p) == "separable"]


def image(nx, ny, seed):
    return np.random.default_rng(seed).standard_normal(nx * ny).astype(np.float32)


def forced(psf, nx, ny, mode, path):
    from trips_py_amd.operators import Blur2D
    A = Blur2D(psf, nx, ny, boundary=mode).set_path(path)
    assert A.path == path
    return A


_REF = {}


def scipy_ref(pname, psf, iname, x, mode, tr):
    """float64 scipy convolve of the case's image (blur_psf_cases.convolve_ref: sound for a PSF of any size, which the direct
    call is not), computed once per (PSF, image, mode, direction)."""
    key = (pname, iname, mode, tr)
    if key not in _REF:
        nx, ny = C.IMAGES[iname]
        _REF[key] = C.convolve_ref(x.astype(np.float64).reshape(nx, ny), psf[::-1, ::-1] if tr else psf, mode)
    return _REF[key]


# ------------------------------------------------------------------------------------------------ both forms, every tile situation
@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("pname", GENERAL)
def test_general_form_is_the_generic_kernel_bit_for_bit(mode, pname):
    psf = C.make_psf(pname)
    for iname, (nx, ny) in C.IMAGES.items():
        At, Ag = forced(psf, nx, ny, mode, "tile"), forced(psf, nx, ny, mode, "generic")
        x = image(nx, ny, nx + ny)
        xd = torch.from_numpy(x).to(At.engine.device)
        for tr in (False, True):
            yt, yg = At.apply(xd, transpose=tr), Ag.apply(xd, transpose=tr)
            assert torch.equal(yt, yg), (iname, tr)
            e = relerr(yt.cpu().numpy(), scipy_ref(pname, psf, iname, x, mode, tr))
            assert e < TOL, (iname, tr, e)


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("pname", SEPARABLE)
def test_separable_form_against_scipy(mode, pname):
    psf = C.make_psf(pname)
    for iname, (nx, ny) in C.IMAGES.items():
        A = forced(psf, nx, ny, mode, "tile")
        x = image(nx, ny, nx + ny)
        xd = torch.from_numpy(x).to(A.engine.device)
        for tr in (False, True):
            e = relerr(A.apply(xd, transpose=tr).cpu().numpy(), scipy_ref(pname, psf, iname, x, mode, tr))
            assert e < TOL, (iname, tr, e)


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("K,shape", [(9, (64, 64)), (9, (130, 520)), (13, (64, 64)), (13, (37, 53))])
def test_slide_and_strip_shapes_forced_to_tile(mode, K, shape):
    """9x9 and 13x13 Gaussians on shapes the sliding and strip kernels own, forced to the tile kernel's separable form."""
    from trips_py_amd.operators import Blur2D
    from trips_py_amd.problems import gauss_psf
    nx, ny = shape
    psf = gauss_psf((K, K), (K / 3.0, K / 2.5))[0]
    A = Blur2D(psf, nx, ny, boundary=mode)
    assert A.path == ("slide" if K == 9 and ny % 4 == 0 else "strip")
    A.set_path("tile")
    assert A.path == "tile"
    x = image(nx, ny, K)
    X = x.astype(np.float64).reshape(nx, ny)
    assert relerr(A @ x.astype(np.float64), convolve(X, psf, mode=mode)) < TOL
    assert relerr(A.T @ x.astype(np.float64), convolve(X, psf[::-1, ::-1], mode=mode)) < TOL


# ------------------------------------------------------------------------------------------------ batched, sum of squares
@pytest.mark.parametrize("mode", ["reflect", "constant", "wrap"])
@pytest.mark.parametrize("pname", ["d21x21", "g17x17", "r64x40", "g33x5"])
@pytest.mark.parametrize("pad", [1, 4])
def test_batched_apply_with_leading_dimension(mode, pname, pad):
    """3 columns at leading dimension n + 1 and n + 4 (the GKS / MMGKS k-column apply): the gap keeps its fill value."""
    psf = C.make_psf(pname)
    nx, ny = C.IMAGES["2x2_partial"]
    n, k = nx * ny, 3
    A = forced(psf, nx, ny, mode, "tile")
    dev = A.engine.device
    big = torch.from_numpy(np.random.default_rng(pad).standard_normal((k, n + pad)).astype(np.float32)).to(dev)
    X = big[:, :n]
    outb = torch.full((k, n + pad), 7.0, device=dev)
    for tr in (False, True):
        Y = A.apply(X, out=outb[:, :n], transpose=tr)
        assert torch.all(outb[:, n:] == 7.0)
        p = psf[::-1, ::-1] if tr else psf
        for j in range(k):
            assert torch.equal(Y[j], A.apply(X[j].contiguous(), transpose=tr)), (tr, j)
        ref = convolve(X[1].cpu().numpy().astype(np.float64).reshape(nx, ny), p, mode=mode)
        assert relerr(Y[1].cpu().numpy(), ref) < TOL, tr


@pytest.mark.parametrize("pname", ["d21x21", "g31x31", "r63x63", "g10x10"])
@pytest.mark.parametrize("iname", ["2x2_partial", "below_one_tile"])
def test_sumsq(pname, iname):
    """The fused sum of squares: block partials + a fixed-order finalize — equal to the float64 sum, y unchanged by it, and the
    same bits on every run (no atomics)."""
    psf = C.make_psf(pname)
    nx, ny = C.IMAGES[iname]
    A = forced(psf, nx, ny, "reflect", "tile")
    eng = A.engine
    x = torch.from_numpy(image(nx, ny, 5)).to(eng.device)
    S = eng.scalars(2)
    for tr in (False, True):
        y0 = A.apply(x, transpose=tr)
        y1 = A.apply(x, transpose=tr, sumsq=S[0:1])
        y2 = A.apply(x, transpose=tr, sumsq=S[1:2])
        h = eng.to_host(S)
        assert torch.equal(y1, y0) and torch.equal(y2, y0)
        assert h[0] == h[1]
        assert np.isclose(h[0], float((y0.double() ** 2).sum()), rtol=1e-7, atol=0)


# ------------------------------------------------------------------------------------------------ the path rule on handles
def test_auto_paths_and_set_path():
    from trips_py_amd.operators import Blur2D, FirstDerivative2D
    from trips_py_amd.problems import defocus_psf, gauss_psf
    rng = np.random.default_rng(0)
    assert Blur2D(gauss_psf((9, 9), 3)[0], 64, 64).path == "slide"
    r13 = rng.random((13, 13))
    assert Blur2D(r13 / r13.sum(), 64, 64).path == "strip"
    for psf in (gauss_psf((10, 10), 2)[0], defocus_psf((21, 21), 9)[0], gauss_psf((31, 31), 5)[0]):
        assert Blur2D(psf, 512, 512).path == "tile"
    big = Blur2D(gauss_psf((65, 65), 9)[0], 80, 80)
    assert big.path == "generic"
    with pytest.raises(NotImplementedError):
        big.set_path("tile")
    assert big.path == "generic"
    A = Blur2D(gauss_psf((9, 9), 3)[0], 64, 64)
    eng = A.engine
    assert eng.op_can_fuse(A._h) == 1 and eng.op_can_recompute(A._h)
    for name in ("generic", "tile"):
        A.set_path(name)
        assert A.path == name and eng.op_can_fuse(A._h) == 0 and not eng.op_can_recompute(A._h) and not A.native_axpby
    A.set_path("auto")
    assert A.path == "slide" and eng.op_can_fuse(A._h) == 1 and eng.op_can_recompute(A._h)
    for bad in ("slide", "strip", "fast", 3):
        with pytest.raises(ValueError):
            A.set_path(bad)
    import ctypes
    for code in (1, 2, 5, -1):                                  # SLIDE, STRIP and unknown values: TRK_EINVAL
        assert eng.lib.trk_blur2d_set_path(A._h, code) == -1
    assert A.path == "slide"
    L = FirstDerivative2D(16)                                   # not a blur: TRK_EINVAL
    path, sep = ctypes.c_int(), ctypes.c_int()
    assert eng.lib.trk_blur2d_path(L._h, ctypes.byref(path), ctypes.byref(sep)) == -1
    assert eng.lib.trk_blur2d_set_path(L._h, 3) == -1


def test_forward_op_psf_type():
    from trips_py_amd.operators import Blur2D
    from trips_py_amd.problems import Deblurring2D, defocus_psf, gauss_psf, motion_psf
    N = 64
    x = torch.from_numpy(image(N, N, 1))
    D = Deblurring2D()
    A = D.forward_Op((9, 9), (3, 3), N, N)                      # the default call: today's operator, bit for bit
    x = x.to(A.engine.device)
    assert A.path == "slide" and torch.equal(A.apply(x), Blur2D(gauss_psf((9, 9), (3, 3))[0], N, N).apply(x))
    assert torch.equal(D.forward_Op((9, 9), (3, 3), N, N, psf_type="gauss").apply(x), A.apply(x))
    Ad = D.forward_Op((21, 21), 9, N, N, psf_type="defocus")
    assert np.array_equal(Ad.psf, defocus_psf((21, 21), 9)[0]) and Ad.path == "tile"
    Am = D.forward_Op((21, 21), (15, 30), N, N, psf_type="motion", boundary_condition="constant")
    assert np.array_equal(Am.psf, motion_psf((21, 21), 15, 30)[0]) and Am.path == "tile" and Am.boundary == "constant"
    psf = C.make_psf("r4x6")
    Aa = D.forward_Op(None, None, N, N, psf_type=psf)
    assert np.array_equal(Aa.psf, psf) and Aa.path == "tile"
    for B in (Ad, Am, Aa):
        xh = x.cpu().numpy().astype(np.float64)
        assert relerr(B @ xh, convolve(xh.reshape(N, N), B.psf, mode=B.boundary)) < TOL
    with pytest.raises(ValueError):
        D.forward_Op((9, 9), 3, N, N, psf_type="box")


# ------------------------------------------------------------------------------------------------ solvers
@pytest.fixture(scope="module")
def defocus_problem():
    """64^2 image, 21x21 defocus PSF, reflect, 1 % noise, and the float64 oracle's CGLS (20 iterations) and GKS (10) on the scipy
    operator: computed once, shared, left unchanged."""
    from oracle import cpu_ref as O
    from trips_py_amd.problems import defocus_psf, synthetic_image
    N = 64
    psf = defocus_psf((21, 21), 9)[0]
    Ao = C.scipy_operator(psf, N, N, "reflect")
    xt = synthetic_image(N, 3).reshape(-1)
    b = Ao @ xt
    e = np.random.default_rng(5).standard_normal(b.size)
    b = (b + 0.01 * np.linalg.norm(b) / np.linalg.norm(e) * e).astype(np.float32).astype(np.float64)
    xc, ic = O.cgls(Ao, b.reshape(-1, 1), np.zeros((N * N, 1)), 20, 0, x_true=xt.reshape(-1, 1))
    xg, ig = O.gks(Ao, b.reshape(-1, 1), O.FirstDerivative2D(N), 3, 10, 1e-2, xt.reshape(-1, 1))
    return {"N": N, "psf": psf, "xt": xt, "b": b, "cgls": (xc, ic), "gks": (xg, ig)}


@pytest.mark.parametrize("solver", ["cgls", "gks"])
def test_solvers_on_a_defocus_blur(defocus_problem, solver):
    """CGLS (20 iterations) and GKS (10, fixed lambda, L = 2-D first derivative: A is applied to k columns at a leading dimension)
    through the tile kernel against the float64 oracle.  The bar for x is the same solve on the generic kernel — the kernel of
    every such PSF before the tile kernel existed: the two applies give the same bits and differ only in how the partials of
    ||w||^2 are grouped, so the tile run may be at most 2x as far from the oracle.  Measured on the MI355X: CGLS 1.940e-02 on
    both paths (20 fp32 iterations on this ill-conditioned blur against float64), GKS 8.182e-07 on both."""
    from trips_py_amd import solvers as S
    from trips_py_amd.operators import Blur2D, FirstDerivative2D
    p = defocus_problem
    N, xt, b = p["N"], p["xt"], p["b"]
    xo, io = p[solver]
    err = {}
    for path in ("generic", "tile"):
        A = Blur2D(p["psf"], N, N)
        assert A.path == "tile"
        A.set_path(path)
        if solver == "cgls":
            x, info = S.CGLS(A, b, np.zeros((N * N, 1)), 20, 0, x_true=xt)
        else:
            x, info = S.GKS(A, b, FirstDerivative2D(N), 3, 10, 1e-2, xt)
        err[path] = relerr(x, xo)
        if path == "tile":
            assert info["its"] == io["its"]
            assert np.allclose(np.asarray(info["relError"]).reshape(-1)[:15], np.asarray(io["relError"]).reshape(-1)[:15], rtol=1e-3)
    print(f"{solver}: |x - x_oracle| / |x_oracle|  generic {err['generic']:.3e}  tile {err['tile']:.3e}")
    bar(f"psf.defocus21.{solver}.generic", err["generic"], float("inf"))
    bar(f"psf.defocus21.{solver}.tile", err["tile"], 2 * err["generic"] + np.finfo(np.float64).tiny)
