"""Host-side checks of the blur's PSF surface (no GPU): the path rule trk_blur2d_plan, the new entry points' NULL handling, the
case table of tests/blur_psf_cases.py, the defocus / motion PSF builders, Deblurring1D.Defocus1D against the reference's arrays,
and what the fp32 one-chain sum of the tile kernel costs against float64 scipy at the largest PSF."""
import ctypes

import numpy as np
import pytest
from scipy.ndimage import convolve

import blur_psf_cases as C
from conftest import load_golden, relerr

AUTO, SLIDE, STRIP, TILE, GENERIC = range(5)


def plan(kh, kw, sep, nx, ny):
    from trips_py_amd import _lib
    path = ctypes.c_int(-1)
    assert _lib.load().trk_blur2d_plan(kh, kw, int(sep), nx, ny, ctypes.byref(path)) == 0
    return path.value


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_reaches_both_forms_and_every_tile_situation():
    forms = {name: C.expected_form(name) for name in C.PSFS}
    assert forms == {"r2x2": "general", "r4x6": "general", "g10x10": "separable", "g16x16": "separable", "g17x17": "separable",
                     "d21x21": "general", "m21x21": "general", "g31x31": "separable", "g33x5": "separable",
                     "r1x64": "separable", "r64x1": "separable", "r64x40": "general", "g63x63": "separable",
                     "r63x63": "general"}
    for name in C.PSFS:
        psf = C.make_psf(name)
        assert psf.shape == C.PSFS[name][1] and abs(psf.sum() - 1) < 1e-12 and psf.min() >= 0
    shapes = list(C.IMAGES.values())
    assert any(nx < C.TH and ny < C.TW for nx, ny in shapes)                                  # smaller than one tile
    assert (C.TH, C.TW) in shapes and (C.TH + 1, C.TW + 1) in shapes                          # exactly one; one more row and column
    assert any(2 * C.TH < nx < 3 * C.TH and 2 * C.TW < ny < 3 * C.TW and ny % 4 for nx, ny in shapes)   # partial last tiles
    assert any(ny == 1 for _, ny in shapes) and any(nx == 1 for nx, _ in shapes)
    # a PSF larger than the image in one axis and in both, beyond one period of the extension
    both = [(p, i) for p, i in C.CASES if C.PSFS[p][1][0] > 2 * C.IMAGES[i][0] and C.PSFS[p][1][1] > 2 * C.IMAGES[i][1]]
    one = [(p, i) for p, i in C.CASES if (C.PSFS[p][1][0] > 2 * C.IMAGES[i][0]) != (C.PSFS[p][1][1] > 2 * C.IMAGES[i][1])]
    assert both and one
    for form in ("general", "separable"):
        assert any(forms[p] == form for p, _ in both) and any(forms[p] == form for p, _ in one)


@pytest.mark.parametrize("mode", C.MODES)
def test_reference_at_any_distance_is_scipy(mode):
    """convolve_ref — scipy on the explicitly extended image — equals scipy called directly on every case of the table where the
    direct call is sound (the largest PSFs on the largest images left out: the extension is what differs between the cases, and
    theirs is one period)."""
    unsound = 0
    for p, i in C.CASES:
        psf, (nx, ny) = C.make_psf(p), C.IMAGES[i]
        if psf.size * nx * ny > 2e6:
            continue
        if not C.scipy_direct_is_sound(psf.shape, (nx, ny), mode):
            unsound += 1
            continue
        img = np.random.default_rng(nx * ny).standard_normal((nx, ny))
        assert np.allclose(C.convolve_ref(img, psf, mode), convolve(img, psf, mode=mode), rtol=0, atol=1e-12), (p, i)
    assert unsound == (4 if mode == "reflect" else 0)


# ------------------------------------------------------------------------------------------------ the path rule
@pytest.mark.parametrize("kh,kw,sep,nx,ny,want", [
    # today's slide shapes, unchanged
    (3, 3, 1, 64, 64, SLIDE), (5, 5, 1, 37, 64, SLIDE), (7, 7, 1, 100, 520, SLIDE), (9, 9, 1, 4096, 4096, SLIDE), (9, 9, 1, 300, 8, SLIDE),
    # slide shapes the sliding kernel does not take (ny % 4, ny < 8, too many pixels, not separable): the strip kernel, as today
    (9, 9, 1, 64, 130, STRIP), (9, 9, 1, 64, 4, STRIP), (9, 9, 1, 32768, 16384, STRIP), (9, 9, 0, 64, 64, STRIP), (3, 3, 0, 37, 53, STRIP),
    # today's strip shapes, unchanged
    (11, 11, 1, 130, 260, STRIP), (13, 13, 1, 64, 64, STRIP), (15, 15, 1, 37, 53, STRIP), (13, 13, 0, 130, 260, STRIP), (15, 15, 0, 64, 64, STRIP),
    # everything else up to 64 x 64: the tile kernel
    (1, 1, 1, 8, 8, TILE), (2, 2, 0, 64, 64, TILE), (4, 6, 0, 20, 28, TILE), (10, 10, 1, 512, 512, TILE), (16, 16, 1, 64, 64, TILE),
    (17, 17, 1, 64, 64, TILE), (17, 17, 0, 5, 8, TILE), (21, 21, 0, 512, 512, TILE), (31, 31, 1, 4096, 4096, TILE), (33, 5, 1, 69, 150, TILE),
    (5, 7, 1, 24, 40, TILE), (9, 7, 1, 64, 64, TILE), (1, 64, 1, 64, 64, TILE), (64, 1, 1, 256, 1, TILE), (64, 40, 0, 69, 150, TILE),
    (63, 63, 1, 69, 150, TILE), (63, 63, 0, 4096, 4096, TILE), (64, 64, 0, 1, 1, TILE), (25, 31, 0, 9, 14, TILE),
    # a side above 64: the generic kernel
    (65, 65, 1, 512, 512, GENERIC), (65, 3, 0, 64, 64, GENERIC), (3, 65, 1, 64, 64, GENERIC), (256, 1, 1, 256, 1, GENERIC), (1, 256, 1, 1, 256, GENERIC),
])
def test_plan(kh, kw, sep, nx, ny, want):
    assert plan(kh, kw, sep, nx, ny) == want


def test_plan_of_every_case_is_tile():
    for p, i in C.CASES:
        kh, kw = C.PSFS[p][1]
        assert plan(kh, kw, C.expected_form(p) == "separable", *C.IMAGES[i]) == TILE, (p, i)


def test_new_entry_points_reject_null_before_any_device_call():
    from trips_py_amd import _lib
    lib = _lib.load()
    path, sep = ctypes.c_int(7), ctypes.c_int(7)
    assert lib.trk_blur2d_plan(9, 9, 1, 64, 64, None) == -1 and b"NULL" in lib.trk_last_error()
    assert lib.trk_blur2d_plan(0, 9, 1, 64, 64, ctypes.byref(path)) == -1
    assert lib.trk_blur2d_path(None, ctypes.byref(path), ctypes.byref(sep)) == -1 and b"NULL" in lib.trk_last_error()
    assert lib.trk_blur2d_set_path(None, TILE) == -1 and b"NULL" in lib.trk_last_error()
    assert path.value == 7 and sep.value == 7


def test_python_surface_is_lazy():
    """Blur2D has `path` (a property) and `set_path`; neither new entry point is called at construction."""
    import inspect

    from trips_py_amd.operators import Blur2D
    assert isinstance(Blur2D.path, property) and callable(Blur2D.set_path)
    assert "trk_blur2d_path" not in inspect.getsource(Blur2D.__init__) and "trk_blur2d_set_path" not in inspect.getsource(Blur2D.__init__)
    assert Blur2D.PATHS == {"auto": AUTO, "slide": SLIDE, "strip": STRIP, "tile": TILE, "generic": GENERIC}


# ------------------------------------------------------------------------------------------------ PSF builders
@pytest.mark.parametrize("dim", [(21, 21), (10, 10), (16, 31), (63, 63), (64, 40)])
def test_defocus_psf(dim):
    from trips_py_amd.problems import defocus_psf, gauss_psf
    m, n = dim
    for radius in (0, 0.5, 3, 7.5, 100):
        psf, center = defocus_psf(dim, radius)
        assert psf.shape == dim and abs(psf.sum() - 1) < 1e-14 and psf.min() >= 0
        assert list(center) == [m // 2, n // 2]
        assert len(np.unique(psf[psf > 0])) == 1                         # a uniform disc
    delta, center = defocus_psf(dim, 0)
    assert delta[center[0], center[1]] == 1.0 and np.count_nonzero(delta) == 1
    assert np.count_nonzero(defocus_psf(dim, 100)[0]) == m * n
    # on gauss_psf's grid: the disc of radius r is where the unit-spread Gaussian is >= exp(-r^2 / 2)
    g = gauss_psf(dim, 1.0)[0]
    r = 4.0
    assert np.array_equal(defocus_psf(dim, r)[0] > 0, g >= g.max() * np.exp(-r * r / 2) * (1 - 1e-12))
    if m % 2 and n % 2:
        d = defocus_psf(dim, 6.3)[0]
        assert np.array_equal(d, d[::-1, :]) and np.array_equal(d, d[:, ::-1])
    with pytest.raises(ValueError):
        defocus_psf(dim, -1)


def test_motion_psf():
    from trips_py_amd.problems import motion_psf
    for dim, length, angle in [((21, 21), 15, 30), ((31, 31), 20, 30), ((9, 33), 25, 0), ((33, 9), 25, 90), ((10, 10), 5, 45), ((21, 21), 0, 10)]:
        psf, center = motion_psf(dim, length, angle)
        assert psf.shape == dim and abs(psf.sum() - 1) < 1e-14 and psf.min() >= 0 and psf.dtype == np.float64
        assert list(center) == [dim[0] // 2, dim[1] // 2]
    delta, c = motion_psf((7, 9), 0, 33)
    assert delta[c[0], c[1]] == 1.0 and np.count_nonzero(delta) == 1
    h, c = motion_psf((21, 21), 15, 0)                                   # along the column axis: one row
    assert np.count_nonzero(h.sum(axis=1)) == 1 and h[c[0]].sum() == pytest.approx(1.0, abs=1e-14)
    assert np.count_nonzero(h[c[0]]) >= 15
    v, c = motion_psf((21, 21), 15, 90)                                  # one column, up to cos(90 deg) = 6e-17
    off = v.copy()
    off[:, c[1]] = 0
    assert off.max() <= 1e-15 and v[:, c[1]].sum() == pytest.approx(1.0, abs=1e-14)
    d = motion_psf((21, 21), 15, 30)[0]
    assert not C.is_rank1(d)
    # counter-clockwise from the column axis, rows going down: at 30 degrees the right end of the segment is ABOVE the centre
    rows, cols = np.nonzero(d)
    assert rows[cols == cols.max()].max() < 10 < rows[cols == cols.min()].min()
    with pytest.raises(ValueError):
        motion_psf((21, 21), 25, 30)                                     # the segment leaves the array
    with pytest.raises(ValueError):
        motion_psf((5, 21), 15, 80)
    with pytest.raises(ValueError):
        motion_psf((21, 21), -1, 0)


def test_deblurring2d_psf_methods():
    from trips_py_amd.problems import Deblurring2D, defocus_psf, motion_psf
    D = Deblurring2D()
    assert np.array_equal(D.Defocus((21, 21), 9)[0], defocus_psf((21, 21), 9)[0]) and D.spread == 9
    assert np.array_equal(D.Motion((21, 21), 15, 30)[0], motion_psf((21, 21), 15, 30)[0]) and D.spread == (15, 30)


def test_defocus1d_is_the_reference():
    """Deblurring1D.Defocus1D returns the reference's arrays exactly (tools/make_psf_goldens.py): the un-normalised PSF, with the
    normalised one in self.PSF."""
    from trips_py_amd.problems import Deblurring1D
    g = load_golden("psf_defocus1d")
    assert list(g["grid_points"]) == [16, 17, 64] and list(g["parameters"]) == [0, 3, 7.5]
    for n in g["grid_points"]:
        for p in g["parameters"]:
            key = f"{int(n)}_{str(int(p) if p == int(p) else float(p)).replace('.', 'p')}"
            D1 = Deblurring1D()
            ret, center = D1.Defocus1D(int(n), int(p) if p == int(p) else float(p))
            assert np.array_equal(ret, g["ret_" + key]) and np.array_equal(D1.PSF, g["psf_" + key]), key
            assert int(center) == int(g["center_" + key]) and D1.grid_points == n
            if p:
                assert abs(D1.PSF.sum() - 1) < 1e-15 and not np.array_equal(ret, D1.PSF)


# ------------------------------------------------------------------------------------------------ the arithmetic's share of the bar
@pytest.mark.parametrize("name,mode", [("r63x63", "reflect"), ("r63x63", "constant"), ("d63x63", "reflect")])
def test_one_chain_fp32_sum_is_well_inside_the_bar(name, mode):
    """One fp32 fmaf chain of 3969 terms against float64 scipy on the partial-tiles image: measured 1.0e-6 (random, reflect),
    0.9e-6 (random, constant) and 0.7e-6 (defocus, reflect) — the GPU tests' 1e-5 bar has about 9x headroom for the arithmetic
    alone, so a failure there points at the kernel."""
    from trips_py_amd.problems import defocus_psf
    psf = C.make_psf(name) if name in C.PSFS else defocus_psf((63, 63), 28)[0]
    nx, ny = C.IMAGES["2x2_partial"]
    img = np.random.default_rng(63).standard_normal((nx, ny)).astype(np.float32)
    e = relerr(C.chain_fp32(img, psf, mode), convolve(img.astype(np.float64), psf, mode=mode))
    assert np.array_equal(C.convolve_ref(img, psf, mode), convolve(img.astype(np.float64), psf, mode=mode)) or \
        np.allclose(C.convolve_ref(img, psf, mode), convolve(img.astype(np.float64), psf, mode=mode), rtol=0, atol=1e-12)
    print(f"chain_fp32 {name} {mode}: {e:.3e}")
    assert e < 3e-6
