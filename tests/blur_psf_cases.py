"""Cases of the blur's LDS tile kernel (csrc/blur_tile.hip, any PSF up to 64x64), shared by tests/test_blur_psf_host.py and
tests/test_gpu_blur_tile.py: the PSFs, the image shapes that reach every tile situation, a NumPy restatement of the library's
rank-1 test, scipy's boundary extension at any distance, an fp32 emulation of the kernel's one-chain sum and the float64
operator the solver tests hand to the oracle."""
import numpy as np

#: the output tile of k_blur_tile — MIRRORS TILE_H / TILE_W of trips_py_amd/csrc/blur_tile.hip (a 256-thread workgroup owns
#: TH x TW outputs); the image shapes below are built from them
TH, TW = 32, 64

MODES = ["reflect", "constant", "nearest", "mirror", "wrap"]

#: name -> (kind, PSF shape); kinds: 'random' (non-separable unless one side is 1), 'gauss' (separable), 'defocus', 'motion'
PSFS = {
    "r2x2": ("random", (2, 2)),
    "r4x6": ("random", (4, 6)),
    "g10x10": ("gauss", (10, 10)),
    "g16x16": ("gauss", (16, 16)),
    "g17x17": ("gauss", (17, 17)),
    "d21x21": ("defocus", (21, 21)),
    "m21x21": ("motion", (21, 21)),
    "g31x31": ("gauss", (31, 31)),
    "g33x5": ("gauss", (33, 5)),
    "r1x64": ("random", (1, 64)),
    "r64x1": ("random", (64, 1)),
    "r64x40": ("random", (64, 40)),
    "g63x63": ("gauss", (63, 63)),
    "r63x63": ("random", (63, 63)),
}

#: name -> image shape (nx, ny)
IMAGES = {
    "below_one_tile": (5, 8),                    # also: most PSFs above are larger than this image in BOTH axes
    "one_tile": (TH, TW),
    "tile_plus_one": (TH + 1, TW + 1),
    "2x2_partial": (2 * TH + 5, 2 * TW + 22),    # (69, 150): partial last tile row and column, ny % 4 != 0
    "ny_1": (TH + 5, 1),                         # PSFs with kw > 1 are larger than the image in ONE axis
    "nx_1": (1, TW + 6),                         # likewise with kh > 1
}
assert IMAGES["2x2_partial"][1] % 4 != 0

#: the case table: (PSF kind, PSF shape, image shape) by name
CASES = [(p, i) for p in PSFS for i in IMAGES]


def make_psf(name):
    """The float64 PSF of a case, normalised to sum 1 (seeded)."""
    from trips_py_amd.problems import defocus_psf, gauss_psf, motion_psf
    kind, (kh, kw) = PSFS[name]
    if kind == "gauss":
        return gauss_psf((kh, kw), (max(kw / 5.0, 0.8), max(kh / 6.0, 0.8)))[0]
    if kind == "defocus":
        return defocus_psf((kh, kw), 0.45 * min(kh, kw))[0]
    if kind == "motion":
        return motion_psf((kh, kw), 0.7 * min(kh, kw), 30.0)[0]
    rng = np.random.default_rng(1000 * kh + kw)
    psf = rng.random((kh, kw))
    return psf / psf.sum()


def is_rank1(psf):
    """The library's test at creation (trk_blur2d_create_bc), restated: pivot = the first entry of largest magnitude in row-major
    order, col = its column, row = its row / pivot; separable iff every |psf - col row^T| <= 1e-12 max|psf|."""
    psf = np.asarray(psf, dtype=np.float64)
    a = np.abs(psf)
    pmax = a.max()
    if not pmax > 0:
        return False
    pa, pb = np.unravel_index(int(np.argmax(a)), psf.shape)        # argmax: the first maximum, as the strict '>' scan finds
    col, row = psf[:, pb], psf[pa, :] / psf[pa, pb]
    return bool(np.all(np.abs(psf - np.outer(col, row)) <= 1e-12 * pmax))


def expected_form(name):
    return "separable" if is_rank1(make_psf(name)) else "general"


def ext_index(i, n, mode):
    """Image index of sample positions i of a length-n line extended by `mode`, -1 where constant mode reads 0: scipy.ndimage's
    extension rules at any distance."""
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


def convolve_ref(img, psf, mode):
    """float64 scipy.ndimage.convolve(img, psf, mode=mode), valid for a PSF of any size: the image is extended explicitly by
    ext_index to the PSF's whole reach and convolved in 'constant' mode, whose padding the kept part never sees.  Called directly,
    scipy returns garbage (1e250 and the like) once the PSF is many times larger than the image — 64x40 on 5x8 under 'reflect',
    for one — so the direct call cannot be the reference there; tests/test_blur_psf_host.py checks that the two agree to 1e-12 on
    every case and mode of the table but those (scipy_direct_is_sound)."""
    from scipy.ndimage import convolve
    img = np.asarray(img, dtype=np.float64)
    psf = np.asarray(psf, dtype=np.float64)
    kh, kw = psf.shape
    nx, ny = img.shape
    T, L = kh - 1 - kh // 2, kw - 1 - kw // 2
    ri = ext_index(np.arange(-T, nx + kh // 2), nx, mode)
    ci = ext_index(np.arange(-L, ny + kw // 2), ny, mode)
    win = img[np.ix_(np.maximum(ri, 0), np.maximum(ci, 0))]
    win[ri < 0, :] = 0.0
    win[:, ci < 0] = 0.0
    return convolve(win, psf, mode="constant")[T:T + nx, L:L + ny]


def scipy_direct_is_sound(psf_shape, img_shape, mode):
    """False where scipy.ndimage.convolve called directly was seen to return garbage on the table's cases: 'reflect' with a PSF
    more than 12 times as tall as an image of several rows (63 or 64 rows on 5; one-row images are sound)."""
    return not (mode == "reflect" and img_shape[0] > 1 and psf_shape[0] > 12 * img_shape[0])


def chain_fp32(img, psf, mode):
    """scipy.ndimage.convolve(img, psf, mode) as the kernel sums it: fp32 samples and weights, ONE fmaf chain per output from 0,
    PSF rows (of the correlation) ascending outside, columns ascending inside.  Each step is formed in float64 — the product of two
    fp32 numbers is exact there — and rounded to fp32 (a double rounding of the sum, which moves a step by at most half an fp32
    ulp in rare ties: an emulation of the arithmetic's size, not of its bits)."""
    img32 = np.asarray(img, dtype=np.float32)
    kh, kw = psf.shape
    nx, ny = img32.shape
    T, L = kh - 1 - kh // 2, kw - 1 - kw // 2
    c = np.asarray(psf, dtype=np.float64)[::-1, ::-1].astype(np.float32)       # correlation weights
    ri = ext_index(np.arange(-T, nx + kh // 2), nx, mode)
    ci = ext_index(np.arange(-L, ny + kw // 2), ny, mode)
    win = img32[np.ix_(np.maximum(ri, 0), np.maximum(ci, 0))].astype(np.float64)
    win[ri < 0, :] = 0.0
    win[:, ci < 0] = 0.0
    acc = np.zeros((nx, ny), dtype=np.float32)
    for a in range(kh):
        for b in range(kw):
            acc = (np.float64(c[a, b]) * win[a:a + nx, b:b + ny] + acc.astype(np.float64)).astype(np.float32)
    return acc


def scipy_operator(psf, nx, ny, mode):
    """float64 restatement of Blur2D(psf, nx, ny, boundary=mode) for the oracle's solvers: convolve(X, psf, mode) and the
    flipped-PSF "transpose"."""
    from scipy.ndimage import convolve

    from oracle import cpu_ref as O

    class _Op(O._Op):
        def _fwd(s, x):
            return convolve(x.reshape(nx, ny), psf, mode=mode).reshape(-1)

        def _adj(s, y):
            return convolve(y.reshape(nx, ny), psf[::-1, ::-1], mode=mode).reshape(-1)
    op = _Op()
    op.shape = (nx * ny, nx * ny)
    return op
