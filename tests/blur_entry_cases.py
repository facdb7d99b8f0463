"""Cases of the blur's entry-wise tests (tests/test_gpu_blur_entrywise.py), importable without a GPU and checked on the CPU by
tests/test_blur_entry_cases_host.py:

  * a float64 oracle of the blur in Kronecker-factor form, A = sum_a R_a (x) (sum_b psf[a,b] C_b), which returns A x, S = |A||x| and
    T = the count of non-zero products per output (and, for rank-1 PSFs, the same from the two 1-D factor matrices);
  * the blur's dispatch restated in Python with the CU count as an argument — blur_plan and strip_grid MIRROR
    trips_py_amd/csrc/blur_internal.h, slide_grid, the sliding kernel's band geometry and stream_nontemporal MIRROR
    trips_py_amd/csrc/blur2d.hip (and trk_internal.h) — and situations(), which lists the structural situations a shape reaches;
  * the case table: for each situation the smallest shape that reaches it on 256 CUs;
  * the unit combs of the larger shapes and the positions they must cover;
  * fp32 emulations of the two arithmetic families and the per-entry bounds (derived in tests/test_gpu_blur_entrywise.py).
"""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

from blur_psf_cases import IMAGES, MODES, PSFS, chain_fp32, ext_index, is_rank1, make_psf  # noqa: F401  (re-exported)

U32 = 2.0 ** -24                                  # unit roundoff of fp32
CU = 256                                          # compute units of the MI355X: the table is built for it
RANK1_TOL = 1e-12                                 # the library's rank-1 test (trk_blur2d_create_bc)


# ==================================================================================================== oracle
def _line(w, n, mode):
    """The 1-D convolution y[i] = sum_a w[a] x[ext(i + k//2 - a)] of a length-n line extended by `mode` as three sparse n x n
    matrices: the operator, the same with |w| (each tap's magnitude, also where two taps meet on one sample), and the tap count."""
    w = np.asarray(w, dtype=np.float64)
    k, i = len(w), np.arange(n)
    r, c, v = [], [], []
    for a in range(k):
        g = ext_index(i + k // 2 - a, n, mode)
        ok = g >= 0                                # a -1 entry drops the term
        r.append(i[ok])
        c.append(g[ok])
        v.append(np.full(int(ok.sum()), w[a]))
    r, c, v = np.concatenate(r), np.concatenate(c), np.concatenate(v)
    mk = lambda vals: sp.csr_matrix((vals, (r, c)), shape=(n, n))        # noqa: E731  (duplicates are summed)
    return mk(v), mk(np.abs(v)), mk((v != 0).astype(np.float64))


def _select(a, k, n, mode):
    """R_a (or C_b): the 0/1 selection matrix of tap a of a length-k PSF side."""
    e = np.zeros(k)
    e[a] = 1.0
    return _line(e, n, mode)[2]


def rank1_factors(psf):
    """(col, row) with psf ~ col row^T as trk_blur2d_create_bc forms them: pivot = the first entry of largest magnitude."""
    psf = np.asarray(psf, dtype=np.float64)
    pa, pb = np.unravel_index(int(np.argmax(np.abs(psf))), psf.shape)
    return psf[:, pb].copy(), psf[pa, :] / psf[pa, pb]


def _rmul(M, X):
    """X M^T for a sparse M and a dense X, 64 rows at a time (the two transposes then stay in cache: half the time at 4096^2)."""
    out = np.empty(X.shape)
    for r in range(0, X.shape[0], 64):
        out[r:r + 64] = (M @ np.ascontiguousarray(X[r:r + 64].T)).T
    return out


class Oracle:
    """float64 scipy.ndimage.convolve(X, p, mode) with p = psf (tr = False) or psf[::-1, ::-1] (the "transpose").

    apply(x) -> dict of (nx, ny) float64 arrays for an fp32 image x:
        y  = A x
        S  = |A||x|  (every tap's magnitude times every sample's)
        T  = the number of non-zero products of each output
        P  = sum_j pattern_ij |x_j|  (the factorisation term of the separable bound; rank-1 PSFs only)
        Tc = the number of non-zero terms of each output's COLUMN chain (rank-1 PSFs only: the row pass's results that are not 0)
    For a PSF that passes the library's rank-1 test the four come from the two 1-D factor matrices, A x = A_r X A_c^T (two sparse
    products); otherwise from kh row / column factor pairs.  matrix() returns the explicit sparse (A, |A|, count): small images."""

    def __init__(self, psf, nx, ny, mode, tr=False):
        psf = np.asarray(psf, dtype=np.float64)
        self.nx, self.ny, self.mode, self.tr = nx, ny, mode, tr
        self.kh, self.kw = psf.shape
        self.pmax = float(np.abs(psf).max())
        self.rank1 = is_rank1(psf)                 # the library tests the PSF as given, once, for both directions
        self.p = psf[::-1, ::-1] if tr else psf
        if self.rank1:
            col, row = rank1_factors(psf)
            if tr:
                col, row = col[::-1], row[::-1]
            self.Ar, self.Ac = _line(col, nx, mode), _line(row, ny, mode)
        else:
            self.R = [_select(a, self.kh, nx, mode) for a in range(self.kh)]
            self.M = [_line(self.p[a], ny, mode) for a in range(self.kh)]

    def _sum(self, which, X):
        if self.rank1:
            return self.Ar[which] @ _rmul(self.Ac[which], X)
        out = np.zeros((self.nx, self.ny))
        for Ra, Ma in zip(self.R, self.M):
            out += Ra @ _rmul(Ma[which], X)
        return out

    def apply(self, x):
        X = np.asarray(x, dtype=np.float64).reshape(self.nx, self.ny)
        aX, nz = np.abs(X), (X != 0).astype(np.float64)
        out = {"y": self._sum(0, X), "S": self._sum(1, aX)}
        ones = lambda M: np.asarray(M.sum(axis=1)).reshape(-1)                  # noqa: E731
        if self.rank1:
            out["P"] = self._sum(2, aX)
            if nz.all():                           # no zero sample: the counts are those of the pattern alone
                out["T"], out["Tc"] = np.outer(ones(self.Ar[2]), ones(self.Ac[2])), np.outer(ones(self.Ar[2]), np.ones(self.ny))
            else:
                out["T"] = np.rint(self._sum(2, nz))
                out["Tc"] = np.rint(self.Ar[2] @ (_rmul(self.Ac[2], nz) > 0).astype(np.float64))
        elif nz.all():
            out["T"] = sum(np.outer(ones(Ra), ones(Ma[2])) for Ra, Ma in zip(self.R, self.M))
        else:
            out["T"] = np.rint(self._sum(2, nz))
        return out

    def matrix(self):
        if self.rank1:
            return tuple(sp.kron(self.Ar[w], self.Ac[w], format="csr") for w in range(3))
        return tuple(sum(sp.kron(Ra, Ma[w], format="csr") for Ra, Ma in zip(self.R, self.M)).tocsr() for w in range(3))


def bound(family, kh, kw, S, T, P=None, pmax=None):
    """The per-entry bound of tests/test_gpu_blur_entrywise.py's docstring (derived there): 'general' (T + 2) u S; 'separable'
    (min(T, kw) + min(T, kh) + 3) u S + 1e-12 max|psf| P."""
    if family == "general":
        return (T + 2.0) * U32 * S
    return (np.minimum(T, kw) + np.minimum(T, kh) + 3.0) * U32 * S + RANK1_TOL * pmax * P


def worst_ratio(got, o, family, kh, kw, pmax):
    """(largest |got - A x| / bound over the entries with a non-zero bound, the entry it sits at, number of entries that are not
    exactly 0 where S = 0)."""
    b = bound(family, kh, kw, o["S"], o["T"], o.get("P"), pmax)
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(o["y"].shape) - o["y"])
    pos = b > 0
    bad_zero = int(np.count_nonzero(err[~pos]))
    if not pos.any():
        return 0.0, (0, 0), bad_zero
    ratio = np.divide(err, b, out=np.zeros_like(err), where=pos)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(v) for v in at), bad_zero


# ==================================================================================================== restated dispatch
def _ceil_div(a, b):
    return -(-a // b)


SLIDE_U = {3: 6, 5: 5, 7: 7, 9: 9}                 # lcm(KH, D) of k_blur_slide's instantiations (D = 6, 5, 7, 9)
SPAN, STRIP_TW, STRIP_TH = 256, 128, 32            # blur2d.hip: SPAN, TW, TH
NT_MIN_FLOATS = 11 << 20                           # trk_internal.h kNontemporalMinFloats (stream_nontemporal)


def blur_plan(kh, kw, separable, nx, ny):
    """MIRRORS blur_plan / blur_slide_shape / blur_strip_shape of csrc/blur_internal.h: the kernel of a contiguous, 16-byte aligned
    one-vector apply."""
    if separable and kh == kw and kh % 2 == 1 and 3 <= kh <= 9 and ny % 4 == 0 and ny >= 8 and nx * ny < (1 << 29):
        return "slide"
    if kh == kw and kh % 2 == 1 and 3 <= kh <= 15:
        return "strip"
    if kh <= 64 and kw <= 64:
        return "tile"
    return "generic"


def strip_shape(kh, kw):
    return kh == kw and kh % 2 == 1 and 3 <= kh <= 15


def slide_grid(nx, ny, batch, kh, cus):
    """MIRRORS slide_grid of csrc/blur2d.hip: (spans_x, nbands, rows_per_band)."""
    U = SLIDE_U[kh]
    sx = _ceil_div(ny, SPAN)
    slots = 4.0 * cus
    nb = batch if batch > 0 else 1
    rows = U
    while rows - (kh - 1) < kh + 1:
        rows += U
    rpb, best = rows - (kh - 1), 1e300
    while True:
        r = rows - (kh - 1)
        x = float(sx) * _ceil_div(nx, r) * nb / slots
        g = 1.0 if x <= 1.0 else 0.6 + 0.45 * x + 0.5 * (np.ceil(x) - 1.0)
        last = x <= 1.0 or r >= nx
        if (x * slots <= 3840.0 or last) and rows * g < best:
            best, rpb = rows * g, r
        if last:
            break
        rows += U
    return sx, _ceil_div(nx, rpb), rpb


def strip_grid(nx, ny, batch, cus):
    """MIRRORS strip_grid of csrc/blur_internal.h with tw = 128, th = 32: (strips_x, rows_per_band, nband)."""
    sx, steps = _ceil_div(ny, STRIP_TW), _ceil_div(nx, STRIP_TH)
    want = (4 * cus) // (sx * (batch if batch > 0 else 1))
    want = min(max(want, 1), steps)
    rpb = _ceil_div(steps, want) * STRIP_TH
    return sx, rpb, _ceil_div(nx, rpb)


Band = namedtuple("Band", "i_begin i_end up total interior")


def slide_bands(nx, ny, batch, kh, cus):
    """The bands of k_blur_slide (MIRRORS the kernel's prologue): rows [i_begin, i_end), marching up (odd bands) or down, the
    staged rows it processes (a multiple of U) and whether all of them lie inside the image (no row extension)."""
    U = SLIDE_U[kh]
    _, nbands, rpb = slide_grid(nx, ny, batch, kh, cus)
    out = []
    for b in range(nbands):
        i0, i1 = b * rpb, min(b * rpb + rpb, nx)
        up = b % 2 == 1
        total = _ceil_div(i1 - i0 + kh - 1, U) * U
        first = i1 - 1 + kh // 2 if up else i0 - (kh - 1 - kh // 2)
        last = first + (-1 if up else 1) * (total - 1)
        out.append(Band(i0, i1, up, total, 0 <= first < nx and 0 <= last < nx))
    return out


SLIDE_SITUATIONS = ("slide.ny8", "slide.one_span_inactive_lanes", "slide.interior_span", "slide.band_down", "slide.band_up",
                    "slide.partial_last_band", "slide.band_rows_leave_image", "slide.band_rows_inside_image",
                    "slide.psf_taller_than_image", "slide.unguarded_block", "slide.nt_store")
STRIP_SITUATIONS = ("strip.separable", "strip.direct", "strip.scalar_columns", "strip.last_strip_partial", "strip.several_strips",
                    "strip.several_bands", "strip.several_steps_ring_wrap", "strip.nx_below_k")


def situations(nx, ny, kh, kw, separable, cus, path=None, batch=1):
    """The structural situations an apply of `batch` vectors of an nx x ny image reaches on `cus` compute units; path = 'strip' for
    a slide shape whose operand is not 16-byte aligned (the library routes it to the strip kernel)."""
    path = path or blur_plan(kh, kw, separable, nx, ny)
    out = set()
    if path == "slide":
        U = SLIDE_U[kh]
        sx, nbands, rpb = slide_grid(nx, ny, batch, kh, cus)
        bands = slide_bands(nx, ny, batch, kh, cus)
        if ny == 8:
            out.add("slide.ny8")
        if sx == 1 and ny < SPAN:
            out.add("slide.one_span_inactive_lanes")
        if sx >= 3:
            out.add("slide.interior_span")
        out.add("slide.band_down")
        if nbands >= 2:
            out.add("slide.band_up")
        if nbands >= 2 and nx % rpb:
            out.add("slide.partial_last_band")
        if any(not b.interior for b in bands):
            out.add("slide.band_rows_leave_image")
        if any(b.interior for b in bands):
            out.add("slide.band_rows_inside_image")
        if kh > nx:
            out.add("slide.psf_taller_than_image")
        if any(b.total >= 3 * U for b in bands):       # `for (t0 = U; t0 + U < total; ...)` runs: the unguarded block
            out.add("slide.unguarded_block")
        if nx * ny >= NT_MIN_FLOATS:
            out.add("slide.nt_store")
    elif path == "strip":
        sx, rpb, nband = strip_grid(nx, ny, batch, cus)
        out.add("strip.separable" if separable else "strip.direct")
        if ny % 4:
            out.add("strip.scalar_columns")
        if ny % STRIP_TW:
            out.add("strip.last_strip_partial")
        if sx > 1:
            out.add("strip.several_strips")
        if nband > 1:
            out.add("strip.several_bands")
        if min(rpb, nx) > STRIP_TH:                    # a band of several 32-row steps: the LDS ring wraps around
            out.add("strip.several_steps_ring_wrap")
        if nx < kh:
            out.add("strip.nx_below_k")
    return out


# ==================================================================================================== PSFs and the case table
def entry_psf(name):
    """float64 PSF by name: 'sepK' the outer product of two seeded positive vectors (separable, no symmetry at all), 'rndK' /
    'rndHxW' seeded random (general), else a PSF of blur_psf_cases.PSFS."""
    if name.startswith("sep"):
        k = int(name[3:])
        rng = np.random.default_rng(7000 + k)
        c, r = rng.uniform(0.2, 1.0, k), rng.uniform(0.2, 1.0, k)
        return np.outer(c / c.sum(), r / r.sum())
    if name.startswith("rnd"):
        kh, _, kw = name[3:].partition("x")
        kh = int(kh)
        kw = int(kw) if kw else kh
        psf = np.random.default_rng(9000 + 100 * kh + kw).random((kh, kw))
        return psf / psf.sum()
    return make_psf(name)


Case = namedtuple("Case", "psf shape path")        # path: the kernel of the case's OWN apply on 256 CUs ('strip_view': offset view)


def _family(psf_name, path):
    sep = is_rank1(entry_psf(psf_name))
    return "general" if path == "generic" or not sep else "separable"


# the sliding kernel's shapes, smallest first; which situations each reaches is asserted by the host test
#   (2, 16)     every PSF is taller than the image; one span, inactive lanes; one band
#   (12, 8)     the two edge lanes are neighbours; two or three bands (down, up, partial last)
#   (37, 520)   three spans (one interior, the last with inactive lanes); bands up and down, with and without row extension
SLIDE_SMALL = [(2, 16), (12, 8)]
SLIDE_COMB = [(37, 520)]
# the smallest image whose bands are tall enough for the unguarded steady-state block, by K (ny = 8: one span, so the wave count
# that makes slide_grid choose taller bands comes from the rows alone); asserted by the host test
SLIDE_UNGUARDED = {3: (12289, 8), 5: (6145, 8), 7: (8193, 8), 9: (10241, 8)}
SLIDE_NT = (4096, 4096)                            # the benchmarked size (9x9)
SLIDE_NT_SMALLEST = (2816, 4096)                   # 11 << 20 pixels: the smallest 4096-column image stored non-temporally (3x3 .. 7x7)

# the strip kernel's shapes
#   (5, 7)      nx < K and ny < K for every K >= 7 (9x9 and up are larger than the image both ways), scalar columns
#   (37, 53)    ny % 4 != 0, a last strip that ends outside the image, two bands
#   (70, 260)   three strips, three bands, aligned 16-byte loads and stores
#   (40, 65540) 513 strips: more than 4 x 256 / 2, so both 32-row steps fall to one band and the second wraps around the LDS ring
STRIP_SMALL = [(5, 7), (37, 53)]
STRIP_COMB = [(70, 260)]
STRIP_WRAP = (40, 65540)
STRIP_K_SEP, STRIP_K_DIRECT = (11, 13, 15), (3, 5, 7, 9, 11, 13, 15)


def reaches_unguarded(nx, ny, kh, cus):
    """slide_grid gives the image bands of at least 3 U staged rows (cheaper than situations(): the band height alone)."""
    rpb = slide_grid(nx, ny, 1, kh, cus)[2]
    return _ceil_div(min(rpb, nx) + kh - 1, SLIDE_U[kh]) * SLIDE_U[kh] >= 3 * SLIDE_U[kh]


def small_cases():
    """Cases of at most about 2500 pixels: the whole matrix is compared."""
    out = []
    for k in SLIDE_U:
        out += [Case(f"sep{k}", s, "slide") for s in SLIDE_SMALL]
        out += [Case(f"sep{k}", s, "strip_view") for s in SLIDE_SMALL]
    for k in STRIP_K_SEP:
        out += [Case(f"sep{k}", s, "strip") for s in STRIP_SMALL]
    for k in STRIP_K_DIRECT:
        out += [Case(f"rnd{k}", s, "strip") for s in STRIP_SMALL]
    out += [Case("r2x2", IMAGES["below_one_tile"], "tile"), Case("r4x6", (33, 17), "tile"), Case("g10x10", (33, 17), "tile"),
            Case("r64x40", IMAGES["below_one_tile"], "tile"), Case("g17x17", (33, 17), "tile"),
            Case("rnd65x3", IMAGES["below_one_tile"], "generic"), Case("rnd3x70", (33, 17), "generic")]
    return out


def comb_cases():
    """Larger cases: unit combs and the three real inputs."""
    out = []
    for k in SLIDE_U:
        out += [Case(f"sep{k}", s, "slide") for s in SLIDE_COMB]
        out += [Case(f"sep{k}", s, "strip_view") for s in SLIDE_COMB]
        out.append(Case(f"sep{k}", SLIDE_UNGUARDED[k], "slide"))
    for k in STRIP_K_SEP:
        out += [Case(f"sep{k}", s, "strip") for s in STRIP_COMB]
    for k in STRIP_K_DIRECT:
        out += [Case(f"rnd{k}", s, "strip") for s in STRIP_COMB]
    for p in PSFS:                                  # the tile kernel's table (blur_psf_cases), generic forced on the same
        out.append(Case(p, IMAGES["2x2_partial"], "tile"))
    for p in ("r4x6", "g17x17", "r64x40", "r1x64", "r64x1"):
        for i in ("below_one_tile", "one_tile", "tile_plus_one", "ny_1", "nx_1"):
            out.append(Case(p, IMAGES[i], "tile"))
    out.append(Case("rnd65x3", IMAGES["2x2_partial"], "generic"))
    return out


def wrap_cases():
    """The strip kernel's ring wrap-around: one separable and one direct PSF on the one shape that reaches it on 256 CUs."""
    return [Case("sep11", STRIP_WRAP, "strip"), Case("rnd3", STRIP_WRAP, "strip")]


def assert_coverage(cus):
    """Every listed situation is reached by the case table on `cus` compute units (the host test: 256; the GPU test: the device's)."""
    reached = {}
    cases = small_cases() + comb_cases() + wrap_cases() + nt_cases()
    for c in cases:
        assert planned_path(c) == {"strip_view": "slide"}.get(c.path, c.path), case_id(c)   # (a view: a slide shape, misaligned)
        k = entry_psf(c.psf).shape[0]
        for s in case_situations(c, cus):
            reached.setdefault((s, k if s.startswith("slide") else 0), []).append(case_id(c))
    for k in SLIDE_U:
        for s in SLIDE_SITUATIONS:
            assert (s, k) in reached, (s, k)
    for s in STRIP_SITUATIONS:
        assert (s, 0) in reached, s
    # separable 11 .. 15 and direct 3 .. 15 on the strip kernel, and the slide shapes through the offset view
    strip = {(c.psf, c.path) for c in cases if c.path in ("strip", "strip_view")}
    assert {(f"sep{k}", "strip") for k in STRIP_K_SEP} <= strip and {(f"rnd{k}", "strip") for k in STRIP_K_DIRECT} <= strip
    assert {(f"sep{k}", "strip_view") for k in SLIDE_U} <= strip
    # every PSF and every image of the tile kernel's table
    assert set(PSFS) <= {c.psf for c in cases if c.path == "tile"}
    assert set(IMAGES.values()) <= {c.shape for c in cases if c.path == "tile"}
    return reached


def nt_cases():
    """The images large enough for the sliding kernel's non-temporal stores: 9x9 at the benchmarked size, the others at the threshold."""
    return [Case(f"sep{k}", SLIDE_NT if k == 9 else SLIDE_NT_SMALLEST, "slide") for k in SLIDE_U]


def case_id(c):
    return f"{c.psf}-{c.shape[0]}x{c.shape[1]}-{c.path}"


def case_situations(c, cus):
    psf = entry_psf(c.psf)
    kh, kw = psf.shape
    path = "strip" if c.path == "strip_view" else None
    return situations(c.shape[0], c.shape[1], kh, kw, is_rank1(psf), cus, path=path)


def case_family(c):
    return _family(c.psf, c.path)


def planned_path(c):
    psf = entry_psf(c.psf)
    return blur_plan(psf.shape[0], psf.shape[1], is_rank1(psf), c.shape[0], c.shape[1])


# ==================================================================================================== inputs
def real_inputs(nx, ny, seed):
    """The three inputs of check (D), fp32: white noise; uniform [0, 1) (no cancellation: S = A x for a positive PSF, the bound is
    relative to the output itself); a smooth ramp under a Hanning profile."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    ramp = (1.0 + i / max(nx, 1) + 2.0 * j / max(ny, 1)) * np.outer(np.hanning(nx + 2)[1:-1], np.hanning(ny + 2)[1:-1])
    return {"noise": rng.standard_normal((nx, ny)).astype(np.float32), "uniform": rng.random((nx, ny)).astype(np.float32),
            "ramp": ramp.astype(np.float32)}


def _partition(required, gap):
    """Sorted positions -> lists in each of which neighbours are at least `gap` apart (greedy, first fit)."""
    sets = []
    for p in sorted(set(required)):
        for s in sets:
            if p - s[-1] >= gap:
                s.append(p)
                break
        else:
            sets.append([p])
    return sets


def required_rows(c, cus):
    """Rows a case's combs must hit: both borders; on the slide path the first and last row of the first two (a down- and an
    up-marching) and the last two bands and U consecutive rows of a down- and of an up-marching band (every row phase modulo the
    unroll); on the strip path the first and last row of every band and 32-row step."""
    nx, ny = c.shape
    k = entry_psf(c.psf).shape[0]
    req = {0, nx - 1}
    if c.path == "slide":
        bands = slide_bands(nx, ny, 1, k, cus)
        pick = bands[:2] + bands[-2:]
        for b in pick:
            req |= {b.i_begin, b.i_end - 1}
        for b in bands[:2]:
            req |= set(range(b.i_begin, min(b.i_begin + SLIDE_U[k], b.i_end)))
    elif c.path in ("strip", "strip_view"):
        for i0 in range(0, nx, STRIP_TH):
            req |= {i0, min(i0 + STRIP_TH, nx) - 1}
    else:                                           # tile / generic: the 32-row tile seams
        for i0 in range(0, nx, 32):
            req |= {i0, min(i0 + 32, nx) - 1}
    return sorted(r for r in req if 0 <= r < nx)


def required_cols(c):
    """Columns a case's combs must hit: both borders (the two edge lanes), every column position modulo 4, both sides of every
    span seam (256), strip seam (128) and tile seam (64)."""
    ny = c.shape[1]
    seam = {"slide": SPAN, "strip": STRIP_TW, "strip_view": STRIP_TW}.get(c.path, 64)
    req = {0, 1, 2, 3, ny - 1, ny - 2, ny - 3, ny - 4}
    for s in range(seam, ny, seam):
        req |= {s - 1, s}
    return sorted(q for q in req if 0 <= q < ny)


def combs(c, cus, seed=0):
    """Unit combs of a case, fp32 (nx, ny) images of zeros and ones: ones at rows x columns of sets whose members are at least a PSF
    side apart (so that away from the borders every output is ONE product), the required positions first, then a seeded lattice
    filling the rest.  Together the combs hit every required row and every required column, and the corners."""
    nx, ny = c.shape
    kh, kw = entry_psf(c.psf).shape
    rng = np.random.default_rng(seed + 17 * nx + ny)
    rsets, csets = _partition(required_rows(c, cus), kh), _partition(required_cols(c), kw)
    rsets.insert(0, sorted({0, nx - 1}))            # the corner comb (its ones may be closer than a PSF side on a narrow image)
    csets.insert(0, sorted({0, ny - 1}))
    out = []
    for q in range(max(len(rsets), len(csets))):
        rows, cols = list(rsets[q % len(rsets)]), list(csets[q % len(csets)])
        for pos, n, k in ((rows, nx, kh), (cols, ny, kw)):           # fill with a lattice of a seeded period and offset
            step = k + int(rng.integers(0, 4))
            cand = np.arange(int(rng.integers(0, step)), n, step)          # at least k apart among themselves
            have = np.sort(np.asarray(pos))
            at = np.searchsorted(have, cand)
            lo, hi = have[np.maximum(at - 1, 0)], have[np.minimum(at, len(have) - 1)]
            pos.extend(cand[(np.abs(cand - lo) >= k) & (np.abs(cand - hi) >= k)].tolist())
        x = np.zeros((nx, ny), dtype=np.float32)
        x[np.ix_(sorted(rows), sorted(cols))] = 1.0
        out.append(x)
    return out


# ==================================================================================================== fp32 emulations
def _window(img32, kh, kw, mode):
    nx, ny = img32.shape
    T, L = kh - 1 - kh // 2, kw - 1 - kw // 2
    ri = ext_index(np.arange(-T, nx + kh // 2), nx, mode)
    ci = ext_index(np.arange(-L, ny + kw // 2), ny, mode)
    win = img32[np.ix_(np.maximum(ri, 0), np.maximum(ci, 0))].astype(np.float64)
    win[ri < 0, :] = 0.0
    win[:, ci < 0] = 0.0
    return win


def sep_weights(psf, tr):
    """(wr, wc): the fp32 row and column correlation weights of the separable kernels, sf / st of trk_blur2d_create_bc."""
    col, row = rank1_factors(psf)
    if tr:
        return row.astype(np.float32), col.astype(np.float32)
    return row[::-1].astype(np.float32), col[::-1].astype(np.float32)


def sep_fp32(img, psf, mode, tr=False, up_rows=None, wr=None, wc=None, win=None):
    """The separable kernels' arithmetic: fp32 factors, a row pass (one fmaf chain per staged row and column, taps ascending), then a
    column pass over the row pass's results — image rows ascending (a band marching down, the strip and tile kernels), or descending
    for the rows flagged in `up_rows` (a band marching up).  Each step is formed in float64 and rounded to fp32 (an emulation of the
    arithmetic's size, as blur_psf_cases.chain_fp32).  wr / wc / win replace the weights or the extended window (mutations)."""
    img32 = np.asarray(img, dtype=np.float32)
    kh, kw = psf.shape
    nx, ny = img32.shape
    w_r, w_c = sep_weights(psf, tr)
    wr = w_r if wr is None else wr
    wc = w_c if wc is None else wc
    win = _window(img32, kh, kw, mode) if win is None else win
    h = np.zeros((nx + kh - 1, ny), dtype=np.float32)
    for b in range(kw):
        h = (np.float64(wr[b]) * win[:, b:b + ny] + h.astype(np.float64)).astype(np.float32)
    h = h.astype(np.float64)
    down = np.zeros((nx, ny), dtype=np.float32)
    for a in range(kh):
        down = (np.float64(wc[a]) * h[a:a + nx] + down.astype(np.float64)).astype(np.float32)
    if up_rows is None or not np.any(up_rows):
        return down
    up = np.zeros((nx, ny), dtype=np.float32)
    for a in range(kh - 1, -1, -1):
        up = (np.float64(wc[a]) * h[a:a + nx] + up.astype(np.float64)).astype(np.float32)
    return np.where(np.asarray(up_rows, dtype=bool)[:, None], up, down)


def up_rows_of(c, cus, batch=1):
    """Boolean per image row: the row belongs to a band of the sliding kernel that marches upward (all False on other paths)."""
    nx, ny = c.shape
    up = np.zeros(nx, dtype=bool)
    if c.path == "slide":
        for b in slide_bands(nx, ny, batch, entry_psf(c.psf).shape[0], cus):
            up[b.i_begin:b.i_end] = b.up
    return up
