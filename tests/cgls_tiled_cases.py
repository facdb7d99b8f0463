"""Cases, float64 references and bounds of ONE iteration of the tiled small-image CGLS (csrc/cgls_tiled.hip: k_cgls_tile_a,
k_cgls_tile_b<HAS_XT>, k_cgls_tile_a2, k_cgls_tile_b2<HAS_XT> behind trk_cgls_iterate_tiled / trk_cgls_iterate_tiled2), built with NumPy
alone: tests/test_cgls_tiled_cases_host.py checks the cases themselves on the CPU, tests/test_gpu_cgls_tiled_entrywise.py runs them
through the kernels.

The iteration, restated in float64 ON THE fp32 OPERANDS EACH STAGE HAS (`iteration`): a later stage is evaluated on the device's own
earlier outputs when the GPU test hands them in (`dev`), so every stage is judged alone.  A / A^T are
blur_entry_cases.Oracle(psf, nx, ny, "reflect", tr): y = A x with S = |A||x|, T and P for the bound.

  scalars     gk = sum of the gamma partials handed in (n_g of them);  beta32 = (float)(gk / gprev), 0 when `first`;
              delta = sum of the device's PD;  alpha32 = (float)(gk / delta)                          (vec_cases.step32)
  form 1      p' = fma32(beta, p_old, t)                                  K_A, bit for bit
              PD[tile] = sum over the tile of w^2, w = A p'               K_A forms w as fma32(beta, fl(A p_old), fl(A t))
              r' = fma32(-alpha, w, r_old), w = fl(A p') again            K_B
              t' = A^T r'                                                 K_B
              d = fl32(alpha p'),  x' = fma32(alpha, p', x)               K_B: the kernel's `xv + alpha * p` is compiled contracted, the one
                                                                          correctly rounded operation of trk.h's other x updates
  form 2      q = A t ;  w' = fma32(beta, w_old, q)                       K_A2 (w_old, p_old not read when `first`)
              p' as above;  PD[tile] = sum of w'^2 (the device's w')      K_A2
              r' = fma32(-alpha, w', r_old)                               K_B2, bit for bit given the device's w'
              t', d, x' as above                                          K_B2
  both        PG[tile] = sum t'^2;  NP[3 tile + 0, 1, 2] = sum x'^2, sum d^2, sum (x' - x_true)^2 (0 without x_true)

Exact cases make every stage exact in float32, so a device result must EQUAL its reference:
  PSFs       rank 1, col row^T / 16 with integer factor taps (`taps`): distinct, signs mixed, no factor equal to its flip, the two factors
             of a square PSF different, the largest tap of each factor a power of two (the library divides the pivot row by the
             pivot: it must stay dyadic).  A flipped factor, the forward weights in place of the transposed ones, a row factor in
             place of a column factor or an anchor off by one changes entries.
  vectors    integers in [-3, 3] drawn per index (`ints`)
  scalars    beta = 1/2 (gprev = 2 gk) and alpha = 1/4 (gk = delta / 4, delta the exact sum of the exact PD), the gamma partials
             vec_cases.partials(n_g, 1) with the last one moved so that they total gk
  `exact_margins` proves the precondition: every intermediate of both passes of every blur, every update and every sum is an integer
  multiple of its unit below 2^24 units (float32) or 2^53 (the float64 sums), in the manner of framelet_cases.exact_margin.

General cases: gauss_psf PSFs of 3, 5, 7 and 9 taps, a rectangular spread, an asymmetric real rank-1 PSF; standard-normal vectors;
beta near 3/7.  Bounds, u = 2^-24 (each is the arithmetic below, none is a measured number):
  a blurred stage y = fl(A v)        b(v) = blur_entry_cases.bound("separable", kh, kw, S, T, P, max|psf|)
                                          = (min(T, kw) + min(T, kh) + 3) u S + 1e-12 max|psf| P
                                     which fits blur_lds as written: one rounding per factor tap, at most kw fmas on one accumulator
                                     (the taps a narrower PSF is padded with are zeros: fma(0, v, a) = a), an fp32 store between the
                                     passes, at most kh fmas.  Where b = 0 the result must be exactly 0.
  form 1, r'                         alpha b(p') + u (|r'| + alpha b(p'))
  form 1, PD[tile]                   K_A's w = fl(beta fl(A p_old) + fl(A t)) against A p' with p' = fl(t + beta p_old):
                                     e = b(t) + |beta| b(p_old);  bw = e + u (|A p'| + e) + u |A||p'|   (the last term: p' is rounded)
                                     PD: sum over the tile of 2 |A p'| bw + bw^2, plus the float64 sum's (1024 + 64) 2^-53 sum w^2
  form 2, w'                         b(t) + u (|w'| + b(t))
  t'                                 b(r') with the transposed oracle
  PG, NP, form 2's PD                float64 sums of exact squares of the device's own fp32 values: (1024 + 64) 2^-53 of the sum
  delta, S[5k]                       ntiles 2^-52 relative to the float64 sum of the device's PD
`emulated_fraction` runs blur_entry_cases.sep_fp32 (the two fp32 passes on the CPU) for information: over the general PSFs on 35 x 33
it reaches 0.04 (g9) to 0.21 (g3) of b in either direction (test_cgls_tiled_cases_host.test_fp32_emulation_stays_inside_the_bound
prints the figures); the kernels on the MI355X reach 0.07 - 0.32 over all shapes (profiles/cgls_tiled/bars.txt).

The shape table (`SHAPES`): for each structural situation of the 32 x 32 tiles with their 4- and 8-pixel halos the smallest shape that
reaches it; `situations` lists what a shape reaches from a restatement of the kernels' index arithmetic (`refl`, the mirror fill).
`tile_model` restates the four kernels' index logic tile by tile in float64 (LDS tiles, centred 9-tap weights, reflective loads, mirror
fill); on the exact cases it equals `iteration`, and with one of MUTANTS applied it must not.
"""
import functools
import math

import numpy as np

import blur_entry_cases as B
import vec_cases as V

CT, CH = 32, 4
E1, E2 = CT + 2 * CH, CT + 4 * CH
U32, U53 = 2.0 ** -24, 2.0 ** -53
MAX_TILES = 1024                     # partials_issue reads 64 lanes x 16 partials
PMAX_PARTIALS = 1024
SUM_TERMS = CT * CT + 64             # additions of one tile's float64 sum: 1024 terms and the wave / block trees

# ------------------------------------------------------------------------------------------------------------ shape table
#: (nx, ny): nx rows of ny pixels.  Axis lengths 16 (one partial tile, folds clamped), 19 / 20 (last clamped / first unclamped), 32 (one
#: full tile, every halo cell a mirror), 33 / 35 / 36 (a second tile of 1 - 3 rows folds past the far edge; 36 is the first that does
#: not), 40 (the second tile exactly two halos deep), 64, 65, 100 (interior tiles with all eight neighbours and a partial one) on both
#: axes; ny = 17, 19, 33, 35 are reached through the C ABI only; (100, 16) is the tall-narrow pair, (16, 65) the wide one.
SHAPES = [(16, 16), (19, 17), (20, 19), (32, 32), (33, 35), (35, 33), (36, 20), (40, 36), (64, 40), (65, 64), (100, 100), (100, 16),
          (16, 65)]
AXIS_LENGTHS = (16, 19, 20, 32, 33, 35, 36, 40, 64, 65, 100)
PSF_SIDES = [(3, 3), (5, 5), (7, 7), (9, 9), (1, 9), (9, 1), (3, 9), (2, 2), (4, 6), (8, 8)]
GENERAL_PSFS = ("g3", "g5", "g7", "g9", "g5x9", "asym7x4")
N_G = (1, 3, 64, 65, 1024, 1025, 2048, 4096)
PCAP = 4096
SITUATIONS = ("fold.clamped.x", "fold.clamped.y", "fold.clamped.one_tile", "fold.clamped.second_tile", "fold.unclamped.far",
              "mirror.inside.near", "mirror.inside.far", "mirror.outside.x", "mirror.outside.y", "tile.interior", "tile.full_single",
              "tile.partial.x", "tile.partial.y", "tile.partial.both", "tile.two_halos_deep", "tiles.several.x", "tiles.several.y")


def ceil_div(a, b):
    return -(-a // b)


def tiles(nx, ny):
    """(tiles along x (rows), tiles along y): tile `ty * tiles_y + tx` owns rows [32 ty, 32 ty + 32) and columns [32 tx, ...)."""
    return ceil_div(nx, CT), ceil_div(ny, CT)


def ntiles(nx, ny):
    a, b = tiles(nx, ny)
    return a * b


def refl(i, n, clamp=True):
    """refl of cgls_tiled.hip: one half-sample fold, then the clamp."""
    i = np.asarray(i)
    f = np.where(i < 0, -1 - i, np.where(i >= n, 2 * n - 1 - i, i))
    return np.clip(f, 0, n - 1) if clamp else f


def axis_facts(n):
    """What the tiles of one axis of length n reach: a set of 'clamped', 'clamped.one_tile', 'clamped.second_tile', 'unclamped.far',
    'mirror.near', 'mirror.far', 'mirror.outside', 'partial', 'interior', 'two_halos_deep', 'several', 'full_single'."""
    out = set()
    nt = ceil_div(n, CT)
    if nt > 1:
        out.add("several")
    if n == CT:
        out.add("full_single")
    for k in range(nt):
        i0 = k * CT
        load = np.arange(i0 - 2 * CH, i0 - 2 * CH + E2)            # K_B's p on tile + 8 (K_A's tile + 4 lies inside it)
        f = refl(load, n, clamp=False)
        if ((f < 0) | (f >= n)).any():
            out.update(("clamped", "clamped.one_tile" if nt == 1 else "clamped.second_tile"))
        elif (load >= n).any():
            out.add("unclamped.far")
        cells = np.arange(i0 - CH, i0 - CH + E1)
        outside = (cells < 0) | (cells >= n)
        m = refl(cells, n) - (i0 - CH)
        inside = (m >= 0) & (m < E1)
        if (outside & inside & (cells < 0)).any():
            out.add("mirror.near")
        if (outside & inside & (cells >= n)).any():
            out.add("mirror.far")
        if (outside & ~inside).any():
            out.add("mirror.outside")
        if i0 + CT > n:
            out.add("partial")
        if n - i0 == 2 * CH:
            out.add("two_halos_deep")
        if 0 < k and i0 + 2 * CT <= n:
            out.add("interior")
    return out


def situations(nx, ny):
    """The structural situations (of SITUATIONS) the kernels reach on an nx x ny image."""
    fx, fy = axis_facts(nx), axis_facts(ny)
    out = set()
    for f, a in ((fx, "x"), (fy, "y")):
        if "clamped" in f:
            out.add("fold.clamped." + a)
        for s in ("clamped.one_tile", "clamped.second_tile", "unclamped.far"):
            if s in f:
                out.add("fold." + s)
        if "mirror.near" in f:
            out.add("mirror.inside.near")
        if "mirror.far" in f:
            out.add("mirror.inside.far")
        if "mirror.outside" in f:
            out.add("mirror.outside." + a)
        if "partial" in f:
            out.add("tile.partial." + a)
        if "two_halos_deep" in f:
            out.add("tile.two_halos_deep")
        if "several" in f:
            out.add("tiles.several." + a)
    if "partial" in fx and "partial" in fy:
        out.add("tile.partial.both")
    if "interior" in fx and "interior" in fy:
        out.add("tile.interior")
    if "full_single" in fx and "full_single" in fy:
        out.add("tile.full_single")
    return out


def tile_sums(a, nx, ny):
    """Per-tile float64 sums of an (nx, ny) float64 array, in the kernels' tile order."""
    a = np.asarray(a, dtype=np.float64).reshape(nx, ny)
    tx, ty = tiles(nx, ny)
    return np.array([math.fsum(a[i * CT:(i + 1) * CT, j * CT:(j + 1) * CT].reshape(-1)) for i in range(tx) for j in range(ty)])


def tile_of(i, j, ny):
    return (i // CT) * ceil_div(ny, CT) + j // CT


# ------------------------------------------------------------------------------------------------------------ PSFs
_SMALL = ([3, -2, 1, -3, 2, -1, -4, 4], [1, -2, 3, -1, 2, -3, 4, -4])


def taps(k, which):
    """Integer taps of one factor of an exact PSF (`which` 0: the column factor, kh taps; 1: the row factor, kw taps): distinct, the
    largest a power of two and alone in magnitude, no factor its own flip, the two factors of one length different."""
    if k == 1:
        return np.array([4.0])
    s = _SMALL[which][:k - 1]
    top = 2 ** int(max(abs(v) for v in s)).bit_length()            # the smallest power of two above every other tap
    j = k // 3 if which else (2 * k) // 3
    return np.array(s[:j] + [top] + s[j:], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def exact_psf(kh, kw):
    """col row^T / 16 with col = taps(kh, 0), row = taps(kw, 1): every entry a multiple of 1/16."""
    return np.outer(taps(kh, 0) / 4.0, taps(kw, 1) / 4.0)


@functools.lru_cache(maxsize=None)
def general_psf(name):
    from trips_py_amd.problems import gauss_psf
    if name == "g5x9":
        return gauss_psf((5, 9), (2.5, 1.25))[0]
    if name == "asym7x4":                                         # real, rank 1, neither factor symmetric, an even side
        col = np.array([0.02, 0.11, 0.31, 0.27, 0.16, 0.09, 0.04])
        row = np.array([0.45, 0.3, 0.17, 0.08])
        return np.outer(col, row)
    k = int(name[1:])
    return gauss_psf((k, k), (k / 3.0, k / 3.0))[0]


def psf_of(case):
    return exact_psf(*case.psf) if case.exact else general_psf(case.psf)


@functools.lru_cache(maxsize=64)
def oracles(psf_key, exact, nx, ny):
    psf = exact_psf(*psf_key) if exact else general_psf(psf_key)
    return B.Oracle(psf, nx, ny, "reflect", False), B.Oracle(psf, nx, ny, "reflect", True)


def blur_bound(o, orc):
    return B.bound("separable", orc.kh, orc.kw, o["S"], o["T"], o["P"], orc.pmax)


# ------------------------------------------------------------------------------------------------------------ cases
class Case:
    """One call with n_iters = 1: the shape, the PSF (a (kh, kw) pair of exact_psf or a name of general_psf), the form, k_first, the
    number of gamma partials handed in, whether x_true is given, keep_history."""

    def __init__(self, nx, ny, psf, exact, form, k_first=1, n_g=3, with_xt=True, keep=0):
        self.nx, self.ny, self.psf, self.exact, self.form = nx, ny, psf, bool(exact), form
        self.k_first, self.n_g, self.with_xt, self.keep = k_first, n_g, bool(with_xt), int(keep)

    @property
    def n(self):
        return self.nx * self.ny

    @property
    def first(self):
        return self.k_first == 1

    @property
    def id(self):
        p = "%dx%d" % self.psf if self.exact else self.psf
        return f"f{self.form}-{self.nx}x{self.ny}-{p}-k{self.k_first}-g{self.n_g}-{'xt' if self.with_xt else 'noxt'}-h{self.keep}"

    def key(self):
        return (self.nx, self.ny, self.psf, self.exact, self.form, self.k_first, self.n_g, self.with_xt, self.keep)


def shape_cases(exact):
    """Every shape with every PSF of its kind and both forms; k_first, x_true and keep_history rotate so that each value meets each
    form, clamped and unclamped shapes, one tile and several."""
    out = []
    psfs = PSF_SIDES if exact else GENERAL_PSFS
    i = 0
    for s, (nx, ny) in enumerate(SHAPES):
        for p in psfs:
            for form in (1, 2):
                out.append(Case(nx, ny, p, exact, form, k_first=1 + (i + s) % 3, n_g=(3, 1, 64)[(i // 2) % 3],
                                with_xt=(i // 3) % 2 == 0, keep=(i // 5) % 2))
                i += 1
    return out


def source_cases():
    """The gamma sources: every n_g of N_G, both forms, k_first = 1, 2, 3, on one two-tile shape with exact operands."""
    return [Case(33, 35, (3, 3), True, form, k_first=k, n_g=g, with_xt=(g % 2 == 1), keep=k % 2)
            for form in (1, 2) for g in N_G for k in (1, 2, 3)]


def ints(n, *key):
    return np.random.default_rng([7, n, *key]).integers(-3, 4, size=n).astype(np.float32)


def normals(n, *key):
    return np.random.default_rng([11, n, *key]).standard_normal(n).astype(np.float32)


def _partials_to(total, n_g, unit):
    pg, tot = V.partials(n_g, unit)
    pg = pg.copy()
    pg[-1] += total - tot
    return pg


@functools.lru_cache(maxsize=None)
def _state(key):
    case = Case(*key)
    n, gen = case.n, ints if case.exact else normals
    seed = (case.nx, case.ny, case.form, case.k_first)
    st = {name: gen(n, i, *seed) for i, name in enumerate(("t", "p", "w", "r", "x", "xt"))}
    if not case.with_xt:
        st["xt"] = None
    oF, _ = oracles(case.psf, case.exact, case.nx, case.ny)
    if case.exact:
        beta = np.float32(0.0 if case.first else 0.5)
        p_old = np.zeros(n, np.float32) if (case.first and case.form == 2) else st["p"]
        if case.form == 1:
            w = oF.apply(V.fma32(beta, p_old, st["t"]))["y"]
        else:
            w = oF.apply(st["t"])["y"] + np.float64(beta) * (0.0 if case.first else st["w"].astype(np.float64).reshape(case.nx, case.ny))
        delta = float(np.sum(w * w))
        gk = delta / 4.0
        st["gprev"] = 2.0 * gk
        st["pg"] = _partials_to(gk, case.n_g, 1)
    else:
        gk = float(np.sum(st["t"].astype(np.float64) ** 2))
        rng = np.random.default_rng([13, case.n_g, *seed])
        pg = rng.random(case.n_g) + 0.5
        st["pg"] = pg * (gk / math.fsum(pg))
        st["gprev"] = math.fsum(st["pg"]) * 7.0 / 3.0
    for v in st.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return st


def state(case):
    """The crafted state of a case (shared: read-only): fp32 t, p, w, r, x, xt (None without x_true), the float64 gamma partials pg and
    gprev (gamma_{k-2}; not read when k_first = 1)."""
    return _state(case.key())


# ------------------------------------------------------------------------------------------------------------ reference
class Stage:
    """ref: float64 (bound given) or the float32 the device must equal (bound None)."""

    def __init__(self, ref, bound=None):
        self.ref, self.bound = ref, bound


def iteration(case, st, dev=None):
    """One iteration restated (module docstring).  dev: the device's own 'p1', 'w1' (form 2), 'PD', 'r1', 't1', 'x1' — each later stage
    is then evaluated on them; absent entries are taken from the reference itself (exact cases: the two are equal).  Returns a dict of
    Stage: p1, w1 (form 2), PD, delta, r1, t1, x1, d, PG, NP, plus the scalars gamma, beta, alpha."""
    dev = dev or {}
    nx, ny, n, exact = case.nx, case.ny, case.n, case.exact
    oF, oT = oracles(case.psf, case.exact, nx, ny)
    f64 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64).reshape(nx, ny)   # noqa: E731
    out = {}
    gk = math.fsum(st["pg"])
    beta = np.float32(0.0) if case.first else V.step32(gk, st["gprev"])
    out["gamma"], out["beta"] = gk, beta
    t = st["t"]
    p_old = np.zeros(n, np.float32) if (case.first and case.form == 2) else st["p"]
    p1 = V.fma32(beta, p_old, t)
    out["p1"] = Stage(p1)
    p1d = np.asarray(dev.get("p1", p1), dtype=np.float32).reshape(-1)
    sum_b = lambda sq: None if exact else SUM_TERMS * U53 * tile_sums(sq, nx, ny)        # noqa: E731
    if case.form == 1:
        ow = oF.apply(p1d)
        bw = blur_bound(ow, oF)
        sq = ow["y"] ** 2
        if exact:
            out["PD"] = Stage(tile_sums(sq, nx, ny))
        else:
            e = blur_bound(oF.apply(t), oF) + abs(float(beta)) * blur_bound(oF.apply(p_old), oF)
            bwa = e + U32 * (np.abs(ow["y"]) + e) + U32 * ow["S"]
            out["PD"] = Stage(tile_sums(sq, nx, ny), tile_sums(2.0 * np.abs(ow["y"]) * bwa + bwa * bwa, nx, ny) + sum_b(sq))
        wB, bwB = ow["y"], bw
    else:
        oq = oF.apply(t)
        w_old = np.zeros(n, np.float32) if case.first else st["w"]
        if exact:
            w1 = (oq["y"] + np.float64(beta) * f64(w_old)).astype(np.float32).reshape(-1)
            out["w1"] = Stage(w1)
        else:
            ref = oq["y"] + np.float64(beta) * f64(w_old)
            b = blur_bound(oq, oF)
            out["w1"] = Stage(ref, b + U32 * (np.abs(ref) + b))
            w1 = ref.astype(np.float32).reshape(-1)
        w1d = np.asarray(dev.get("w1", w1), dtype=np.float32).reshape(-1)
        sq = f64(w1d) ** 2
        out["PD"] = Stage(tile_sums(sq, nx, ny), sum_b(sq))
        wB, bwB = f64(w1d), None
    PDd = np.asarray(dev.get("PD", out["PD"].ref), dtype=np.float64)
    delta = math.fsum(PDd)
    out["delta"] = Stage(delta, None if exact else ntiles(nx, ny) * 2.0 ** -52 * abs(delta))
    alpha = V.step32(gk, delta)
    out["alpha"] = alpha
    r_old = st["r"]
    if case.form == 2:
        r1 = V.fma32(-alpha, w1d, r_old)
        out["r1"] = Stage(r1)
    elif exact:
        r1 = (f64(r_old) - np.float64(alpha) * wB).astype(np.float32).reshape(-1)
        out["r1"] = Stage(r1)
    else:
        ref = f64(r_old) - np.float64(alpha) * wB
        ab = float(alpha) * bwB
        out["r1"] = Stage(ref, ab + U32 * (np.abs(ref) + ab))
        r1 = ref.astype(np.float32).reshape(-1)
    r1d = np.asarray(dev.get("r1", r1), dtype=np.float32).reshape(-1)
    ot = oT.apply(r1d)
    if exact:
        t1 = ot["y"].astype(np.float32).reshape(-1)
        out["t1"] = Stage(t1)
    else:
        out["t1"] = Stage(ot["y"], blur_bound(ot, oT))
        t1 = ot["y"].astype(np.float32).reshape(-1)
    t1d = np.asarray(dev.get("t1", t1), dtype=np.float32).reshape(-1)
    d = np.float32(alpha) * p1d
    x1 = V.fma32(alpha, p1d, st["x"])
    out["d"], out["x1"] = Stage(d), Stage(x1)
    x1d = np.asarray(dev.get("x1", x1), dtype=np.float32).reshape(-1)
    sq = f64(t1d) ** 2
    out["PG"] = Stage(tile_sums(sq, nx, ny), sum_b(sq))
    terms = [f64(x1d) ** 2, f64(d) ** 2, (f64(x1d) - f64(st["xt"])) ** 2 if st["xt"] is not None else np.zeros((nx, ny))]
    NP = np.stack([tile_sums(v, nx, ny) for v in terms], axis=1).reshape(-1)
    out["NP"] = Stage(NP, None if exact else np.stack([sum_b(v) for v in terms], axis=1).reshape(-1))
    return out


def worst(got, stage, nx, ny):
    """(largest |got - ref| / bound over the entries with a non-zero bound, where it sits (flat index), entries that are not exactly 0
    where the bound is 0)."""
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(-1) - np.asarray(stage.ref, dtype=np.float64).reshape(-1))
    b = np.asarray(stage.bound, dtype=np.float64).reshape(-1)
    pos = b > 0
    bad_zero = int(np.count_nonzero(err[~pos]))
    if not pos.any():
        return 0.0, 0, bad_zero
    ratio = np.divide(err, b, out=np.zeros_like(err), where=pos)
    at = int(np.argmax(ratio))
    return float(ratio[at]), at, bad_zero


def where(at, ny):
    i, j = divmod(int(at), ny)
    return f"(row {i}, column {j}, tile {tile_of(i, j, ny)})"


# ------------------------------------------------------------------------------------------------------------ exactness
def unit_of(a):
    """The largest power of two (at most 1) that divides every entry of a."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    for k in range(0, 80):
        s = a * 2.0 ** k
        if np.array_equal(s, np.rint(s)):
            return 2.0 ** -k
    raise AssertionError("not dyadic")


def _blur_margin(orc, v, nx, ny):
    """Both passes of y = fl(A v) for v in units of unit_of(v): the row pass's partial sums are bounded by |A_c||v| in units
    u_row u_v, the column pass's by |A||v| = S in units u_col u_row u_v.  Returns the larger count of units."""
    assert orc.rank1
    col, row = B.rank1_factors(orc.p[::-1, ::-1] if orc.tr else orc.p)
    ur, uc, uv = unit_of(row), unit_of(col), unit_of(v)
    assert np.array_equal(col.astype(np.float32), col) and np.array_equal(row.astype(np.float32), row)
    aV = np.abs(np.asarray(v, dtype=np.float64).reshape(nx, ny))
    rows = B._rmul(orc.Ac[1], aV)
    return max(float(rows.max()) / (ur * uv), float((orc.Ar[1] @ rows).max()) / (ur * uc * uv))


def _fma_margin(a, b, c):
    a, b, c = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, b, c))
    u = min(unit_of(a) * unit_of(b), unit_of(c))
    return float((np.abs(a * b) + np.abs(c)).max()) / u


def _sum_margin(terms):
    t = np.asarray(terms, dtype=np.float64).reshape(-1)
    return float(np.abs(t).sum()) / unit_of(t)


def exact_margins(case):
    """name -> (units, limit) of every intermediate of an exact case: float32 stages against 2^24, float64 sums against 2^53."""
    assert case.exact
    st, nx, ny, n = state(case), case.nx, case.ny, case.n
    oF, oT = oracles(case.psf, True, nx, ny)
    ref = iteration(case, st)
    beta, alpha = float(ref["beta"]), float(ref["alpha"])
    F, D = 2.0 ** 24, 2.0 ** 53
    m = {}
    p_old = np.zeros(n, np.float32) if (case.first and case.form == 2) else st["p"]
    m["p1"] = (_fma_margin(beta, p_old, st["t"]), F)
    m["A t"] = (_blur_margin(oF, st["t"], nx, ny), F)
    if case.form == 1:
        At, Ap = oF.apply(st["t"])["y"], oF.apply(p_old)["y"]
        m["A p_old"] = (_blur_margin(oF, p_old, nx, ny), F)
        m["w (K_A)"] = (_fma_margin(beta, Ap, At), F)
        m["A p1"] = (_blur_margin(oF, ref["p1"].ref, nx, ny), F)
        w = oF.apply(ref["p1"].ref)["y"]
        assert np.array_equal(w, np.float64(beta) * Ap + At)
    else:
        w_old = np.zeros(n, np.float32) if case.first else st["w"]
        m["w1"] = (_fma_margin(beta, w_old, oF.apply(st["t"])["y"]), F)
        w = ref["w1"].ref.astype(np.float64)
    m["PD"] = (_sum_margin(w * w), D)
    m["r1"] = (_fma_margin(alpha, w, st["r"]), F)
    m["A^T r1"] = (_blur_margin(oT, ref["r1"].ref, nx, ny), F)
    m["d"] = (_fma_margin(alpha, ref["p1"].ref, np.zeros(n)), F)
    m["x1"] = (_fma_margin(alpha, ref["p1"].ref, st["x"]), F)
    m["PG"] = (_sum_margin(ref["t1"].ref.astype(np.float64) ** 2), D)
    x1 = ref["x1"].ref.astype(np.float64)
    m["NP"] = (max(_sum_margin(x1 * x1), _sum_margin(ref["d"].ref.astype(np.float64) ** 2),
                   _sum_margin((x1 - st["xt"]) ** 2) if st["xt"] is not None else 0.0), D)
    m["pg"] = (_sum_margin(np.concatenate([st["pg"], [ref["gamma"], st["gprev"]]])), D)
    assert alpha == 0.25 and beta == (0.0 if case.first else 0.5) and ref["gamma"] == float(np.sum(st["pg"]))
    return m


def emulated_fraction(psf_name, nx, ny, tr, seed=0):
    """The largest error of blur_entry_cases.sep_fp32 (the two fp32 passes, on the CPU) over the separable bound, on normals."""
    psf = general_psf(psf_name)
    v = normals(nx * ny, 99, seed)
    orc = oracles(psf_name, False, nx, ny)[1 if tr else 0]
    o = orc.apply(v)
    got = B.sep_fp32(v.reshape(nx, ny), psf, "reflect", tr)
    return B.worst_ratio(got, o, "separable", orc.kh, orc.kw, orc.pmax)[0]


# ------------------------------------------------------------------------------------------------------------ the kernels' index logic
MUTANTS = ("swap_rwf_rwt", "anchor_even_kh", "fold_at_n_minus_2", "mirror_fill_self")


def geom(psf, mutant=None):
    """tiled_geom: the centred 9-tap weights (rwf, cwf, rwt, cwt) from the separable factors as the library stores them."""
    kh, kw = psf.shape
    out = []
    for tr in (False, True):
        wr, wc = B.sep_weights(psf, tr)
        T = kh // 2 if mutant == "anchor_even_kh" else kh - 1 - kh // 2
        L = kw - 1 - kw // 2
        rw, cw = np.zeros(9), np.zeros(9)
        rw[np.arange(kw) - L + 4] = wr
        cw[np.arange(kh) - T + 4] = wc
        out += [rw, cw]
    rwf, cwf, rwt, cwt = out
    if mutant == "swap_rwf_rwt":
        rwf, rwt = rwt, rwf
    return rwf, cwf, rwt, cwt


def _blur_lds(a, rw, cw):
    """blur_lds: out[R][C] from in[R + 8][C + 8], row pass then column pass."""
    R, C = a.shape[0] - 8, a.shape[1] - 8
    tmp = sum(rw[o] * a[:, o:o + C] for o in range(9))
    return sum(cw[o] * tmp[o:o + R] for o in range(9))


def tile_model(case, st, beta, alpha, mutant=None):
    """The four kernels' index logic in float64, tile by tile: returns (p1, w of the tile pass (form 1: K_A's A t + beta A p_old; form 2:
    w'), r1, t1, out_of_bounds) as (nx, ny) arrays.  out_of_bounds: a load index left [0, n) (possible only with a mutated fold)."""
    nx, ny = case.nx, case.ny
    psf = psf_of(case)
    rwf, cwf, rwt, cwt = geom(psf, mutant)
    img = lambda v: np.asarray(v, dtype=np.float64).reshape(nx, ny)                      # noqa: E731
    t, r_old = img(st["t"]), img(st["r"])
    p_old = np.zeros((nx, ny)) if (case.first and case.form == 2) else img(st["p"])
    w_old = np.zeros((nx, ny)) if case.first else img(st["w"])
    oob = [False]

    def fold(i, n):
        if mutant == "fold_at_n_minus_2":
            i = np.asarray(i)
            f = np.where(i < 0, -1 - i, np.where(i >= n, 2 * n - 2 - i, i))
            if ((f < 0) | (f >= n)).any():
                oob[0] = True
            return np.clip(f, 0, n - 1)              # (the model stays in bounds; the kernel would not)
        return refl(i, n)

    p1, wA, r1, t1 = (np.full((nx, ny), np.nan) for _ in range(4))
    tx, ty = tiles(nx, ny)
    own = lambda i0, j0: (slice(i0, min(i0 + CT, nx)), slice(j0, min(j0 + CT, ny)))      # noqa: E731
    for a in range(tx):
        for b in range(ty):
            i0, j0 = a * CT, b * CT
            ri, ci = fold(np.arange(i0 - CH, i0 - CH + E1), nx), fold(np.arange(j0 - CH, j0 - CH + E1), ny)
            T1 = t[np.ix_(ri, ci)]
            s = own(i0, j0)
            h, w_ = s[0].stop - i0, s[1].stop - j0
            p1[s] = (T1[CH:CH + CT, CH:CH + CT] + beta * p_old[np.ix_(ri, ci)][CH:CH + CT, CH:CH + CT])[:h, :w_]
            q = _blur_lds(T1, rwf, cwf)
            if case.form == 1:
                wA[s] = (q + beta * _blur_lds(p_old[np.ix_(ri, ci)], rwf, cwf))[:h, :w_]
            else:
                wA[s] = (q[:h, :w_] + beta * w_old[s])
    for a in range(tx):
        for b in range(ty):
            i0, j0 = a * CT, b * CT
            ii, jj = np.arange(i0 - CH, i0 - CH + E1), np.arange(j0 - CH, j0 - CH + E1)
            ins = ((ii >= 0) & (ii < nx))[:, None] & ((jj >= 0) & (jj < ny))[None, :]
            ic, jc = np.clip(ii, 0, nx - 1), np.clip(jj, 0, ny - 1)
            if case.form == 1:
                r2, c2 = fold(np.arange(i0 - 2 * CH, i0 - 2 * CH + E2), nx), fold(np.arange(j0 - 2 * CH, j0 - 2 * CH + E2), ny)
                W = _blur_lds(p1[np.ix_(r2, c2)], rwf, cwf)                 # w = A p' on tile + halo
            else:
                W = np.where(ins, wA[np.ix_(ic, jc)], np.nan)               # form 2 never writes the cells outside the image
            W = np.where(ins, r_old[np.ix_(ic, jc)] - alpha * W, W)
            if mutant != "mirror_fill_self":
                mr, mc = fold(ii, nx) - (i0 - CH), fold(jj, ny) - (j0 - CH)
                okr, okc = (mr >= 0) & (mr < E1), (mc >= 0) & (mc < E1)
                M = np.where(okr[:, None] & okc[None, :], W[np.ix_(np.clip(mr, 0, E1 - 1), np.clip(mc, 0, E1 - 1))], 0.0)
                W = np.where(ins, W, M)
            s = own(i0, j0)
            h, w_ = s[0].stop - i0, s[1].stop - j0
            r1[s] = W[CH:CH + CT, CH:CH + CT][:h, :w_]
            t1[s] = _blur_lds(W, rwt, cwt)[:h, :w_]
    return p1, wA, r1, t1, oob[0]
