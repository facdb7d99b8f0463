"""Operands, references, bounds and launch plans of the weighted-Gram tests (csrc/wgram.hip), built from sizes and seeds alone and with
NumPy alone: tests/test_wgram_cases_host.py checks the cases themselves on the CPU, tests/test_gpu_wgram_entrywise.py runs them
through the kernels.

Exact operands make every order of summation, every split and every arithmetic mode exact, so a device result must EQUAL its float64
reference:
  basis rows, b, z, images   m / 8, m an integer, |m| <= 8 (zero included)
  weights                    one of 0, 0.5, 1, 2
Stored rows (trk_wgram): a weighted operand w W is (m / 8) {0, 0.5, 1, 2}, a multiple of 2^-4 of magnitude <= 2: at most 6
significant bits, rounded nowhere; w w and W (w w) (the tile-pair kernel, k_gemv_t<2>) are multiples of 2^-2 and 2^-5.  A product of
two weighted operands is a multiple of 2^-8 of magnitude <= 4 (11 bits); a 32-element fp32 partial sum of them is a multiple of 2^-8
below 2^7: 15 bits of float32's 24.  TV Gram: a difference of two pixels is m / 8 with |m| <= 16, weighted a multiple of 2^-4 of
magnitude <= 4: at most 7 significant bits, so it IS its first bf16 piece (8 bits) and the further pieces are zero; a product is a
multiple of 2^-8 of magnitude <= 16 and the 64 differences of an image row of a strip sum to a multiple of 2^-8 below 2^10: 18 bits
(the issue's count, with all of it in one accumulator: 20).  The float64 totals are multiples of 2^-8 below 2^-8 2^53 for every size
used (N^2, m <= 2^24: below 2^29, 37 bits).  `exactness_by_brute_force` (host test) sums random groups in float32 in several orders
and round-trips the bf16 pieces.  One element dropped, doubled or taken from a neighbour changes an entry by a multiple of 2^-8.

General operands: standard normals with magnitudes clipped into [2^-6, 2^6] (nothing near the denormal range), weights in
[0.25, 1.25) as the existing tests use.

Launch plans: `wgram_plan` and `wgram_tv_plan` restate the decisions of trk_wgram and wgram_tv_run (kernel, template arguments, grid,
groups / chunks / units per wave or workgroup) as functions of the shape, the alignment and the number of compute units; the case lists
are built from them with `cus` as a parameter, and every named case asserts that it reaches the branch it is named for (`expect`).

References: float64 from the float32 operands.  trk_wgram: G = (W w^2) W^T, c1 = W (w b), c2 = W (w^2 b) with exact float64 products
(24 + 24 bits) summed in float64 in chunks (`gram_ref`); the TV Gram: d = fl32(fl32(x - x') w) as the kernels form it, then float64
(`tv_ref_host` for N <= 256; on the device with torch slicing beyond, tests/test_gpu_wgram_entrywise.py).

Bounds of the general operands on trk_wgram, u = 2^-24, per entry, S = sum_i |w_i^2 W_a,i W_b,i| (the sum of the absolute terms):
  k_wgram_t16, k_wgram_mfma   Both stage x = fl32(w W): one rounding per operand, (1 + u)^2 - 1 <= 2 u + u^2 of every term.  A group of 32
                              elements (k_wgram_t16: 8 v_mfma_f32_16x16x4 of 4 elements into one fp32 tile from zero; k_wgram_mfma:
                              16 v_mfma_f32_32x32x2 of 2 elements) is 32 products added into an fp32 accumulator: one rounding for the
                              first product, one per further addition, each at most u of a partial sum that is itself at most
                              (1 + 32 u) times the group's absolute terms: (1 + 31) u.  The tile is flushed into float64 after every
                              group (exact conversion), and the float64 additions of a wave, of the four waves and of the block
                              partials (finalize_sums) are at most m / 32 + 4 + 2048 roundings of 2^-53.  Together (2 + 1 + 31) u S
                              = 34 u S to first order; the second-order terms are below 34 * 34 u^2 S < 0.001 u S; 36 u S leaves two
                              units for them and for an MFMA that adds its 2 or 4 products in an order of its own.  Row k (the
                              plain b) and unweighted calls round less.  c1 = (w W) . b and c2 = (w W) . (w b) are entries of the
                              same augmented Gram: the same bound with their own S.
  k_wgram (k + 2 > 64)        ww = fl32(w w), va = fl32(W ww): two roundings of one operand, 2 u + u^2; the products va W are exact in
                              float64 and summed in float64 (at most m + 1024 additions): 3 u S covers it, 4 u S with the slack.
                              c1, c2 come from k_gemv_t<1>, <2>: tests/gemv_cases.py's dot bound n 2^-53 S against the reference that
                              repeats fl32(w b), fl32(b fl32(w w)) (`gemv_cases.weighted`, `gemv_cases.dots`).
The float64 term (m + 4096) 2^-53 S is added to both.  The reference's own error must stay below 1e-6 of the bound: checked against
np.longdouble on the host.

TV Gram, general operands: the contract of include/trk.h, per entry relative to sqrt(G_aa G_bb): 1e-6 for auto, bf16x3, fp32; 1.2e-5
for bf16x2.
"""
import functools

import numpy as np

import gemv_cases as GC

NT = 256
U24, U53 = 2.0 ** -24, 2.0 ** -53
WIDE = np.longdouble
MFMA_C, PAIR_C = 36.0, 4.0          # the constants of the two bounds above
MAX_PARTIAL_BLOCKS = 1024           # kMaxPartialBlocks
TV_MODES = ("auto", "bf16x2", "bf16x3", "fp32")
TV_LIMIT = {"auto": 1e-6, "bf16x2": 1.2e-5, "bf16x3": 1e-6, "fp32": 1e-6}
TV_BF = {"auto": 4, "bf16x2": 2, "bf16x3": 3, "fp32": 0}


def _rng(*key):
    return np.random.default_rng([int(v) for v in key])


def ceil_div(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------------------------------------- operands
EXACT_W = np.array([0.0, 0.5, 1.0, 2.0], dtype=np.float32)


def eighths(rng, shape):
    """float32 multiples of 1 / 8 in [-1, 1]."""
    return (rng.integers(-8, 9, shape, dtype=np.int8).astype(np.float32)) * np.float32(0.125)


def clipped_normals(rng, shape):
    """float32 standard normals with magnitudes clipped into [2^-6, 2^6]."""
    g = rng.standard_normal(shape, dtype=np.float32)
    return np.copysign(np.clip(np.abs(g), np.float32(2.0 ** -6), np.float32(2.0 ** 6)), g)


class Rows:
    """The operands of one trk_wgram case: `rows` rows of m floats (V), the weights w and the vector b.  The first and the last
    element of every row, of b and of w are non-zero (an element dropped at either end always shows)."""

    def __init__(self, rows, m, exact, seed=0):
        self.rows, self.n, self.m, self.exact = int(rows), int(m), int(m), bool(exact)
        rng = _rng(11, rows, m, exact, seed)
        draw = eighths if exact else clipped_normals
        self.V = draw(rng, (self.rows, self.m))
        self.b = draw(rng, self.m)
        self.w = rng.choice(EXACT_W, self.m) if exact else (rng.random(self.m, dtype=np.float32) + np.float32(0.25))
        if self.m:
            for a in (self.V, self.b):
                for e in (0, -1):
                    a[..., e] = np.where(a[..., e] == 0, np.float32(1.0), a[..., e])
            if exact:
                self.w[0], self.w[-1] = 0.5, 2.0

    def vec(self, name):
        return {"b": self.b, "w": self.w}[name]


@functools.lru_cache(maxsize=2)
def rows_case(rows, m, exact, seed=0):
    return Rows(rows, m, exact, seed)


def tv_operands(k, N, exact, seed=0, as_int8=False):
    """(V [k, N^2], w [2 N (N - 1)], z [N^2]) of a TV case.  Exact: the whole last column of w_h and the last row of w_v are 2 and
    the image's last column and row are +-1 (the largest values), so an index that runs beyond a row of the layout shows.
    as_int8 (exact only): V and z as eighths in int8 (to be scaled by 1 / 8 where they are used)."""
    rng = _rng(12, k, N, exact, seed)
    n, ph = N * N, N * (N - 1)
    if exact:
        V = rng.integers(-8, 9, (k, N, N), dtype=np.int8)
        edge = (rng.integers(0, 2, (k, N), dtype=np.int8) * 16 - 8).astype(np.int8)
        V[:, :, N - 1] = edge
        V[:, N - 1, :] = edge[:, ::-1]
        V = V.reshape(k, n)
        z = rng.integers(-8, 9, n, dtype=np.int8)
        w = rng.choice(EXACT_W, 2 * ph)
        w[:ph].reshape(N, N - 1)[:, N - 2] = 2.0
        w[ph:].reshape(N - 1, N)[N - 2, :] = 2.0
        if not as_int8:
            V, z = V.astype(np.float32) * np.float32(0.125), z.astype(np.float32) * np.float32(0.125)
        return V, w, z
    assert not as_int8
    return clipped_normals(rng, (k, n)), rng.random(2 * ph, dtype=np.float32) + np.float32(0.25), clipped_normals(rng, n)


# ----------------------------------------------------------------------------------------------------------- references, bounds
class Ref:
    """A reference (float64), its bound per entry (None: exact operands only) and the sum of the absolute terms."""

    def __init__(self, ref, bound=None, S=None):
        self.ref, self.bound, self.S = ref, bound, S

    def error(self, got):
        return np.abs(np.asarray(got, dtype=np.float64).reshape(self.ref.shape) - self.ref)


CHUNK = 1 << 15


def gram_ref(V, k, w, b, m, pair_path=False, exact=False, dtype=np.float64):
    """References of one trk_wgram call: {'G': Ref [k k, row-major], 'c1': Ref [k], 'c2': Ref [k]} (the last two with b).  A term w^2 W_a W_b
    has 96 bits: the reference takes  sum (w^2 W_a) W_b  with w^2 (48 bits, exact), w^2 W_a and the product each rounded to float64
    (2^-52 of a term, 2^-28 of the bounds' constants) and chunked float64 sums; exact operands: nothing is rounded.  The host test
    measures the whole against np.longdouble (dtype).  pair_path: c1, c2 as k_gemv_t<1>, <2> form them (gemv_cases)."""
    V = np.asarray(V[:k], dtype=np.float32)[:, :m]
    w64 = np.ones(m, dtype=dtype) if w is None else np.asarray(w[:m]).astype(dtype)
    A = V.astype(dtype) * (w64 * w64)
    B = V.astype(dtype)
    G = _gram_wide(A, B, dtype)
    S = G if exact else _gram_wide(np.abs(A), np.abs(B), dtype)        # (exact operands have no bound)
    const = PAIR_C if pair_path else MFMA_C
    f64 = (m + 4096) * U53

    def bound(Sx):
        return None if exact else (const * U24 + f64) * np.asarray(Sx, dtype=np.float64)
    out = {"G": Ref(G.reshape(-1), None if exact else bound(S).reshape(-1), S.reshape(-1))}
    if b is not None:
        b = np.asarray(b[:m], dtype=np.float32)
        if pair_path:
            wf = np.ones(m, dtype=np.float32) if w is None else np.asarray(w[:m], dtype=np.float32)
            for name, wpow in (("c1", 1), ("c2", 2)):
                R = GC.dots(V, GC.weighted(b, wf, wpow if w is not None else 0), exact)
                out[name] = R                                              # (np.longdouble reference, gemv_cases' own Ref)
        else:
            b64 = b.astype(dtype)
            for name, t in (("c1", b64 * w64), ("c2", b64 * w64 * w64)):
                c = _gram_wide(B, t[None, :], dtype)[:, 0]
                Sc = c if exact else _gram_wide(np.abs(B), np.abs(t)[None, :], dtype)[:, 0]
                out[name] = Ref(c, bound(Sc), Sc)
    return out


def gram_rows_wide(V, k, w, b, m, rows):
    """Rows `rows` of the augmented Gram [w W | b | w b] [w W | b | w b]^T in np.longdouble (the products of the float64-exact
    weighted rows, pairwise sums): what G, c1 and c2 are entries of."""
    V = np.asarray(V[:k], dtype=np.float32)[:, :m].astype(WIDE)
    w_ = np.ones(m, dtype=WIDE) if w is None else np.asarray(w[:m]).astype(WIDE)
    R = V * w_
    if b is not None:
        b_ = np.asarray(b[:m]).astype(WIDE)
        R = np.concatenate([R, b_[None, :], (b_ * w_)[None, :]], axis=0)
    return np.stack([(R[a][None, :] * R).sum(axis=1) for a in rows])


def _gram_wide(A, B, dtype):
    out = np.zeros((A.shape[0], B.shape[0]), dtype=dtype)
    for i0 in range(0, A.shape[1], CHUNK):
        a, b = A[:, i0:i0 + CHUNK], B[:, i0:i0 + CHUNK]
        out += a @ b.T if dtype is np.float64 else np.einsum("ai,bi->ab", a, b)
    return out


def tv_diffs(V, N, w):
    """The weighted differences as the kernels form them, d = fl32(fl32(x - x') w): [k, 2 N (N - 1)] float32, laid out as L does
    (N rows of N - 1 horizontal differences, then N - 1 rows of N vertical ones)."""
    V = np.asarray(V, dtype=np.float32)
    k = V.shape[0]
    X = V.reshape(k, N, N)
    w = np.asarray(w, dtype=np.float32)
    wh, wv = w[:N * (N - 1)].reshape(N, N - 1), w[N * (N - 1):].reshape(N - 1, N)
    dh = (X[:, :, :-1] - X[:, :, 1:]) * wh
    dv = (X[:, :-1, :] - X[:, 1:, :]) * wv
    return np.concatenate([dh.reshape(k, -1), dv.reshape(k, -1)], axis=1)


def tv_ref_host(V, N, w, z=None, dtype=np.float64):
    """(G, h) of trk_wgram_tv(_z) in float64 on the host (N <= 256)."""
    D = tv_diffs(V, N, w)
    G = _gram_wide(D.astype(dtype), D.astype(dtype), dtype)
    h = None if z is None else _gram_wide(np.asarray(V).astype(dtype), np.asarray(z).astype(dtype)[None, :], dtype)[:, 0]
    return G, h


def tv_ref_oracle(V, N, w):
    """The same Gram through the oracle's sparse L (float64 differences, weighted in float64): pins the layout of the differences."""
    from oracle.cpu_ref import first_derivative_2d
    L = first_derivative_2d(N, N)
    LV = (L @ np.asarray(V, dtype=np.float64).T).T * np.asarray(w, dtype=np.float64)
    return LV @ LV.T


def tv_relative(got, ref):
    """max over the entries of |got - ref| / sqrt(ref_aa ref_bb)."""
    dg = np.sqrt(np.abs(np.diag(ref)))
    return float(np.max(np.abs(got - ref) / np.maximum(np.outer(dg, dg), 1e-300)))


# ----------------------------------------------------------------------------------------------------------- exactness
def bf16_pieces(d):
    """(hi, mid, lo) of float32 values as bf16_split8x3 makes them (round to nearest even on the upper 16 bits)."""
    def bf(x):
        b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
        r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
        return r.astype(np.uint32).view(np.float32)
    d = np.asarray(d, dtype=np.float32)
    hi = bf(d)
    r1 = d - hi
    mid = bf(r1)
    return hi, mid, bf(r1 - mid)


def exactness_by_brute_force(groups=4000, seed=0):
    """Random groups of products of exact operands summed in float32 in several orders, against float64; the bf16 pieces of the
    weighted differences.  Returns the number of sums compared."""
    rng = _rng(13, seed)
    n = 0
    for size, top in ((32, 1), (64, 2)):                         # stored rows: 32 products of (w W)(w W); TV: 64 of (w d)(w d), |d| <= 2
        a = (eighths(rng, (groups, size)) * top) * rng.choice(EXACT_W, (groups, size))
        b = (eighths(rng, (groups, size)) * top) * rng.choice(EXACT_W, (groups, size))
        assert a.dtype == np.float32
        hi, mid, lo = bf16_pieces(a)
        assert np.array_equal(hi, a) and not mid.any() and not lo.any()
        p32 = a * b
        p64 = a.astype(np.float64) * b.astype(np.float64)
        assert np.array_equal(p32.astype(np.float64), p64)
        want = p64.sum(axis=1)
        for order in (np.arange(size), np.arange(size)[::-1], rng.permutation(size), np.argsort(-np.abs(p32[0]))):
            acc = np.zeros(groups, dtype=np.float32)
            for j in order:
                acc = acc + p32[:, j]                            # one float32 rounding per addition
            assert acc.dtype == np.float32 and np.array_equal(acc.astype(np.float64), want)
            n += groups
        pair = p32.reshape(groups, size // 4, 4).sum(axis=2, dtype=np.float32).sum(axis=1, dtype=np.float32)   # four at a time, as an MFMA may
        assert np.array_equal(pair.astype(np.float64), want)
        n += groups
    return n


# ----------------------------------------------------------------------------------------------------------- launch plans
def _mis(aligned):
    """`aligned`: True (every operand on a 16-byte boundary) or the names of the operands that are not: 'W', 'w', 'b1'."""
    if aligned is True:
        return frozenset()
    if aligned is False:
        return frozenset(("W",))
    return frozenset((aligned,) if isinstance(aligned, str) else aligned)


def stream_grid(n, cus):
    want = ceil_div(n, NT * 4)
    return max(1, min(want, min(cus * 4, MAX_PARTIAL_BLOCKS)))


def wgram_plan(k, m, ld, has_w, has_b, aligned, cus):
    """What trk_wgram launches.  Keys: kernel, targs, grid, and
      k_wgram_t16   gs (waves of the launch), ngroup, groups (most / fewest full groups of a wave), branch (of the wave with the most:
                    'none', 'lone' = consume(0) alone, 'pair' = the g + gs < ngroup branch, 'trip+else', 'trip+pair', with the number of
                    trips of the two-group loop in `trips`), tail (elements of the scalar tail)
      k_wgram_mfma  nchunk, chunks (most / fewest per workgroup), vec_ok, ragged (the last chunk is not full)
      k_wgram       npairs, vec, tail (elements after the 16-byte body), c_kernel (what forms c1, c2)"""
    assert 1 <= k <= 512 and m >= 0 and ld >= m
    mis = _mis(aligned)
    KA = k + (2 if has_b else 0)
    al16 = ld % 4 == 0 and "W" not in mis and not (has_w and "w" in mis) and not (has_b and "b1" in mis)
    if KA <= 64:
        direct = al16 and KA <= 48
        T = ceil_div(KA, 16)
        per_cu = (8, 4, 2)[T - 1] if direct else 3
        nchunk = ceil_div(m, 128)
        bx = min(max(nchunk, 1), cus * per_cu, 2 * MAX_PARTIAL_BLOCKS)
        if direct:
            gs, ngroup = 4 * bx, m // 32
            most = ceil_div(ngroup, gs)
            fewest = max(0, ceil_div(ngroup - (gs - 1), gs))
            trips = (most - 1) // 2 if most else 0
            branch = "none" if most == 0 else ("trip+" if trips else "") + ("pair" if (most - 1) % 2 else ("else" if trips else "lone"))
            return dict(kernel="k_wgram_t16", targs=(T, has_w, has_b), grid=bx, KA=KA, gs=gs, ngroup=ngroup, groups=(most, fewest),
                        trips=trips, branch=branch, tail=m % 32)
        return dict(kernel="k_wgram_mfma", targs=(1 if KA <= 32 else 2, has_w, has_b), grid=bx, KA=KA, nchunk=nchunk,
                    chunks=(ceil_div(nchunk, bx), nchunk // bx), vec_ok=al16, ragged=m % 128 != 0)
    nt = ceil_div(k, 4)
    npairs = nt * (nt + 1) // 2
    bx = min(stream_grid(m, cus), max(1, ceil_div(cus * 8, npairs)))
    vec = ld % 4 == 0 and "W" not in mis and not (has_w and "w" in mis)
    return dict(kernel="k_wgram", targs=(has_w, vec), grid=(bx, npairs), KA=KA, npairs=npairs, vec=vec, tail=m % 4 if vec else m,
                c_kernel=None if not has_b else ("k_gemv_t<1>,<2>" if has_w else "k_gemv_t<0>"))


def wgram_tv_plan(k, N, with_z, mode, cus):
    """What wgram_tv_run launches.  Keys: kernel, targs, grid, lock, xcd_map, use_lds, two_pass, nbands, band_rows, units, per (units
    per wave (k_wgram_tv) or per workgroup (k_wgram_tv_lds): most / fewest), and for the LDS kernel `pieces`: per wave, the number
    of staged loads per image row its vmcnt waits count (nv_mine + the extra)."""
    assert 1 <= k <= 48 and N >= 32 and N % 32 == 0 and mode in TV_MODES
    T = ceil_div(k, 16)
    strips = N // 32
    z = bool(with_z)
    ls_pays = k >= 12 if T == 1 else ((k >= 22 if z else True) if T == 2 else False)
    lock = strips % 4 == 0 and ls_pays
    if lock:
        per_cu = (3 if T == 1 else 2) if z else 3
    elif z:
        per_cu = 3 if T == 1 else 2
    else:
        per_cu = (4 if k <= 11 else 2 if k <= 14 else 1) if T == 1 else ((3 if k <= 25 else 1) if T == 2 else 2)
    bx = cus * per_cu
    band_rows = min(64, N)
    nbands = ceil_div(N, band_rows)
    units = strips * nbands
    if bx * 4 > units:
        bx = ceil_div(units, 4)
    use_lds = T <= 2 and N % 256 == 0 and N >= 2048
    two_pass = z and T == 3
    BF = TV_BF[mode]
    if use_lds:
        band_rows, nbands = 64, N // 64
        tiles = N // 256
        units = tiles * nbands
        bx = min(cus * (2 if T == 1 else 1), units)
        pieces = tuple(sum(1 for j in range(2 * T) if wv + 8 * j < k) + (1 if (wv <= 4 or (wv == 5 and z) or wv == 6) else 0) for wv in range(8))
        return dict(kernel="k_wgram_tv_lds", targs=(T, z, BF), grid=bx, lock=False, xcd_map=tiles % 8 == 0 and bx % 8 == 0, use_lds=True,
                    two_pass=False, nbands=nbands, band_rows=band_rows, units=units, per=(ceil_div(units, bx), units // bx), pieces=pieces)
    groups = strips // 4
    xcd_map = strips % 4 == 0 and groups % 8 == 0 and bx % 8 == 0
    return dict(kernel="k_wgram_tv", targs=(T, z and not two_pass, 3, BF), grid=bx, lock=bool(lock), xcd_map=xcd_map, use_lds=False,
                two_pass=two_pass, nbands=nbands, band_rows=band_rows, units=units, per=(ceil_div(units, 4 * bx), units // (4 * bx)),
                last_band=N - (nbands - 1) * band_rows)


# ----------------------------------------------------------------------------------------------------------- the cases
def pad4(m):
    return ceil_div(max(m, 1), 4) * 4


def odd_ld(m):
    return m + 1 if (m + 1) % 4 else m + 3


class RowCase:
    """One shape of trk_wgram: k rows of m floats at leading dimension ld, with or without b, `mis` the one misaligned operand (or
    None), and what its plan must show (`expect`: a subset of the plan's items, checked for BOTH weighted and unweighted calls unless
    a value is a dict {has_w: value})."""

    def __init__(self, name, k, m, ld, has_b, mis=None, **expect):
        self.name, self.k, self.m, self.ld, self.has_b, self.mis, self.expect = name, k, m, ld, has_b, mis, expect

    @property
    def KA(self):
        return self.k + (2 if self.has_b else 0)

    def plan(self, has_w, cus):
        return wgram_plan(self.k, self.m, self.ld, has_w, self.has_b, True if self.mis is None else self.mis, cus)

    def check(self, has_w, cus):
        """Asserts that the case reaches, on `cus` compute units, the branch it is named for; returns the plan."""
        p = self.plan(has_w, cus)
        for key, want in self.expect.items():
            want = want[has_w] if isinstance(want, dict) else want
            assert p.get(key) == want, (self.name, has_w, key, p.get(key), want)
        return p

    def __repr__(self):
        return self.name


def k_of(KA, has_b):
    return KA - 2 if has_b else KA


LAYOUT_KA = (3, 16, 17, 32, 33, 48)
LAYOUT_M = 2080                                # 65 groups of 32, 16.25 chunks of 128
LADDER = tuple((k, True) for k in (46, 47, 62, 63)) + tuple((k, False) for k in (16, 17, 32, 33, 48, 49, 64, 65))
EDGE_M = (0, 1, 31, 33, 127, 129)
T16_PER_CU = {1: 8, 2: 4, 3: 2}


def layout_cases(KA):
    """Row layouts of one augmented row count: ld == m; ld padded with m % 4 = 1, 2, 3 (m % 32 below and above 16); ld % 4 != 0; each of
    W, w, b1 one float off a 16-byte boundary."""
    T = ceil_div(KA, 16)
    direct = dict(kernel="k_wgram_t16")
    fallback = dict(kernel="k_wgram_mfma")
    out = []
    for has_b in (True, False):
        k, tag = k_of(KA, has_b), f"KA{KA}{'b' if has_b else ''}"
        out.append(RowCase(f"{tag}-ld_eq_m", k, LAYOUT_M, LAYOUT_M, has_b, tail=0, **direct))
        for m in (LAYOUT_M + 5, LAYOUT_M + 18, LAYOUT_M + 27):
            out.append(RowCase(f"{tag}-pad{m % 4}-tail{m % 32}", k, m, pad4(m), has_b, tail=m % 32, **direct))
        m = LAYOUT_M + 5
        out.append(RowCase(f"{tag}-odd_ld", k, m, odd_ld(m), has_b, vec_ok=False, **fallback))
        m = LAYOUT_M + 4
        out.append(RowCase(f"{tag}-W_off", k, m, m, has_b, "W", vec_ok=False, **fallback))
        out.append(RowCase(f"{tag}-w_off", k, m, m, has_b, "w", kernel={True: "k_wgram_mfma", False: "k_wgram_t16"}))
        if has_b:
            out.append(RowCase(f"{tag}-b1_off", k, m, m, has_b, "b1", vec_ok=False, **fallback))
    for c in out:
        c.expect.setdefault("targs", {hw: ((T if c.plan(hw, 256)["kernel"] == "k_wgram_t16" else (1 if KA <= 32 else 2)), hw, c.has_b)
                                      for hw in (True, False)})
    return out


def ladder_cases():
    """The boundaries 48 | 49 and 64 | 65 of KA (and 16 | 17, 32 | 33 without b), aligned and with an odd leading dimension."""
    out = []
    for k, has_b in LADDER:
        KA = k + (2 if has_b else 0)
        tag = f"k{k}{'b' if has_b else ''}"
        m = LAYOUT_M + 4
        kern = "k_wgram_t16" if KA <= 48 else "k_wgram_mfma" if KA <= 64 else "k_wgram"
        extra = dict(vec_ok=True) if kern == "k_wgram_mfma" else dict(vec=True) if kern == "k_wgram" else {}
        out.append(RowCase(f"{tag}-aligned", k, m, m, has_b, kernel=kern, **extra))
        m = LAYOUT_M + 5
        kern = "k_wgram_mfma" if KA <= 64 else "k_wgram"
        extra = dict(vec_ok=False) if kern == "k_wgram_mfma" else dict(vec=False)
        out.append(RowCase(f"{tag}-odd_ld", k, m, odd_ld(m), has_b, kernel=kern, **extra))
    return out


def group_cases(T, cus):
    """Groups per wave of k_wgram_t16<T>: m = 32 (j gs + r) + tail with gs = 4 cus per_cu waves."""
    gs = 4 * min(cus * T16_PER_CU[T], 2 * MAX_PARTIAL_BLOCKS)          # (the launcher's cap on the grid)
    out = []
    for has_b in (True, False):
        k = k_of(16 * T, has_b)
        tag = f"T{T}{'b' if has_b else ''}"
        for j, branch in ((1, "lone"), (2, "pair"), (3, "trip+else"), (4, "trip+pair")):
            m = 32 * j * gs
            out.append(RowCase(f"{tag}-j{j}-{branch}", k, m, m, has_b, kernel="k_wgram_t16", branch=branch, groups=(j, j), tail=0, gs=gs))
        m = 32 * (2 * gs + gs // 2)
        out.append(RowCase(f"{tag}-j2-half", k, m, m, has_b, kernel="k_wgram_t16", groups=(3, 2), branch="trip+else", tail=0, gs=gs))
        m = 32 * 2 * gs + 17
        out.append(RowCase(f"{tag}-j2-tail17", k, m, pad4(m), has_b, kernel="k_wgram_t16", groups=(2, 2), branch="pair", tail=17, gs=gs))
    return out


def chunk_cases(ntile, cus):
    """Chunks per workgroup of k_wgram_mfma<ntile>: m = 128 (j 3 cus) + r.  <1>: odd ld; <2>: aligned (full chunks, then a ragged one) and
    odd ld."""
    KA = 32 * ntile
    out = []
    for has_b in (True, False):
        k = k_of(KA, has_b)
        for how in (("odd",) if ntile == 1 else ("aligned", "odd")):
            for j, r in ((1, 0), (1, 1), (2, 0), (2, 127)):
                m = 128 * j * 3 * cus + r
                ld = odd_ld(m) if how == "odd" else pad4(m)
                most = j + (1 if r else 0)
                out.append(RowCase(f"mfma{ntile}{'b' if has_b else ''}-{how}-j{j}-r{r}", k, m, ld, has_b, kernel="k_wgram_mfma",
                                   chunks=(most, j), vec_ok=how == "aligned", ragged=r != 0, grid=3 * cus))
    return out


def edge_cases():
    """Short rows on every kernel, each with a padded (16-byte) and an odd leading dimension; k = 1; k = 512."""
    out = []
    for k, has_b in ((1, False), (1, True), (3, True), (46, True), (62, True), (70, True)):
        KA = k + (2 if has_b else 0)
        for m in EDGE_M:
            tag = f"k{k}{'b' if has_b else ''}-m{m}"
            a = "k_wgram_t16" if KA <= 48 else "k_wgram_mfma" if KA <= 64 else "k_wgram"
            o = "k_wgram_mfma" if KA <= 64 else "k_wgram"
            out.append(RowCase(f"{tag}-pad", k, m, pad4(m), has_b, kernel=a))
            out.append(RowCase(f"{tag}-odd", k, m, odd_ld(m), has_b, kernel=o))
    for has_b in (True, False):
        out.append(RowCase(f"k512{'b' if has_b else ''}-m260", 512, 260, 260, has_b, kernel="k_wgram", npairs=8256, vec=True))
        out.append(RowCase(f"k512{'b' if has_b else ''}-m261-odd", 512, 261, 263, has_b, kernel="k_wgram", npairs=8256, vec=False))
    return out


def all_row_cases(cus):
    out = []
    for KA in LAYOUT_KA:
        out += layout_cases(KA)
    out += ladder_cases()
    for T in (1, 2, 3):
        out += group_cases(T, cus)
    for ntile in (1, 2):
        out += chunk_cases(ntile, cus)
    return out + edge_cases()


# TV Gram: (N, k, with_z or None for both, what the plan must show)
TV_SMALL = ((32, 1), (32, 5), (64, 16), (64, 17), (96, 7), (96, 32), (160, 33), (128, 48), (128, 16), (256, 13), (256, 25))   # host reference
TV_SMALL_DEVICE = ((512, 20), (384, 30), (1024, 3))                                                                          # device reference


class TvCase:
    def __init__(self, N, k, with_z, **expect):
        self.N, self.k, self.with_z, self.expect = N, k, with_z, expect
        self.name = f"N{N}-k{k}{'-z' if with_z else ''}"

    def check(self, mode, cus):
        p = wgram_tv_plan(self.k, self.N, self.with_z, mode, cus)
        for key, want in self.expect.items():
            assert p.get(key) == want, (self.name, mode, key, p.get(key), want)
        assert p["targs"][-1] == TV_BF[mode]
        return p

    def __repr__(self):
        return self.name


def tv_register_cases():
    """The register-fed kernel: the existing small list and the branches of the launcher it leaves out."""
    out = []
    for N, k in TV_SMALL + TV_SMALL_DEVICE:
        for z in (False, True):
            out.append(TvCase(N, k, z, kernel="k_wgram_tv"))
    named = [
        (1024, 12, None, dict(lock=True, xcd_map=True)), (1024, 20, None, dict(lock={False: True, True: False}, xcd_map=True)),
        (1024, 32, None, dict(lock=True, xcd_map=True)),
        (1024, 11, None, dict(lock=False, xcd_map=True)), (1024, 33, None, dict(lock=False, xcd_map=True)),
        (1024, 21, True, dict(lock=False, xcd_map=True)), (1024, 22, True, dict(lock=True, xcd_map=True)),
        (96, 33, True, dict(two_pass=True)), (128, 48, True, dict(two_pass=True)),
        (32, 16, None, dict(units=1, nbands=1)),
        (96, 20, None, dict(last_band=32, lock=False)),
        (2048, 33, None, dict(use_lds=False, two_pass={False: False, True: True})),
        (2048, 48, None, dict(use_lds=False, two_pass={False: False, True: True})),
    ]
    for N, k, z, exp in named:
        for zz in ((False, True) if z is None else (z,)):
            e = {key: (v[zz] if isinstance(v, dict) else v) for key, v in exp.items()}
            if not any(c.N == N and c.k == k and c.with_z == zz for c in out):
                out.append(TvCase(N, k, zz, kernel="k_wgram_tv", **e))
            else:
                next(c for c in out if c.N == N and c.k == k and c.with_z == zz).expect.update(e)
    return out


def tv_lds_cases():
    """k_wgram_tv_lds: every k from 1 to 32 at N = 2048 (every pattern of staged loads per wave), and k = 20 at N = 2304 (9 tiles: no
    XCD map)."""
    out = [TvCase(2048, k, z, kernel="k_wgram_tv_lds", use_lds=True, xcd_map=True) for k in range(1, 33) for z in (False, True)]
    out += [TvCase(2304, 20, z, kernel="k_wgram_tv_lds", use_lds=True, xcd_map=False) for z in (False, True)]
    return out


TV_GENERAL = ((96, 7), (96, 32), (160, 33), (1024, 20))          # one of each T, and lockstep with the XCD map


def coverage(cus):
    """{(kernel, template arguments)} reached by the named cases on `cus` compute units (every case checked on the way)."""
    seen = set()
    for c in all_row_cases(cus):
        for has_w in (False, True):
            p = c.check(has_w, cus)
            seen.add((p["kernel"], p["targs"]))
    for c in tv_register_cases() + tv_lds_cases():
        for mode in TV_MODES:
            p = c.check(mode, cus)
            seen.add((p["kernel"], p["targs"]))
    return seen


def coverage_table():
    """Every (kernel, template arguments) the two launchers can instantiate."""
    bools = (False, True)
    want = {("k_wgram", (hw, vec)) for hw in bools for vec in bools}
    want |= {("k_wgram_mfma", (nt, hw, hb)) for nt in (1, 2) for hw in bools for hb in bools}
    want |= {("k_wgram_t16", (T, hw, hb)) for T in (1, 2, 3) for hw in bools for hb in bools}
    want |= {("k_wgram_tv", (T, z, 3, bf)) for T in (1, 2, 3) for z in bools for bf in (0, 2, 3, 4) if not (T == 3 and z)}
    want |= {("k_wgram_tv_lds", (T, z, bf)) for T in (1, 2) for z in bools for bf in (0, 2, 3, 4)}
    return want
