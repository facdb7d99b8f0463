"""Operands, references and bounds of the basis-sweep tests (csrc/gemv.hip), built from sizes and seeds alone and with NumPy alone:
tests/test_gemv_cases_host.py checks the cases themselves on the CPU, tests/test_gpu_gemv_entrywise.py runs them through the kernels.

Two kinds of operands.

Exact operands make every order of summation exact, so a device result must EQUAL its reference:
  basis entries          m / 64, m a non-zero integer, |m| <= 64
  vectors                non-zero integers in [-31, 31]  (r, r2, the right-hand sides, xrow, base, w_in, ref)
  weights                one of 0.5, 1, 2, 4: r w and r (w w) are exact in float32
  coefficients           m / 8, m a non-zero integer, |m| <= 32 (y, c, h); a, s dyadic; rho2 0.25 or 4, so that 1 / sqrt is 2 or 0.5
Every term of a dot is a multiple of 2^-8 (of 2^-9 with the coefficients: a combination's), every partial sum in ANY order is such
a multiple far below 2^53 times its unit, a float64; the stored float32 outputs are exact while the value fits 24 bits of its
unit (checked on the values themselves: `fits_float32`).  One element dropped, counted twice or taken from a neighbouring row or
column changes a result by at least 1 / 64.

General operands tell a float64 accumulator from a float32 one, which exact ones cannot.  Dot cases draw magnitudes from [0.5, 2]
with a random sign (`band`), so that the dot bound  n 2^-53 sum |t_i|  stays below the smallest single term |t_i| and one missing
element cannot hide inside it; coefficients are standard normals (float64, as the kernels read them).  References repeat the
kernels' float32 steps (`weighted`: r w and r (w w) in float32; vectors a kernel has stored are taken AS STORED); their own error is
at least 2^8 below the bounds (`dots`, `combination`: exact float64 products, error-free or split sums, np.longdouble results).

Bounds (derived from the arithmetic, not measured):
  dots                   |got - ref| <= n 2^-53 sum_i |t_i|                       (float64 accumulation of exact products)
  rounded once           |got - ref| <= 2^-24 |ref| + (k + 3) 2^-53 S_i + 2^-149   (k fused multiply-adds in float64, the scaling and
                                                                                  1 / sqrt, one rounding to float32; S_i: sum of the
                                                                                  absolute terms of entry i)
  sums of squares        |got - sum| <= n 2^-53 sum                               (of the squares of the outputs as stored)
  damped-LSQR update     the rotations repeated in float64 (`lsqr_coefficients`), 16 2^-53 relative slack on the three coefficients
"""
import functools

import numpy as np

NT = 256                       # threads of a workgroup
JT = 8                         # rows of a tile of the dot kernels
KMAX_LDS = 1024                # coefficients a combination stages in LDS
NT_MIN = 11 << 20              # floats from which basis rows are loaded non-temporally (stream_nontemporal)
U53, U24, DENORM = 2.0 ** -53, 2.0 ** -24, 2.0 ** -149
LSQR_SLACK = 16

WIDE = np.longdouble
assert np.finfo(WIDE).nmant >= 63, "the references need a significand wider than float64's"


def wide(a):
    return np.asarray(a, dtype=WIDE)


def _rng(*key):
    return np.random.default_rng([int(v) for v in key])


def _nonzero_ints(rng, shape, top):
    """Non-zero integers in [-top, top]."""
    m = rng.integers(0, 2 * top, shape, dtype=np.int16) - np.int16(top)
    m[m >= 0] += 1
    return m


def band(rng, shape):
    """float32 magnitudes in [0.5, 2], random sign."""
    u = rng.random(shape, dtype=np.float32) * np.float32(3.0) - np.float32(1.5)
    return u + np.copysign(np.float32(0.5), u)


class Case:
    """The operands of one (k, n): a basis of `rows` >= k rows of n floats and vectors / weights / coefficients by name, each drawn from
    its own seed (so the same name gives the same data whatever else was asked for).  Built lazily, cached; do not modify."""

    VECTORS = ("r", "r2", "r3", "r4", "xrow", "base", "w_in", "ref", "vk", "w_old", "x_in")

    def __init__(self, k, n, exact, rows=None):
        self.k, self.n, self.exact = int(k), int(n), bool(exact)
        self.rows = self.k + 1 if rows is None else int(rows)
        self._cache = {}

    def _get(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    @property
    def V(self):
        def make():
            rng = _rng(1, self.k, self.n, self.exact)
            if self.exact:
                return _nonzero_ints(rng, (self.rows, self.n), 64).astype(np.float32) / np.float32(64.0)
            return band(rng, (self.rows, self.n))
        return self._get("V", make)

    def vec(self, name):
        def make():
            rng = _rng(2, self.k, self.n, self.exact, self.VECTORS.index(name))
            if self.exact:
                return _nonzero_ints(rng, self.n, 31).astype(np.float32)
            return band(rng, self.n)
        return self._get(name, make)

    @property
    def w(self):
        """Weights: 0.5, 1, 2 or 4 (exact), U[0.5, 2) (general)."""
        def make():
            rng = _rng(3, self.k, self.n, self.exact)
            if self.exact:
                return rng.choice(np.array([0.5, 1.0, 2.0, 4.0], dtype=np.float32), self.n)
            return rng.uniform(0.5, 2.0, self.n).astype(np.float32)
        return self._get("w", make)

    def coef(self, name, m=None):
        """m (default k + 1) float64 coefficients: non-zero multiples of 1 / 8 in [-4, 4] (exact), standard normals (general)."""
        m = self.k + 1 if m is None else m

        def make():
            rng = _rng(4, self.k, self.n, self.exact, sum(name.encode()))
            if self.exact:
                return _nonzero_ints(rng, m, 32) / 8.0
            return rng.standard_normal(m)
        return self._get(("coef", name, m), make)

    @property
    def rho2(self):
        return 0.25 if (self.k + self.n) % 2 else 4.0


@functools.lru_cache(maxsize=4)
def case(k, n, exact, rows=None):
    return Case(k, n, exact, rows)


# ----------------------------------------------------------------------------------------------------------- references, bounds
class Ref:
    """A reference (np.longdouble), its bound per entry (float64), the sum S of the absolute terms of every entry and, for dots, the
    smallest absolute term."""

    def __init__(self, ref, bound, tmin=None, S=None, lo=None):
        self.ref, self.bound, self.tmin, self.S, self.lo = ref, bound, tmin, S, lo

    def value(self):
        """The reference as np.longdouble (a long combination keeps it as a pair of float64 arrays, ref + lo)."""
        return wide(self.ref) if self.lo is None else wide(self.ref) + wide(self.lo)

    def error(self, got):
        """|got - reference| per entry.  For a pair: got - ref is exact where the two are within a factor of two of each other, and
        taking lo off errs by 2^-53 of the difference."""
        got = np.asarray(got).reshape(-1)
        if self.lo is None:
            return np.abs(wide(got) - self.ref)
        return np.abs((got.astype(np.float64) - self.ref) - self.lo)


def weighted(r, w, wpow):
    """The float32 vector the dot kernels multiply the rows with: r, r w or r (w w), each product rounded to float32 as k_gemv_t does."""
    r = np.asarray(r, dtype=np.float32)
    if wpow == 0:
        return r
    w = np.asarray(w, dtype=np.float32)
    return r * w if wpow == 1 else r * (w * w)


def dots(V, t, exact=False):
    """ref[j] = sum_i V[j][i] t[i] with the bound n 2^-53 sum_i |V[j][i] t[i]| and the smallest |V[j][i] t[i]| over all j, i.
    The products p_i are exact in float64 (24 + 24 bits).  Exact operands: so is their sum in any order.  General operands:
    p_i = hi_i + lo_i with hi_i the multiple of a unit u nearest to p_i, u such that |hi_i| <= 2^25 u: the sum of the hi_i is exact in
    float64 in any order (n <= 2^24), that of the lo_i (|lo_i| <= u / 2) errs by at most n 2^-53 n u / 2, which must be — and is
    checked to be — 2^8 below the bound (np.longdouble otherwise: n 2^-64 of the absolute terms)."""
    V = np.asarray(V, dtype=np.float32)
    k, n = V.shape
    assert np.shape(t) == (n,)
    assert n <= 1 << 24
    t64 = np.asarray(t, dtype=np.float64)
    ref = np.zeros(k, dtype=WIDE)
    S = np.zeros(k)
    tmin = np.inf
    for j in range(k):
        p = V[j].astype(np.float64) * t64
        a = np.abs(p)
        S[j] = a.sum()
        if n:
            tmin = min(tmin, float(a.min()))
        top = float(a.max()) if n else 0.0
        if exact or top == 0.0:
            ref[j] = p.sum()
            continue
        u = 2.0 ** (np.ceil(np.log2(top)) - 25)
        if n * (u / 2) * 2.0 ** 8 <= S[j]:
            hi = np.rint(p / u) * u
            ref[j] = WIDE(hi.sum()) + WIDE((p - hi).sum())
        else:
            ref[j] = wide(p).sum()
    return Ref(ref, n * U53 * S, tmin, S)


def _two_sum(a, b):
    """a + b = s + e exactly (Knuth)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(y):
    """y = hi + lo with at most 26 significant bits each (Veltkamp): their products with a float32 are exact in float64."""
    c = 134217729.0 * y
    hi = c - (c - y)
    return hi, y - hi


CHUNK = 1 << 16


def combination(V, coef, a=0.0, base=None, s=1.0, post=1.0):
    """ref = post (a base + sum_j (s coef[j]) V[j]) over the len(coef) rows of V (an array or a list of rows), entry by entry, with the
    bound of an output rounded once from float64.  s coef[j] is formed in float64 as the kernels stage it; post: the scaling
    1 / sqrt(rho2) of the new basis vector, a power of two.  Every term is split into two exact float64 products and the sum is
    carried as a pair (sum, compensation) by error-free additions: the reference errs by about k 2^-105 of the absolute terms."""
    coef = np.asarray(coef, dtype=np.float64)
    k = coef.size
    assert len(V) == k and all(V[j].dtype == np.float32 for j in range(k))
    n = len(V[0])
    ys = [_split(np.float64(s) * c) for c in coef]
    ah, al = _split(np.float64(a))
    assert post != 0 and np.frexp(post)[0] in (0.5, -0.5), "post: a power of two"
    ref, low, S = np.zeros(n), np.zeros(n), np.zeros(n)
    for i0 in range(0, n, CHUNK):
        sl = slice(i0, min(n, i0 + CHUNK))
        acc, comp, Sc = np.zeros(sl.stop - i0), np.zeros(sl.stop - i0), np.zeros(sl.stop - i0)
        terms = [] if base is None else [(ah, al, np.asarray(base[sl], dtype=np.float64))]
        terms += [(ys[j][0], ys[j][1], V[j][sl].astype(np.float64)) for j in range(k)]
        for hi, lo, row in terms:
            for part in (hi, lo):
                acc, e = _two_sum(acc, part * row)
                comp += e
            Sc += abs(hi + lo) * np.abs(row)
        ref[sl], low[sl] = _two_sum(acc, comp)
        S[sl] = Sc
    ref *= post
    low *= post
    S *= abs(post)
    return Ref(ref, U24 * np.abs(ref) + (k + 3) * U53 * S + DENORM, S=S, lo=low)


def sum_of_squares(stored, minus=None):
    """sum_i (stored[i] - minus[i])^2 of float32 vectors as stored, with the bound n 2^-53 of the sum."""
    d = wide(stored) - (0 if minus is None else wide(minus))
    s = (d * d).sum() if d.size else WIDE(0)
    return Ref(np.array([s], dtype=WIDE), np.array([d.size * U53 * float(s)]))


def chk_sum(V, c, w):
    """||w - V c||^2 as trk_gemv_orth_iterate's `chk` forms it: the float64 entries o_i (each within (k + 3) 2^-53 S_i) squared and summed."""
    o = combination(V, c, a=1.0, base=w, s=-1.0)
    v = o.value()
    s = (v * v).sum()
    slack = o.bound - U24 * np.abs(o.ref)                                 # the float64 part of the entries' bound
    return Ref(np.array([s], dtype=WIDE), np.array([v.size * U53 * float(s) + 2.0 * float((np.abs(o.ref) * slack).sum())]))


def lsqr_coefficients(alpha_sq, beta_sq, beta0_sq, damp, state_in, first):
    """k_lsqr_damped_update's rotations in float64: (1 / alpha, theta / rho_prev, phi / rho) and the state {cs, sn, rho, phibar} it leaves."""
    alpha, beta = np.sqrt(np.float64(alpha_sq)), np.sqrt(np.float64(beta_sq))
    tw = 0.0
    if first:
        rhobar, phibar = alpha, np.sqrt(np.float64(beta0_sq))
    else:
        rhobar = -state_in[0] * alpha
        tw = state_in[1] * alpha / state_in[2]
        phibar = state_in[3]
    rhobar1 = np.sqrt(rhobar * rhobar + damp * damp)
    phibar = phibar * (rhobar / rhobar1)
    rho = np.sqrt(rhobar1 * rhobar1 + beta * beta)
    cs, sn = rhobar1 / rho, beta / rho
    return (1.0 / alpha, tw, cs * phibar / rho), np.array([cs, sn, rho, sn * phibar])


def lsqr_w(vk, w_old, coefs, first):
    """w = vk / alpha - (theta / rho_prev) w_old, rounded once; the coefficients within LSQR_SLACK 2^-53."""
    ia, tw, _ = coefs
    ref = WIDE(ia) * wide(vk)
    S = abs(ia) * np.abs(np.asarray(vk, dtype=np.float64))
    if not first:
        ref = ref - WIDE(tw) * wide(w_old)
        S = S + abs(tw) * np.abs(np.asarray(w_old, dtype=np.float64))
    return Ref(ref, U24 * np.abs(ref).astype(np.float64) + (LSQR_SLACK + 3) * U53 * S + DENORM)


def lsqr_x(x_in, w_stored, coefs):
    """x = x_in + (phi / rho) w with w as stored."""
    px = coefs[2]
    ref = WIDE(px) * wide(w_stored)
    S = abs(px) * np.abs(np.asarray(w_stored, dtype=np.float64))
    if x_in is not None:
        ref = ref + wide(x_in)
        S = S + np.abs(np.asarray(x_in, dtype=np.float64))
    return Ref(ref, U24 * np.abs(ref).astype(np.float64) + (LSQR_SLACK + 3) * U53 * S + DENORM)


# ----------------------------------------------------------------------------------------------------------- exactness
def _keep(a):
    a = np.asarray(a)
    return a if a.dtype == np.float64 else wide(a)


def is_multiple(a, unit):
    """Whether every value is a multiple of `unit`, a power of two (the division is exact)."""
    q = _keep(a) / unit
    return bool(np.all(q == np.rint(q)))


def fits_float32(ref, unit):
    """Whether every value is a multiple of `unit` (a power of two) below 2^24 units: its rounding to float32 is exact."""
    r = _keep(ref)
    return is_multiple(r, unit) and bool(np.all(np.abs(r) < 2.0 ** 24 * unit)) and bool(np.all(r.astype(np.float32) == r))


# ----------------------------------------------------------------------------------------------------------- the cases
#: (k, n) of every case the device tests run, by group.  The leading dimension and the alignment are the device test's business.
LAYOUT_K = 13
LAYOUT_N = (1028, 1029, 1030, 1031)
WGRAM_K = 63                                  # k + 2 > 64: trk_wgram leaves c1, c2 to k_gemv_t<1>, <2>
TILE_KMAX, TILE_N = 41, 1030
GRID_CASES = ((9, 2048), (9, 2052), (9, 1 << 20), (9, (1 << 20) + 4), (25, 1_200_003))
LADDER_K = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 21)
LADDER_N = 1030
KMAX_N = 260
SPLIT_K = (12, 13, 14, 15, 17)
SPLIT_N = 1028                                # n / 4 = 257 = 4 x 64 + 1: a last workgroup of one column
NT_K, NT_N = 3, NT_MIN + 4


def split_edge(cus):
    """The longest vector k_gemv_n_split serves on `cus` compute units: n / 4 = 64 x 4 x cus."""
    return 4 * 64 * 4 * cus
