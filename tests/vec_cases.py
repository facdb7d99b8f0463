"""Operands, references, bounds and launch plans of the vector-update tests (csrc/vecops.hip, csrc/cgls_update.hip and the scalar
plumbing they feed: scalar_from_wave, finalize_block_256, coef_eval, finalize_sums, trk_finalize_batched), built from sizes and seeds
alone and with NumPy alone: tests/test_vec_cases_host.py checks the cases themselves on the CPU, tests/test_gpu_vec_entrywise.py runs
them through the kernels.

Exact operands make every product, every update and every sum exact, so a device result must EQUAL its reference:
  vectors                    m / 8, m an integer, |m| <= 8; the first and the last element non-zero; drawn per index from a seeded
                             generator, so a value taken from a neighbour or from another vector differs
  steps, coefficients        one of 0.25, 0.5, 0.75, 1, 1.5 (at most 2 significant bits, multiples of 2^-2), the quotient of two
                             device scalars or of two sets of block partials whose totals have exactly that ratio
  block partials             u (i + 1) / 16 for partial i (`partials`): distinct per index, multiples of 2^-4, total u n (n + 1) / 32;
                             with n <= 1024 and u <= 7 a total is below 2^18 in units of 2^-4: 22 bits, exact in any order
The bit count: a product step p is a multiple of 2^-5 of magnitude <= 1.5; an iterate after up to 8 chained steps is a multiple of
2^-5 of magnitude <= 1 + 8 x 1.5 = 13 < 2^4: 9 significant bits of float32's 24, rounded nowhere, fused or not.  r - step w,
t + b p and a x + b y are multiples of 2^-5 below 4.  A square (of an iterate, of step p, of x' - x_true, |.| <= 14) is a multiple of
2^-10 below 2^8, so a float64 sum of up to n = 2^25 of them is a multiple of 2^-10 below 2^33: 43 bits of float64's 53, exact in ANY
order.  x . y and (a x) . z are multiples of 2^-6 / 2^-8 below 2 / 4; w (x - y) a multiple of 2^-6 below 2.  `test_vec_cases_host`
sums such terms in float32 in several orders by brute force.  One element dropped, doubled or taken from a neighbour changes a result.

General operands: standard normals with magnitudes clipped into [2^-6, 2^6] (`wgram_cases.clipped_normals`), scalars whose ratio is
not dyadic (3 / 7, 5 / 3).

Launch plans: `stream_plan(n, cus, offsets)` restates stream_grid, stream_nontemporal and the VEC decision (every operand's byte
offset a multiple of 16) of the launchers; the size lists (`sizes`) are built from `cus`, and every named size asserts the branch it is
named for (`expect`).

References, float64 from the float32 operands:
  x update       x' = fl32(x + step p), step = fl32(gamma / delta), ONE rounding (`fma32`): the float64 value x + step p (the product is
                 exact in float64, the sum rounded once, 2^-53 relative = 2^-29 ulp of float32) rounded to float32, except where it lies
                 within 2^-20 ulp of a float32 tie: there `fractions.Fraction` decides (exactly, ties to even).  The two-rounding form
                 fl32(x + fl32(step p)) is float32 arithmetic as NumPy does it.  d = fl32(step p) in both.
  r, p, axpby    fmaf(-step, w, r); fmaf(b, p, t) (`p_update`, one rounding; the two-rounding fl32(t + fl32(b p)) is `p_update_two`, which
                 no CGLS kernel computes); fmaf(a, x, fl32(b y)) for trk_axpby, whose product b y IS rounded on its own.
  sums           float64 sums of the float64-exact terms of those float32 values (`sums`), bound (n + 4096) 2^-53 S with S the sum of
                 the absolute terms (the form of gemv_cases.dots: n additions and the finalize tree, one rounding per term for a
                 square of a difference); the reference's own error is measured against np.longdouble on the host.
  mm_weights     float64 (fl32(fmaf(v, v, eps2)))^e with v = fl32(x - y), eps2 = fl32(eps^2), e = fl32(p / 2 - 1)
  group_weights  the float64 sum of squares taken sequentially, as the kernel's loop does (not np.sum's pairwise order), then pow.
"""
import fractions

import numpy as np

from wgram_cases import clipped_normals, eighths

NT = 256
U24, U53 = 2.0 ** -24, 2.0 ** -53
WIDE = np.longdouble
MAX_PARTIAL_BLOCKS = 1024           # kMaxPartialBlocks
NT_STORES, NT_LOADS = 11 << 20, 20 << 20   # kNontemporalMinFloats, kNontemporalLoadsMinFloats
STEPS = (0.25, 0.5, 0.75, 1.0, 1.5)
UNITS = {0.25: (1, 4), 0.5: (1, 2), 0.75: (3, 4), 1.0: (2, 2), 1.5: (3, 2), 3 / 7: (3, 7), 5 / 3: (5, 3)}   # ratio: (num, den) units
N_PARTIALS = (1, 2, 63, 64, 65, 448, 449, 511, 512, 513, 960, 961, 1023, 1024)
FINALIZE_BLOCKS = (1, 255, 256, 257, 767, 768, 769, 1023, 1024)
POISON = 2.0 ** 40                  # in the slots before the first and after the last partial handed to a consumer
TIE_MARGIN = 2.0 ** -20             # of a float32 ulp


def _rng(*key):
    return np.random.default_rng([sum(ord(ch) << (8 * i) for i, ch in enumerate(v[:7])) if isinstance(v, str) else int(v) for v in key])


# ----------------------------------------------------------------------------------------------------------- operands
def vec(n, exact, *key):
    """A float32 vector of n elements: eighths (exact) or clipped normals; first and last element non-zero."""
    rng = _rng(21, n, exact, *key)
    a = eighths(rng, n) if exact else clipped_normals(rng, n)
    if n:
        for e in (0, -1):
            if a[e] == 0:
                a[e] = np.float32(1.0 if e == 0 else -0.5)
    return a


def partials(n, unit):
    """n block partials unit (i + 1) / 16 (float64) and their exact total unit n (n + 1) / 32."""
    p = unit * np.arange(1, n + 1, dtype=np.float64) / 16.0
    total = unit * n * (n + 1) / 32.0
    assert total * 16 == int(total * 16) and total < 2.0 ** 40
    return p, total


def poisoned(p):
    """The partials between two slots of 2^40 (a read before the first or beyond the last ruins the scalar)."""
    return np.concatenate([[POISON], np.asarray(p, dtype=np.float64), [POISON]])


def ratio_sources(ratio, n_num, n_den):
    """(num partials, num total, den partials, den total) with num total / den total == `ratio` when n_num == n_den (for any counts
    the float64 quotient of the two exact totals is what the device forms, bit for bit)."""
    un, ud = UNITS[ratio]
    pn, tn = partials(n_num, un)
    pd, td = partials(n_den, ud)
    if n_num == n_den:
        assert np.float32(tn / td) == np.float32(ratio)
    return pn, tn, pd, td


def step32(num, den):
    """(float)(num / den) with the quotient formed in float64, as every kernel forms its step."""
    return np.float32(np.float64(num) / np.float64(den))


# ----------------------------------------------------------------------------------------------------------- one-rounding arithmetic
def _round_fraction(q, r, lo, hi):
    """The float32 among r and its neighbours lo < r < hi nearest to the Fraction q, ties to even."""
    best = None
    for c in (lo, r, hi):
        d = abs(fractions.Fraction(float(c)) - q)
        even = (int(np.float32(c).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, c, even)
    return np.float32(best[1])


def fma32(a, b, c, count=None):
    """fl32(a b + c) per element with ONE rounding (fmaf) from float32 a, b, c (a may be a scalar).  count: a list that receives the
    number of elements decided by Fraction (those within TIE_MARGIN ulp of a float32 tie)."""
    a = np.asarray(a, dtype=np.float32)
    b, c = np.asarray(b, dtype=np.float32), np.asarray(c, dtype=np.float32)
    v = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    r = v.astype(np.float32)
    lo, hi = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
    r64 = r.astype(np.float64)
    mid_lo, mid_hi = 0.5 * (r64 + lo.astype(np.float64)), 0.5 * (r64 + hi.astype(np.float64))
    ulp = np.minimum(hi.astype(np.float64) - r64, r64 - lo.astype(np.float64))
    near = np.flatnonzero(np.minimum(np.abs(v - mid_lo), np.abs(v - mid_hi)) <= TIE_MARGIN * ulp)
    if count is not None:
        count.append(int(near.size))
    if near.size:
        r = r.copy()
        ab = np.broadcast_to(a, r.shape)
        for i in near:
            q = fractions.Fraction(float(ab[i])) * fractions.Fraction(float(b[i])) + fractions.Fraction(float(c[i]))
            r[i] = _round_fraction(q, r[i], lo[i], hi[i])
    return r


def x_update(x, p, step, count=None):
    """(x' fused = fl32(x + step p), x' in two roundings = fl32(x + fl32(step p)), d = fl32(step p))."""
    step = np.float32(step)
    d = step * np.asarray(p, dtype=np.float32)
    return fma32(step, p, x, count), np.asarray(x, dtype=np.float32) + d, d


def r_update(r, w, step, count=None):
    return fma32(-np.float32(step), w, r, count)


def p_update(t, p, b, count=None):
    """p' = fl32(t + b p), ONE rounding: fmaf(b, p, t), what the CGLS kernels compute (include/trk.h)."""
    return fma32(np.float32(b), p, t, count)


def p_update_two(t, p, b):
    """fl32(t + fl32(b p)): the two-rounding form (trk_axpby(1, t, b, p); no CGLS kernel computes it)."""
    return np.asarray(t, dtype=np.float32) + np.float32(b) * np.asarray(p, dtype=np.float32)


def axpby(a, x, b=None, y=None, count=None):
    """fmaf(a, x, fl32(b y)), or fl32(a x) without y."""
    if y is None:
        return np.float32(a) * np.asarray(x, dtype=np.float32)
    return fma32(np.float32(a), x, np.float32(b) * np.asarray(y, dtype=np.float32), count)


def coef(c, num=None, den=None, flags=0):
    """coef_eval in float64: c (sqrt?)(num) / (sqrt?)(den)."""
    v = np.float64(c)
    if num is not None:
        v = v * (np.sqrt(np.float64(num)) if flags & 1 else np.float64(num))
    if den is not None:
        v = v / (np.sqrt(np.float64(den)) if flags & 2 else np.float64(den))
    return v


# every combination of num / den / TRK_SQRT_*: (c, num, den, flags) with exact squares under the roots; all evaluate to 2-bit dyadics
COEFS = ((0.75, None, None, 0), (0.25, 3.0, None, 0), (0.5, 9.0, None, 1), (3.0, None, 4.0, 0), (3.0, None, 16.0, 2),
         (0.5, 3.0, 4.0, 0), (0.5, 9.0, 4.0, 1), (0.5, 3.0, 16.0, 2), (0.5, 9.0, 16.0, 3), (1.0, 3.0, 2.0, 0))


# ----------------------------------------------------------------------------------------------------------- sums
class Ref:
    """A float64 reference, its bound (None: exact operands, the result must be equal) and the sum of the absolute terms."""

    def __init__(self, ref, bound, S):
        self.ref, self.bound, self.S = ref, bound, S

    def error(self, got):
        return np.abs(np.asarray(got, dtype=np.float64) - self.ref)


def sums(terms, exact, dtype=np.float64):
    """The sum of float64 terms with the bound (n + 4096) 2^-53 S."""
    t = np.asarray(terms, dtype=dtype)
    S = float(np.abs(t).sum())
    return Ref(t.sum(), None if exact else (t.size + 4096) * U53 * S, S)


def dot_terms(mode, x, y=None, dtype=np.float64):
    """The terms of k_reduce2: 0: x y, 1: x x, 2: (x - y)^2 (products of two float32 are exact in float64; the difference is exact,
    its square rounded once)."""
    x = np.asarray(x, dtype=np.float32).astype(dtype)
    if mode == 1:
        return x * x
    y = np.asarray(y, dtype=np.float32).astype(dtype)
    return x * y if mode == 0 else (x - y) * (x - y)


def x_norm_terms(xn, d, xt=None, dtype=np.float64):
    """The terms of the three norms of an x update from the float32 x', d and x_true."""
    out = [dot_terms(1, xn, dtype=dtype), dot_terms(1, d, dtype=dtype)]
    out.append(np.zeros(0, dtype=dtype) if xt is None else dot_terms(2, xn, xt, dtype=dtype))
    return out


# ----------------------------------------------------------------------------------------------------------- weights
def mm_weights(x, y, eps, p):
    """(reference float64, special) of trk_mm_weights: special 1: exactly 1; 2: the reciprocal square root; 0: powf."""
    v = np.asarray(x, dtype=np.float32) if y is None else np.asarray(x, dtype=np.float32) - np.asarray(y, dtype=np.float32)
    eps2, e = np.float32(eps * eps), np.float32(p / 2.0 - 1.0)
    t = fma32(v, v, np.full(v.shape, eps2, dtype=np.float32)).astype(np.float64)
    special = 1 if p == 2.0 else 2 if p == 1.0 else 0
    if special == 1:
        return np.ones(v.shape), special
    return (1.0 / np.sqrt(t) if special == 2 else t ** np.float64(e)), special


def group_weights(d, groups, glen, add, expo, copies):
    g = np.asarray(d, dtype=np.float32)[:groups * glen].reshape(groups, glen).astype(np.float64)
    s = np.zeros(groups)
    for t in range(glen):
        s = s + g[:, t] * g[:, t]
    return np.tile(np.power(s + add, expo), copies)


def ulps32(got, ref):
    """|got - ref| in units of the float32 ulp at ref (float64 reference)."""
    ref = np.asarray(ref, dtype=np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref) / ulp


def far_from_tie(ref, rel=2.0 ** -40):
    """Where the float64 `ref` is farther than `rel` (relative) from the midpoint of two neighbouring float32."""
    ref = np.asarray(ref, dtype=np.float64)
    r = ref.astype(np.float32)
    lo, hi = np.nextafter(r, np.float32(-np.inf)).astype(np.float64), np.nextafter(r, np.float32(np.inf)).astype(np.float64)
    r64 = r.astype(np.float64)
    dist = np.minimum(np.abs(ref - 0.5 * (r64 + lo)), np.abs(ref - 0.5 * (r64 + hi)))
    return dist > rel * np.abs(ref)


# ----------------------------------------------------------------------------------------------------------- launch plans
def ceil_div(a, b):
    return -(-a // b)


def stream_cap(cus):
    return min(4 * cus, MAX_PARTIAL_BLOCKS)


def stream_grid(n, cus):
    return max(1, min(ceil_div(n, NT * 4), stream_cap(cus)))


def stream_nontemporal(n):
    return (51 | 192) if n >= NT_LOADS else (3 | 192) if n >= NT_STORES else 0


def stream_plan(n, cus, offsets=(), m=None):
    """What a streaming launch over n floats does (m: a second length, the residual of k_cgls_update; the grid follows the longer):
    grid, nt mask, vec (every operand's BYTE offset a multiple of 16), body (float4 per thread and pass), passes of the grid-stride
    loop over the body, tail elements."""
    big = n if m is None else max(n, m)
    grid = stream_grid(big, cus)
    vec = all(o % 16 == 0 for o in offsets)
    body = n // 4 if vec else n
    return dict(grid=grid, nt=stream_nontemporal(n), vec=vec, passes=ceil_div(body, grid * NT) if body else 0,
                tail=n % 4 if vec else 0, threads=grid * NT)


def expect(plan, **want):
    for k, v in want.items():
        assert plan[k] == v, (k, plan[k], v, plan)
    return plan


def sizes(cus):
    """The named sizes, {name: n}, each the smallest that reaches its branch on a part of `cus` compute units (aligned operands)."""
    one = stream_cap(cus) * NT * 4                      # floats one pass of the full grid covers
    S = {"empty": 0, "one": 1, "three": 3, "four": 4, "five": 5, "block-1": 1023, "block": 1024, "block+1": 1025,
         "pass-4": one - 4, "pass": one, "pass+1": one + 1, "two-passes+tail": 2 * one + 1024 + 3}
    for name, n in S.items():
        p = stream_plan(n, cus, (0,))
        expect(p, nt=0, vec=True)
        if name in ("empty", "one", "three"):
            expect(p, passes=0, grid=1, tail=n)
        elif name in ("four", "five", "block-1", "block", "block+1"):
            expect(p, passes=1, grid=1 if n <= 1024 else 2, tail=n % 4)
        elif name in ("pass-4", "pass"):
            expect(p, passes=1, grid=stream_cap(cus), tail=0)
        elif name == "pass+1":
            expect(p, passes=1, grid=stream_cap(cus), tail=1)      # (the tail alone goes beyond one float4 per thread)
        else:
            expect(p, passes=3, grid=stream_cap(cus), tail=3)      # a second full pass and a ragged third
    return S


def nt_sizes():
    """{name: n} of the non-temporal variants: stores hinted from 11 x 2^20 floats, loads from 20 x 2^20."""
    S = {"nt-4": NT_STORES - 4, "nt-stores+3": NT_STORES + 3, "nt-loads+3": NT_LOADS + 3}
    assert stream_nontemporal(S["nt-4"]) == 0 and stream_nontemporal(S["nt-stores+3"]) == 195
    assert stream_nontemporal(S["nt-loads+3"]) == 243 and stream_nontemporal(NT_LOADS - 1) == 195
    return S


def n_for_blocks(nblocks, cus):
    """The smallest n whose reduction leaves `nblocks` block partials (None: the part's grid is capped below)."""
    if nblocks > stream_cap(cus):
        return None
    n = (nblocks - 1) * NT * 4 + 1
    assert stream_grid(n, cus) == nblocks
    return n


def xs_nt(n, count, p_out_is_last):
    """The hint mask of trk_cgls_xs_update."""
    return stream_nontemporal(n) | ((256 | 32 | (0 if p_out_is_last else 512 | 1024)) if count > 1 else 0)


def xs_slots(count, s_slots, first):
    """The slots (0 = p, j = ring row j - 1) of the `count` directions, oldest first."""
    return [(first + c) % s_slots for c in range(count)]


def xs_first(count, s_slots, where):
    """`first` such that slot 0 (p) is the first, a middle or the last of the count directions (None: impossible for this count)."""
    pos = {"first": 0, "middle": count // 2, "last": count - 1}[where]
    if where == "middle" and not 0 < pos < count - 1:
        return None
    first = (-pos) % s_slots
    assert xs_slots(count, s_slots, first)[pos] == 0
    return first


def xs_scalars(count, k_last, exact):
    """S (5 (k_last + 1) + 2 doubles of -1 except the entries read) and the count float32 steps of iterations k_last - count + 1 ..
    k_last: step_j = gamma_{j-1} / delta_j with gamma_0 = S[0], gamma_j = S[5 j + 1], delta_j = S[5 j]."""
    S = np.full(5 * (k_last + 1) + 2, -1.0)
    gam = lambda j: 3.0 * 2.0 ** (j % 3) if exact else 3.0 + j          # noqa: E731
    steps = []
    for c in range(count):
        j = k_last - count + 1 + c
        g = gam(j - 1)
        S[0 if j == 1 else 5 * (j - 1) + 1] = g
        st = STEPS[(j + c) % len(STEPS)] if exact else (3.0 + c) / 7.0
        S[5 * j] = g / st if exact else g * 7.0 / (3.0 + c) * (1.0 + 2.0 ** -30)
        steps.append(step32(g, S[5 * j]))
        if exact:
            assert steps[-1] == np.float32(st)
    return S, steps
