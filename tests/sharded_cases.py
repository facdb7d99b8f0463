"""Operands, references, bounds and launch plans of the sharded CGLS kernels' tests (csrc/cgls_sharded.hip: k_dot_pair,
k_sharded_scalars, k_sharded_finalize, k_cgls_sharded_update), built from sizes and seeds alone and with NumPy alone:
tests/test_sharded_cases_host.py checks the cases themselves on the CPU, tests/test_gpu_sharded_entrywise.py runs them through the
kernels.  Operands, one-rounding arithmetic, sums and the streaming launch plan are those of tests/vec_cases.py and are not restated:
`grid_for` of cgls_sharded.hip is `stream_grid` (ceil(n / 1024) blocks of 256 threads, capped at min(4 CUs, 1024)) under another name.

The scalars kernel has two forms (`scalars_plan`): ONE workgroup of 1024 threads iff m <= 2^14 and n_g <= 2^16, else k_dot_pair on
stream_grid(m) blocks and k_sharded_finalize (four workgroups, one per entry of G4).

References, float64 from the float32 operands:
  qq, qw, ww     float64 sums of the float64-exact products q q, q w, w w (`dot_pair`); without w the last two are 0
  G0             the float64 sum of the gamma partials
  beta_d         g / gprev (one float64 division), 0 when first;  beta = fl32(beta_d)
  delta          qq + 2 beta_d qw + beta_d^2 ww (qq when first), evaluated with fractions.Fraction from the float64 inputs and beta_d;
                 alpha = fl32(g / delta)
  p', w'         fmaf(beta, p, t), fmaf(beta, w, q); t, q when first
  d, x', r'      fl32(alpha p'); fmaf(alpha, p', x), ONE rounding (vec_cases.x_update); fmaf(-alpha, w', r)
  norm terms     x'^2, d^2, (x' - x_true)^2 with the difference taken in float64 (vec_cases.x_norm_terms)

Exact operands: vectors are eighths with |v| <= 1.  First step G4 = {0.75, 3, NaN, NaN}: alpha = 1 / 4 (the NaN slots must not be
used).  Later steps G4 = {1, 2, 1, 4} with gprev = 2: beta = 1 / 2, delta = 2 + 2 (1 / 2) 1 + (1 / 4) 4 = 4, alpha = 1 / 4.  Then p'
and w' are multiples of 2^-4 of magnitude <= 1.5, d, x' and r' multiples of 2^-6 below 2: at most 8 significant bits of float32's 24,
rounded nowhere, fused or not.  Squares (of x', d, x' - x_true with |.| < 3) are multiples of 2^-12 below 9, products of eighths
multiples of 2^-6 of magnitude <= 1: a float64 sum of up to 2^21 of either stays below 2^25 in units of 2^-12, 37 bits of float64's
53, exact in ANY order.  The device must EQUAL the reference.  `CHAIN` holds three successive G4 of that kind (gamma halves each step).

Gamma partials: vec_cases.partials(n_g, unit), partial i = unit (i + 1) / 16, total unit n (n + 1) / 32; at n_g = 65537 and unit <= 7
the total is below 2^35 in units of 2^-4 — exact in any order —, between poison slots of 2^40 (`vec_cases.poisoned`).

General operands: clipped normals; G4 and gprev with non-dyadic ratios (`GENERAL_FIRST`, `GENERAL_LATER`).
Bounds, all arithmetic and no measurement:
  sums     (n + 4096) 2^-53 S, S the sum of the absolute terms (vec_cases.sums)
  delta    the kernel's float64 expression may or may not be contracted: 4 x 2^-53 (|qq| + 2 |beta_d qw| + beta_d^2 ww) about the
           Fraction value covers every such evaluation (three products, one square and two sums, each rounded at most once).
           `scalars` asserts that fl32(g / delta) is the same float32 over that whole interval, so alpha is unambiguous and every
           vector entry is compared bit for bit.
  entries  0 ulp: every entry is one correctly rounded operation (two for d); vec_cases.fma32 decides entries within TIE_MARGIN of
           a float32 tie with Fraction, so no entry is left out.
"""
import fractions
import types

import numpy as np

import vec_cases as V
from vec_cases import (U53, Ref, dot_terms, expect, fma32, p_update, partials, poisoned, r_update, stream_grid,  # noqa: F401
                       stream_plan, sums, vec, x_norm_terms, x_update)

NT1 = 1024                          # threads of the one-workgroup form
ONE_BLOCK_MAX_M = 1 << 14           # kOneBlockMax
ONE_BLOCK_MAX_NG = 1 << 16

EXACT_FIRST = dict(G4=(0.75, 3.0, float("nan"), float("nan")), gprev=None, beta=0.0, delta=3.0, alpha=0.25)
EXACT_LATER = dict(G4=(1.0, 2.0, 1.0, 4.0), gprev=2.0, beta=0.5, delta=4.0, alpha=0.25)
# three chained steps: gamma_{k-1} = 0.75, 0.375, 0.1875 (gprev of step k is the gamma of step k - 1), alpha = 1 / 4, beta = 1 / 2
CHAIN = ((0.75, 3.0, float("nan"), float("nan")), (0.375, 0.5, 0.5, 2.0), (0.1875, 0.25, 0.25, 1.0))
GENERAL_FIRST = ((3.0, 7.0, float("nan"), float("nan")), (5.0, 3.0, float("nan"), float("nan")))
GENERAL_LATER = (((3.0, 7.0, 1.3, 5.0), 5.0), ((5.0, 11.0, -2.7, 3.0), 7.0), ((1.7, 0.9, 0.35, 0.6), 2.3))
N_GAMMA = (0, 1, 2, 1023, 1024, 1025, 4096, 65536, 65537)
M_SIZES = {"empty": 0, "one": 1, "three": 3, "four": 4, "body+tail": 1027, "last-one-block": 1 << 14, "first-multi": (1 << 14) + 1,
           "first-multi-vec": (1 << 14) + 4, "multi-66-blocks": 66561, "capped": 1300003}
NG_ONE_ROW_M = 3                    # with n_g = 65537: the multi-block form with ONE row of partials
NM_SHAPES = ((1, 1), (3, 5), (1027, 515), (515, 1027), (4096, 0), (0, 4096), (66561, 66561), (1300003, 1027), (1027, 1300003))


# ----------------------------------------------------------------------------------------------------------- launch plans
def scalars_plan(m, n_g, cus, offsets=(0,)):
    """What trk_cgls_sharded_scalars launches: form 'one_block' (k_sharded_scalars, grid 1, 1024 threads) or 'multi' (k_dot_pair on
    stream_grid(m) blocks, then k_sharded_finalize over that many rows); vec: every given operand's BYTE offset a multiple of 16."""
    one = m <= ONE_BLOCK_MAX_M and n_g <= ONE_BLOCK_MAX_NG
    is_vec = all(o % 16 == 0 for o in offsets)
    body = m // 4 if is_vec else m
    threads = NT1 if one else stream_grid(m, cus) * V.NT
    return dict(form="one_block" if one else "multi", grid=1 if one else stream_grid(m, cus), vec=is_vec,
                passes=V.ceil_div(body, threads) if body else 0, tail=m % 4 if is_vec else 0,
                g_passes=V.ceil_div(n_g, NT1 if one else 256))


def m_sizes(cus):
    """{name: m} of the scalar kernels, every name asserting the side it is named for on a part of `cus` compute units."""
    cap = V.stream_cap(cus)
    for name, m in M_SIZES.items():
        p, d = scalars_plan(m, 3, cus), stream_plan(m, cus, (0, 0))
        if name in ("empty", "one", "three"):
            expect(p, form="one_block", passes=0, tail=m), expect(d, grid=1, passes=0, tail=m)
        elif name in ("four", "body+tail"):
            expect(p, form="one_block", passes=1, tail=m % 4), expect(d, grid=V.ceil_div(m, 1024), passes=1)
        elif name == "last-one-block":
            expect(p, form="one_block", passes=4, tail=0), expect(d, grid=min(16, cap))
        elif name in ("first-multi", "first-multi-vec"):
            expect(p, form="multi", grid=min(17, cap), tail=m % 4), expect(d, grid=min(17, cap))
        elif name == "multi-66-blocks":
            expect(p, form="multi", grid=min(66, cap), tail=1)
        else:
            expect(p, form="multi", grid=cap, tail=3)
            assert p["passes"] >= 2 and m > 1024 * 1024 >= cap * 1024                    # the capped grid strides
    return dict(M_SIZES)


def n_gamma_plans(cus):
    """{n_g: plan at m = 1027}: one block up to 2^16 partials (1, 2 and 64 passes of its 1024 threads); beyond, the multi-block form
    on a vector one workgroup would hold: k_dot_pair on 2 blocks at m = 1027, and at m = 3 on ONE, so that k_sharded_finalize runs
    with nblocks = 1 (`NG_ONE_ROW_M`)."""
    out = {}
    for n_g in N_GAMMA:
        p = scalars_plan(1027, n_g, cus)
        expect(p, form="one_block", grid=1) if n_g <= 65536 else expect(p, form="multi", grid=2)
        out[n_g] = p
    expect(out[1024], g_passes=1), expect(out[1025], g_passes=2), expect(out[65536], g_passes=64), expect(out[65537], g_passes=257)
    expect(scalars_plan(NG_ONE_ROW_M, 65537, cus), form="multi", grid=1, passes=0, tail=3)
    expect(scalars_plan(NG_ONE_ROW_M, 65536, cus), form="one_block")
    return out


def update_plan(n, m, cus, offsets=(0,)):
    """k_cgls_sharded_update: the grid follows the longer of n and m; (plan over n, plan over m)."""
    return stream_plan(n, cus, offsets, m=m), stream_plan(m, cus, offsets, m=n)


def nm_shapes(cus):
    """The (n, m) of the update, each asserting its branch: tails of both lengths, an empty side, two blocks, the capped grid."""
    cap = V.stream_cap(cus)
    for n, m in NM_SHAPES:
        pn, pm = update_plan(n, m, cus)
        assert pn["grid"] == pm["grid"] == stream_grid(max(n, m), cus)
        expect(pn, tail=n % 4, vec=True), expect(pm, tail=m % 4)
        if max(n, m) > 1 << 20:
            assert pn["grid"] == cap and max(pn["passes"], pm["passes"]) >= 2 and min(pn["passes"], pm["passes"]) == 1
        elif n == m == 66561:
            expect(pn, grid=min(66, cap), passes=1, tail=1)
    return NM_SHAPES


# ----------------------------------------------------------------------------------------------------------- the scalar kernels
def dot_pair(q, w, exact):
    """[qq, qw, ww] as Refs; w None: the last two are exactly 0."""
    zero = Ref(np.float64(0.0), None, 0.0)
    if w is None:
        return [sums(dot_terms(1, q), exact), zero, zero]
    return [sums(dot_terms(1, q), exact), sums(dot_terms(0, q, w), exact), sums(dot_terms(1, w), exact)]


def gamma_source(n_g, unit=3):
    """(the n_g partials between two poison slots, their exact total); n_g = 0: two poison slots and no total."""
    p, total = partials(n_g, unit)
    assert n_g <= 65537 and unit <= 7 and total * 16 < 2.0 ** 35
    return poisoned(p), (total if n_g else None)


# ----------------------------------------------------------------------------------------------------------- the update
def scalars(G4, gprev, first, exact):
    """g, beta_d, beta, alpha, and delta as a Ref (bound None: the published delta must be equal) of one update."""
    g, qq, qw, ww = (np.float64(v) for v in G4)
    F = fractions.Fraction
    s = types.SimpleNamespace(g=g)
    if first:
        s.beta_d, dF, mag = np.float64(0.0), F(float(qq)), 0.0
    else:
        s.beta_d = g / np.float64(gprev)
        b = F(float(s.beta_d))
        dF = F(float(qq)) + 2 * b * F(float(qw)) + b * b * F(float(ww))
        mag = abs(float(qq)) + 2.0 * abs(float(s.beta_d) * float(qw)) + float(s.beta_d) ** 2 * float(ww)
    ref = np.float64(float(dF))
    bound = 0.0 if first else 4.0 * U53 * mag
    if exact:
        assert F(float(ref)) == dF
    s.delta = Ref(ref, None if (exact or first) else bound, mag)
    s.beta = np.float32(s.beta_d)
    lo, hi = np.float64(float(dF - F(bound))), np.float64(float(dF + F(bound)))
    s.alpha = np.float32(g / ref)
    assert np.float32(g / lo) == s.alpha == np.float32(g / hi), ("alpha is ambiguous over delta's interval", G4, gprev)
    return s


def update(G4, gprev, first, x, p, t, r, q, w, xt, exact, count=None):
    """The reference of one k_cgls_sharded_update as a dict: sc (`scalars`), p, w, d, x, x2 (the two-rounding x'), r, norms (three Refs,
    the third None without x_true)."""
    sc = scalars(G4, gprev, first, exact)
    pn = np.array(t, dtype=np.float32) if first else p_update(t, p, sc.beta, count)
    wn = np.array(q, dtype=np.float32) if first else fma32(sc.beta, w, q, count)
    xf, x2, d = x_update(x, pn, sc.alpha, count)
    rn = r_update(r, wn, sc.alpha, count)
    terms = x_norm_terms(xf, d, xt)
    norms = [sums(terms[0], exact), sums(terms[1], exact), None if xt is None else sums(terms[2], exact)]
    return dict(sc=sc, p=pn, w=wn, d=d, x=xf, x2=x2, r=rn, norms=norms)


def one_rounding_case(n=1027):
    """(x, p, t) general for a FIRST step with GENERAL_FIRST[0] (p' = t, alpha = fl32(3 / 7)): the entries behind the float4 body (the
    tail of an aligned launch) are copies of body entries on which the one-rounding and the two-rounding x' differ."""
    body = n // 4 * 4
    x, p, t = vec(n, False, "x", "1r"), vec(n, False, "p", "1r"), vec(n, False, "t", "1r")
    alpha = scalars(GENERAL_FIRST[0], None, True, False).alpha
    fused, two, _ = x_update(x, t, alpha)
    pick = np.flatnonzero(fused[:body] != two[:body])[:n - body]
    assert pick.size == n - body
    x[body:], t[body:] = x[pick], t[pick]
    return x, p, t
