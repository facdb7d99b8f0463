"""The cases of tests/sharded_cases.py checked on the CPU: the exactness margins by brute force, every named size on its branch for
three compute-unit counts, the alpha-unambiguity of the general G4 sets, the share of general entries on which the one-rounding and
the two-rounding x' differ, and that every general entry is decided (float64 or, near a tie, Fraction)."""
import fractions

import numpy as np
import pytest

import sharded_cases as C
import vec_cases as V

CUS = (256, 304, 64)


def operands(n, m, exact, *key):
    x, p, t, xt = (C.vec(n, exact, k, *key) for k in ("x", "p", "t", "xt"))
    r, q, w = (C.vec(m, exact, k, *key) for k in ("r", "q", "w"))
    return x, p, t, xt, r, q, w


def orders_agree(terms, rng):
    """A float64 sum forwards, backwards, shuffled, running and in longdouble; float32 sums of 32 terms in three orders."""
    total = terms.sum()
    perm = rng.permutation(terms.size)
    assert total == terms[::-1].sum() == terms[perm].sum() == np.cumsum(terms)[-1] == np.cumsum(terms[perm])[-1]
    assert total == float(terms.astype(V.WIDE).sum())
    k = terms.size // 32 * 32
    g32 = terms[:k].astype(np.float32).reshape(-1, 32)
    assert np.array_equal(g32.astype(np.float64), terms[:k].reshape(-1, 32))
    want = terms[:k].reshape(-1, 32).sum(axis=1)
    for order in (np.arange(32), np.arange(32)[::-1], rng.permutation(32)):
        acc = np.zeros(g32.shape[0], dtype=np.float32)
        for j in order:
            acc = acc + g32[:, j]
        assert np.array_equal(acc.astype(np.float64), want)


@pytest.mark.parametrize("first", [True, False])
def test_exact_operands_are_exact_in_every_order(first):
    """The exact first and later step at n = m = 2^20: every vector equals plain float64 arithmetic on the same operands, lies on the
    grid the docstring names, the fused and the two-rounding x' coincide, and every sum is the same in every order."""
    n = 1 << 20
    x, p, t, xt, r, q, w = operands(n, n, True)
    E = C.EXACT_FIRST if first else C.EXACT_LATER
    if first:
        p, w = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
    R = C.update(E["G4"], E["gprev"], first, x, p, t, r, q, w, xt, True)
    sc = R["sc"]
    assert (float(sc.beta), float(sc.alpha), float(sc.delta.ref)) == (E["beta"], E["alpha"], E["delta"]) and sc.delta.bound is None
    d64 = lambda a: a.astype(np.float64)                                              # noqa: E731
    p64 = d64(t) if first else d64(t) + 0.5 * d64(p)
    w64 = d64(q) if first else d64(q) + 0.5 * d64(w)
    for got, want, grid, top in ((R["p"], p64, 16, 1.5), (R["w"], w64, 16, 1.5), (R["d"], 0.25 * p64, 64, 0.375),
                                 (R["x"], d64(x) + 0.25 * p64, 64, 1.375), (R["r"], d64(r) - 0.25 * w64, 64, 1.375)):
        assert np.array_equal(d64(got), want) and np.abs(want).max() <= top < 2.0
        assert np.array_equal(want * grid, np.rint(want * grid))
    assert np.array_equal(R["x"], R["x2"])
    rng = np.random.default_rng(7)
    families = C.x_norm_terms(R["x"], R["d"], xt) + [C.dot_terms(1, q), C.dot_terms(0, q, w if not first else t), C.dot_terms(1, t)]
    for terms in families:
        assert np.array_equal(terms * 4096, np.rint(terms * 4096)) and terms.max() < 9.0
        orders_agree(terms, rng)
    for ref, terms in zip(R["norms"], families):
        assert ref.bound is None and ref.ref == terms.sum()
    # the margin of the docstring: 2^21 terms below 9 in units of 2^-12 stay below 2^53
    assert 9.0 * 2.0 ** 21 * 2.0 ** 12 < 2.0 ** 53


def test_the_chain_stays_exact():
    """Three chained exact steps (CHAIN) at (1027, 515): alpha = 1 / 4 throughout, beta = 0, 1 / 2, 1 / 2; every iterate equals plain
    float64 arithmetic and the fused and two-rounding forms coincide."""
    n, m = 1027, 515
    x, p, w, r = C.vec(n, True, "x"), None, None, C.vec(m, True, "r")
    x64, r64, p64, w64 = x.astype(np.float64), r.astype(np.float64), 0.0, 0.0
    for k, G4 in enumerate(C.CHAIN, 1):
        t, q = C.vec(n, True, "t", k), C.vec(m, True, "q", k)
        R = C.update(G4, None if k == 1 else C.CHAIN[k - 2][0], k == 1, x, p, t, r, q, w, None, True)
        assert float(R["sc"].alpha) == 0.25 and float(R["sc"].beta) == (0.0 if k == 1 else 0.5)
        p64, w64 = t.astype(np.float64) + 0.5 * p64, q.astype(np.float64) + 0.5 * w64
        x64, r64 = x64 + 0.25 * p64, r64 - 0.25 * w64
        for got, want in ((R["p"], p64), (R["w"], w64), (R["x"], x64), (R["r"], r64), (R["x2"], x64)):
            assert np.array_equal(got.astype(np.float64), want) and np.abs(want).max() < 4.0
        assert np.array_equal(x64 * 128, np.rint(x64 * 128))
        for ref in R["norms"][:2]:
            assert ref.bound is None
        x, p, w, r = R["x"], R["p"], R["w"], R["r"]


def test_gamma_partials_sum_exactly_in_any_order():
    rng = np.random.default_rng(11)
    for n_g in C.N_GAMMA:
        for unit in (3, 7):
            src, total = C.gamma_source(n_g, unit)
            assert src[0] == src[-1] == V.POISON and src.size == n_g + 2
            if n_g == 0:
                assert total is None
                continue
            parts = src[1:-1]
            assert parts.sum() == parts[::-1].sum() == parts[rng.permutation(n_g)].sum() == np.cumsum(parts)[-1] == total
            if n_g <= 4096:
                assert total == float(sum(fractions.Fraction(v) for v in parts))
            assert len(set(parts.tolist())) == n_g and total * 16 < 2.0 ** 35 and total < V.POISON
            # the order of the kernels: 1024 (one workgroup) or 256 (finalize) strided accumulators, then a tree
            for lanes in (1024, 256):
                acc = np.zeros(lanes)
                for lo in range(0, n_g, lanes):
                    seg = parts[lo:lo + lanes]
                    acc[:seg.size] += seg
                assert acc.sum() == total


@pytest.mark.parametrize("cus", CUS)
def test_every_named_size_reaches_its_branch(cus):
    S = C.m_sizes(cus)                                                                # asserts every plan
    assert sorted(S.values()) == [0, 1, 3, 4, 1027, 16384, 16385, 16388, 66561, 1300003]
    G = C.n_gamma_plans(cus)
    assert tuple(G) == (0, 1, 2, 1023, 1024, 1025, 4096, 65536, 65537)
    assert C.nm_shapes(cus) == ((1, 1), (3, 5), (1027, 515), (515, 1027), (4096, 0), (0, 4096), (66561, 66561), (1300003, 1027),
                                (1027, 1300003))
    # the threshold is a conjunction: either side alone leaves the one-workgroup form
    for m, n_g, form in ((16384, 65536, "one_block"), (16385, 65536, "multi"), (16384, 65537, "multi"), (0, 0, "one_block"),
                         (0, 65537, "multi")):
        C.expect(C.scalars_plan(m, n_g, cus), form=form)
    C.expect(C.scalars_plan(16385, 0, cus), grid=min(17, V.stream_cap(cus)))
    # one operand off a 16-byte boundary switches the float4 body off in both forms; grid_for is stream_grid
    for m in (1027, 16388):
        for offs in ((4, 0), (0, 8)):
            C.expect(C.scalars_plan(m, 3, cus, offs), vec=False, tail=0, passes=V.ceil_div(m, 1024 if m == 1027 else 17 * 256))
    assert C.stream_grid is V.stream_grid and C.stream_plan is V.stream_plan
    pn, pm = C.update_plan(1300003, 1027, cus)
    C.expect(pn, grid=V.stream_cap(cus), tail=3), C.expect(pm, grid=V.stream_cap(cus), passes=1, tail=3)
    C.expect(C.update_plan(1027, 515, cus, (0, 4))[0], vec=False, tail=0, grid=2)


def test_alpha_is_unambiguous_for_every_general_g4():
    """`scalars` asserts that fl32(g / delta) is one float32 over delta's whole interval; here also that the ratios are not dyadic,
    that delta's bound is a few float64 ulps, and that alpha sits far from a float32 tie compared with that bound."""
    sets = [(G4, None, True) for G4 in C.GENERAL_FIRST] + [(G4, gp, False) for G4, gp in C.GENERAL_LATER]
    for G4, gprev, first in sets:
        s = C.scalars(G4, gprev, first, False)
        assert s.delta.ref > 0 and float(s.alpha) != float(s.g / s.delta.ref)                # not representable: a general step
        if first:
            assert s.delta.bound is None and s.delta.ref == G4[1] and s.beta == 0
            continue
        assert float(s.beta) != float(s.beta_d)
        assert 0 < s.delta.bound <= 8 * np.spacing(s.delta.ref)
        a = s.g / s.delta.ref
        rel = s.delta.bound / s.delta.ref                                                  # the relative width of alpha's interval
        assert V.far_from_tie(np.array([a]), rel=64 * rel)[0]
        F = fractions.Fraction
        b = F(float(s.beta_d))
        assert F(float(s.delta.ref)) != F(G4[1]) + 2 * b * F(G4[2]) + b * b * F(G4[3])       # delta itself is rounded: a real bound
    for E, first in ((C.EXACT_FIRST, True), (C.EXACT_LATER, False)):
        s = C.scalars(E["G4"], E["gprev"], first, True)
        assert (float(s.alpha), float(s.beta), float(s.delta.ref), s.delta.bound) == (E["alpha"], E["beta"], E["delta"], None)


@pytest.mark.parametrize("n", [1027, 66561])
def test_general_entries_are_decided_and_the_two_forms_differ(n):
    """On general operands the one-rounding x' differs from the two-rounding x' in at least a tenth of the entries — a device that
    rounded alpha p' first would fail the GPU test's equality —, in the float4 body's part and in a tail of 3 alike; the entries
    within TIE_MARGIN of a tie (decided by Fraction) are few, and Fraction agrees with float64 on a sample of the others."""
    m = 515
    x, p, t, xt, r, q, w = operands(n, m, False)
    rng = np.random.default_rng(n)
    for G4, gprev, first in [(C.GENERAL_FIRST[0], None, True)] + [(G4, gp, False) for G4, gp in C.GENERAL_LATER]:
        flagged = []
        R = C.update(G4, gprev, first, x, p, t, r, q, w, xt, False, flagged)
        assert len(flagged) == (2 if first else 4) and sum(flagged) < max(4, 1e-3 * (n + m)), flagged
        differ = R["x"] != R["x2"]
        assert differ.sum() >= 0.1 * n, (differ.sum(), n)
        assert differ.sum() <= 0.4 * n
        alpha = R["sc"].alpha
        for i in rng.integers(0, n, 300):
            exact = fractions.Fraction(float(alpha)) * fractions.Fraction(float(R["p"][i])) + fractions.Fraction(float(x[i]))
            lo, hi = np.nextafter(R["x"][i], np.float32(-np.inf)), np.nextafter(R["x"][i], np.float32(np.inf))
            assert V._round_fraction(exact, R["x"][i], lo, hi) == R["x"][i]
        for ref in R["norms"]:
            assert ref.bound > 0 and ref.bound < 1e-9 * ref.S + 1e-300
    # the GPU test's one-rounding check: a tail of 3 built from body entries that tell the forms apart
    xs, ps, ts = C.one_rounding_case(1027)
    R = C.update(C.GENERAL_FIRST[0], None, True, xs, None, ts, r, q, None, None, False)
    differ = R["x"] != R["x2"]
    assert differ[1024:].all() and differ[:1024].sum() >= 102


def test_dot_pair_references():
    """qq, qw, ww against np.longdouble; without w the last two are exact zeros."""
    for m in (1027, 66561):
        q, w = C.vec(m, False, "q"), C.vec(m, False, "w")
        for ref, wide in zip(C.dot_pair(q, w, False), (C.dot_terms(1, q, dtype=V.WIDE), C.dot_terms(0, q, w, dtype=V.WIDE),
                                                       C.dot_terms(1, w, dtype=V.WIDE))):
            assert abs(float(V.WIDE(ref.ref) - wide.sum())) < max(1e-6, 2.0 / 4096) * ref.bound
        z = C.dot_pair(q, None, False)
        assert z[1].ref == 0.0 and z[2].ref == 0.0 and z[1].bound is None and z[2].bound is None
    e = C.dot_pair(C.vec(0, True, "q"), C.vec(0, True, "w"), True)
    assert [float(v.ref) for v in e] == [0.0, 0.0, 0.0]
