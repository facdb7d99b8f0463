"""The cases of tests/vec_cases.py checked on the CPU: the exactness claims by brute force, the tie handling of the one-rounding
reference, the launch plans' branches on three compute-unit counts, the float64 references against np.longdouble, and
tests/cpu_engine.py's cgls_update against the two forms of the x update."""
import fractions

import numpy as np
import pytest
import torch

import vec_cases as C

CUS = (256, 304, 64)


def chained(n, count, exact, with_count=None):
    """x_0 and `count` chained x updates: lists of the fused iterates, the two-rounding iterates and the d of every step."""
    x = C.vec(n, exact, "x")
    S, steps = C.xs_scalars(count, count + 3, exact)
    xf, x2, ds = [x], [x], []
    for c, st in enumerate(steps):
        p = C.vec(n, exact, "p", c)
        f, _, d = C.x_update(xf[-1], p, st, with_count)
        _, t, _ = C.x_update(x2[-1], p, st)
        xf.append(f), x2.append(t), ds.append(d)
    return xf, x2, ds, steps


def forms_apart(x, d, xf, x2):
    """|x' fused - x' in two roundings| in ulps of the largest of |x|, |d|, |x'|.  With e = x + step p exact: |x2 - e| <= ulp(d) / 2 +
    ulp(x2) / 2 and |xf - e| <= ulp(xf) / 2, so the two are at most 1.5 such ulps apart — and, where x and step p cancel, many ulps of the
    small result: `one ulp of the result` holds only where nothing cancels."""
    top = np.maximum(np.maximum(np.abs(x), np.abs(d)), np.maximum(np.abs(xf), np.abs(x2)))
    return np.abs(xf.astype(np.float64) - x2.astype(np.float64)) / np.spacing(top).astype(np.float64)


def test_exact_operands_are_exact_in_every_order():
    """8 chained steps: the fused and the two-rounding form give the same float32 values, which are the exact rationals; float32 sums
    of 32 terms and float64 sums of 2^20 terms give the same total forwards, backwards, shuffled and pairwise."""
    n = 1 << 20
    xf, x2, ds, steps = chained(n, 8, True)
    assert [float(s) for s in steps] == [C.STEPS[(j + c) % 5] for c, j in enumerate(range(4, 12))]
    for a, b in zip(xf, x2):
        assert np.array_equal(a, b)
    x64 = xf[0].astype(np.float64)
    for c, st in enumerate(steps):
        x64 = x64 + np.float64(st) * C.vec(n, True, "p", c).astype(np.float64)           # 9 bits: exact in float64 beyond doubt
        assert np.array_equal(xf[c + 1].astype(np.float64), x64) and np.abs(x64).max() <= 13.0
        assert np.array_equal(x64 * 32, np.rint(x64 * 32))
    rng = np.random.default_rng(5)
    xt = C.vec(n, True, "xt")
    r, w, t = C.vec(n, True, "r"), C.vec(n, True, "w"), C.vec(n, True, "t")
    families = C.x_norm_terms(xf[8], ds[7], xt) + [C.dot_terms(0, r, w), C.dot_terms(2, r, w),
                                                   C.dot_terms(0, C.axpby(0.375, r), t)]
    for st in C.STEPS:
        assert np.array_equal(C.r_update(r, w, st).astype(np.float64), r.astype(np.float64) - st * w.astype(np.float64))
        assert np.array_equal(C.p_update(t, r, st).astype(np.float64), t.astype(np.float64) + st * r.astype(np.float64))
        assert np.array_equal(C.axpby(st, r, 0.75, w).astype(np.float64), st * r.astype(np.float64) + 0.75 * w.astype(np.float64))
    for terms in families:
        total = terms.sum()
        perm = rng.permutation(n)
        assert total == terms[::-1].sum() == terms[perm].sum() == np.cumsum(terms)[-1] == np.cumsum(terms[perm])[-1]
        assert total == float(terms.astype(C.WIDE).sum())
        g32 = terms[:1 << 15].astype(np.float32).reshape(-1, 32)
        assert np.array_equal(g32.astype(np.float64), terms[:1 << 15].reshape(-1, 32))
        want = terms[:1 << 15].reshape(-1, 32).sum(axis=1)
        for order in (np.arange(32), np.arange(32)[::-1], rng.permutation(32)):
            acc = np.zeros(g32.shape[0], dtype=np.float32)
            for j in order:
                acc = acc + g32[:, j]
            assert np.array_equal(acc.astype(np.float64), want)
    # the bit count of the docstring at n = 2^25: the largest square times n stays below 2^53 units of 2^-10
    assert 14.0 ** 2 * 2.0 ** 25 * 2.0 ** 10 < 2.0 ** 53


def test_partials_are_distinct_multiples_with_exact_totals():
    for n in C.N_PARTIALS:
        for ratio, (un, ud) in C.UNITS.items():
            pn, tn, pd, td = C.ratio_sources(ratio, n, n)
            for p, tot in ((pn, tn), (pd, td)):
                assert np.array_equal(p * 16, np.rint(p * 16)) and len(set(p.tolist())) == n
                assert p.sum() == p[::-1].sum() == tot == float(sum(fractions.Fraction(v) for v in p))
            assert C.step32(tn, td) == np.float32(ratio)
    for c in C.COEFS:
        v = C.coef(*c)
        assert v in (0.375, 0.75, 1.5) and np.float32(v) == v


@pytest.mark.parametrize("n", [4099, (1 << 20) + 1, (11 << 20) + 3])
def test_tie_handling_of_the_one_rounding_reference(n):
    """Fraction and float64 agree away from ties; the share decided by Fraction stays below 1e-3 (below 10 elements under 2^20); the two
    forms of the x update differ on a fifth of general data, by at most 1.5 ulp of the largest of |x|, |d|, |x'| (`forms_apart`)."""
    x, p = C.vec(n, False, "x"), C.vec(n, False, "p")
    step = C.step32(3.0, 7.0)
    flagged = []
    xf, x2, d = C.x_update(x, p, step, flagged)
    assert flagged[0] < 1e-3 * n and (n >= 1 << 20 or flagged[0] < 10), (n, flagged)
    rng = np.random.default_rng(n)
    for i in rng.integers(0, n, 1500):
        q = fractions.Fraction(float(step)) * fractions.Fraction(float(p[i])) + fractions.Fraction(float(x[i]))
        lo, hi = np.nextafter(xf[i], np.float32(-np.inf)), np.nextafter(xf[i], np.float32(np.inf))
        assert C._round_fraction(q, xf[i], lo, hi) == xf[i]
    differ = np.count_nonzero(xf != x2)
    assert 0.1 * n < differ < 0.35 * n, differ
    assert np.all(forms_apart(x, d, xf, x2) <= 1.5)
    for got in (C.r_update(x, p, step, flagged), C.axpby(step, x, np.float32(5.0 / 3.0), p, flagged)):
        assert flagged[-1] < 1e-3 * n and (n >= 1 << 20 or flagged[-1] < 10)


def test_an_exact_tie_goes_to_even():
    """x + step p exactly halfway between two float32: float64 sees the tie and Fraction decides it; one float64 ulp beside it, the
    float64 value decides."""
    one, u = np.float32(1.0), np.float32(2.0 ** -24)
    flagged = []
    got = C.fma32(np.float32(1.0), np.array([u, 3 * u, u * np.float32(1 + 2.0 ** -20)], dtype=np.float32),
                  np.array([one, one, one]), flagged)
    assert flagged == [3]
    assert got[0] == one and got[1] == np.float32(1 + 2.0 ** -22) and got[2] == np.float32(1 + 2.0 ** -23)
    # a product whose low bits break the tie below float64's resolution of the sum: a b = 2^-24 (1 - 2^-46), so c + a b lies 2^-70
    # BELOW the tie between 1 + 2^-23 and 1 + 2^-22; float64 rounds the sum onto the tie and would go to even, 1 + 2^-22
    a, b, c = np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24 * (1 - 2.0 ** -23)), np.float32(1 + 2.0 ** -23)
    assert (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32) == np.float32(1 + 2.0 ** -22)
    assert C.fma32(a, np.array([b]), np.array([c]))[0] == c


@pytest.mark.parametrize("cus", CUS)
def test_every_named_size_reaches_its_branch(cus):
    S = C.sizes(cus)                                       # asserts every plan
    one = C.stream_cap(cus) * 1024
    assert S["pass"] == one and C.stream_plan(S["two-passes+tail"], cus, (0, 0))["passes"] == 3
    assert max(S.values()) < C.NT_STORES
    for n in C.nt_sizes().values():
        assert C.stream_plan(n, cus, (0,))["passes"] >= 11 and C.stream_plan(n, cus, (0,))["tail"] in (0, 3)
    # the VEC decision is a function of the byte offsets: one operand 4, 8 or 12 bytes off switches the float4 body off
    for off in (4, 8, 12):
        for k in range(3):
            offs = [0, 0, 0]
            offs[k] = off
            C.expect(C.stream_plan(4099, cus, offs), vec=False, tail=0, passes=4, grid=5)
    C.expect(C.stream_plan(4099, cus, (0, 16, 32)), vec=True, tail=3)
    # k_cgls_update: the grid follows the longer of n and m
    C.expect(C.stream_plan(777, cus, (0,), m=4099), grid=5, passes=1, tail=1)
    C.expect(C.stream_plan(4099, cus, (0,), m=777), grid=5, passes=1, tail=3)
    for nb in C.FINALIZE_BLOCKS:
        n = C.n_for_blocks(nb, cus)
        assert (n is None) == (nb > C.stream_cap(cus))
    # the hint bits of the batched x update
    assert C.xs_nt(1027, 1, False) == 0 and C.xs_nt(1027, 3, True) == 288 and C.xs_nt(1027, 3, False) == 288 | 1536
    assert C.xs_nt(C.NT_STORES + 3, 3, False) == 195 | 288 | 1536
    for count in range(1, 9):
        for s_slots in (count, 8):
            for where in ("first", "middle", "last"):
                first = C.xs_first(count, s_slots, where)
                assert (first is None) == (where == "middle" and count < 3)
    for k_last in (5, 10):
        S5, steps = C.xs_scalars(5, k_last, True)
        assert (S5[0] != -1) == (k_last == 5) and S5[5 * k_last + 1] == -1 and len(steps) == 5


@pytest.mark.parametrize("n", [4099, (1 << 20) + 1])
def test_sum_references_against_longdouble(n):
    """The float64 references of the general operands err by less than 1e-6 of their bound (np.longdouble as the instrument)."""
    x, y = C.vec(n, False, "x"), C.vec(n, False, "p")
    xf, _, d = C.x_update(x, y, C.step32(3.0, 7.0))
    for terms64, termsw in zip(C.x_norm_terms(xf, d, y) + [C.dot_terms(0, x, y)],
                               C.x_norm_terms(xf, d, y, dtype=C.WIDE) + [C.dot_terms(0, x, y, dtype=C.WIDE)]):
        R = C.sums(terms64, False)
        wide = termsw.sum()
        assert abs(float(C.WIDE(R.ref) - wide)) < max(1e-6, 2.0 / 4096) * R.bound


def test_weights_references():
    x, y = C.vec(1027, False, "x"), C.vec(1027, False, "y")
    ref, special = C.mm_weights(x, y, 1e-3, 1.0)
    v = (x - y).astype(np.float64)
    assert special == 2 and np.allclose(ref, (v * v + 1e-6) ** -0.5, rtol=1e-6)
    assert np.array_equal(C.mm_weights(x, None, 0.1, 2.0)[0], np.ones(1027))
    d = C.vec(257 * 32, False, "d")
    g = C.group_weights(d, 257, 32, np.exp(2), -0.75, 3)
    want = ((d.astype(np.float64).reshape(257, 32) ** 2).sum(axis=1) + np.exp(2)) ** -0.75
    assert g.shape == (3 * 257,) and np.allclose(g, np.tile(want, 3), rtol=1e-14)
    assert np.all(C.ulps32(np.float32(1 + 2.0 ** -23), np.array([1.0])) == 1.0)
    assert not C.far_from_tie(np.array([1 + 2.0 ** -24]))[0] and C.far_from_tie(np.array([1 + 2.0 ** -25]))[0]


def test_cpu_engine_cgls_update_is_the_two_rounding_form():
    """tests/cpu_engine.py forms x + fl32(step p): equal to the two-rounding reference, within one ulp of the fused one the kernels
    compute; its r update is r - fl32(step w) likewise."""
    from cpu_engine import CpuEngine
    eng = CpuEngine()
    n = 4099
    x, p, r, w, xt = (C.vec(n, False, k) for k in ("x", "p", "r", "w", "xt"))
    S = eng.scalars(8)
    S.a[0], S.a[1] = 3.0, 7.0
    tx, tp, tr, tw, tt = (torch.from_numpy(a.copy()) for a in (x, p, r, w, xt))
    out = torch.empty(n)
    eng.cgls_update(S.ref(0), S.ref(1), tx, tp, out, tr, tw, tt, S.ref(2))
    xf, x2, d = C.x_update(x, p, C.step32(3.0, 7.0))
    got = out.numpy()
    assert np.array_equal(got, x2)
    apart = forms_apart(x, d, xf, got)
    assert np.all(apart <= 1.5)
    plain = np.abs(xf) >= np.maximum(np.abs(x), np.abs(d))            # nothing cancels: one ulp of the result itself
    assert plain.sum() > n // 4
    assert np.all(np.abs(got.astype(np.float64) - xf.astype(np.float64))[plain] <= np.spacing(np.maximum(np.abs(xf), np.abs(got)))[plain])
    assert np.count_nonzero(got != xf) > n // 10
    for terms, s in zip(C.x_norm_terms(x2, d, xt), S.a[2:5]):
        R = C.sums(terms, False)
        assert abs(s - R.ref) <= R.bound
