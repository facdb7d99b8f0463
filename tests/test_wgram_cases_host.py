"""The cases of tests/wgram_cases.py checked on the CPU: the exact operands are what the docstring says and every sum they enter is
exact; the launch plans put every named case on the branch it is named for, at 256 compute units and at two other counts, and between
them the cases reach every (kernel, template arguments) the two launchers can instantiate; the float64 references stay below 1e-6
of the bounds (against np.longdouble); the TV reference agrees with the oracle's sparse L."""
import numpy as np
import pytest

import wgram_cases as C

CUS = 256
ROW_CASES = C.all_row_cases(CUS)
TV_CASES = C.tv_register_cases() + C.tv_lds_cases()
REF_SLACK = 1e-6


def test_exact_operands_are_exact_in_every_order_and_every_bf16_split():
    assert C.exactness_by_brute_force(groups=4000) >= 8000


@pytest.mark.parametrize("exact", [True, False])
def test_operands_are_what_the_docstring_says(exact):
    d = C.Rows(5, 1031, exact)
    V, w, z = C.tv_operands(3, 32, exact)
    assert all(a.dtype == np.float32 for a in (d.V, d.b, d.w, V, w, z))
    assert d.V.shape == (5, 1031) and V.shape == (3, 1024) and w.shape == (2 * 32 * 31,) and z.shape == (1024,)
    if exact:
        for a in (d.V, d.b, V, z):
            assert np.array_equal(a * 8, np.rint(a * 8)) and np.abs(a).max() <= 1.0
        assert np.all(np.isin(d.w, C.EXACT_W)) and np.all(np.isin(w, C.EXACT_W)) and (w == 0).any() and (d.w == 0).any()
        assert np.all(w[:32 * 31].reshape(32, 31)[:, 30] == 2) and np.all(w[32 * 31:].reshape(31, 32)[30] == 2)
        assert np.all(np.abs(V.reshape(3, 32, 32)[:, :, 31]) == 1) and np.all(np.abs(V.reshape(3, 32, 32)[:, 31, :]) == 1)
        V8, w8, z8 = C.tv_operands(3, 32, True, as_int8=True)
        assert V8.dtype == np.int8 and np.array_equal(V8 * np.float32(0.125), V) and np.array_equal(z8 * np.float32(0.125), z)
        # the weighted differences fit one bf16 piece; the totals are multiples of 2^-8 that float64 holds
        D = C.tv_diffs(V, 32, w)
        hi, mid, lo = C.bf16_pieces(D)
        assert np.array_equal(hi, D) and not mid.any() and not lo.any()
        G, _ = C.tv_ref_host(V, 32, w)
        assert np.array_equal(G * 256, np.rint(G * 256))
    else:
        for a in (d.V, d.b, V, z):
            assert np.abs(a).min() >= 2.0 ** -6 and np.abs(a).max() <= 2.0 ** 6
        assert d.w.min() >= 0.25 and d.w.max() < 1.25 and w.min() >= 0.25 and w.max() < 1.25
    assert np.all(d.V[:, [0, -1]] != 0) and np.all(d.b[[0, -1]] != 0) and np.all(d.w[[0, -1]] != 0)


@pytest.mark.parametrize("case", ROW_CASES, ids=repr)
def test_stored_row_case_reaches_its_branch_at_256_compute_units(case):
    for has_w in (False, True):
        p = case.check(has_w, CUS)
        assert p["KA"] == case.KA and case.ld >= case.m
        if p["kernel"] == "k_wgram_t16":
            assert case.ld % 4 == 0 and case.KA <= 48


@pytest.mark.parametrize("case", TV_CASES, ids=repr)
def test_tv_case_reaches_its_branch_at_256_compute_units(case):
    for mode in C.TV_MODES:
        p = case.check(mode, CUS)
        assert (p["kernel"] == "k_wgram_tv_lds") == p["use_lds"]


def test_every_wait_pattern_of_the_lds_kernel_is_run():
    """The staged loads per wave and image row (what wait_vm_le counts) differ for every k from 1 to 32, with and without z."""
    for z in (False, True):
        seen = {C.wgram_tv_plan(k, 2048, z, "fp32", CUS)["pieces"] for k in range(1, 33)}
        assert len(seen) == 32 and all(max(p) <= 5 for p in seen)


def test_every_instantiation_is_reached_by_a_named_case():
    want = C.coverage_table()
    assert len(want) == 60
    assert C.coverage(CUS) == want


@pytest.mark.parametrize("cus", [64, 304])
def test_the_case_builder_finds_every_branch_on_other_compute_unit_counts(cus):
    assert C.coverage(cus) == C.coverage_table()
    sizes = {c.name: c.m for c in C.all_row_cases(cus)}
    base = {c.name: c.m for c in ROW_CASES}
    assert sizes.keys() == base.keys() and any(sizes[n] != base[n] for n in sizes)      # the sizes moved, the names did not


def test_the_older_shapes_miss_the_branches_the_new_cases_are_named_for():
    """tests/test_gpu_kernels.py::test_wgram at 256 compute units: no wave of k_wgram_t16 gets a second group, no workgroup of
    k_wgram_mfma a second chunk, and the scalar tail of k_wgram_t16 starts at a multiple of 4 with ld == m — from the plans alone."""
    older = [(1, 64), (3, 5000), (4, 4096), (7, 10_001), (13, 33_000), (14, 96), (20, 40_004), (30, 8_200), (31, 4_100), (33, 70_001),
             (45, 12_004), (61, 20_000), (90, 9_000)]
    for k, m in older:
        for has_w in (False, True):
            p = C.wgram_plan(k, m, m, has_w, True, True, CUS)
            if p["kernel"] == "k_wgram_t16":
                assert p["groups"][0] <= 1 and p["branch"] in ("lone", "none") and m % 4 == 0
            elif p["kernel"] == "k_wgram_mfma":
                assert p["chunks"][0] == 1
                assert p["targs"][2] is True                                             # HAS_B always
            else:
                assert p["vec"] == (m % 4 == 0)


def _distinct(cases):
    seen, out = set(), []
    for c in cases:
        key = (c.k, c.m, c.has_b)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("case", _distinct(ROW_CASES), ids=repr)
def test_float64_reference_against_longdouble(case):
    """General operands of every distinct (k, m, b): the float64 reference's own error below 1e-6 of the bound (on the first and the
    last rows of the augmented Gram — G's first and last row, c1, c2 — for the long cases; weighted calls: the unweighted ones round
    less); exact operands: reference and np.longdouble agree to the bit and are multiples of 2^-8."""
    k, m, KA = case.k, case.m, case.KA
    pair_path = KA > 64
    for exact in (False, True):
        d = C.rows_case(k, m, exact)
        b = d.b if case.has_b else None
        R = C.gram_ref(d.V, k, d.w, b, m, pair_path=pair_path, exact=exact)
        rows = sorted({0, k - 1} | ({KA - 2, KA - 1} if case.has_b else set())) if k * m > 1 << 16 else list(range(KA))
        Wd = C.gram_rows_wide(d.V, k, d.w, b, m, rows)
        G = R["G"].ref.reshape(k, k)
        pieces = [(G[a], Wd[i][:k], None if exact else R["G"].bound.reshape(k, k)[a]) for i, a in enumerate(rows) if a < k]
        if case.has_b and not pair_path:                       # (the tile-pair path's c1, c2 repeat k_gemv_t's float32 steps: gemv_cases' own test)
            pieces.append((R["c1"].ref, Wd[rows.index(KA - 2)][:k], R["c1"].bound))
            pieces.append((R["c2"].ref, Wd[rows.index(KA - 1)][:k], R["c2"].bound))
        for ref, wide, bound in pieces:
            if exact:
                assert np.array_equal(ref.astype(C.WIDE), wide) and np.array_equal(ref * 256, np.rint(ref * 256))
                assert np.abs(ref).max(initial=0.0) < 2.0 ** 44
            else:
                err = np.abs(ref.astype(C.WIDE) - wide).astype(np.float64)
                assert np.all(err <= REF_SLACK * bound), (case.name, float(np.max(err / np.maximum(bound, 1e-300))))
                assert m == 0 or np.all(bound > 0)


@pytest.mark.parametrize("N,k", C.TV_SMALL)
def test_small_tv_reference_against_the_oracles_sparse_L(N, k):
    for exact in (True, False):
        V, w, z = C.tv_operands(k, N, exact)
        G, h = C.tv_ref_host(V, N, w, z)
        Go = C.tv_ref_oracle(V, N, w)
        assert np.array_equal(G, G.T)
        if exact:
            assert np.array_equal(G, Go) and np.array_equal(h, V.astype(np.float64) @ z.astype(np.float64))
        else:
            # the oracle weights float64 differences, the kernels' form rounds d twice: 2 x 2^-24 per operand
            assert C.tv_relative(G, Go) < 4 * 2.0 ** -24 * (1 + 2.0 ** -20)
            Gw, hw = C.tv_ref_host(V[:2], N, w, z, dtype=C.WIDE)
            assert C.tv_relative(G[:2, :2], Gw.astype(np.float64)) < 1e-12 and np.allclose(h[:2], hw.astype(np.float64), rtol=1e-12)
