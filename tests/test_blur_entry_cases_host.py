"""CPU checks of tests/blur_entry_cases.py, the table of tests/test_gpu_blur_entrywise.py: the Kronecker-factor oracle against scipy,
the case table's coverage of every structural situation on 256 CUs, the combs' coverage of the positions they must hit, fp32
emulations of both arithmetic families inside the per-entry bounds, and seeded mutations of the emulations outside them (with the
norm-wise figure the older 1e-5 bar looks at printed beside)."""
import numpy as np
import pytest

import blur_entry_cases as E
from blur_psf_cases import MODES, chain_fp32, convolve_ref
from conftest import relerr

ALL_CASES = E.small_cases() + E.comb_cases()


# ------------------------------------------------------------------------------------------------ oracle against scipy
@pytest.mark.parametrize("mode", MODES)
def test_oracle_is_scipy_on_every_case(mode):
    worst = 0.0
    for c in {(c.psf, c.shape): c for c in ALL_CASES}.values():  # (a slide shape and its offset view are one operator)
        if c.shape[0] * c.shape[1] > 40000:
            continue                                             # (the tall unguarded-block shapes: same code, see below)
        nx, ny = c.shape
        psf = E.entry_psf(c.psf)
        x = np.random.default_rng(nx + ny).standard_normal((nx, ny)).astype(np.float32)
        for tr in (False, True):
            p = psf[::-1, ::-1] if tr else psf
            ref = convolve_ref(x, p, mode)
            o = E.Oracle(psf, nx, ny, mode, tr).apply(x)
            e = float(np.abs(o["y"] - ref).max() / np.abs(ref).max())
            worst = max(worst, e)
            assert e < 1e-13, (E.case_id(c), mode, tr, e)
            assert np.all(o["S"] >= np.abs(o["y"]) * (1 - 1e-12))
    print(f"oracle vs scipy, {mode}: worst {worst:.2e} of max|ref|")


@pytest.mark.parametrize("mode", MODES)
def test_oracle_is_scipy_on_a_tall_unguarded_shape(mode):
    c = E.Case("sep9", E.SLIDE_UNGUARDED[9], "slide")
    nx, ny = c.shape
    psf = E.entry_psf(c.psf)
    x = np.random.default_rng(3).standard_normal((nx, ny)).astype(np.float32)
    for tr in (False, True):
        ref = convolve_ref(x, psf[::-1, ::-1] if tr else psf, mode)
        o = E.Oracle(psf, nx, ny, mode, tr).apply(x)
        assert float(np.abs(o["y"] - ref).max() / np.abs(ref).max()) < 1e-13


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["sep3", "rnd5", "r4x6", "sep11"])
def test_explicit_matrix_is_scipy_column_by_column(name, mode):
    nx, ny = 6, 7
    psf = E.entry_psf(name)
    for tr in (False, True):
        p = psf[::-1, ::-1] if tr else psf
        A, Aabs, cnt = (m.toarray() for m in E.Oracle(psf, nx, ny, mode, tr).matrix())
        ref = np.zeros((nx * ny, nx * ny))
        for j in range(nx * ny):
            e = np.zeros(nx * ny)
            e[j] = 1.0
            ref[:, j] = convolve_ref(e.reshape(nx, ny), p, mode).reshape(-1)
        assert np.abs(A - ref).max() < 1e-13 * np.abs(ref).max()
        assert np.all(Aabs >= np.abs(A) - 1e-18) and np.all((cnt > 0) == (Aabs > 0))
        # the matrix and the factored apply are one operator
        x = np.random.default_rng(1).standard_normal((nx, ny)).astype(np.float32)
        o = E.Oracle(psf, nx, ny, mode, tr).apply(x)
        assert np.allclose(A @ x.reshape(-1).astype(np.float64), o["y"].reshape(-1), rtol=0, atol=1e-14)
        assert np.allclose(cnt @ (x.reshape(-1) != 0), o["T"].reshape(-1))


# ------------------------------------------------------------------------------------------------ coverage on 256 CUs
def test_restated_grids_match_known_values():
    """Figures the library's own tests and documents state: 2600 x 776 at 9x9 gets 19-row bands (tests/test_gpu_blur_norm_interior.py),
    4096^2 at 9x9 64-row bands (csrc/blur2d.hip's comment on slide_grid)."""
    assert E.slide_grid(2600, 776, 1, 9, 256) == (4, 137, 19)
    assert E.slide_grid(4096, 4096, 1, 9, 256)[2] == 64
    assert E.strip_grid(4096, 4096, 1, 256) == (32, 128, 32)


def test_case_table_reaches_every_situation_on_256_cus():
    """Fails when a later change of the grid rules silently un-reaches a situation."""
    E.assert_coverage(E.CU)


@pytest.mark.parametrize("k", sorted(E.SLIDE_U))
def test_unguarded_shapes_are_the_smallest(k):
    nx, ny = E.SLIDE_UNGUARDED[k]
    assert ny == 8 and E.reaches_unguarded(nx, ny, k, E.CU)
    assert "slide.unguarded_block" in E.situations(nx, ny, k, k, True, E.CU)
    # no shorter 8-column image does: every nx of the last 64 below it, and every 61st below that
    assert not any(E.reaches_unguarded(m, ny, k, E.CU) for m in list(range(nx - 64, nx)) + list(range(1, nx, 61)))


def test_small_cases_are_small():
    assert all(c.shape[0] * c.shape[1] <= 2500 for c in E.small_cases())


def test_combs_cover_the_required_positions():
    for c in E.comb_cases() + E.wrap_cases():
        nx, ny = c.shape
        k = E.entry_psf(c.psf).shape[0]
        xs = E.combs(c, E.CU)
        rows = set(np.flatnonzero(sum(x.any(axis=1) for x in xs)).tolist())
        cols = set(np.flatnonzero(sum(x.any(axis=0) for x in xs)).tolist())
        assert set(E.required_rows(c, E.CU)) <= rows and set(E.required_cols(c)) <= cols, E.case_id(c)
        assert {0, 1, 2, 3} <= {q % 4 for q in cols} or ny < 4
        corners = sum(x for x in xs)
        assert corners[0, 0] and corners[0, -1] and corners[-1, 0] and corners[-1, -1], E.case_id(c)
        if c.path == "slide":
            bands = E.slide_bands(nx, ny, 1, k, E.CU)
            U = E.SLIDE_U[k]
            for b in bands[:2]:                                  # every row phase modulo U, marching down and marching up
                want = set(range(min(U, b.i_end - b.i_begin)))
                assert want <= {(r - b.i_begin) % U for r in rows if b.i_begin <= r < b.i_end}, (E.case_id(c), b)
                assert b.i_begin in rows and b.i_end - 1 in rows
            if len(bands) > 1:
                assert not bands[0].up and bands[1].up
            for s in range(E.SPAN, ny, E.SPAN):
                assert {s - 1, s} <= cols
            assert {0, ny - 1} <= cols                           # both edge lanes


# ------------------------------------------------------------------------------------------------ emulations inside the bounds
def _inputs(c, cus=E.CU):
    nx, ny = c.shape
    d = dict(E.real_inputs(nx, ny, nx * 31 + ny))
    for q, x in enumerate(E.combs(c, cus)[:3]):
        d[f"comb{q}"] = x
    return d


def _emulate(c, psf, x, mode, tr):
    if E.case_family(c) == "general":
        return chain_fp32(x, psf[::-1, ::-1] if tr else psf, mode)
    return E.sep_fp32(x, psf, mode, tr, up_rows=E.up_rows_of(c, E.CU))


@pytest.mark.parametrize("mode", MODES)
def test_emulations_stay_inside_the_bounds(mode):
    worst = {"general": (0.0, ""), "separable": (0.0, "")}
    for c in {(c.psf, c.shape, E.case_family(c), c.path == "slide"): c for c in ALL_CASES}.values():
        nx, ny = c.shape
        psf = E.entry_psf(c.psf)
        fam = E.case_family(c)
        for tr in (False, True):
            orc = E.Oracle(psf, nx, ny, mode, tr)
            for name, x in _inputs(c).items():
                o = orc.apply(x)
                r, at, bad = E.worst_ratio(_emulate(c, psf, x, mode, tr), o, fam, *psf.shape, orc.pmax)
                assert bad == 0 and r < 1.0, (E.case_id(c), mode, tr, name, r, at, bad)
                if r > worst[fam][0]:
                    worst[fam] = (r, f"{E.case_id(c)} {name} tr={tr} at {at}")
    for fam, (r, where) in worst.items():
        print(f"emulation / bound, {mode}, {fam}: worst {r:.3f} ({where})")


# ------------------------------------------------------------------------------------------------ mutations outside the bounds
MUT_CASE = E.Case("sep9", (37, 520), "slide")


def _mut_setup(mode, tr, inp):
    c = MUT_CASE
    nx, ny = c.shape
    psf = E.entry_psf(c.psf)
    x = E.real_inputs(nx, ny, 5)[inp]
    orc = E.Oracle(psf, nx, ny, mode, tr)
    return c, psf, x, orc, orc.apply(x)


def _report(name, got, o, orc, psf):
    r, at, bad = E.worst_ratio(got, o, "separable", *psf.shape, orc.pmax)
    print(f"mutation {name}: per-entry ratio {r:.3g} at {at} (zero-pattern violations {bad}); norm-wise {relerr(got, o['y']):.2e}"
          f" -> the 1e-5 bar {'passes' if relerr(got, o['y']) < 1e-5 else 'fails'} it")
    return r, bad


@pytest.mark.parametrize("inp", ["noise", "uniform"])
def test_unmutated_reference_passes(inp):
    c, psf, x, orc, o = _mut_setup("mirror", True, inp)
    r, bad = _report("none", E.sep_fp32(x, psf, "mirror", True, up_rows=E.up_rows_of(c, E.CU)), o, orc, psf)
    assert r < 1.0 and bad == 0


def test_mutation_dropped_corner_tap():
    c, psf, x, orc, o = _mut_setup("reflect", False, "noise")
    got = E.sep_fp32(x, psf, "reflect", False, up_rows=E.up_rows_of(c, E.CU))
    wr, wc = E.sep_weights(psf, False)
    win = E._window(x, 9, 9, "reflect")
    got[0, 0] -= np.float32(np.float64(wc[8]) * np.float64(wr[8]) * win[8, 8])        # the last tap of pixel (0, 0) is never added
    r, _ = _report("one tap dropped at one corner pixel", got, o, orc, psf)
    assert r > 1.0


def test_mutation_mirror_rule_in_one_band():
    c, psf, x, orc, o = _mut_setup("mirror", False, "noise")
    up = E.up_rows_of(c, E.CU)
    got = E.sep_fp32(x, psf, "mirror", False, up_rows=up)
    win = E._window(x, 9, 9, "mirror")
    assert np.array_equal(win[4:-4, 0], x[:, 4].astype(np.float64))                    # window column 0 is image column -4 = 4
    win[:, 0] = win[:, 4]                                                              # ... reads column 0 instead
    bad = E.sep_fp32(x, psf, "mirror", False, up_rows=up, win=win)
    b = E.slide_bands(*c.shape, 1, 9, E.CU)[1]
    got[b.i_begin:b.i_end] = bad[b.i_begin:b.i_end]                                    # in one band only
    r, _ = _report("mirror rule reads column 0 for column -4 in one band", got, o, orc, psf)
    assert r > 1.0


def test_mutation_forward_weights_for_the_transpose():
    c, psf, x, orc, o = _mut_setup("reflect", True, "noise")
    got = E.sep_fp32(x, psf, "reflect", False, up_rows=E.up_rows_of(c, E.CU))          # sf where st belongs
    r, _ = _report("forward weights used for the transpose", got, o, orc, psf)
    assert r > 1.0


def test_mutation_column_weights_not_reversed_in_up_bands():
    c, psf, x, orc, o = _mut_setup("reflect", False, "noise")
    up = E.up_rows_of(c, E.CU)
    got = E.sep_fp32(x, psf, "reflect", False, up_rows=up)
    wr, wc = E.sep_weights(psf, False)
    bad = E.sep_fp32(x, psf, "reflect", False, up_rows=up, wc=wc[::-1].copy())
    got[up] = bad[up]
    r, _ = _report("column weights not reversed in up-marching bands", got, o, orc, psf)
    assert r > 1.0


@pytest.mark.parametrize("inp", ["noise", "uniform", "ramp"])
def test_mutation_every_weight_perturbed_2e_6(inp):
    c, psf, x, orc, o = _mut_setup("reflect", False, inp)
    wr, wc = E.sep_weights(psf, False)
    got = E.sep_fp32(x, psf, "reflect", False, up_rows=E.up_rows_of(c, E.CU), wr=(wr * np.float32(1 + 2e-6)).astype(np.float32))
    r, _ = _report(f"every weight off by a relative 2e-6 ({inp})", got, o, orc, psf)
    # 2e-6 |y| against (9 + 9 + 3) u S = 1.25e-6 S: outside wherever |y| > 0.63 S — everywhere on the inputs without cancellation;
    # on white noise |y| is a small part of S at most pixels, and the figure is printed only
    assert r > 1.0 or inp == "noise"


def test_mutation_store_one_column_past_the_last_strip():
    c, psf, x, orc, o = _mut_setup("reflect", False, "noise")
    nx, ny = c.shape
    got = E.sep_fp32(x, psf, "reflect", False, up_rows=E.up_rows_of(c, E.CU))
    buf = np.full(nx * ny + 128, np.float32(-7.5))                                     # 64 floats of sentinel on either side
    buf[64:-64] = got.reshape(-1)
    col = got[:, ny - 1].copy()
    for i in range(nx):                                                                # column ny of every row is written too
        buf[64 + i * ny + ny] = col[i]
    r, _ = _report("a store one column past the last strip", buf[64:-64].reshape(nx, ny), o, orc, psf)
    assert r > 1.0                                                                     # rows 1 .. nx-1: column 0 is overwritten
    assert buf[-64] != np.float32(-7.5)                                                # the last row's lands in the sentinel
