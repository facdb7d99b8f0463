"""The cases of tests/test_gpu_cgls_tiled_entrywise.py checked on the CPU (tests/cgls_tiled_cases.py): the shape table reaches every
structural situation of the tiles, the exact cases are exact (every intermediate an integer multiple of its unit below 2^24 / 2^53),
the restated blur is scipy.ndimage.convolve for every PSF side (even and rectangular ones included), the restated tile logic equals
the float64 iteration and each of the four one-line mutants of the issue changes an exact case, and the fp32 emulation of the two
passes stays inside the per-entry bound."""
import numpy as np
import pytest
from scipy.ndimage import convolve

import blur_entry_cases as B
import cgls_tiled_cases as C


def test_shape_table_reaches_every_situation():
    reached = set()
    for nx, ny in C.SHAPES:
        s = C.situations(nx, ny)
        assert s <= set(C.SITUATIONS), s - set(C.SITUATIONS)
        reached |= s
        assert nx >= 16 and ny >= 16 and C.ntiles(nx, ny) <= C.MAX_TILES
    assert reached == set(C.SITUATIONS), set(C.SITUATIONS) - reached
    for n in C.AXIS_LENGTHS:
        assert any(nx == n for nx, _ in C.SHAPES) and any(ny == n for _, ny in C.SHAPES), n
    assert {17, 19, 33, 35} <= {ny for _, ny in C.SHAPES}                 # ny that is no multiple of 4: the C ABI only
    assert any(nx >= 6 * ny for nx, ny in C.SHAPES) and any(ny >= 4 * nx for nx, ny in C.SHAPES)
    assert 12 <= len(C.SHAPES) <= 14


def test_axis_lengths_are_the_thresholds_they_are_named_for():
    f = C.axis_facts
    assert "clamped.one_tile" in f(16) and "clamped.one_tile" in f(19) and "clamped" not in f(20) and "unclamped.far" in f(20)
    assert "full_single" in f(32) and "clamped" not in f(32) and {"mirror.near", "mirror.far"} <= f(32) and "partial" not in f(32)
    for n in (33, 34, 35):
        assert "clamped.second_tile" in f(n), n
    assert "clamped" not in f(36) and "two_halos_deep" in f(40) and "interior" in f(100) and "partial" in f(100)
    assert "interior" not in f(65) and "mirror.outside" in f(65) and "mirror.outside" not in f(64) and "partial" not in f(64)
    # the clamp is what keeps the fold inside the buffer: n < (i0 + 40) / 2, and only there
    for n in range(16, 140):
        i0 = (C.ceil_div(n, C.CT) - 1) * C.CT
        assert ("clamped" in f(n)) == (2 * n < i0 + 40), n
        load = np.arange(-2 * C.CH, i0 + C.CT + 2 * C.CH)
        assert ((C.refl(load, n) >= 0) & (C.refl(load, n) < n)).all()


def test_exact_psfs_are_dyadic_asymmetric_and_rank_one():
    for kh, kw in C.PSF_SIDES:
        col, row = C.taps(kh, 0), C.taps(kw, 1)
        for w in (col, row):
            assert len(set(w.tolist())) == len(w) and 0 not in w and np.array_equal(w, np.rint(w))
            assert len(w) == 1 or not np.array_equal(w, w[::-1]) and not np.array_equal(np.abs(w), np.abs(w[::-1]))
            top = np.abs(w).max()
            assert np.log2(top) == int(np.log2(top)) and int(np.sum(np.abs(w) == top)) == 1
        if kh == kw and kh > 1:
            assert not np.array_equal(col, row) and not np.array_equal(col, row[::-1])
        psf = C.exact_psf(kh, kw)
        assert psf.shape == (kh, kw) and B.is_rank1(psf) and np.array_equal(psf * 16, np.rint(psf * 16))
        c, r = B.rank1_factors(psf)                                       # as the library forms them: still dyadic float32
        assert np.array_equal(np.outer(c, r), psf)
        for w in (c, r):
            assert np.array_equal(w.astype(np.float32).astype(np.float64), w) and C.unit_of(w) >= 2.0 ** -6
        if kh > 1 and kw > 1:
            assert not np.array_equal(psf, psf[::-1, ::-1]) and not np.array_equal(psf, psf[::-1]) and not np.array_equal(psf, psf[:, ::-1])


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "%dx%d" % s)
def test_exact_cases_are_exact(shape):
    """Every intermediate of every exact case of this shape is an integer multiple of its unit below 2^24 units (float32: row pass,
    column pass, each update, both forms, every PSF) or 2^53 (the float64 sums): the precondition of the GPU test's equalities."""
    cases = [c for c in C.shape_cases(True) if (c.nx, c.ny) == shape]
    if shape == (33, 35):
        cases += C.source_cases()
    assert cases
    worst = 0.0
    for c in cases:
        for name, (units, limit) in C.exact_margins(c).items():
            assert units < limit, (c.id, name, units, limit)
            worst = max(worst, units / limit)
        ref = C.iteration(c, C.state(c))
        for k in ("p1", "r1", "t1", "x1", "d"):
            assert ref[k].bound is None and ref[k].ref.dtype == np.float32
        assert np.count_nonzero(ref["t1"].ref) > 0.5 * c.n and np.count_nonzero(ref["r1"].ref) > 0.5 * c.n
    print(f"{shape}: largest margin {worst:.3f} of its limit over {len(cases)} cases")


def test_case_tables():
    ex, ge, src = C.shape_cases(True), C.shape_cases(False), C.source_cases()
    for cases, psfs in ((ex, C.PSF_SIDES), (ge, C.GENERAL_PSFS)):
        assert {(c.nx, c.ny) for c in cases} == set(C.SHAPES) and {c.psf for c in cases} == set(psfs)
        for form in (1, 2):
            mine = [c for c in cases if c.form == form]
            assert {c.k_first for c in mine} == {1, 2, 3} and {c.with_xt for c in mine} == {True, False}
            assert {c.keep for c in mine} == {0, 1} and {c.n_g for c in mine} == {1, 3, 64}
            for s in C.SHAPES:                                            # every shape meets every k_first in each form
                assert {c.k_first for c in mine if (c.nx, c.ny) == s} == {1, 2, 3}, (form, s)
    assert {c.n_g for c in src} == set(C.N_G) and max(C.N_G) == C.PCAP and {c.k_first for c in src} == {1, 2, 3}
    assert len({c.id for c in ex + ge + src}) == len(ex + ge + src)
    sizes = {k.shape for k in map(C.general_psf, C.GENERAL_PSFS)}
    assert {(3, 3), (5, 5), (7, 7), (9, 9)} <= sizes and any(a != b for a, b in sizes)
    asym = C.general_psf("asym7x4")
    assert B.is_rank1(asym) and not np.allclose(asym, asym[::-1, ::-1])
    for name in C.GENERAL_PSFS:
        assert B.is_rank1(C.general_psf(name)), name


@pytest.mark.parametrize("kind", ["exact", "general"])
def test_restated_blur_is_scipy_convolve(kind):
    """Oracle(psf, 'reflect') against scipy.ndimage.convolve(X, psf, mode='reflect'), and the "transpose" against the same with the
    flipped PSF — for every PSF side used, the even and rectangular ones included, on clamped, one-tile and several-tile shapes."""
    psfs = [C.exact_psf(*s) for s in C.PSF_SIDES] if kind == "exact" else [C.general_psf(n) for n in C.GENERAL_PSFS]
    for nx, ny in ((16, 16), (19, 17), (33, 35), (40, 36)):
        X = np.random.default_rng(nx * ny).standard_normal((nx, ny)).astype(np.float32)
        for psf in psfs:
            for tr in (False, True):
                o = B.Oracle(psf, nx, ny, "reflect", tr).apply(X)
                ref = convolve(X.astype(np.float64), psf[::-1, ::-1] if tr else psf, mode="reflect")
                assert np.abs(o["y"] - ref).max() <= 1e-13 * max(np.abs(ref).max(), 1.0), (psf.shape, nx, ny, tr)
                assert (o["S"] >= np.abs(o["y"]) * (1 - 1e-12)).all()


def _model_cases():
    """Every shape with three of the exact PSF sides (rotating, so that every side meets clamped and unclamped shapes), both forms."""
    out = []
    for s, (nx, ny) in enumerate(C.SHAPES):
        for j in range(3):
            side = C.PSF_SIDES[(3 * s + j) % len(C.PSF_SIDES)]
            out += [c for c in C.shape_cases(True) if (c.nx, c.ny, c.psf) == (nx, ny, side)]
    return out


def _model_differs(c, mutant):
    st = C.state(c)
    ref = C.iteration(c, st)
    p1, w, r1, t1, oob = C.tile_model(c, st, float(ref["beta"]), float(ref["alpha"]), mutant)
    same = (np.array_equal(p1.reshape(-1), ref["p1"].ref) and np.array_equal(r1.reshape(-1), ref["r1"].ref)
            and np.array_equal(t1.reshape(-1), ref["t1"].ref) and np.array_equal(C.tile_sums(w * w, c.nx, c.ny), ref["PD"].ref))
    if c.form == 2:
        same = same and np.array_equal(w.reshape(-1), ref["w1"].ref)
    return not same, oob


def test_tile_logic_restated_equals_the_float64_iteration():
    """The kernels' index logic (tiled_geom's centred taps and anchors, the clamped fold, the halo loads, the mirror fill, tile
    ownership) restated tile by tile gives, on the exact cases, exactly the Oracle-based iteration: two independent statements."""
    cases = _model_cases()
    assert {c.psf for c in cases} == set(C.PSF_SIDES) and {(c.nx, c.ny) for c in cases} == set(C.SHAPES)
    for c in cases:
        differs, oob = _model_differs(c, None)
        assert not differs and not oob, c.id


@pytest.mark.parametrize("mutant", C.MUTANTS)
def test_each_mutant_changes_an_exact_case(mutant):
    """The four one-line mutants of the kernels' index logic, applied to the restated tile logic: each turns exact cases red.
    rwf / rwt swapped and the anchor of an even kh shifted by one change entries (asymmetric PSFs); a fold at n - 2 without the clamp
    changes entries on every shape and leaves the buffer on the clamped ones (the kernel would read out of bounds: never run); a
    mirror fill that keeps W[r][c] changes t' along the image's edges."""
    cases = _model_cases()
    red = [c for c in cases if _model_differs(c, mutant)[0]]
    assert red, mutant
    print(f"{mutant}: {len(red)} of {len(cases)} exact cases change")
    if mutant == "anchor_even_kh":
        assert {c.psf for c in red} == {(2, 2), (4, 6), (8, 8)} and len(red) == len([c for c in cases if c.psf[0] % 2 == 0])
    elif mutant == "swap_rwf_rwt":
        assert len(red) == len([c for c in cases if c.psf[1] > 1])          # every PSF with more than one row tap
    elif mutant == "fold_at_n_minus_2":
        for c in cases:
            clamped = "clamped" in C.axis_facts(c.nx) or "clamped" in C.axis_facts(c.ny)
            if clamped and c.form == 1:                                     # K_B's loads on tile + 8 leave the buffer there
                assert _model_differs(c, mutant)[1], c.id
        assert any(not _model_differs(c, mutant)[1] for c in red)           # and entries change where every index stays inside
    else:
        assert len(red) == len([c for c in cases if max(c.psf) > 1])


def test_fp32_emulation_stays_inside_the_bound():
    """blur_entry_cases.sep_fp32 — the two fp32 passes of blur_lds, taps ascending, an fp32 store between them — on normals: the
    fraction of the separable bound it reaches (information; the bound is the arithmetic of the module docstring)."""
    got = {}
    for name in C.GENERAL_PSFS:
        for tr in (False, True):
            got[(name, tr)] = C.emulated_fraction(name, 35, 33, tr)
            assert 0 < got[(name, tr)] < 1, (name, tr, got[(name, tr)])
    print({k: round(v, 3) for k, v in got.items()})
