"""One iteration of the tiled small-image CGLS against its float64 restatement, entry by entry (tests/cgls_tiled_cases.py holds the
cases, the references and the bounds; tests/test_cgls_tiled_cases_host.py proves them on the CPU).

Every case is ONE call with n_iters = 1 on a CRAFTED state — nothing comes from a previous solve — on a handle made by
trk_blur2d_create, so the shapes the Python driver never offers (even and rectangular PSF sides, ny no multiple of 4) are reached.

  entry point               kernel<template arguments>        reached by
  trk_cgls_iterate_tiled    k_cgls_tile_a                     form 1 cases: every shape x every PSF, k_first 1 (first) / 2 / 3
                            k_cgls_tile_b<true>               form 1 cases with x_true
                            k_cgls_tile_b<false>              form 1 cases without (NP[3 i + 2] == 0)
  trk_cgls_iterate_tiled2   k_cgls_tile_a2                    form 2 cases (p and w NaN at k_first = 1: not read)
                            k_cgls_tile_b2<true> / <false>    form 2 cases with / without x_true
  both                      k_finalize (core.hip)             n_g = 1025, 2048, 4096: the gamma partials are summed before the first K_A
  trk_cgls_tiled_caps       -                                 the refusals; every case asserts *can == 1 first

What is checked, per case:
  buffers     every buffer lies between guard elements that must survive; outputs start as NaN (a skipped store shows); p_ld, r_ld,
              x_ld exceed n and the pads stay untouched; the halves of P, R and X the iteration only reads, x_true and (form 1) nothing
              else changes; PG beyond n_g is NaN going in; PG, PD, NP beyond the tile count and NP's rows of other iterations stay
  scalars     S[gpub] (S[0], S[6], S[11] for k_first = 1, 2, 3) is the sum of the gamma partials handed in — EQUAL to it for exactly
              summing partials —, S[5 k] is within ntiles 2^-52 of the float64 sum of the device's own PD, every other slot of S is
              unchanged; *n_g_inout and *n_np_inout come back as the tile count
  exact       p', w' (form 2), r', t', x' EQUAL the reference (np.array_equal), PD, PG, NP per tile too
  general     p', x' and form 2's r' (given the device's w') are bit for bit the correctly rounded fused operation (vec_cases.fma32
              decides rounding ties exactly, so no entry is left out); blurred stages stay within the per-entry bound of
              cgls_tiled_cases (no entry left out; where the bound is 0 the result must be 0); PD, PG, NP within their bounds;
              the worst error / bound of each stage goes through conftest.bar (profiles/cgls_tiled/bars.txt)
  repeat      every case runs twice from the same state: identical bits in every buffer (no atomics)
Failure messages name (row, column, tile).

The x update: the kernels' `x + alpha * p` is compiled contracted, x' = fmaf(alpha, p', x) — the one-rounding update of the streaming
forms (trk.h) —, while ||x' - x||^2 is measured on d = (float)(alpha p').  The reference follows: x' = fma32(alpha, p', x), not the
twice-rounded fl(x + d); on general operands the two differ in a share of the entries, which test_general_iteration counts.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import blur_entry_cases as B
import cgls_tiled_cases as C
import vec_cases as V
from conftest import bar

pytestmark = pytest.mark.gpu

GUARD = 64
SENT32, SENT64 = -12345.5, -98765.25
PAD = 13                                   # p_ld = r_ld = x_ld = n + 13: the second half of a pair is not 16-byte aligned
EINVAL, EUNSUPPORTED = -1, -4
NEEDS = "needs a reflect-boundary separable blur <= 9x9 on an image >= 16x16"


@pytest.fixture(scope="module")
def eng():
    from trips_py_amd.engine import default_engine
    return default_engine()


@pytest.fixture(scope="module")
def cus(eng):
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


def make_blur(eng, psf, nx, ny, boundary=None):
    from trips_py_amd.operators import _HandleOperator
    arr = np.ascontiguousarray(psf, dtype=np.float64)
    h = ctypes.c_void_p()
    p = arr.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    if boundary is None:
        rc = eng.lib.trk_blur2d_create(p, arr.shape[0], arr.shape[1], nx, ny, ctypes.byref(h))
    else:
        rc = eng.lib.trk_blur2d_create_bc(p, arr.shape[0], arr.shape[1], nx, ny, boundary, ctypes.byref(h))
    assert rc == 0, eng.lib.trk_last_error()
    return _HandleOperator(h, eng)


class Buf:
    """`count` elements between two guards of GUARD sentinels; `v` is the payload view."""

    def __init__(self, eng, count, dtype=torch.float32, fill=float("nan")):
        self.full = torch.full((count + 2 * GUARD,), SENT32 if dtype == torch.float32 else SENT64, dtype=dtype, device=eng.device)
        self.v = self.full[GUARD:GUARD + count]
        self.v.fill_(fill)

    def put(self, lo, a):
        a = np.asarray(a)
        self.v[lo:lo + a.size] = torch.from_numpy(np.ascontiguousarray(a)).to(self.v.device, self.v.dtype)

    def host(self):
        return self.full.cpu().numpy()

    def rows(self, k, ld):
        return self.v.view(k, ld)


def bits(a):
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def same_bits(a, b):
    return np.array_equal(bits(np.ascontiguousarray(a)), bits(np.ascontiguousarray(b)))


def layout(case):
    k, n = case.k_first, case.n
    ld = n + PAD
    xrows = k if case.keep else 2
    x_new = (k - 1) if case.keep else ((k - 1) & 1)
    x_prev = None if (case.keep and k == 1) else ((k - 2) if case.keep else (k & 1))      # None: a buffer of its own
    nt = C.ntiles(case.nx, case.ny)
    return dict(ld=ld, xrows=xrows, x_new=x_new, x_prev=x_prev, old=(k - 1) & 1, new=k & 1, nt=nt, np_cap=nt + 3,
                gprev=0 if k <= 2 else 5 * (k - 2) + 1, gpub=0 if k == 1 else 5 * k - 4, dpub=5 * k, ns=5 * k + 8)


def setup(eng, case, st):
    L, n, f1 = layout(case), case.n, case.form == 1
    nan = np.float32("nan")
    b = {}
    if f1:
        b["P"] = Buf(eng, 2 * L["ld"], fill=SENT32)
        b["P"].put(L["old"] * L["ld"], st["p"])
        b["P"].put(L["new"] * L["ld"], np.full(n, nan))
    else:
        for name in ("p", "w"):
            b[name] = Buf(eng, n)
            if not case.first:
                b[name].put(0, st[name])
    b["R"] = Buf(eng, 2 * L["ld"], fill=SENT32)
    b["R"].put(L["old"] * L["ld"], st["r"])
    b["R"].put(L["new"] * L["ld"], np.full(n, nan))
    b["t"] = Buf(eng, n)
    b["t"].put(0, st["t"])
    b["X"] = Buf(eng, L["xrows"] * L["ld"], fill=SENT32)
    for r in range(L["xrows"]):
        b["X"].put(r * L["ld"], st["x"] if r == L["x_prev"] else np.full(n, nan))
    if L["x_prev"] is None:
        b["xp"] = Buf(eng, n)
        b["xp"].put(0, st["x"])
    if st["xt"] is not None:
        b["xt"] = Buf(eng, n)
        b["xt"].put(0, st["xt"])
    b["S"] = Buf(eng, L["ns"], torch.float64, 0.0)
    b["S"].put(0, 1000.0 + np.arange(L["ns"]))
    if not case.first:
        b["S"].put(L["gprev"], [st["gprev"]])
    b["PG"] = Buf(eng, C.PCAP, torch.float64)
    b["PG"].put(0, st["pg"])
    b["PD"] = Buf(eng, C.PCAP, torch.float64)
    b["NP"] = Buf(eng, 3 * L["np_cap"] * case.k_first, torch.float64)
    return b


def launch(eng, A, case, b):
    L = layout(case)
    X = b["X"].rows(L["xrows"], L["ld"])
    xp = b["xp"].v if L["x_prev"] is None else X[L["x_prev"]]
    xt = b["xt"].v if "xt" in b else None
    R = b["R"].rows(2, L["ld"])
    args = (X, case.keep, xp, xt, b["S"].v, b["PG"].v, b["PD"].v, C.PCAP, b["NP"].v, L["np_cap"], case.n_g, 0)
    if case.form == 1:
        out = eng.cgls_iterate_tiled(A._h, case.k_first, 1, b["P"].rows(2, L["ld"]), R, b["t"].v, *args)
    else:
        out = eng.cgls_iterate_tiled2(A._h, case.k_first, 1, b["p"].v, b["w"].v, R, b["t"].v, *args)
    eng.synchronize()
    return out


def run_case(eng, case, A=None):
    """Run the case twice from its crafted state; check everything structural; return (state, device outputs by stage)."""
    st = C.state(case)
    A = A or make_blur(eng, C.psf_of(case), case.nx, case.ny)
    assert eng.cgls_tiled_caps(A._h, C.ntiles(case.nx, case.ny), C.PCAP), case.id
    L, n, nt = layout(case), case.n, C.ntiles(case.nx, case.ny)
    b0 = setup(eng, case, st)
    before = {k: v.host() for k, v in b0.items()}
    snaps = []
    for b in (b0, setup(eng, case, st)):
        assert launch(eng, A, case, b) == (nt, nt), case.id
        snaps.append({k: v.host() for k, v in b.items()})
    for k in snaps[0]:
        assert same_bits(snaps[0][k], snaps[1][k]), (case.id, k, "two identical calls differ")
    after = snaps[0]
    G = GUARD
    for k, a in after.items():                                             # the guards
        assert same_bits(a[:G], before[k][:G]) and same_bits(a[-G:], before[k][-G:]), (case.id, k, "guard overwritten")
    pay = {k: a[G:-G] for k, a in after.items()}
    was = {k: a[G:-G] for k, a in before.items()}
    ld = L["ld"]

    def pair(name, new_row, rows):
        """The written row's first n entries; everything else of the buffer must be as before (pads, the row only read)."""
        mask = np.ones(rows * ld, dtype=bool)
        mask[new_row * ld:new_row * ld + n] = False
        assert same_bits(pay[name][mask], was[name][mask]), (case.id, name, "changed outside the row written")
        return pay[name][new_row * ld:new_row * ld + n].copy()

    dev = {}
    if case.form == 1:
        dev["p1"] = pair("P", L["new"], 2)
    else:
        dev["p1"], dev["w1"] = pay["p"].copy(), pay["w"].copy()
    dev["r1"] = pair("R", L["new"], 2)
    dev["x1"] = pair("X", L["x_new"], L["xrows"])
    dev["t1"] = pay["t"].copy()
    for name in ("xp", "xt"):
        if name in pay:
            assert same_bits(pay[name], was[name]), (case.id, name)
    for name, a in dev.items():
        assert np.isfinite(a).all(), (case.id, name, "an entry was not stored", C.where(int(np.flatnonzero(~np.isfinite(a))[0]), case.ny))
    dev["PD"], dev["PG"] = pay["PD"][:nt].copy(), pay["PG"][:nt].copy()
    assert same_bits(pay["PD"][nt:], was["PD"][nt:]) and same_bits(pay["PG"][nt:], was["PG"][nt:]), (case.id, "PD / PG beyond the tiles")
    lo = 3 * nt * (case.k_first - 1)
    dev["NP"] = pay["NP"][lo:lo + 3 * nt].copy()
    mask = np.ones(pay["NP"].size, dtype=bool)
    mask[lo:lo + 3 * nt] = False
    assert same_bits(pay["NP"][mask], was["NP"][mask]), (case.id, "NP outside this iteration's rows")
    assert np.isfinite(dev["PD"]).all() and np.isfinite(dev["PG"]).all() and np.isfinite(dev["NP"]).all(), case.id
    if st["xt"] is None:
        assert (dev["NP"][2::3] == 0.0).all(), case.id
    S, S0 = pay["S"], was["S"]
    mask = np.ones(S.size, dtype=bool)
    mask[[L["gpub"], L["dpub"]]] = False
    assert same_bits(S[mask], S0[mask]), (case.id, "a slot of S beside the two published ones changed", np.flatnonzero(bits(S) != bits(S0)))
    dev["gamma"], dev["delta"] = float(S[L["gpub"]]), float(S[L["dpub"]])
    delta = math.fsum(dev["PD"])
    assert abs(dev["delta"] - delta) <= nt * 2.0 ** -52 * abs(delta), (case.id, dev["delta"], delta)
    return st, dev


def check_equal(case, name, got, ref):
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    if np.array_equal(got, ref):
        return
    bad = np.flatnonzero(got != ref)
    at = int(bad[0])
    if got.size == case.n:
        loc = C.where(at, case.ny)
    else:
        loc = f"(tile {at // (got.size // C.ntiles(case.nx, case.ny))})"
    ulps = f", worst {float(np.max(V.ulps32(got[bad], ref[bad]))):.3g} ulp" if got.dtype == np.float32 and np.all(ref[bad] != 0) else ""
    raise AssertionError(f"{case.id}: {name} differs in {bad.size} of {got.size} entries{ulps}, first at {loc}: "
                         f"got {got[at]!r}, want {ref[at]!r}")


def check_exact(case, st, dev):
    ref = C.iteration(case, st)
    assert dev["gamma"] == ref["gamma"], (case.id, dev["gamma"], ref["gamma"])
    for name in ("p1", "w1", "r1", "t1", "x1", "PD", "PG", "NP"):
        if name in ref:
            check_equal(case, name, dev[name], ref[name].ref)
    assert dev["delta"] == ref["delta"].ref, case.id


def exact_cases(pred):
    return [c for c in C.shape_cases(True) if pred(c)]


# ------------------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "%dx%d" % s)
def test_exact_iteration(eng, shape, form):
    """Dyadic asymmetric rank-1 PSFs of every side (3, 5, 7, 9 square; 1 x 9, 9 x 1, 3 x 9, 2 x 2, 4 x 6, 8 x 8), integer vectors,
    beta = 1/2, alpha = 1/4: every vector and every per-tile partial EQUALS the float64 reference."""
    cases = exact_cases(lambda c: (c.nx, c.ny) == shape and c.form == form)
    assert {c.psf for c in cases} == set(C.PSF_SIDES)
    for case in cases:
        st, dev = run_case(eng, case)
        check_exact(case, st, dev)


# ------------------------------------------------------------------------------------------------------------ gamma sources
@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("n_g", C.N_G)
def test_gamma_sources(eng, n_g, form):
    """n_g gamma partials handed in (1, 3, 64, 65, 1024, and 1025, 2048, 4096 = pcap, which are summed by the finalize kernel before the
    first K_A), k_first = 1, 2, 3 (gprev / gpub = - / S[0], S[0] / S[6], S[6] / S[11]): the published gamma EQUALS the exact total, beta and
    alpha are the powers of two the case was built for (every vector equals the reference), the neighbouring slots of S stay."""
    cases = [c for c in C.source_cases() if c.n_g == n_g and c.form == form]
    assert [c.k_first for c in cases] == [1, 2, 3]
    A = make_blur(eng, C.psf_of(cases[0]), cases[0].nx, cases[0].ny)
    for case in cases:
        st, dev = run_case(eng, case, A)
        assert len(st["pg"]) == n_g and dev["gamma"] == float(np.sum(st["pg"])), (case.id, dev["gamma"], float(np.sum(st["pg"])))
        check_exact(case, st, dev)


# ------------------------------------------------------------------------------------------------------------ general
@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("psf", C.GENERAL_PSFS)
def test_general_iteration(eng, psf, form):
    """Real PSFs (Gaussians of 3, 5, 7, 9 taps, a rectangular spread, an asymmetric rank-1 PSF), standard-normal vectors, on every
    shape: the unblurred updates bit for bit, the blurred stages and the per-tile sums within the bounds of cgls_tiled_cases, each
    evaluated on the device's own earlier outputs."""
    cases = [c for c in C.shape_cases(False) if c.psf == psf and c.form == form]
    assert {(c.nx, c.ny) for c in cases} == set(C.SHAPES)
    worst, twice, total = {}, 0, 0
    for case in cases:
        st, dev = run_case(eng, case)
        ref = C.iteration(case, st, dev)
        g = ref["gamma"]
        assert abs(dev["gamma"] - g) <= case.n_g * 2.0 ** -52 * abs(g), (case.id, dev["gamma"], g)
        check_equal(case, "p1", dev["p1"], ref["p1"].ref)
        check_equal(case, "x1", dev["x1"], ref["x1"].ref)
        two = st["x"] + ref["d"].ref                                        # the twice-rounded update: NOT what the kernels compute
        twice, total = twice + int(np.count_nonzero(two != dev["x1"])), total + case.n
        if form == 2:
            check_equal(case, "r1", dev["r1"], ref["r1"].ref)
        for name in ("w1", "r1", "t1", "PD", "PG", "NP"):
            if name in ref and ref[name].bound is not None:
                ratio, at, bad_zero = C.worst(dev[name], ref[name], case.nx, case.ny)
                print(f"{case.id} {name}: {ratio:.3f} of the bound")
                loc = C.where(at, case.ny) if np.size(ref[name].ref) == case.n else f"(slot {at})"
                assert bad_zero == 0, (case.id, name, "not 0 where the bound is 0")
                assert ratio < 1.0, (case.id, name, ratio, loc)
                worst[name] = max(worst.get(name, 0.0), ratio)
    print(f"x' differs from the twice-rounded fl(x + fl(alpha p)) in {twice} of {total} entries")
    for name, ratio in sorted(worst.items()):
        bar(f"cgls_tiled.form{form}.{psf}.{name}", ratio, 1.0)


# ------------------------------------------------------------------------------------------------------------ refusals
def _call(eng, form, A, n, k_first=1, pcap=C.PCAP, np_cap=4096, n_g=1):
    """One call with real-size buffers (NaN outputs); returns (rc, error text, whether any buffer changed)."""
    f = lambda k=1: torch.full((k, n + 4), float("nan"), device=eng.device)                # noqa: E731
    P, R, X, t, p, w, xp = f(2), f(2), f(2), f()[0], f()[0], f()[0], torch.zeros(n, device=eng.device)
    D = [torch.full((c,), float("nan"), dtype=torch.float64, device=eng.device) for c in (64, max(pcap, 1), max(pcap, 1), 3 * max(np_cap, 1))]
    S, PG, PD, NP = D
    cg, cn = ctypes.c_int(n_g), ctypes.c_int(0)
    tail = (X.data_ptr(), X.stride(0), 0, xp.data_ptr(), None, S.data_ptr(), PG.data_ptr(), PD.data_ptr(), pcap, NP.data_ptr(), np_cap,
            ctypes.byref(cg), ctypes.byref(cn), eng.stream())
    if form == 1:
        rc = eng.lib.trk_cgls_iterate_tiled(A._h, k_first, 1, P.data_ptr(), P.stride(0), R.data_ptr(), R.stride(0), t.data_ptr(), *tail)
    else:
        rc = eng.lib.trk_cgls_iterate_tiled2(A._h, k_first, 1, p.data_ptr(), w.data_ptr(), R.data_ptr(), R.stride(0), t.data_ptr(), *tail)
    msg = eng.lib.trk_last_error().decode() if rc else ""
    eng.synchronize()
    touched = any(bool((~torch.isnan(v)).any()) for v in (P, R, X, t, p, w, S, PG, PD, NP))
    return rc, msg, touched


def _caps(eng, A, np_cap=4096, pcap=C.PCAP):
    can = ctypes.c_int(7)
    assert eng.lib.trk_cgls_tiled_caps(A._h, np_cap, pcap, ctypes.byref(can)) == 0
    return can.value


def test_refusals_before_any_launch(eng):
    """What the tiled forms do not serve is refused by both entry points with *can == 0 and TRK_EUNSUPPORTED and its text, before
    anything is launched (every buffer still NaN): an axis of 15, a 10-tap side, a boundary mode other than reflect, a handle forced
    to the LDS tile path, a rank-2 PSF, more than 1024 tiles.  Tile counts above pcap or np_capacity_blocks, and more gamma partials
    than pcap, are TRK_EINVAL."""
    rng = np.random.default_rng(5)
    g3 = C.general_psf("g3")
    col10 = np.outer(np.linspace(1.0, 2.0, 10), [1.0, 2.0, 1.0]) / 60.0
    forced = make_blur(eng, g3, 32, 32)
    assert eng.lib.trk_blur2d_set_path(forced._h, 3) == 0                  # TRK_BLUR_PATH_TILE, before the handle is ever asked
    unsupported = [("nx = 15", make_blur(eng, g3, 15, 32), 15 * 32), ("ny = 15", make_blur(eng, g3, 32, 15), 32 * 15),
                   ("10 x 3", make_blur(eng, col10, 32, 32), 1024), ("3 x 10", make_blur(eng, col10.T.copy(), 32, 32), 1024),
                   ("constant boundary", make_blur(eng, g3, 32, 32, boundary=1), 1024), ("forced tile path", forced, 1024),
                   ("rank 2", make_blur(eng, rng.random((3, 3)), 32, 32), 1024)]
    for what, A, n in unsupported:
        assert _caps(eng, A) == 0, what
        for form in (1, 2):
            rc, msg, touched = _call(eng, form, A, n)
            assert rc == EUNSUPPORTED and NEEDS in msg and not touched, (what, form, rc, msg, touched)
    A = make_blur(eng, g3, 33, 35)                                          # four tiles
    assert _caps(eng, A, 4, 4) == 1 and _caps(eng, A, 3, 4) == 0 and _caps(eng, A, 4, 3) == 0
    for form in (1, 2):
        for kw in (dict(pcap=3), dict(np_cap=3)):
            rc, msg, touched = _call(eng, form, A, 33 * 35, **kw)
            assert rc == EINVAL and "4 tiles exceed the partial buffers" in msg and not touched, (form, kw, rc, msg)
        rc, msg, touched = _call(eng, form, A, 33 * 35, pcap=8, n_g=9)
        assert rc == EINVAL and "9 gamma partials exceed" in msg and not touched, (form, rc, msg)
    big = make_blur(eng, g3, 1100, 1100)                                    # 35 x 35 = 1225 tiles
    assert _caps(eng, big, 4096, 4096) == 0
    for form in (1, 2):
        rc, msg, touched = _call(eng, form, big, 1100 * 1100)
        assert rc == EUNSUPPORTED and "1225 tiles, at most 1024" in msg and not touched, (form, rc, msg, touched)


# ------------------------------------------------------------------------------------------------------------ the product path
def _tall_shape(nx, ny, cus):
    """(nx, ny) itself if the sliding blur leaves more than 1024 gamma partials for it on this device, else the first taller image of
    the same width that does (restated dispatch: blur_entry_cases.slide_grid) and that the tiled forms still serve."""
    while True:
        sx, nb, _ = B.slide_grid(nx, ny, 1, 3, cus)
        if sx * nb > C.PMAX_PARTIALS:
            assert C.ntiles(nx, ny) <= C.MAX_TILES and nx * ny <= 1 << 20, (nx, ny, cus)
            return nx, ny, sx * nb
        nx += 4


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("nx,ny", [(4100, 16), (8192, 128)])
def test_tall_images_whose_first_gamma_has_more_than_1024_partials(eng, cus, nx, ny, form):
    """CGLS() on tall images under a 3 x 3 Gaussian: the streaming blur's t_0 = A^T r_0 leaves more than 1024 gamma partials (1025 and
    2048 on 256 CUs), which the first tiled iteration must sum completely.  Against the four-launch streaming form to 2e-6 per iterate,
    as test_tiled_two_launch_cgls_equals_the_streaming_form."""
    from trips_py_amd.operators import Blur2D
    from trips_py_amd.problems import gauss_psf
    from trips_py_amd.solvers import CGLS
    from trips_py_amd.solvers.CGLS import CGLSRunFused
    nx, ny, want = _tall_shape(nx, ny, cus)
    A = Blur2D(gauss_psf((3, 3), (1, 1))[0], nx, ny)
    assert CGLSRunFused.tiled_usable(A, A.engine)
    dev, n = A.engine.device, nx * ny
    xt = torch.rand(n, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    b = A.apply(xt)
    b = b + 0.01 * torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(8)) * b.norm() / n ** 0.5
    x0 = torch.zeros(n, device=dev)
    run = CGLSRunFused(A, b, x0, 5, xt, True, tiled=form)
    assert run.n_g == want > C.PMAX_PARTIALS, (run.n_g, want)
    xa, ia = CGLS(A, b, x0, 5, 0, xt, tiled=False, fused=False)
    xb, ib = CGLS(A, b, x0, 5, 0, xt, tiled=form)
    for k in range(5):
        ra, rb = ia["xHistory"][k].reshape(-1), ib["xHistory"][k].reshape(-1)
        assert float(torch.linalg.norm(ra - rb) / torch.linalg.norm(ra)) < 2e-6, k
