"""The 2-D blur against float64, entry by entry, on every kernel path, boundary mode and direction (csrc/blur2d.hip: k_blur_slide,
k_blur_strip separable and direct, k_blur_generic; csrc/blur_tile.hip: k_blur_tile, k_blur_tile_sep).  Oracle, dispatch restatement,
case table, combs and emulations: tests/blur_entry_cases.py, checked on the CPU by tests/test_blur_entry_cases_host.py.

Bounds (u = 2^-24; x is fp32 and exact; A, S = |A||x| — every tap's magnitude times every sample's — and T_i = the number of non-zero
products of output i come from the float64 oracle).  Derived from the kernels' code, never fitted to their output:

  general family (k_blur_strip<SEP = false>, k_blur_tile, k_blur_generic).  A tap is (float)psf[a][b]: one rounding, relative u.  An
    output is ONE fmaf chain from 0.f over the taps; a step whose product is 0 (a zero sample, constant mode's padding) leaves the
    sum as it is, the other T_i steps round once each, so the computed sum is  sum_t c_t x_t (1 + d_t)  with |1 + d_t| <= (1 + u)^(T_i + 1):
        |y_i - (A x)_i| <= (T_i + 1) u S_i + O(u^2)  <=  (T_i + 2) u S_i          (T_i <= 64 * 64: the second-order part is < u / 2)

  separable family (k_blur_slide, k_blur_strip<SEP = true>, k_blur_tile_sep).  psf = col row^T (the library's pivot factorisation, in
    double); a tap is the product of (float)row[b] and (float)col[a]: two roundings.  The row pass is one fmaf chain per staged row with at
    most min(T_i, kw) non-zero products, the column pass one chain (fmaf in the strip and tile kernels; `w * h + acc` on float2 in the
    sliding kernel, which hipcc contracts to v_pk_fma_f32: one rounding) over at most min(T_i, kh) non-zero row results:
        |y_i - (A x)_i| <= (min(T_i, kw) + min(T_i, kh) + 2) u S_i + O(u^2)  <=  (min(T_i, kw) + min(T_i, kh) + 3) u S_i
    plus 1e-12 max|psf| sum_j pattern_ij |x_j|, because the library takes a PSF for rank-1 when |psf - col row^T| <= 1e-12 max|psf|
    and the oracle convolves with col row^T.

  zero pattern: where S_i = 0 no product is non-zero and the output is exactly 0 (every chain starts from 0.f).

Each bound has one u to spare, for the second-order terms.  The order of a chain does not enter: bands of the sliding kernel that
march upward add the same column terms in descending row order, and which multiply of a step the compiler fuses does not either.

Bit-equal pairs (asserted bit for bit on the unit combs), from the code:
  * k_blur_strip direct == k_blur_tile == k_blur_generic, every entry, any input: all three run the one chain from 0.f with PSF rows
    ascending outside and columns ascending inside (k_blur_generic skips constant mode's zero rows, whose steps change nothing).
  * k_blur_strip separable == k_blur_tile_sep, every entry: the same row chain (taps ascending from 0.f), the same column chain
    (rows ascending, the first step fmaf(w, h, 0.f) = w * h).
  * k_blur_slide == k_blur_strip separable == k_blur_tile_sep wherever the column chain has at most one non-zero term (Tc <= 1).  The
    row chains are fmaf calls in all three and agree for any T.  The sliding kernel writes its column steps as `w * h + acc` on float2
    and leaves the contraction to the compiler, which fuses either multiply of `w1 * h1 + w0 * h0` (hipcc 7.2 forms
    fma(w0, h0, fl(w1 * h1)) where the strip kernel's fmaf calls form fma(w1, h1, fl(w0 * h0)): measured, one fp32 ulp apart under
    reflect, nearest and wrap, where a border row is read twice), and bands that march upward add the terms in descending row order:
    with two or more terms the bits may differ, the number of roundings — the bound — does not.
  * a batch of three == three single applies, entry for entry, on the strip, tile and generic kernels (the grid changes, the chains do
    not); on the sliding kernel the batch changes the band heights and with them the marching direction of a row: where Tc <= 1.
  * across the two families nothing is bit-equal: a separable entry is fl(fl(col) fl(row) x) with two roundings, a general one fl(fl(psf) x).
  * the flipped-PSF "transpose" of an odd PSF under constant and wrap on an image larger than the PSF is the forward matrix
    transposed, bit for bit: entry (i, j) is one product of the same fp32 factors in both (one tap, or the same row and column weight).

Every output buffer has 64 floats of sentinel on either side (and in the gap a leading dimension leaves) that must be intact
afterwards, and is pre-filled with NaN.  Figures measured on the MI355X: profiles/blur_entrywise/bars.txt (worst ratio to the bound per
case, mode and direction)."""
import functools

import numpy as np
import pytest
import torch

import blur_entry_cases as E
from blur_psf_cases import MODES
from conftest import bar, relerr

pytestmark = pytest.mark.gpu

SENT, PAD = -7.5, 64
SMALL, COMB, WRAP = E.small_cases(), E.comb_cases(), E.wrap_cases()


@functools.lru_cache(maxsize=None)
def _cus():
    from trips_py_amd.engine import default_engine
    return int(torch.cuda.get_device_properties(default_engine().device).multi_processor_count)


def _op(c, mode, force=None):
    from trips_py_amd.operators import Blur2D
    A = Blur2D(E.entry_psf(c.psf), c.shape[0], c.shape[1], boundary=mode)
    assert A.path == E.planned_path(c), (E.case_id(c), A.path)
    if force:
        A.set_path(force)
        assert A.path == force
    return A


def _apply(A, xs, tr, offset=0, ld=None):
    """A (or its "transpose") on the fp32 images xs: one vector (ld None; `offset` floats off 16-byte alignment for operand and
    output) or a batch at leading dimension ld.  The output sits between sentinels and starts as NaN; returns float32 arrays."""
    dev = A.engine.device
    xs = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in xs]
    n, k = xs[0].size, len(xs)
    if ld is None:
        assert k == 1
        ld = n
    xb = torch.zeros(PAD + offset + k * ld + PAD, dtype=torch.float32, device=dev)
    yb = torch.full((PAD + offset + k * ld + PAD,), SENT, dtype=torch.float32, device=dev)
    lo = PAD + offset
    xv = xb[lo:lo + k * ld].view(k, ld)[:, :n]
    yv = yb[lo:lo + k * ld].view(k, ld)[:, :n]
    xv.copy_(torch.from_numpy(np.stack(xs)).to(dev))
    yv.fill_(float("nan"))
    assert (xv.data_ptr() % 16 == 0) == (offset % 4 == 0)
    if k == 1:
        A.apply(xv[0], out=yv[0], transpose=tr)
    else:
        A.apply(xv, out=yv, transpose=tr)
    torch.cuda.synchronize()
    full = yb.cpu().numpy()
    assert np.all(full[:lo] == SENT) and np.all(full[lo + k * ld:] == SENT), "a store outside the output buffer"
    body = full[lo:lo + k * ld].reshape(k, ld)
    assert np.all(body[:, n:] == SENT), "a store into the leading dimension's gap"
    out = body[:, :n]
    assert not np.isnan(out).any(), "an output entry was never written"
    return [np.array(o) for o in out]


def _locate(c, at, mode, tr):
    """Where an entry sits: pixel, and on the sliding kernel band, marching direction, span and lane."""
    i, j = at
    s = f"{E.case_id(c)} {mode} {'transpose' if tr else 'forward'} pixel ({i}, {j})"
    if c.path == "slide":
        k = E.entry_psf(c.psf).shape[0]
        for q, b in enumerate(E.slide_bands(c.shape[0], c.shape[1], 1, k, _cus())):
            if b.i_begin <= i < b.i_end:
                s += f" band {q} rows [{b.i_begin}, {b.i_end}) {'up' if b.up else 'down'} span {j // 256} lane {(j % 256) // 4}"
    return s


def _ratio(c, got, o, orc, fam, mode, tr, what):
    r, at, bad = E.worst_ratio(got, o, fam, orc.kh, orc.kw, orc.pmax)
    assert bad == 0, f"{what}: {bad} entries are not exactly 0 where no tap reaches; {_locate(c, at, mode, tr)}"
    assert r < 1.0, f"{what}: {r:.3f} of the bound at {_locate(c, at, mode, tr)}"
    return r


def _own(c):
    """(offset, forced path) of the case's own apply."""
    return (1 if c.path == "strip_view" else 0), None


def _fam(c, kernel):
    sep = E.is_rank1(E.entry_psf(c.psf))
    return "separable" if sep and kernel != "generic" else "general"


# ------------------------------------------------------------------------------------------------ coverage with the device's CUs
def test_case_table_reaches_every_situation_on_this_device():
    E.assert_coverage(_cus())


# ------------------------------------------------------------------------------------------------ (A) + (C) every entry
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", SMALL, ids=E.case_id)
def test_every_entry_of_the_matrix(c, mode):
    """(A) The operator applied to the identity, in batches of columns, against the oracle's explicit matrix: every entry inside the
    bound, exactly 0 where the oracle has no entry.  (C) For an odd PSF under constant / wrap on an image larger than the PSF the
    "transpose" matrix is the forward matrix transposed, bit for bit."""
    nx, ny = c.shape
    n = nx * ny
    psf = E.entry_psf(c.psf)
    kh, kw = psf.shape
    A = _op(c, mode)
    fam = _fam(c, c.path)
    # the sliding kernel takes a batch at a leading dimension that is a multiple of 4; any other sends a slide shape to the strip kernel
    ld = (n + 3) // 4 * 4 + 4 if c.path == "slide" else n + 5 - n % 4
    eye = np.eye(n, dtype=np.float32)
    mats = {}
    for tr in (False, True):
        cols = []
        for k0 in range(0, n, 500):
            cols += _apply(A, list(eye[k0:k0 + 500]), tr, ld=ld) if min(500, n - k0) > 1 else _apply(A, [eye[k0]], tr)
        G = np.stack(cols, axis=1).astype(np.float64)                          # G[:, k] = A e_k
        mats[tr] = G
        orc = E.Oracle(psf, nx, ny, mode, tr)
        M, Mabs, cnt = (m.toarray() for m in orc.matrix())
        b = E.bound(fam, kh, kw, Mabs, cnt, cnt, orc.pmax)
        assert np.all(G[b == 0] == 0.0), (E.case_id(c), mode, tr, "non-zero where no tap reaches")
        ratio = np.abs(G - M)[b > 0] / b[b > 0]
        worst = float(ratio.max())
        if worst >= 1.0:
            i, j = np.argwhere((np.abs(G - M) >= b) & (b > 0))[0]
            raise AssertionError(f"entry ({i}, {j}) = output {_locate(c, divmod(int(i), ny), mode, tr)} of input pixel "
                                 f"{divmod(int(j), ny)}: {worst:.3f} of the bound")
        bar(f"blur_entry.matrix.{E.case_id(c)}.{mode}.{'T' if tr else 'N'}", worst, 1.0)
    if kh % 2 and kw % 2 and mode in ("constant", "wrap") and nx > kh and ny > kw:
        assert np.array_equal(mats[True], mats[False].T), (E.case_id(c), mode)


# ------------------------------------------------------------------------------------------------ (B) + (D) combs and real inputs
def _kernels(c):
    """name -> (offset, forced path, family) of the other kernels the case's operator also runs on."""
    kh, kw = E.entry_psf(c.psf).shape
    out = {}
    if max(kh, kw) <= 64 and c.path != "tile":
        out["tile"] = (0, "tile", _fam(c, "tile"))
    if c.path != "generic":
        out["generic"] = (0, "generic", "general")
    if c.path == "slide":
        out["strip"] = (1, None, "separable")
    return out


def _run_case(c, mode, with_others=True, ncomb=None, inputs=("noise", "uniform", "ramp")):
    nx, ny = c.shape
    n = nx * ny
    psf = E.entry_psf(c.psf)
    cus = _cus()
    A = _op(c, mode)
    off, _ = _own(c)
    fam = _fam(c, c.path)
    combs = E.combs(c, cus)[:ncomb]
    real = {k: v for k, v in E.real_inputs(nx, ny, 31 * nx + ny).items() if k in inputs}
    others = _kernels(c) if with_others else {}
    ops = {name: _op(c, mode, force) for name, (_, force, _) in others.items()}
    for tr in (False, True):
        orc = E.Oracle(psf, nx, ny, mode, tr)
        worst = 0.0
        singles, oracles = [], []
        for q, x in enumerate(combs):                                           # (B) one operator, several kernels
            o = orc.apply(x)
            own = _apply(A, [x], tr, offset=off)[0].reshape(nx, ny)
            worst = max(worst, _ratio(c, own, o, orc, fam, mode, tr, f"comb {q}, own kernel"))
            singles.append(own)
            oracles.append(o)
            got = {}
            for name, (ooff, _, ofam) in others.items():
                got[name] = _apply(ops[name], [x], tr, offset=ooff)[0].reshape(nx, ny)
                worst = max(worst, _ratio(c, got[name], o, orc, ofam, mode, tr, f"comb {q}, {name} kernel"))
            got[{"strip_view": "strip"}.get(c.path, c.path)] = own
            one_term = o["Tc"] <= 1 if "Tc" in o else np.zeros((nx, ny), dtype=bool)
            for a in sorted(got):
                for b2 in sorted(got):
                    if a >= b2 or _fam(c, a) != _fam(c, b2):
                        continue                                                # across the families: inside the bounds only
                    ok = one_term if "slide" in (a, b2) else np.ones((nx, ny), dtype=bool)
                    assert np.array_equal(got[a][ok], got[b2][ok]), (E.case_id(c), mode, tr, q, a, b2)
        if combs:                                                               # a batch of three
            three = [combs[q % len(combs)] for q in range(3)]
            ld = (n + 3) // 4 * 4 + 4 if c.path == "slide" else n + 5 - n % 4
            for q, g in enumerate(_apply(A, three, tr, ld=ld)):
                g, o = g.reshape(nx, ny), oracles[q % len(combs)]
                worst = max(worst, _ratio(c, g, o, orc, fam, mode, tr, f"batch of three, vector {q}"))
                ok = np.ones((nx, ny), dtype=bool)
                if c.path == "slide":                                           # the batch changes the band heights
                    ok = o["Tc"] <= 1
                assert np.array_equal(g[ok], singles[q % len(combs)][ok]), (E.case_id(c), mode, tr, "batch", q)
        for name, x in real.items():                                            # (D) accumulation on real inputs
            o = orc.apply(x)
            own = _apply(A, [x], tr, offset=off)[0].reshape(nx, ny)
            worst = max(worst, _ratio(c, own, o, orc, fam, mode, tr, f"input {name}"))
            assert relerr(own, o["y"]) < 1e-5, (E.case_id(c), mode, tr, name)   # the older norm-wise bar, for continuity
        bar(f"blur_entry.inputs.{E.case_id(c)}.{mode}.{'T' if tr else 'N'}", worst, 1.0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", COMB, ids=E.case_id)
def test_combs_and_real_inputs(c, mode):
    """(B) Unit combs through the case's own kernel, the tile and generic kernels (set_path), the strip kernel (an operand one float
    off alignment) and a batch of three: inside each kernel's bound everywhere, the same bits where the docstring says so.
    (D) White noise, uniform [0, 1) and a smooth ramp under a Hanning profile through the case's own kernel: inside the bound entry
    by entry, and inside the norm-wise 1e-5 bar."""
    _run_case(c, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", WRAP, ids=E.case_id)
def test_strip_ring_wrap_around(c, mode):
    """A strip band of two 32-row steps (the second wraps around the LDS ring): on 256 CUs only an image of more than 512 strips gets
    one, 2.6 M pixels, so the case's own kernel alone, on the corner comb and on white noise."""
    assert "strip.several_steps_ring_wrap" in E.case_situations(c, _cus())
    _run_case(c, mode, with_others=False, ncomb=1, inputs=("noise",))


# ------------------------------------------------------------------------------------------------ 4096^2
@pytest.mark.parametrize("c", E.nt_cases(), ids=E.case_id)
def test_full_size_every_pixel_both_directions(c):
    """The sizes stored non-temporally — 9x9 at the benchmarked 4096^2 (64-row bands on 256 CUs), 3x3 to 7x7 at the threshold of
    11 << 20 pixels — under reflect with an asymmetric separable PSF: EVERY pixel of the forward and of the "transpose" product of a
    white-noise image against the factored oracle (two sparse products per quantity), inside the separable bound."""
    nx, ny = c.shape
    assert "slide.nt_store" in E.case_situations(c, _cus())
    psf = E.entry_psf(c.psf)
    assert not np.allclose(psf, psf[::-1, ::-1], rtol=1e-3) and not np.allclose(psf, psf.T, rtol=1e-3)
    A = _op(c, "reflect")
    x = np.random.default_rng(nx).standard_normal((nx, ny)).astype(np.float32)
    for tr in (False, True):
        orc = E.Oracle(psf, nx, ny, "reflect", tr)
        o = orc.apply(x)
        got = _apply(A, [x], tr)[0].reshape(nx, ny)
        r = _ratio(c, got, o, orc, "separable", "reflect", tr, "full-size white noise")
        assert relerr(got, o["y"]) < 1e-5
        bar(f"blur_entry.fullsize.{E.case_id(c)}.reflect.{'T' if tr else 'N'}", r, 1.0)
