"""The vector kernels (csrc/vecops.hip), the CGLS updates (csrc/cgls_update.hip) and the scalar plumbing they feed (scalar_from_wave,
finalize_block_256, coef_eval, finalize_sums, trk_finalize_batched) entry by entry against float64 on the same float32 operands, on
every path the size, the alignment, the aliasing and the scalar sources select.  Operands, references, bounds and launch plans:
tests/vec_cases.py (checked on the CPU by tests/test_vec_cases_host.py).  All calls go through the C ABI (eng.lib).

Exact operands (multiples of 1 / 8, dyadic steps): every update and every sum is exact, the device result must EQUAL the reference.
General operands: every updated vector must still equal the reference bit for bit (each entry is ONE correctly rounded operation, or
two for trk_axpby with y and for w (x - y)); sums within (n + 4096) 2^-53 S, the worst logged as a fraction of the bound (conftest.bar).

Every output lives between 8 guard floats (4 guard doubles) that must be unchanged after the call; block partials handed to a consumer
sit between two slots of 2^40.  Before a case runs, its launch plan on THIS device's compute-unit count must show the branch it is
named for.

  entry point                               kernel<template arguments>                  reached by
  trk_dot, trk_nrm2sq, trk_diff_nrm2sq      k_reduce2<MODE, VEC>; k_finalize            reductions (sizes, exact and general), reductions_misaligned,
                                                                                        reductions_empty, finalize_sums_block_counts
  trk_finalize_batched                      k_finalize_batched                          finalize_batched
  trk_axpby                                 k_axpby<HAS_Y, SUMSQ, VEC>; coef_eval       axpby (sizes, coefficients, aliases), axpby_misaligned
  trk_scale_dot, trk_mul, trk_mul_diff      k_scale_dot<VEC>, k_mul<VEC>, k_mul_diff    scale_mul_muldiff
  trk_mm_weights                            k_mm_weights<HAS_Y, VEC>; mm_w              mm_weights
  trk_group_weights                         k_group_weights                             group_weights
  scalar_from_wave                          (every consumer below)                      scalar_sources
  trk_cgls_update_xr, _deferred, _src       k_cgls_update<HAS_XT, VEC>                  cgls_update_xr, cgls_update_xr_misaligned, nontemporal
  trk_cgls_r_update                         k_cgls_r_update<VEC>                        r_and_p_updates
  trk_cgls_p_update, _to                    k_cgls_p_update<VEC>, nt = 0 / 3            r_and_p_updates
  trk_cgls_x_update, trk_cgls_xp_update     k_cgls_x_update<HAS_XT>, k_cgls_xp_update   x_and_xp_updates, nontemporal
  trk_cgls_xs_update, _x                    k_cgls_xs_update<HAS_XT, C, XONLY>          xs_update (C = 1 .. 8), xs_update_large
  all that form x'                                                                      x_update_is_one_rounding_everywhere
"""
import ctypes

import numpy as np
import pytest
import torch

import vec_cases as C
from conftest import bar

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD, GUARD_D = 8, 4
EINVAL = -1


@pytest.fixture(scope="module")
def eng():
    from trips_py_amd.engine import default_engine
    return default_engine()


@pytest.fixture(scope="module")
def cus(eng):
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


def ok(eng, name, *args):
    from trips_py_amd import _lib
    _lib.check(getattr(eng.lib, name)(*args, eng.stream()), name)


class FV:
    """n device floats `off` floats behind a 16-byte boundary, between guard floats."""

    def __init__(self, eng, n, host=None, off=0, fill=SENTINEL):
        self.n, self.lo = n, GUARD + off
        self.buf = torch.full((self.lo + n + GUARD,), SENTINEL, dtype=torch.float32, device=eng.device)
        self.view = self.buf[self.lo:self.lo + n]
        self.ptr = self.buf.data_ptr() + 4 * self.lo
        assert (self.ptr % 16 == 0) == (off % 4 == 0)
        if host is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)))
        elif fill != SENTINEL:
            self.view.fill_(fill)

    def get(self):
        h = self.buf.cpu().numpy()
        assert np.all(h[:self.lo] == SENTINEL) and np.all(h[self.lo + self.n:] == SENTINEL), "guard floats overwritten"
        return h[self.lo:self.lo + self.n]


class DV:
    """m device doubles between guard doubles."""

    def __init__(self, eng, m, values=None):
        self.m = m
        self.t = torch.full((m + 2 * GUARD_D,), SENTINEL, dtype=torch.float64, device=eng.device)
        if values is not None:
            self.t[GUARD_D:GUARD_D + m] = torch.from_numpy(np.asarray(values, dtype=np.float64).reshape(m))

    def ptr(self, i=0):
        return self.t.data_ptr() + 8 * (GUARD_D + i)

    def get(self):
        h = self.t.cpu().numpy()
        assert np.all(h[:GUARD_D] == SENTINEL) and np.all(h[GUARD_D + self.m:] == SENTINEL), "guard doubles overwritten"
        return h[GUARD_D:GUARD_D + self.m].copy()


class Src:
    """A scalar source on the device: n block partials between two slots of 2^40 (n = 1: a finished scalar, likewise)."""

    def __init__(self, eng, parts):
        parts = np.atleast_1d(np.asarray(parts, dtype=np.float64))
        self.n, self.host = parts.size, C.poisoned(parts)
        self.d = DV(eng, self.n + 2, self.host)
        self.ptr = self.d.ptr(1)

    def unchanged(self):
        assert np.array_equal(self.d.get(), self.host), "a scalar source was written to"


class Bars(dict):
    def see(self, name, got, R):
        """A sum against its reference: equal (exact operands) or within the bound, the worst ratio kept per name."""
        err = float(R.error(got))
        if R.bound is None:
            assert err == 0.0, (name, "exact operands", got, R.ref)
            return
        assert err <= R.bound, (name, got, R.ref, err, R.bound)
        self[name] = max(self.get(name, 0.0), err / R.bound if R.bound > 0 else 0.0)

    def flush(self, tag):
        for name, v in sorted(self.items()):
            bar(f"vec.entrywise[{name}:{tag}]", v, 1.0)


def same(name, got, want):
    """Entry-wise equality of float32 vectors, to the bit (-0.0 and 0.0 apart)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (name, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def norms_check(W, name, P, grid, xn, d, xt, exact):
    """[grid][3] raw partials summed on the host against the three norms; the third exactly 0.0 without x_true."""
    P = np.asarray(P).reshape(grid, 3)
    for q, terms in enumerate(C.x_norm_terms(xn, d, xt)):
        if q == 2 and xt is None:
            assert np.all(P[:, 2] == 0.0) and not np.any(np.signbit(P[:, 2])), (name, "third norm without x_true")
        else:
            W.see(f"{name}.s{q}", P[:, q].astype(C.WIDE).sum(), C.sums(terms, exact))


# ------------------------------------------------------------------------------------------------------------ reductions
REDUCE = (("trk_dot", 0), ("trk_nrm2sq", 1), ("trk_diff_nrm2sq", 2))


def reduce_call(eng, fn, mode, x, y, n, out):
    if mode == 1:
        ok(eng, fn, x, n, out)
    else:
        ok(eng, fn, x, y, n, out)


@pytest.mark.parametrize("exact", [True, False])
def test_reductions(eng, cus, exact):
    """Every named size, largest first and last (the stream's scratch is reused between calls of different grid sizes)."""
    W = Bars()
    S = C.sizes(cus)
    order = ["two-passes+tail"] + [k for k in S if k != "two-passes+tail"] + ["two-passes+tail"]
    for name in order:
        n = S[name]
        C.expect(C.stream_plan(n, cus, (0, 0)), vec=True)
        x, y = C.vec(n, exact, "x"), C.vec(n, exact, "y")
        dx, dy, out = FV(eng, n, x), FV(eng, n, y), DV(eng, 1)
        for fn, mode in REDUCE:
            reduce_call(eng, fn, mode, dx.ptr, dy.ptr, n, out.ptr())
            W.see(f"{fn}", out.get()[0], C.sums(C.dot_terms(mode, x, y), exact))
        same("x", dx.get(), x), same("y", dy.get(), y)
    W.flush("exact" if exact else "general")


@pytest.mark.parametrize("exact", [True, False])
def test_reductions_misaligned(eng, cus, exact):
    """Each operand in turn 1, 2 and 3 floats off a 16-byte boundary: the scalar kernel."""
    W = Bars()
    n = 4099
    x, y = C.vec(n, exact, "x"), C.vec(n, exact, "y")
    for which in (0, 1):
        for off in (1, 2, 3):
            offs = [0, 0]
            offs[which] = off
            dx, dy, out = FV(eng, n, x, offs[0]), FV(eng, n, y, offs[1]), DV(eng, 1)
            for fn, mode in REDUCE:
                used = offs[:1] if mode == 1 else offs
                C.expect(C.stream_plan(n, cus, [4 * o for o in used]), vec=not any(used), grid=5)
                reduce_call(eng, fn, mode, dx.ptr, dy.ptr, n, out.ptr())
                W.see(fn, out.get()[0], C.sums(C.dot_terms(mode, x, y), exact))
    W.flush("misaligned-" + ("exact" if exact else "general"))


def test_reductions_empty(eng):
    """n = 0 with NULL vectors: 0.0 (one block sums nothing)."""
    for fn, mode in REDUCE:
        out = DV(eng, 1)
        reduce_call(eng, fn, mode, None, None, 0, out.ptr())
        v = out.get()[0]
        assert v == 0.0 and not np.signbit(v), fn


def test_finalize_sums_block_counts(eng, cus):
    """finalize_block_256 through trk_dot: block counts on both sides of its four-accumulator loop (b + 768 < nblocks) and of the
    256-thread stride; exact operands, so a partial dropped or read twice changes the result."""
    ran = 0
    for nb in C.FINALIZE_BLOCKS:
        n = C.n_for_blocks(nb, cus)
        if n is None:
            continue
        x, y = C.vec(n, True, "x"), C.vec(n, True, "y")
        dx, dy, out = FV(eng, n, x), FV(eng, n, y), DV(eng, 1)
        ok(eng, "trk_dot", dx.ptr, dy.ptr, n, out.ptr())
        assert out.get()[0] == C.dot_terms(0, x, y).sum(), nb
        ran += 1
    assert ran >= 5


@pytest.mark.parametrize("nvals", [1, 3, 8])
def test_finalize_batched(eng, nvals):
    """out[b out_stride + o] = sum over blocks of partials[b][block][o]: every entry a distinct multiple of 2^-4 (exact sums), 2^40
    before and behind the partials, out_stride larger than nvals with the gaps and the guards untouched."""
    for nblocks in C.FINALIZE_BLOCKS:
        for batches in (1, 3):
            m = batches * nblocks * nvals
            P = np.arange(1, m + 1, dtype=np.float64) / 16.0
            src = Src(eng, P)
            stride = nvals + 2
            out = DV(eng, batches * stride)
            ok(eng, "trk_finalize_batched", src.ptr, nblocks, nvals, batches, out.ptr(), stride)
            got = out.get().reshape(batches, stride)
            assert np.array_equal(got[:, :nvals], P.reshape(batches, nblocks, nvals).sum(axis=1)), (nblocks, batches)
            assert np.all(got[:, nvals:] == SENTINEL)
            src.unchanged()


# ------------------------------------------------------------------------------------------------------------ axpby
def coef_args(eng, c):
    """(c, num*, den*, flags) of a coefficient as the C ABI takes them, the device scalars between guards."""
    cc, num, den, flags = c
    d = DV(eng, 2, [1.0 if num is None else num, 1.0 if den is None else den])
    return (float(cc), None if num is None else d.ptr(0), None if den is None else d.ptr(1), int(flags)), d


def axpby_run(eng, W, tag, n, exact, ca, cb, has_y, sumsq, offs=(0, 0, 0), alias=None):
    x, y = C.vec(n, exact, "x"), C.vec(n, exact, "y")
    dx, dy = FV(eng, n, x, offs[0]), FV(eng, n, y, offs[1])
    do = {"x": dx, "y": dy}.get(alias) or FV(eng, n, None, offs[2])
    (a4, da), (b4, db) = coef_args(eng, ca), coef_args(eng, cb)
    ss = DV(eng, 1)
    ok(eng, "trk_axpby", n, *a4, dx.ptr, *b4, dy.ptr if has_y else None, do.ptr, ss.ptr() if sumsq else None)
    a, b = np.float32(C.coef(*ca)), np.float32(C.coef(*cb))
    got = do.get()
    same(f"axpby {tag}", got, C.axpby(a, x, b, y) if has_y else C.axpby(a, x))
    if alias != "x":
        same("x", dx.get(), x)
    if alias != "y":
        same("y", dy.get(), y)
    if sumsq:
        W.see("axpby.sumsq", ss.get()[0], C.sums(C.dot_terms(1, got), exact))
    else:
        assert ss.get()[0] == SENTINEL


GENERAL_COEFS = ((1.0, 3.0, 7.0, 0), (1.0, 25.0, 9.0, 3))        # 3 / 7 and 5 / 3: not dyadic


@pytest.mark.parametrize("exact", [True, False])
def test_axpby(eng, cus, exact):
    """HAS_Y x SUMSQ on every named size; out aliasing x and y; every combination of num / den / TRK_SQRT_* (coef_eval)."""
    W = Bars()
    S = C.sizes(cus)
    ca, cb = (C.COEFS[6], C.COEFS[9]) if exact else GENERAL_COEFS
    for name, n in S.items():
        for has_y in (True, False):
            for sumsq in (True, False):
                if n > 1 << 20 and not (has_y and sumsq) and name != "two-passes+tail":
                    continue
                axpby_run(eng, W, name, n, exact, ca, cb, has_y, sumsq)
    for alias in ("x", "y"):
        for n in (4099, S["pass+1"]):
            axpby_run(eng, W, f"alias {alias}", n, exact, ca, cb, True, True, alias=alias)
    for i, c in enumerate(C.COEFS):
        axpby_run(eng, W, f"coef {i}", 1027, exact, c, C.COEFS[(i + 3) % len(C.COEFS)], True, i % 2 == 0)
    W.flush("exact" if exact else "general")


@pytest.mark.parametrize("exact", [True, False])
def test_axpby_misaligned(eng, cus, exact):
    """x, y, out each alone 1, 2 and 3 floats off: VEC off through every single operand; without y its alignment does not count."""
    W = Bars()
    ca, cb = (C.COEFS[1], C.COEFS[4]) if exact else GENERAL_COEFS
    for which in range(3):
        for off in (1, 2, 3):
            offs = [0, 0, 0]
            offs[which] = off
            C.expect(C.stream_plan(4099, cus, [4 * o for o in offs]), vec=False)
            axpby_run(eng, W, f"off {offs}", 4099, exact, ca, cb, True, off == 1, offs)
            axpby_run(eng, W, f"off {offs} no y", 4099, exact, ca, cb, False, off == 2, offs)
    W.flush("misaligned-" + ("exact" if exact else "general"))


# ------------------------------------------------------------------------------------------------------------ scale_dot, mul, mul_diff
@pytest.mark.parametrize("exact", [True, False])
def test_scale_mul_muldiff(eng, cus, exact):
    """Each output entry is one rounding (w (x - y): two, as written); in place and out of place; every operand misaligned in turn."""
    W = Bars()
    S = C.sizes(cus)
    cases = [(n, (0, 0, 0, 0), False) for n in S.values() if n <= 1025 or n == S["two-passes+tail"]]
    cases += [(4099, (0, 0, 0, 0), True)]
    for which in range(4):
        offs = [0, 0, 0, 0]
        offs[which] = 1 + which % 3
        cases.append((4099, tuple(offs), False))
    ca = C.COEFS[8] if exact else GENERAL_COEFS[0]
    a = np.float32(C.coef(*ca))
    for n, offs, inplace in cases:
        w, x, y = C.vec(n, exact, "w"), C.vec(n, exact, "x"), C.vec(n, exact, "y")
        # trk_scale_dot: out = a x, dot = <out, z>
        dx, dz = FV(eng, n, x, offs[1]), FV(eng, n, y, offs[2])
        do = dx if inplace else FV(eng, n, None, offs[3])
        a4, da = coef_args(eng, ca)
        dot = DV(eng, 1)
        C.expect(C.stream_plan(n, cus, [4 * o for o in offs[1:]]), vec=not any(offs[1:]))
        ok(eng, "trk_scale_dot", n, *a4, dx.ptr, do.ptr, dz.ptr, dot.ptr())
        got = do.get()
        same("scale_dot", got, C.axpby(a, x))
        W.see("scale_dot.dot", dot.get()[0], C.sums(C.dot_terms(0, got, y), exact))
        same("z", dz.get(), y)
        # trk_mul: out = x y
        dx, dy = FV(eng, n, x, offs[1]), FV(eng, n, y, offs[2])
        do = dx if inplace else FV(eng, n, None, offs[3])
        ok(eng, "trk_mul", n, dx.ptr, dy.ptr, do.ptr)
        same("mul", do.get(), x * y)
        same("y", dy.get(), y)
        # trk_mul_diff: out = w (x - y)
        dw, dx, dy = FV(eng, n, w, offs[0]), FV(eng, n, x, offs[1]), FV(eng, n, y, offs[2])
        do = dx if inplace else FV(eng, n, None, offs[3])
        C.expect(C.stream_plan(n, cus, [4 * o for o in offs]), vec=not any(offs))
        ok(eng, "trk_mul_diff", n, dw.ptr, dx.ptr, dy.ptr, do.ptr)
        same("mul_diff", do.get(), w * (x - y))
        same("w", dw.get(), w), same("y", dy.get(), y)
    W.flush("exact" if exact else "general")


# ------------------------------------------------------------------------------------------------------------ weights
POWF_LIMIT_ULP = 3.0        # twice the largest error measured on the MI355X (docs/kernels/vector_updates.md), rounded up to a whole ulp


@pytest.mark.parametrize("p", [2.0, 1.0, 0.5, 1.5])
def test_mm_weights(eng, cus, p):
    """p = 2: exactly 1.  p = 1: the hardware reciprocal square root (1 ulp) of a t that carries half an ulp: 2 ulp per entry, and
    1 / sqrtf below eps^2 = 1e-30.  powf: within POWF_LIMIT_ULP of the float64 reference (5e-6 relative, the bar of tests/test_gpu_kernels.py, is 42 ulp)."""
    assert POWF_LIMIT_ULP * 2.0 ** -23 <= 5e-6
    worst = 0.0
    for n, offs in ((1027, (0, 0, 0)), (4099, (0, 0, 0)), (4099, (1, 0, 0)), (4099, (0, 2, 0)), (4099, (0, 0, 3)),
                    (C.sizes(cus)["pass+1"], (0, 0, 0))):
        for eps in (1e-3, 1e-16):
            for with_y in (True, False):
                x, y = C.vec(n, False, "x"), C.vec(n, False, "y")
                x[1::7] = 0.0                                             # v = 0
                if with_y:
                    y[1::7] = 0.0
                    y[2::7] = x[2::7]
                used = offs if with_y else (offs[0], 0, offs[2])
                C.expect(C.stream_plan(n, cus, [4 * o for o in used]), vec=not any(used))
                dx, dy, do = FV(eng, n, x, offs[0]), FV(eng, n, y, offs[1]), FV(eng, n, None, offs[2])
                ok(eng, "trk_mm_weights", n, dx.ptr, dy.ptr if with_y else None, float(eps), float(p), do.ptr)
                got = do.get()
                ref, special = C.mm_weights(x, y if with_y else None, eps, p)
                if special == 1:
                    same("mm_weights p = 2", got, np.ones(n, dtype=np.float32))
                    continue
                assert np.all(np.isfinite(got))
                err = float(C.ulps32(got, ref).max())
                worst = max(worst, err)
    if p != 2.0:
        print(f"mm_weights p = {p}: worst error {worst:.3f} ulp")
        bar(f"vec.entrywise[mm_weights.ulp:p={p}]", worst / (2.0 if p == 1.0 else POWF_LIMIT_ULP), 1.0 + 1e-12)


@pytest.mark.parametrize("expo", [-0.5, -0.75, 0.0])
def test_group_weights(eng, expo):
    """Within 1 ulp of the float64 reference (sequential sum, pow), and equal to its float32 rounding away from ties."""
    for groups in (1, 255, 256, 257):
        for glen in (1, 3, 32):
            for copies in (1, 3):
                d = C.vec(groups * glen, False, "d", glen)
                dd, do = FV(eng, groups * glen, d), FV(eng, groups * copies)
                add = float(np.exp(2))
                ok(eng, "trk_group_weights", dd.ptr, groups, glen, add, float(expo), copies, do.ptr)
                got = do.get()
                ref = C.group_weights(d, groups, glen, add, expo, copies)
                assert np.all(C.ulps32(got, ref) <= 1.0), (groups, glen, copies)
                far = C.far_from_tie(ref)
                same("group_weights", got[far], ref.astype(np.float32)[far])
                same("d", dd.get(), d)


# ------------------------------------------------------------------------------------------------------------ scalar sources
@pytest.mark.parametrize("exact", [True, False])
def test_scalar_sources(eng, cus, exact):
    """scalar_from_wave on both sides of its eight-accumulator loop (i + 448 < n) and of every remainder step, through the four
    consumers: the published scalar equals the exact total, and the step it makes (dyadic, or 3 / 7 of the exact totals) gives the
    reference's vectors."""
    n = 1027
    x, p, r, w, t = (C.vec(n, exact, k) for k in "xprwt")
    ratio = 0.75 if exact else 3 / 7
    W = Bars()
    for npart in C.N_PARTIALS:
        pn, tn, pd, td = C.ratio_sources(ratio, npart, npart)
        st = C.step32(tn, td)
        # r -= (gamma_old / S(delta)) w
        gold, dl, pub = Src(eng, [tn]), Src(eng, pd), DV(eng, 1)
        dr, dw = FV(eng, n, r), FV(eng, n, w)
        ok(eng, "trk_cgls_r_update", n, gold.ptr, dl.ptr, npart, dr.ptr, dw.ptr, pub.ptr())
        assert pub.get()[0] == td, ("r_update", npart)
        same(f"r_update {npart}", dr.get(), C.r_update(r, w, st))
        # p = fmaf((float)(S(gamma_new) / gamma_old), p, t)
        gn, gold = Src(eng, pn), Src(eng, [td])
        dt, dp = FV(eng, n, t), FV(eng, n, p)
        ok(eng, "trk_cgls_p_update", n, dt.ptr, dp.ptr, gn.ptr, npart, gold.ptr, pub.ptr())
        assert pub.get()[0] == tn, ("p_update", npart)
        same(f"p_update {npart}", dp.get(), C.p_update(t, p, st))
        # x' = x + (S(gamma) / S(delta)) p, both from partials, of different counts as well
        for nd in (npart, C.N_PARTIALS[(C.N_PARTIALS.index(npart) + 5) % len(C.N_PARTIALS)]):
            pd2, td2 = C.partials(nd, C.UNITS[ratio][1])
            st2 = C.step32(tn, td2)
            gm, dl, pg, pdl = Src(eng, pn), Src(eng, pd2), DV(eng, 1), DV(eng, 1)
            dx, dp, dxn = FV(eng, n, x), FV(eng, n, p), FV(eng, n)
            grid = C.stream_grid(n, cus)
            NP, nb = DV(eng, 3 * grid), ctypes.c_int(-1)
            if not exact or nd == npart:
                ok(eng, "trk_cgls_x_update", n, gm.ptr, npart, dl.ptr, nd, dx.ptr, dp.ptr, dxn.ptr, None, pdl.ptr(), pg.ptr(), NP.ptr(),
                   grid, ctypes.byref(nb))
                assert (pg.get()[0], pdl.get()[0], nb.value) == (tn, td2, grid), ("x_update", npart, nd)
                xf, _, d = C.x_update(x, p, st2)
                same(f"x_update {npart} {nd}", dxn.get(), xf)
                norms_check(W, "x_update", NP.get(), grid, xf, d, None, exact)
            # the fused [x, r] update with gamma and delta from partials, delta published
            dx, dp, dxn, dr, dw = FV(eng, n, x), FV(eng, n, p), FV(eng, n), FV(eng, n, r), FV(eng, n, w)
            NP, nb = DV(eng, 3 * grid), ctypes.c_int(-1)
            if not exact or nd == npart:
                ok(eng, "trk_cgls_update_xr_src", n, n, gm.ptr, npart, dl.ptr, nd, dx.ptr, dp.ptr, dxn.ptr, dr.ptr, dw.ptr, None, pdl.ptr(),
                   NP.ptr(), grid, ctypes.byref(nb))
                assert (pdl.get()[0], nb.value) == (td2, grid), ("update_xr_src", npart, nd)
                same(f"update_xr_src x {npart} {nd}", dxn.get(), C.x_update(x, p, st2)[0])
                same(f"update_xr_src r {npart} {nd}", dr.get(), C.r_update(r, w, st2))
            gm.unchanged(), dl.unchanged()
    W.flush("scalar-sources-" + ("exact" if exact else "general"))


# ------------------------------------------------------------------------------------------------------------ the fused [x, r] update
def xr_run(eng, cus, W, tag, n, m, exact, entry, with_xt, pub="none", npart=1, offs=(0,) * 6, alias=False):
    """One call of trk_cgls_update_xr (entry 'sums'), _deferred or _src; offs: x, p, x_new, r, w, x_true."""
    x, p, xt = (C.vec(n, exact, k) for k in ("x", "p", "xt"))
    r, w = C.vec(m, exact, "r"), C.vec(m, exact, "w")
    ratio = 0.75 if exact else 3 / 7
    pn, tn, pd, td = C.ratio_sources(ratio, npart, npart)
    st = C.step32(tn, td)
    plan = C.stream_plan(n, cus, [4 * o for o in (offs if with_xt else offs[:5])], m=m)
    C.expect(plan, vec=not any(offs if with_xt else offs[:5]), grid=C.stream_grid(max(n, m), cus))
    grid = plan["grid"]
    dx, dp, dr, dw, dxt = FV(eng, n, x, offs[0]), FV(eng, n, p, offs[1]), FV(eng, m, r, offs[3]), FV(eng, m, w, offs[4]), FV(eng, n, xt, offs[5])
    dxn = dx if alias else FV(eng, n, None, offs[2])
    gm, dl = Src(eng, pn if npart > 1 else [tn]), Src(eng, pd if npart > 1 else [td])
    xtp = dxt.ptr if with_xt else None
    if entry == "sums":
        out = DV(eng, 3)
        ok(eng, "trk_cgls_update_xr", n, m, gm.ptr, dl.ptr, dx.ptr, dp.ptr, dxn.ptr, dr.ptr, dw.ptr, xtp, out.ptr())
        P = out.get().reshape(1, 3)
    else:
        NP, nb = DV(eng, 3 * grid), ctypes.c_int(-1)
        if entry == "deferred":
            ok(eng, "trk_cgls_update_xr_deferred", n, m, gm.ptr, dl.ptr, dx.ptr, dp.ptr, dxn.ptr, dr.ptr, dw.ptr, xtp, NP.ptr(), grid,
               ctypes.byref(nb))
        else:
            pubd = DV(eng, 1)
            pp = {"none": None, "distinct": pubd.ptr(), "delta": dl.ptr}[pub]
            ok(eng, "trk_cgls_update_xr_src", n, m, gm.ptr, npart, dl.ptr, npart, dx.ptr, dp.ptr, dxn.ptr, dr.ptr, dw.ptr, xtp, pp, NP.ptr(),
               grid, ctypes.byref(nb))
            assert pubd.get()[0] == (td if pub == "distinct" else SENTINEL), (tag, "published delta")
        assert nb.value == grid
        P = NP.get().reshape(grid, 3)
    gm.unchanged(), dl.unchanged()                       # (publish_delta == delta with finished scalars: delta stays what it was)
    xf, _, d = C.x_update(x, p, st)
    same(f"{tag} x_new", dxn.get(), xf)
    same(f"{tag} r", dr.get(), C.r_update(r, w, st))
    same("p", dp.get(), p), same("w", dw.get(), w), same("x_true", dxt.get(), xt)
    if not alias:
        same("x", dx.get(), x)
    norms_check(W, f"update_xr[{entry}]", P, P.shape[0], xf, d, xt if with_xt else None, exact)


XR_SHAPES = ((1025, 1025), (4099, 777), (777, 4099), (1024, 0), (0, 1024))


@pytest.mark.parametrize("exact", [True, False])
def test_cgls_update_xr(eng, cus, exact):
    """n != m both ways and an empty side; with and without x_true; finished scalars and partials; publish_delta NULL, distinct and
    delta itself; x_new aliasing x; one size with a second grid-stride pass."""
    W = Bars()
    big = C.sizes(cus)["two-passes+tail"]
    for n, m in XR_SHAPES + ((big, big - 1021),):
        for with_xt in (True, False):
            if n == big and not with_xt:
                continue
            xr_run(eng, cus, W, "sums", n, m, exact, "sums", with_xt)
            xr_run(eng, cus, W, "deferred", n, m, exact, "deferred", with_xt, alias=with_xt)
            for pub in ("none", "distinct", "delta"):
                if n == big and pub != "distinct":
                    continue
                xr_run(eng, cus, W, f"src {pub}", n, m, exact, "src", with_xt, pub=pub, npart=1, alias=pub == "none")
                if pub != "delta":
                    xr_run(eng, cus, W, f"src {pub} partials", n, m, exact, "src", with_xt, pub=pub, npart=65)
    W.flush("update-xr-" + ("exact" if exact else "general"))


@pytest.mark.parametrize("which", range(6))
def test_cgls_update_xr_misaligned(eng, cus, which):
    """Each of x, p, x_new, r, w, x_true alone off a 16-byte boundary: the scalar loops form the same bits."""
    W = Bars()
    for off in (1, 2, 3):
        offs = [0] * 6
        offs[which] = off
        for exact in (True, False):
            xr_run(eng, cus, W, f"off {offs}", 4099, 777, exact, "src", True, pub="distinct", npart=2, offs=tuple(offs))
            if which == 5:                               # without x_true its alignment does not count: the float4 body
                xr_run(eng, cus, W, f"off {offs} no xt", 4099, 777, exact, "deferred", False, offs=tuple(offs))
    W.flush(f"update-xr-misaligned-{which}")


# ------------------------------------------------------------------------------------------------------------ r and p updates
@pytest.mark.parametrize("exact", [True, False])
def test_r_and_p_updates(eng, cus, exact):
    """fmaf(-step, w, r) and fmaf(b, p, t) on every named size; p_update_to with p_out != p (non-temporal loads) and == p;
    each operand misaligned (the scalar kernels)."""
    S = C.sizes(cus)
    ratio = 0.75 if exact else 3 / 7
    pn, tn, pd, td = C.ratio_sources(ratio, 3, 3)
    st = C.step32(tn, td)
    cases = [(n, (0, 0, 0)) for n in S.values()]
    for which in range(3):
        for off in (1, 2, 3):
            offs = [0, 0, 0]
            offs[which] = off
            cases.append((4099, tuple(offs)))
    for n, offs in cases:
        r, w, t, p = (C.vec(n, exact, k) for k in "rwtp")
        if offs[2] == 0:
            C.expect(C.stream_plan(n, cus, [4 * o for o in offs[:2]]), vec=not any(offs[:2]))
            gold, dl, pub = Src(eng, [tn]), Src(eng, pd), DV(eng, 1)
            dr, dw = FV(eng, n, r, offs[0]), FV(eng, n, w, offs[1])
            ok(eng, "trk_cgls_r_update", n, gold.ptr, dl.ptr, 3, dr.ptr, dw.ptr, pub.ptr())
            same(f"r_update {n} {offs}", dr.get(), C.r_update(r, w, st))
            same("w", dw.get(), w)
            assert pub.get()[0] == td
        C.expect(C.stream_plan(n, cus, [4 * o for o in offs]), vec=not any(offs))
        gn, gold, pub = Src(eng, pn), Src(eng, [td]), DV(eng, 1)
        want = C.p_update(t, p, st)
        dt, dp, dpo = FV(eng, n, t, offs[0]), FV(eng, n, p, offs[1]), FV(eng, n, None, offs[2])
        ok(eng, "trk_cgls_p_update_to", n, dt.ptr, dp.ptr, dpo.ptr, gn.ptr, 3, gold.ptr, pub.ptr())
        same(f"p_update_to {n} {offs}", dpo.get(), want)
        same("t", dt.get(), t), same("p", dp.get(), p)
        assert pub.get()[0] == tn
        if offs[2] == 0:
            ok(eng, "trk_cgls_p_update_to", n, dt.ptr, dp.ptr, dp.ptr, gn.ptr, 3, gold.ptr, None)
            same(f"p_update_to in place {n} {offs}", dp.get(), want)
            dp = FV(eng, n, p, offs[1])
            ok(eng, "trk_cgls_p_update", n, dt.ptr, dp.ptr, gn.ptr, 3, gold.ptr, None)
            same(f"p_update {n} {offs}", dp.get(), want)
            same("t", dt.get(), t)


# ------------------------------------------------------------------------------------------------------------ x and [x, p] updates
def x_call(eng, kind, n, st_src, b_src, dx, dp, dt, dxn, xtp, NP, cap, nb):
    """trk_cgls_x_update (kind 'x': step = S(gamma) / S(delta)) or trk_cgls_xp_update ('xp': finished gamma_old, delta; gamma_new a
    source); returns the status."""
    (gm, dl), (gn, pub) = st_src, b_src
    if kind == "x":
        return eng.lib.trk_cgls_x_update(n, gm.ptr, gm.n, dl.ptr, dl.n, dx.ptr, dp.ptr, dxn.ptr, xtp, None, None, NP.ptr(), cap,
                                         ctypes.byref(nb), eng.stream())
    return eng.lib.trk_cgls_xp_update(n, gm.ptr, dl.ptr, gn.ptr, gn.n, dx.ptr, dp.ptr, dt.ptr, dxn.ptr, xtp, pub.ptr(), NP.ptr(), cap,
                                      ctypes.byref(nb), eng.stream())


@pytest.mark.parametrize("kind", ["x", "xp"])
@pytest.mark.parametrize("exact", [True, False])
def test_x_and_xp_updates(eng, cus, exact, kind):
    """Entry-wise equality on every named size, the three norms as raw [block][3] partials, the third exactly 0.0 without x_true; a
    misaligned vector or a capacity one block short is TRK_EINVAL and writes nothing."""
    W = Bars()
    ratio = 1.0 if exact else 3 / 7
    pn, tn, pd, td = C.ratio_sources(ratio, 65, 65)
    gnew, tg = C.partials(65, 3 if exact else 5)          # b = S(gnew) / gamma_old = 1.5 (exact operands) or 5 / 3
    bb = C.step32(tg, tn)
    assert bb == np.float32(1.5 if exact else 5 / 3)
    for name, n in C.sizes(cus).items():
        for with_xt in (True, False):
            if n > 1 << 20 and not with_xt and name != "two-passes+tail":
                continue
            x, p, t, xt = (C.vec(n, exact, k) for k in ("x", "p", "t", "xt"))
            grid = C.stream_grid(n, cus)
            dx, dp, dt, dxt, dxn = FV(eng, n, x), FV(eng, n, p), FV(eng, n, t), FV(eng, n, xt), FV(eng, n)
            if kind == "x":
                st_src, b_src = (Src(eng, pn), Src(eng, pd)), (None, None)
                st = C.step32(tn, td)
            else:
                st_src, b_src = (Src(eng, [tn]), Src(eng, [td])), (Src(eng, gnew), DV(eng, 1))
                st = C.step32(tn, td)
            NP, nb = DV(eng, 3 * grid), ctypes.c_int(-1)
            assert x_call(eng, kind, n, st_src, b_src, dx, dp, dt, dxn, dxt.ptr if with_xt else None, NP, grid, nb) == 0
            xf, _, d = C.x_update(x, p, st)
            same(f"{kind}_update {name} x_new", dxn.get(), xf)
            same("x", dx.get(), x), same("t", dt.get(), t)
            if kind == "xp":
                same(f"xp_update {name} p", dp.get(), C.p_update(t, p, bb))
                assert b_src[1].get()[0] == tg
            else:
                same("p", dp.get(), p)
            assert nb.value == grid
            norms_check(W, f"{kind}_update", NP.get(), grid, xf, d, xt if with_xt else None, exact)
    # refusals: nothing is written
    n = 4099
    grid = C.stream_grid(n, cus)
    x, p, t, xt = (C.vec(n, exact, k) for k in ("x", "p", "t", "xt"))
    st_src = (Src(eng, pn), Src(eng, pd)) if kind == "x" else (Src(eng, [tn]), Src(eng, [td]))
    b_src = (None, None) if kind == "x" else (Src(eng, gnew), DV(eng, 1))
    for which in range(5 if kind == "xp" else 4):        # x, p, x_new, x_true (, t)
        offs = [0] * 5
        offs[which] = 1
        dx, dp, dxn, dxt, dt = (FV(eng, n, h, o) for h, o in zip((x, p, None, xt, t), offs))
        NP, nb = DV(eng, 3 * grid), ctypes.c_int(-1)
        assert x_call(eng, kind, n, st_src, b_src, dx, dp, dt, dxn, dxt.ptr, NP, grid, nb) == EINVAL, which
        assert np.all(dxn.get() == SENTINEL) and np.all(NP.get() == SENTINEL) and nb.value == -1
        same("p", dp.get(), p)
    dx, dp, dxn, dxt, dt = (FV(eng, n, h) for h in (x, p, None, xt, t))
    NP, nb = DV(eng, 3 * grid), ctypes.c_int(-1)
    assert x_call(eng, kind, n, st_src, b_src, dx, dp, dt, dxn, None, NP, grid - 1, nb) == EINVAL
    assert np.all(dxn.get() == SENTINEL) and np.all(NP.get() == SENTINEL) and nb.value == -1
    same("p", dp.get(), p)
    W.flush(f"{kind}-" + ("exact" if exact else "general"))


# ------------------------------------------------------------------------------------------------------------ the batched x update
def xs_run(eng, cus, W, n, count, exact, with_xt, s_slots, where, k_last, alias_x, p_out, xonly=False, tag=""):
    """One call of trk_cgls_xs_update (or _x) against `count` successive one-step references."""
    first = C.xs_first(count, s_slots, where)
    slots = C.xs_slots(count, s_slots, first)
    S0, steps = C.xs_scalars(count, k_last, exact)
    grid = C.stream_grid(n, cus)
    ld = (n + 3) // 4 * 4 + 4
    x, t, xt = (C.vec(n, exact, k) for k in ("x", "t", "xt"))
    dirs = [C.vec(n, exact, "p", c) for c in range(count)]
    # the directions in their slots; the slots not in use hold NaN
    dp = FV(eng, n, None, fill=float("nan"))
    ring = FV(eng, max(s_slots - 1, 1) * ld, None, fill=float("nan"))
    ring_host = np.full(ring.n, np.nan, dtype=np.float32)
    p_host = np.full(n, np.nan, dtype=np.float32)

    def place(slot):
        return (dp.ptr, p_host, 0) if slot == 0 else (ring.ptr + 4 * (slot - 1) * ld, ring_host, (slot - 1) * ld)
    for c, slot in enumerate(slots):
        _, host, o = place(slot)
        host[o:o + n] = dirs[c]
    dp.view.copy_(torch.from_numpy(p_host))
    ring.view.copy_(torch.from_numpy(ring_host))
    dx, dt, dxt = FV(eng, n, x), FV(eng, n, t), FV(eng, n, xt)
    dxn = dx if alias_x else FV(eng, n)
    if p_out == "older" and count == 1:
        p_out = "separate"
    dpo = FV(eng, n)
    po_slot = {"last": slots[-1], "older": slots[0], "separate": None}[p_out]
    po_ptr = dpo.ptr if po_slot is None else place(po_slot)[0]
    assert C.xs_nt(n, count, p_out == "last") == C.stream_nontemporal(n) | (0 if count == 1 else 288 if p_out == "last" else 288 | 1536)
    pn, tn = C.partials(65, 3)                                # gamma_new: 65 partials; b = (float)(total / gamma_{k-1}), any value:
    g_prev = S0[0] if k_last == 1 else S0[5 * (k_last - 1) + 1]   # p_out is two float32 operations, equal for every b
    gn = Src(eng, pn)
    b = C.step32(tn, g_prev)
    S, NP, nb = DV(eng, S0.size, S0), DV(eng, 3 * grid * k_last), ctypes.c_int(-1)
    xtp = dxt.ptr if with_xt else None
    if xonly:
        ok(eng, "trk_cgls_xs_update_x", n, count, k_last, S.ptr(), dx.ptr, dp.ptr, ring.ptr, ld, s_slots, first, dxn.ptr, xtp, NP.ptr(),
           grid, ctypes.byref(nb))
    else:
        ok(eng, "trk_cgls_xs_update", n, count, k_last, S.ptr(), gn.ptr, gn.n, dx.ptr, dp.ptr, ring.ptr, ld, s_slots, first, dt.ptr,
           dxn.ptr, po_ptr, xtp, NP.ptr(), grid, ctypes.byref(nb))
    assert nb.value == grid
    # the references: count one-step updates
    xs, ds = [x], []
    for c in range(count):
        xf, _, d = C.x_update(xs[-1], dirs[c], steps[c])
        xs.append(xf), ds.append(d)
    same(f"xs {tag} x_new", dxn.get(), xs[-1])
    if not alias_x:
        same("x", dx.get(), x)
    same("t", dt.get(), t), same("x_true", dxt.get(), xt)
    P = NP.get().reshape(k_last, grid, 3)
    j0 = k_last - count                                       # iteration j's partials at NP + 3 grid (j - 1)
    assert np.all(P[:j0] == SENTINEL), (tag, "partials of earlier iterations overwritten")
    for c in range(count):
        norms_check(W, f"xs_update<{count}>", P[j0 + c], grid, xs[c + 1], ds[c], xt if with_xt else None, exact)
    Sg = S.get()
    want_S = S0.copy()
    if not xonly:
        want_S[5 * k_last + 1] = tn
        if po_slot is not None:
            _, host, o = place(po_slot)
            host[o:o + n] = C.p_update(t, dirs[-1], b)
        else:
            same(f"xs {tag} p_out", dpo.get(), C.p_update(t, dirs[-1], b))
        gn.unchanged()
    assert np.array_equal(Sg, want_S), (tag, "S", np.flatnonzero(Sg != want_S))
    if xonly or po_slot is not None:
        assert np.all(dpo.get() == SENTINEL)
    # every direction (but the one p_out replaced), the unused slots (NaN) and the ring's padding: bit for bit what they were
    assert np.array_equal(dp.get().view(np.uint32), p_host.view(np.uint32)), (tag, "p")
    assert np.array_equal(ring.get().view(np.uint32), ring_host.view(np.uint32)), (tag, "ring")


@pytest.mark.parametrize("count", range(1, 9))
def test_xs_update(eng, cus, count):
    """C = 1 .. 8 at n = 1027 (a float4 body and a tail of 3): with and without x_true, s_slots = count and 8, slot 0 (p) first, in the
    middle and last, k_last == count (gamma_0 from S[0]) and count + 5, x_new aliasing x or not, p_out the last direction, an older one
    and a buffer of its own; the x-only variant leaves t, p_out and S alone.  Exact and general operands, equality in both."""
    W = Bars()
    idx = 0
    for with_xt in (True, False):
        for s_slots in (count, 8):
            for where in ("first", "middle", "last"):
                if C.xs_first(count, s_slots, where) is None:
                    continue
                for exact in (True, False):
                    for k_last in (count, count + 5):                  # crossed with exact; the aliases cycle with periods 2 x 4 and 3
                        alias_x = (idx // 4) % 2 == 0
                        p_out = ("last", "older", "separate")[idx % 3]
                        tag = f"C={count} xt={with_xt} slots={s_slots} p {where} k_last={k_last} alias={alias_x} p_out={p_out} exact={exact}"
                        xs_run(eng, cus, W, 1027, count, exact, with_xt, s_slots, where, k_last, alias_x, p_out, tag=tag)
                        xs_run(eng, cus, W, 1027, count, exact, with_xt, s_slots, where, k_last, alias_x, p_out, xonly=True,
                               tag=tag + " x-only")
                        idx += 1
    W.flush(f"xs-{count}")


@pytest.mark.parametrize("size", ["two-passes+tail", "nt-stores+3"])
def test_xs_update_large(eng, cus, size):
    """A second grid-stride pass, and 11 x 2^20 + 3 floats: the non-temporal store of x', and with p_out in another slot the hinted
    loads of every direction and the hinted store of p_out (bits 256 | 512 | 1024)."""
    W = Bars()
    n = {**C.sizes(cus), **C.nt_sizes()}[size]
    assert (C.stream_nontemporal(n) != 0) == (size == "nt-stores+3")
    xs_run(eng, cus, W, n, 3, False, True, 3, "middle", 3, True, "older", tag=size)
    if size == "two-passes+tail":
        xs_run(eng, cus, W, n, 2, True, False, 8, "last", 7, False, "last", tag=size)
        xs_run(eng, cus, W, n, 2, False, True, 2, "first", 7, False, "separate", xonly=True, tag=size + " x-only")
    W.flush(f"xs-{size}")


# ------------------------------------------------------------------------------------------------------------ non-temporal variants
@pytest.mark.parametrize("size", ["nt-4", "nt-stores+3", "nt-loads+3"])
def test_nontemporal(eng, cus, size):
    """(11 << 20) - 4: the last size without hints; (11 << 20) + 3: x' stored non-temporally (k_cgls_update, k_cgls_xp_update);
    (20 << 20) + 3: x and t loaded non-temporally as well (k_cgls_xp_update).  General operands, equality entry by entry."""
    W = Bars()
    n = C.nt_sizes()[size]
    nt = C.stream_nontemporal(n)
    assert nt == {"nt-4": 0, "nt-stores+3": 195, "nt-loads+3": 243}[size]
    ratio = 3 / 7
    pn, tn, pd, td = C.ratio_sources(ratio, 65, 65)
    st = C.step32(tn, td)
    x, p, t = (C.vec(n, False, k) for k in "xpt")
    grid = C.stream_grid(n, cus)
    xf, _, d = C.x_update(x, p, st)
    dx, dp, dt, dxn = FV(eng, n, x), FV(eng, n, p), FV(eng, n, t), FV(eng, n)
    NP, nb, pub = DV(eng, 3 * grid), ctypes.c_int(-1), DV(eng, 1)
    s_tn, s_td, s_pn, s_pd = Src(eng, [tn]), Src(eng, [td]), Src(eng, pn), Src(eng, pd)
    gnew, tg = C.partials(65, 5)
    s_gn, bb = Src(eng, gnew), C.step32(tg, tn)                      # b = 5 / 3
    ok(eng, "trk_cgls_xp_update", n, s_tn.ptr, s_td.ptr, s_gn.ptr, 65, dx.ptr, dp.ptr, dt.ptr, dxn.ptr, None,
       pub.ptr(), NP.ptr(), grid, ctypes.byref(nb))
    same(f"xp_update {size} x_new", dxn.get(), xf)
    same(f"xp_update {size} p", dp.get(), C.p_update(t, p, bb))
    norms_check(W, "xp_update", NP.get(), grid, xf, d, None, False)
    if size != "nt-loads+3":
        m = 777
        r, w = C.vec(m, False, "r"), C.vec(m, False, "w")
        dp, dxn, dr, dw = FV(eng, n, p), FV(eng, n), FV(eng, m, r), FV(eng, m, w)
        NP = DV(eng, 3 * grid)
        ok(eng, "trk_cgls_update_xr_src", n, m, s_pn.ptr, 65, s_pd.ptr, 65, dx.ptr, dp.ptr, dxn.ptr, dr.ptr, dw.ptr, None,
           None, NP.ptr(), grid, ctypes.byref(nb))
        same(f"update_xr {size} x_new", dxn.get(), xf)
        same(f"update_xr {size} r", dr.get(), C.r_update(r, w, st))
        norms_check(W, "update_xr", NP.get(), grid, xf, d, None, False)
        dpo = FV(eng, n)
        ok(eng, "trk_cgls_p_update_to", n, dt.ptr, dp.ptr, dpo.ptr, s_gn.ptr, 65, s_tn.ptr, None)
        same(f"p_update_to {size}", dpo.get(), C.p_update(t, p, bb))
    W.flush(size)


# ------------------------------------------------------------------------------------------------------------ the contraction contract
def test_x_update_is_one_rounding_everywhere(eng, cus):
    """Which form of x' (and of the direction p') every kernel computes, on general operands at n = 4099 (a float4 body of 4096 and a tail of 3 whose operands are
    copies of body elements on which the two forms differ): ALL of them the fused form fl32(x + step p), body and tail alike —
    never fl32(x + fl32(step p)); likewise p' = fl32(t + b p).  A kernel, or a tail, compiled the other way fails here by name."""
    n, body = 4099, 4096
    x, p, t, r, w = (C.vec(n, False, k) for k in "xptrw")
    S0, steps = C.xs_scalars(8, 8, False)
    st = steps[0]
    fused, two, _ = C.x_update(x, p, st)
    pick = np.flatnonzero(fused[:body] != two[:body])[:3]
    assert pick.size == 3
    x[body:], p[body:] = x[pick], p[pick]
    fused, two, _ = C.x_update(x, p, st)
    differ = fused != two
    assert differ[body:].all() and differ[:body].sum() > body // 10
    # the direction update p' = fl32(t + b p) with b = step: the tail's t from body elements that tell its two forms apart
    for j in range(body, n):
        pj = np.full(body, p[j], dtype=np.float32)
        t[j] = t[np.flatnonzero(C.p_update(t[:body], pj, st) != C.p_update_two(t[:body], pj, st))[0]]
    pf, p2 = C.p_update(t, p, st), C.p_update_two(t, p, st)
    pdiffer = pf != p2
    assert pdiffer[body:].all() and pdiffer[:body].sum() > body // 10
    grid = C.stream_grid(n, cus)
    g, dl = float(S0[0]), float(S0[5])
    assert C.step32(g, dl) == st
    seen = {}
    sg, sd = Src(eng, [g]), Src(eng, [dl])

    def judge(kernel, got, fused=fused, two=two, differ=differ):
        for part, sl in (("body", slice(0, body)), ("tail", slice(body, n))):
            assert differ[sl].any(), (kernel, part, "no element tells the two forms apart")
            gf, g2 = np.array_equal(got[sl], fused[sl]), np.array_equal(got[sl][differ[sl]], two[sl][differ[sl]])
            seen[f"{kernel} {part}"] = "fused" if gf else "two roundings" if g2 else "neither"

    def fresh(off=0, tt=None):
        return (FV(eng, n, x, off), FV(eng, n, p), FV(eng, n, t if tt is None else tt), FV(eng, n), DV(eng, 3 * grid * 8),
                ctypes.c_int(-1))
    for vec_on in (True, False):
        dx, dp, dt, dxn, NP, nb = fresh(0 if vec_on else 1)
        dr, dw = FV(eng, n, r), FV(eng, n, w)
        ok(eng, "trk_cgls_update_xr_src", n, n, sg.ptr, 1, sd.ptr, 1, dx.ptr, dp.ptr, dxn.ptr, dr.ptr, dw.ptr, None, None,
           NP.ptr(), grid, ctypes.byref(nb))
        judge(f"k_cgls_update<VEC={int(vec_on)}>", dxn.get())
    dx, dp, dt, dxn, NP, nb = fresh()
    ok(eng, "trk_cgls_x_update", n, sg.ptr, 1, sd.ptr, 1, dx.ptr, dp.ptr, dxn.ptr, None, None, None, NP.ptr(), grid,
       ctypes.byref(nb))
    judge("k_cgls_x_update", dxn.get())
    dx, dp, dt, dxn, NP, nb = fresh()
    sgn = Src(eng, [float(st) * g])                         # gamma_new / gamma_old == step exactly: b = step
    assert C.step32(float(st) * g, g) == st
    ok(eng, "trk_cgls_xp_update", n, sg.ptr, sd.ptr, sgn.ptr, 1, dx.ptr, dp.ptr, dt.ptr, dxn.ptr, None, None,
       NP.ptr(), grid, ctypes.byref(nb))
    judge("k_cgls_xp_update", dxn.get())
    judge("k_cgls_xp_update p'", dp.get(), pf, p2, pdiffer)
    for vec_on in (True, False):
        dx, dp, dt, dxn, NP, nb = fresh()
        dpo = FV(eng, n, None, 0 if vec_on else 1)
        ok(eng, "trk_cgls_p_update_to", n, dt.ptr, dp.ptr, dpo.ptr, sg.ptr, 1, sd.ptr, None)
        judge(f"k_cgls_p_update<VEC={int(vec_on)}> p'", dpo.get(), pf, p2, pdiffer)
    # the batched kernel, every C: the first direction is p, the others make further general steps; both chains as references
    ldr = (n + 3) // 4 * 4 + 4
    others = [C.vec(n, False, "p", c) for c in range(1, 8)]
    keep = []
    GN = 11.0                                               # gamma_new: 11 / gamma_{C-1} is no power of two for gamma = 3 .. 10
    for count in range(1, 9):
        f, s2 = x, x
        for c in range(count):
            pc = p if c == 0 else others[c - 1]
            f, s2 = C.x_update(f, pc, steps[c])[0], C.x_update(s2, pc, steps[c])[1]
        # p_out = fmaf(b, p_C, t) with b = (float)(GN / gamma_{C-1}): the tail's t from body elements that tell its two forms apart for THIS b
        pc, bc = (p if count == 1 else others[count - 2]), C.step32(GN, S0[0] if count == 1 else S0[5 * (count - 1) + 1])
        tc = t.copy()
        for j in range(body, n):
            pj = np.full(body, pc[j], dtype=np.float32)
            tc[j] = t[np.flatnonzero(C.p_update(t[:body], pj, bc) != C.p_update_two(t[:body], pj, bc))[0]]
        for xonly in (False, True):
            dx, dp, dt, dxn, NP, nb = fresh(tt=tc)
            S = DV(eng, S0.size, S0)
            ring = FV(eng, 7 * ldr, None, fill=float("nan"))
            for c, o in enumerate(others):
                ring.view[c * ldr:c * ldr + n].copy_(torch.from_numpy(o))
            if xonly:
                ok(eng, "trk_cgls_xs_update_x", n, count, count, S.ptr(), dx.ptr, dp.ptr, ring.ptr, ldr, 8, 0, dxn.ptr, None, NP.ptr(), grid,
                   ctypes.byref(nb))
            else:
                dpo = FV(eng, n)
                keep.append(Src(eng, [GN]))
                ok(eng, "trk_cgls_xs_update", n, count, count, S.ptr(), keep[-1].ptr, 1, dx.ptr, dp.ptr, ring.ptr, ldr, 8, 0, dt.ptr,
                   dxn.ptr, dpo.ptr, None, NP.ptr(), grid, ctypes.byref(nb))
            d2 = f != s2
            assert d2[body:].any() and d2[:body].any()
            judge(f"k_cgls_xs_update<C={count},XONLY={int(xonly)}>", dxn.get(), f, s2, d2)
            if not xonly:
                qf, q2 = C.p_update(tc, pc, bc), C.p_update_two(tc, pc, bc)
                qd = qf != q2
                assert qd[:body].any() and qd[body:].all()
                judge(f"k_cgls_xs_update<C={count}> p'", dpo.get(), qf, q2, qd)
    for name, form in sorted(seen.items()):
        print(f"{name}: {form}")
    wrong = {k: v for k, v in seen.items() if v != "fused"}
    assert not wrong, wrong
