"""The four kernels of the one-reduction CGLS (csrc/cgls_sharded.hip) entry by entry against float64 on the same float32 operands, on
every path the sizes, the alignment, the aliasing, `first`, w = NULL and the number of gamma partials select.  Operands, references,
bounds and launch plans: tests/sharded_cases.py on top of tests/vec_cases.py (checked on the CPU by tests/test_sharded_cases_host.py).
All calls go through the C ABI (eng.lib) on crafted vectors; nothing comes from a solve.

Exact operands (eighths, alpha = 1 / 4, beta = 1 / 2, gamma partials that are multiples of 2^-4): every vector entry, every sum, delta
and G4[0] must EQUAL the reference — so the one-workgroup form, the multi-block form and trk_dot_pair equal each other.
General operands: every vector entry still at 0 ulp (alpha is unambiguous by the choice of G4, sharded_cases.scalars), sums within
(n + 4096) 2^-53 S, delta within 4 x 2^-53 (|qq| + 2 |beta_d qw| + beta_d^2 ww); each as a fraction of its bound through conftest.bar
(profiles/cgls_sharded/bars.txt).

Every vector lives between 8 guard floats, every double output between 4 guard doubles, unchanged after the call; outputs start as
NaN or a sentinel; the gamma partials sit between two slots of 2^40.  Before a case runs, its launch plan on THIS device's
compute-unit count must show the branch it is named for.

  entry point                  kernel<template arguments>                     reached by
  trk_dot_pair                 k_dot_pair<VEC = 1>; k_finalize                dot_pair (every m, exact and general, w given / NULL)
                               k_dot_pair<VEC = 0>                            dot_pair (q or w one float off, exact and general)
  trk_cgls_sharded_scalars     k_sharded_scalars<VEC = 1>                     sharded_scalars (m <= 2^14 and n_g <= 2^16, exact and general)
                               k_sharded_scalars<VEC = 0>                     sharded_scalars_misaligned (m = 1027)
                               k_dot_pair<VEC = 1>; k_sharded_finalize        sharded_scalars (m > 2^14 or n_g = 65537; nblocks = 1 at m = 3)
                               k_dot_pair<VEC = 0>; k_sharded_finalize        sharded_scalars_misaligned (m = 16388)
  trk_cgls_sharded_update      k_cgls_sharded_update<HAS_XT = 1, VEC = 1>     sharded_update (every (n, m), first 1 / 0, in place), chained_launches
                               k_cgls_sharded_update<HAS_XT = 0, VEC = 1>     sharded_update, sharded_update_misaligned[7], x_update_is_one_rounding[aligned]
                               k_cgls_sharded_update<HAS_XT = 1, VEC = 0>     sharded_update_misaligned[0 .. 7]
                               k_cgls_sharded_update<HAS_XT = 0, VEC = 0>     sharded_update_misaligned[0 .. 6], x_update_is_one_rounding[misaligned]
  all three                    (nothing launched)                             refusals
Every row is reached with exact and with general operands.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sharded_cases as C
import vec_cases as V
from conftest import bar

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
G_SENTINEL = 6.02214076e23          # what G4 holds before trk_cgls_sharded_scalars
GUARD, GUARD_D = 8, 4
EINVAL = -1
NAN = float("nan")


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
    """n device floats `off` floats behind a 16-byte boundary, between guard floats; payload `host`, else `fill`."""

    def __init__(self, eng, n, host=None, off=0, fill=NAN):
        self.n, self.lo = n, GUARD + off
        self.buf = torch.full((self.lo + n + GUARD,), SENTINEL, dtype=torch.float32, device=eng.device)
        self.view = self.buf[self.lo:self.lo + n]
        self.ptr = self.buf.data_ptr() + 4 * self.lo
        assert (self.ptr % 16 == 0) == (off % 4 == 0)
        if host is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)))
        else:
            self.view.fill_(fill)

    def get(self):
        h = self.buf.cpu().numpy()
        assert np.all(h[:self.lo] == SENTINEL) and np.all(h[self.lo + self.n:] == SENTINEL), "guard floats overwritten"
        return h[self.lo:self.lo + self.n]


class DV:
    """m device doubles between guard doubles, SENTINEL unless given."""

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


class Bars(dict):
    def see(self, name, got, R):
        """A scalar against its reference: equal (bound None) or within the bound, the worst ratio kept per name."""
        print(f"{name}: got {float(got)!r} ref {float(R.ref)!r} bound {R.bound!r}")
        err = float(R.error(got))
        if R.bound is None:
            assert err == 0.0, (name, "must be equal", got, R.ref)
            return
        assert err <= R.bound, (name, got, R.ref, err, R.bound)
        self[name] = max(self.get(name, 0.0), err / R.bound if R.bound > 0 else 0.0)

    def flush(self, tag):
        for name, v in sorted(self.items()):
            bar(f"sharded.entrywise[{name}:{tag}]", v, 1.0)


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same(name, got, want):
    """Entry-wise equality of float32 vectors, to the bit (-0.0 and 0.0 apart; NaN equal to the same NaN)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (name, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def kind(exact):
    return "exact" if exact else "general"


# ------------------------------------------------------------------------------------------------------------ trk_dot_pair
NAMES3 = ("qq", "qw", "ww")


def pair_check(W, name, got3, q, w, exact):
    for j, R in enumerate(C.dot_pair(q, w, exact)):
        W.see(f"{name}.{NAMES3[j]}", got3[j], R)
    if w is None:
        assert np.array_equal(bits64(got3[1:]), bits64([0.0, 0.0])), (name, "w = NULL: 0, 0", got3)


@pytest.mark.parametrize("exact", [True, False])
def test_dot_pair(eng, cus, exact):
    """Every m (0: zeros), w given and NULL, and q or w one float off a 16-byte boundary at a one-block and a 17-block size."""
    W = Bars()
    for name, m in C.m_sizes(cus).items():
        q, w = C.vec(m, exact, "q"), C.vec(m, exact, "w")
        for offs in ((0, 0), (1, 0), (0, 1)) if m in (1027, 16388) else ((0, 0),):
            for with_w in (True, False):
                if not with_w and offs[1]:
                    continue
                C.expect(C.stream_plan(m, cus, [4 * o for o in (offs if with_w else offs[:1])]), vec=not any(offs),
                         grid=C.stream_grid(m, cus))
                dq, dw, out = FV(eng, m, q, offs[0]), FV(eng, m, w, offs[1]), DV(eng, 3)
                ok(eng, "trk_dot_pair", dq.ptr, dw.ptr if with_w else None, m, out.ptr())
                pair_check(W, "dot_pair" + ("" if not any(offs) else ".scalar"), out.get(), q, w if with_w else None, exact)
                same("q", dq.get(), q), same("w", dw.get(), w)
    W.flush(kind(exact))


# ------------------------------------------------------------------------------------------------------------ trk_cgls_sharded_scalars
def scalars_run(eng, cus, W, m, n_g, exact, with_w, form, offs=(0, 0), unit=3):
    """One call on a G4 of sentinels, and a second identical one: G4[0] untouched (n_g = 0) or the exact total, G4[1:] the three sums
    (0, 0 without w), the same bits twice; in exact cases trk_dot_pair on the same vectors gives the same three doubles."""
    used = offs if with_w else offs[:1]
    plan = C.expect(C.scalars_plan(m, n_g, cus, [4 * o for o in used]), form=form, vec=not any(used))
    q, w = C.vec(m, exact, "q"), C.vec(m, exact, "w")
    src, total = C.gamma_source(n_g, unit)
    dq, dw, dsrc = FV(eng, m, q, offs[0]), FV(eng, m, w, offs[1]), DV(eng, src.size, src)
    tag = f"scalars.{plan['form']}" + ("" if plan["vec"] else ".scalar")
    outs = []
    for rep in range(2):
        G = DV(eng, 4, [G_SENTINEL] * 4)
        ok(eng, "trk_cgls_sharded_scalars", dq.ptr, dw.ptr if with_w else None, m, dsrc.ptr(1) if (n_g or with_w) else None, n_g, G.ptr())
        outs.append(G.get())
    got = outs[0]
    assert np.array_equal(bits64(outs[0]), bits64(outs[1])), (tag, m, n_g, "two identical calls differ", outs)
    if n_g == 0:
        assert bits64(got[:1])[0] == bits64([G_SENTINEL])[0], (tag, m, "n_gamma = 0 must leave G4[0]", got[0])
    else:
        assert got[0] == total, (tag, m, n_g, "G4[0]", got[0], total)
    pair_check(W, tag, got[1:], q, w if with_w else None, exact)
    assert np.array_equal(dsrc.get(), src), "the gamma partials were written to"
    same("q", dq.get(), q), same("w", dw.get(), w)
    if exact:
        out = DV(eng, 3)
        ok(eng, "trk_dot_pair", dq.ptr, dw.ptr if with_w else None, m, out.ptr())
        assert np.array_equal(bits64(out.get()), bits64(got[1:])), (tag, m, "trk_dot_pair and the scalars kernel differ")


def scalars_cases(cus):
    """(m, n_g, form): every n_g at m = 1027 and 16388, every m at n_g = 0, 3 and 1025, and the one-row finalize (m = 3, n_g = 65537)."""
    S, plans = C.m_sizes(cus), C.n_gamma_plans(cus)
    cases = [(1027, n_g, plans[n_g]["form"]) for n_g in C.N_GAMMA] + [(16388, n_g, "multi") for n_g in C.N_GAMMA]
    for m in S.values():
        for n_g in (0, 3, 1025):
            cases.append((m, n_g, "one_block" if m <= 1 << 14 else "multi"))
    cases.append((C.NG_ONE_ROW_M, 65537, "multi"))
    return list(dict.fromkeys(cases))


@pytest.mark.parametrize("exact", [True, False])
def test_sharded_scalars(eng, cus, exact):
    """Both forms on both sides of both thresholds (m = 2^14 | 2^14 + 1, n_g = 2^16 | 2^16 + 1), w given and NULL."""
    W = Bars()
    cases = scalars_cases(cus)
    assert {f for _, _, f in cases} == {"one_block", "multi"}
    for i, (m, n_g, form) in enumerate(cases):
        for with_w in (True, False):
            scalars_run(eng, cus, W, m, n_g, exact, with_w, form, unit=3 if i % 2 else 7)
    W.flush(kind(exact))


@pytest.mark.parametrize("exact", [True, False])
def test_sharded_scalars_misaligned(eng, cus, exact):
    """q or w one float off: the scalar loops of k_sharded_scalars (m = 1027) and of k_dot_pair before the finalize (m = 16388);
    without w its alignment does not count."""
    W = Bars()
    for m, form in ((1027, "one_block"), (16388, "multi")):
        for n_g in (0, 3, 1025):
            scalars_run(eng, cus, W, m, n_g, exact, True, form, offs=(1, 0))
            scalars_run(eng, cus, W, m, n_g, exact, True, form, offs=(0, 1))
            scalars_run(eng, cus, W, m, n_g, exact, False, form, offs=(1, 0))
            scalars_run(eng, cus, W, m, n_g, exact, False, form, offs=(0, 1))        # w NULL: the float4 body
    W.flush("misaligned-" + kind(exact))


# ------------------------------------------------------------------------------------------------------------ trk_cgls_sharded_update
OPERANDS = ("x", "p", "t", "x_new", "r", "q", "w", "x_true")


def g4_set(first, exact, i=0):
    if exact:
        E = C.EXACT_FIRST if first else C.EXACT_LATER
        return E["G4"], E["gprev"]
    return (C.GENERAL_FIRST[i % len(C.GENERAL_FIRST)], None) if first else C.GENERAL_LATER[i % len(C.GENERAL_LATER)]


@functools.lru_cache(maxsize=4)
def update_case(n, m, first, exact, i):
    """(operands, reference) of one update, shared between the calls that differ in alignment, x_true and aliasing only."""
    x, p, t, xt = (C.vec(n, exact, k) for k in ("x", "p", "t", "xt"))
    r, q, w = (C.vec(m, exact, k) for k in ("r", "q", "w"))
    G4, gprev = g4_set(first, exact, i)
    return (x, p, t, xt, r, q, w), C.update(G4, gprev, first, x, p, t, r, q, w, xt, exact)


def update_call(eng, n, m, G4, gprev, first, ptrs, xtp, cap):
    """The call itself; ptrs: x, p, t, x_new, r, q, w.  Returns (rc, published delta, published gamma, NP, n_blocks, the G4 and gprev buffers)."""
    DG, dgp = DV(eng, 4, G4), (None if gprev is None else DV(eng, 1, [gprev]))
    pubd, pubg, NP, nb = DV(eng, 1), DV(eng, 1), DV(eng, 3 * max(cap, 0) + 3), ctypes.c_int(-1)
    rc = eng.lib.trk_cgls_sharded_update(n, m, DG.ptr(), None if dgp is None else dgp.ptr(), int(first), *ptrs, xtp, pubd.ptr(),
                                         pubg.ptr(), NP.ptr(), cap, ctypes.byref(nb), eng.stream())
    return rc, pubd, pubg, NP, nb, DG, dgp


def update_run(eng, cus, W, tag, n, m, first, with_xt, exact, i=0, offs=(0,) * 8, inplace=False, case=None):
    """One call of trk_cgls_sharded_update and every check of it; returns the device's x'."""
    (x, p, t, xt, r, q, w), R = case or update_case(n, m, first, exact, i)
    G4, gprev = g4_set(first, exact, i)
    used = offs if with_xt else offs[:7]
    pn, pm = C.update_plan(n, m, cus, [4 * o for o in used])
    grid = C.stream_grid(max(n, m), cus)
    C.expect(pn, vec=not any(used), grid=grid), C.expect(pm, grid=grid)
    dx, dt, dr, dq, dxt = FV(eng, n, x, offs[0]), FV(eng, n, t, offs[2]), FV(eng, m, r, offs[4]), FV(eng, m, q, offs[5]), FV(eng, n, xt, offs[7])
    dp, dw = FV(eng, n, None if first else p, offs[1]), FV(eng, m, None if first else w, offs[6])      # first: NaN, not to be read
    dxn = dx if inplace else FV(eng, n, None, offs[3])
    cap = grid + 2
    rc, pubd, pubg, NP, nb, DG, dgp = update_call(eng, n, m, G4, gprev, first, (dx.ptr, dp.ptr, dt.ptr, dxn.ptr, dr.ptr, dq.ptr, dw.ptr),
                                                  dxt.ptr if with_xt else None, cap)
    assert rc == 0, (tag, eng.lib.trk_last_error())
    assert nb.value == grid, (tag, "n_blocks", nb.value, grid)
    P = NP.get()
    assert np.all(P[3 * grid:] == SENTINEL), (tag, "norm_partials beyond 3 n_blocks written")
    P = P[:3 * grid].reshape(grid, 3)
    sc = R["sc"]
    W.see(f"{tag}.delta", pubd.get()[0], sc.delta)
    assert bits64(pubg.get())[0] == bits64([G4[0]])[0], (tag, "publish_gamma")
    assert np.array_equal(bits64(DG.get()), bits64(G4)) and (dgp is None or dgp.get()[0] == gprev), (tag, "G4 / gamma_prev written to")
    got_x = dxn.get()
    same(f"{tag} p'", dp.get(), R["p"]), same(f"{tag} w'", dw.get(), R["w"])
    same(f"{tag} x'", got_x, R["x"]), same(f"{tag} r'", dr.get(), R["r"])
    same("t", dt.get(), t), same("q", dq.get(), q), same("x_true", dxt.get(), xt)
    if not inplace:
        same("x", dx.get(), x)
    for j in range(3):
        if j == 2 and not with_xt:
            assert np.array_equal(bits64(P[:, 2]), bits64(np.zeros(grid))), (tag, "third norm without x_true")
        else:
            W.see(f"{tag}.s{j}", P[:, j].astype(V.WIDE).sum(), R["norms"][j])
    return got_x


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("shape", range(len(C.NM_SHAPES)))
def test_sharded_update(eng, cus, shape, exact):
    """Every (n, m) x first 1 / 0 x x_true given / NULL, and x_new == x against x_new distinct.  With first = 1, p and w hold NaN on
    entry and come back as t and q."""
    W = Bars()
    n, m = C.nm_shapes(cus)[shape]
    for first in (True, False):
        for with_xt in (True, False):
            tag = f"update<XT={int(with_xt)},VEC=1>"
            apart = update_run(eng, cus, W, tag, n, m, first, with_xt, exact, i=shape)
            if with_xt != first:
                same("x_new == x", update_run(eng, cus, W, tag, n, m, first, with_xt, exact, i=shape, inplace=True), apart)
    W.flush(f"{n}x{m}-" + kind(exact))


@pytest.mark.parametrize("which", range(8))
def test_sharded_update_misaligned(eng, cus, which):
    """Each of x, p, t, x_new, r, q, w, x_true alone one float off a 16-byte boundary: the scalar loops form the same bits; x_true
    off counts only when it is given."""
    W = Bars()
    offs = tuple(int(k == which) for k in range(8))
    n, m = 1027, 515
    for exact in (True, False):
        for first in (True, False):
            for with_xt in (True, False):
                vec_on = which == 7 and not with_xt
                update_run(eng, cus, W, f"update<XT={int(with_xt)},VEC={int(vec_on)}>", n, m, first, with_xt, exact, i=which, offs=offs)
    W.flush(f"{OPERANDS[which]}-off")


@pytest.mark.parametrize("path", ["aligned", "misaligned"])
def test_x_update_is_one_rounding(eng, cus, path):
    """x' = fmaf(alpha, p', x), never fl32(x + fl32(alpha p')): general operands at n = 1027 whose last 3 entries are copies of body
    entries on which the two forms differ.  Aligned: a float4 body of 1024 and a scalar tail of 3, judged separately; misaligned: the
    scalar loop over all of it."""
    n, m, body = 1027, 515, 1024
    x, p, t = C.one_rounding_case(n)
    r, q, w, xt = C.vec(m, False, "r"), C.vec(m, False, "q"), C.vec(m, False, "w"), C.vec(n, False, "xt")
    seen = {}
    for first in (True,):                                   # p' = t: the operands of x' are the crafted ones
        G4, gprev = g4_set(first, False, 0)
        R = C.update(G4, gprev, first, x, p, t, r, q, w, xt, False)
        differ = R["x"] != R["x2"]
        offs = (0,) * 8 if path == "aligned" else (1,) + (0,) * 7
        got = update_run(eng, cus, Bars(), f"one-rounding {path}", n, m, first, False, False, offs=offs, case=((x, p, t, xt, r, q, w), R))
        for part, sl in (("body", slice(0, body)), ("tail", slice(body, n))):
            assert differ[sl].any() and differ[body:].all(), (part, "no entry tells the two forms apart")
            fused = np.array_equal(got[sl], R["x"][sl])
            two = np.array_equal(got[sl][differ[sl]], R["x2"][sl][differ[sl]])
            seen[f"first={int(first)} {path} {part}"] = "fused" if fused else "two roundings" if two else "neither"
    for name, form in sorted(seen.items()):
        print(f"k_cgls_sharded_update {name}: {form}")
    wrong = {k: v for k, v in seen.items() if v != "fused"}
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("what", ["x_new == p", "x_new == t", "gamma_prev NULL", "capacity", "negative n", "negative m"])
def test_update_refusals(eng, cus, what):
    """TRK_EINVAL with a message, and nothing launched: outputs, guards and operands are what they were."""
    n, m = 1027, 515
    grid = C.stream_grid(n, cus)
    assert grid == 2
    x, p, t, r, q, w = (C.vec(n if k in "xpt" else m, True, k) for k in "xptrqw")
    dx, dp, dt, dxn, dr, dq, dw = FV(eng, n, x), FV(eng, n, p), FV(eng, n, t), FV(eng, n), FV(eng, m, r), FV(eng, m, q), FV(eng, m, w)
    xn = {"x_new == p": dp, "x_new == t": dt}.get(what, dxn)
    G4, gprev = C.EXACT_LATER["G4"], C.EXACT_LATER["gprev"]
    rc, pubd, pubg, NP, nb, DG, dgp = update_call(eng, -1 if what == "negative n" else n, -1 if what == "negative m" else m, G4,
                                                  None if what == "gamma_prev NULL" else gprev, False,
                                                  (dx.ptr, dp.ptr, dt.ptr, xn.ptr, dr.ptr, dq.ptr, dw.ptr), None,
                                                  grid - 1 if what == "capacity" else grid)
    assert rc == EINVAL, (what, rc)
    msg = eng.lib.trk_last_error().decode()
    want = {"x_new == p": "alias", "x_new == t": "alias", "gamma_prev NULL": "gamma_prev", "capacity": "too small",
            "negative n": "negative", "negative m": "negative"}[what]
    assert "trk_cgls_sharded_update" in msg and want in msg, (what, msg)
    torch.cuda.synchronize()
    assert np.all(np.isnan(dxn.get())) and np.all(NP.get() == SENTINEL) and nb.value == -1
    assert pubd.get()[0] == SENTINEL and pubg.get()[0] == SENTINEL
    for d, h in ((dx, x), (dp, p), (dt, t), (dr, r), (dq, q), (dw, w)):
        same(what, d.get(), h)


def test_scalar_entry_refusals(eng):
    """A negative size, and gamma partials counted but not given: TRK_EINVAL with the entry point's name, outputs untouched."""
    q = FV(eng, 4, C.vec(4, True, "q"))
    out, G = DV(eng, 3), DV(eng, 4, [G_SENTINEL] * 4)
    for name, args in (("trk_dot_pair", (q.ptr, None, -1, out.ptr())), ("trk_cgls_sharded_scalars", (q.ptr, None, -1, None, 0, G.ptr())),
                       ("trk_cgls_sharded_scalars", (q.ptr, None, 4, None, 3, G.ptr()))):
        rc = getattr(eng.lib, name)(*args, eng.stream())
        assert rc == EINVAL and name in eng.lib.trk_last_error().decode(), (name, args, rc)
    torch.cuda.synchronize()
    assert np.all(out.get() == SENTINEL) and np.all(G.get() == G_SENTINEL)


# ------------------------------------------------------------------------------------------------------------ chained launches
def test_chained_launches(eng, cus):
    """Three launches as trk_cgls_iterate_sharded issues them — first, then two later steps — on the exact (1027, 515) case, the slot
    arithmetic mirrored by hand: iteration k publishes delta_k at S[5 k] and gamma_{k-1} at S[0] (k = 1) or S[5 k - 4], reads
    gamma_{k-2} from S[0] (k = 2) or S[5 k - 9], leaves its partials at NP + 3 n_np (k - 1); trk_finalize_batched then sums the three
    rows into S[5 k + 2 .. 5 k + 4].  Everything equals the reference chained the same way."""
    n, m, K = 1027, 515, 3
    n_np = C.stream_grid(max(n, m), cus)
    x0, r0, xt = C.vec(n, True, "x"), C.vec(m, True, "r"), C.vec(n, True, "xt")
    S, NP = DV(eng, 5 * K + 5), DV(eng, 3 * n_np * K)
    dp, dw, dr, dxt = FV(eng, n), FV(eng, m), FV(eng, m, r0), FV(eng, n, xt)
    dx = [FV(eng, n, x0)] + [FV(eng, n) for _ in range(K)]
    x, p, w, r = x0, None, None, r0
    want_S = np.full(5 * K + 5, SENTINEL)
    for k in range(1, K + 1):
        G4 = C.CHAIN[k - 1]
        t, q = C.vec(n, True, "t", k), C.vec(m, True, "q", k)
        R = C.update(G4, None if k == 1 else C.CHAIN[k - 2][0], k == 1, x, p, t, r, q, w, xt, True)
        dt, dq, DG, nb = FV(eng, n, t), FV(eng, m, q), DV(eng, 4, G4), ctypes.c_int(-1)
        row = 5 * k
        gpub, gprev = (0 if k == 1 else row - 4), (0 if k == 2 else row - 9)
        ok(eng, "trk_cgls_sharded_update", n, m, DG.ptr(), None if k == 1 else S.ptr(gprev), int(k == 1), dx[k - 1].ptr, dp.ptr, dt.ptr,
           dx[k].ptr, dr.ptr, dq.ptr, dw.ptr, dxt.ptr, S.ptr(row), S.ptr(gpub), NP.ptr(3 * n_np * (k - 1)), n_np, ctypes.byref(nb))
        assert nb.value == n_np
        for name, d, key in (("p", dp, "p"), ("w", dw, "w"), ("x", dx[k], "x"), ("r", dr, "r")):
            same(f"step {k} {name}", d.get(), R[key])
        want_S[row], want_S[gpub] = R["sc"].delta.ref, G4[0]
        want_S[row + 2:row + 5] = [v.ref for v in R["norms"]]
        x, p, w, r = R["x"], R["p"], R["w"], R["r"]
    assert [5 * k - 4 for k in (2, 3)] == [6, 11] and [5 * k - 9 for k in (3,)] == [6]          # gamma_1: published by 2, read by 3
    ok(eng, "trk_finalize_batched", NP.ptr(), n_np, 3, K, S.ptr(7), 5)
    got = S.get()
    assert np.array_equal(got, want_S), (np.flatnonzero(got != want_S), got, want_S)
    same("x_0", dx[0].get(), x0), same("x_true", dxt.get(), xt)
