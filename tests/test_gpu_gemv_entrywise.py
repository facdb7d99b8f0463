"""The sweeps over the tall-skinny basis (csrc/gemv.hip) entry by entry against float64 / np.longdouble on the same float32
operands, on every path the row layout, the alignment, k and n select.  Operands, references and bounds: tests/gemv_cases.py
(checked on the CPU by tests/test_gemv_cases_host.py).  All calls go through HipEngine / the C ABI.

Exact operands (multiples of 1 / 64, small integers, dyadic weights and coefficients): every order of summation is exact, the
device result must EQUAL the reference.  General operands: within the bounds derived in gemv_cases' docstring; the worst deviation
of every entry point and path is logged as a fraction of its bound (conftest.bar, limit 1).

Row layouts: ld == n (n % 4 == 0); ld = n rounded up to a multiple of 4 with n % 4 = 1, 2, 3 (the 16-byte body AND the scalar
tail; the padding columns hold NaN, so a read beyond n in any row poisons a sum); ld % 4 != 0 (the scalar kernel); ld % 4 == 0 with
one operand of the launcher's `vec` predicate one float off a 16-byte boundary, each in turn.  Every vector lives inside a larger
allocation whose guard floats must be unchanged after the call, and so must the basis, padding included.

Which case reaches which instantiation launched from gemv.hip's C ABI.  VEC on: test_row_layouts[ld, pad1, pad2, pad3] (below: "layouts")
and the cases named; VEC off: test_row_layouts[odd, odd_ld] and test_misaligned_operand[<entry>], every operand of the predicate in turn.

  entry point (launcher)              kernel<template arguments>                VEC on                                   VEC off
  trk_gemv_t, w2 == NULL              k_gemv_t<0, VEC>                          layouts, row_tiles[t], grid_shapes       odd, misaligned[t]
  trk_gemv_t, w2 given                k_gemv_t<1, VEC>                          layouts, weight_squared (c1)             odd, misaligned[t_w1]
  trk_wgram's c2 (launch_gemv_t)      k_gemv_t<2, VEC>                          weight_squared_through_wgram             the same test: odd ld, V / r / w misaligned
  trk_gemv_t_x                        k_gemv_t<0, VEC>, xrow != NULL            layouts, row_tiles[t_x], grid_shapes     odd, misaligned[t_x]
  trk_gemv_t2                         k_gemv_t2<VEC>                            layouts, row_tiles[t2], grid_shapes      odd, misaligned[t2]
  trk_gemv_tn, n_rhs = 3              k_gemv_tr<VEC, 3>                         layouts, row_tiles[tn3], grid_shapes     odd, misaligned[tn3]
  trk_gemv_tn, n_rhs = 4              k_gemv_tr<VEC, 4>                         layouts, row_tiles[tn4], grid_shapes     odd, misaligned[tn4]
  trk_gemv_n, no base, no sumsq       k_gemv_n<false, false, VEC>               layouts                                  odd
  trk_gemv_n, no base, sumsq          k_gemv_n<false, true, VEC>                layouts, row_ladder, nontemporal_loads   odd
  trk_gemv_n, base, no sumsq          k_gemv_n<true, false, VEC>                layouts (k_gemv_n_split: below)          odd, rows_split (misaligned base)
  trk_gemv_n, base, sumsq             k_gemv_n<true, true, VEC>                 layouts, row_ladder, aliased_outputs     odd, misaligned[n]
  trk_gemv_n, base, k >= 12, short n  k_gemv_n_split<true>, den2 == NULL        rows_split_over_the_waves                (16-byte accesses only)
  trk_gemv_n_err                      k_gemv_n<false, true, VEC, true>          layouts, row_ladder                      odd, misaligned[n_err]
  trk_gemv_n_hosty, ref == NULL       k_gemv_n<false, false, VEC, false, YArg>  layouts                                  odd
  trk_gemv_n_hosty, ref given         k_gemv_n<false, true, VEC, true, YArg>    layouts                                  odd, misaligned[n_hosty]
  trk_gemv_n_hosty, k > 128           k_gemv_n<true, ERR, VEC, ERR, YArg>       host_coefficients_beyond_one_launch      —
  trk_gemv_orth_iterate, vn only      k_gemv_orth_iter<VEC, false, false>       layouts (also with chk)                  odd, rows_split (misaligned w)
  ... short n, no chk (image form)    k_gemv_n_split<true>, den2 given          rows_split_over_the_waves                (16-byte accesses only)
  ... with x_next                     k_gemv_orth_iter<VEC, true, false>        layouts (with chk), row_ladder, nontemporal_loads   odd
  ... with x_next and ref             k_gemv_orth_iter<VEC, true, true>         layouts                                  odd, misaligned[orth] (with chk)
  trk_gemv_nt, k <= 8                 k_gemv_nt<8, VEC>                         accept_reject_limits (8), aliased_outputs (5)       aliased_outputs[odd]
  trk_gemv_nt, 9 <= k <= 16           k_gemv_nt<16, VEC>                        layouts (13), accept_reject_limits (9, 16)          odd, misaligned[nt]
  trk_lsqr_damped_update              k_lsqr_damped_update<float, VEC>          lsqr_damped_update (first / later, ref or not)      the same test, each operand misaligned
  any of the above, n >= 11 x 2^20    ld4_nt on the basis rows (nt & 64, 128)   nontemporal_loads                        —
k_scale_fin is reached through the Arnoldi step only and is not covered here; k_lsqr_damped_update<float / double, false> of
lsqr_damped_update_any belongs to ref64.hip's chain (tests/test_gpu_ref64.py).
"""
import numpy as np
import pytest
import torch

import gemv_cases as C
from conftest import bar

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 8                      # floats (a multiple of 4: alignment is that of the allocation) on both sides of every device vector
GUARD_D = 4                    # doubles on both sides of every block of device scalars
CAP = 1024                     # capacity of the error-partial buffers


@pytest.fixture(scope="module")
def eng():
    from trips_py_amd.engine import default_engine
    return default_engine()


def up(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


class Scal:
    """m device doubles between guards."""

    def __init__(self, eng, m, values=None):
        self.S, self.m = eng.scalars(m + 2 * GUARD_D), m
        self.S.t[:] = SENTINEL
        if values is not None:
            self.S.t[GUARD_D:GUARD_D + m] = up(eng, np.asarray(values, dtype=np.float64).reshape(m))

    def ref(self, i=0):
        return self.S.ref(GUARD_D + i)

    def values(self):
        h = self.S.t.cpu().numpy()
        assert np.all(h[:GUARD_D] == SENTINEL) and np.all(h[GUARD_D + self.m:] == SENTINEL), "guard doubles overwritten"
        return h[GUARD_D:GUARD_D + self.m].copy()


class Dev:
    """The operands of a case on the device: a basis of leading dimension ld whose padding is NaN, and vectors, each in an allocation
    of its own between guard floats; the names in `mis` start one float behind a 16-byte boundary."""

    def __init__(self, eng, case, ld=None, mis=(), rows=None):
        self.eng, self.c, self.n = eng, case, case.n
        self.ld = case.n if ld is None else ld
        self.rows = case.rows if rows is None else rows
        self.mis = frozenset(mis)
        self.bufs, self.V, self.snap = {}, None, None
        assert self.ld >= self.n

    def _alloc(self, name, length, fill):
        off = GUARD + (1 if name in self.mis else 0)
        buf = torch.full((off + length + GUARD,), fill, dtype=torch.float32, device=self.eng.device)
        buf[:off] = SENTINEL
        buf[off + length:] = SENTINEL
        self.bufs[name] = (buf, off, length)
        view = buf[off:off + length]
        assert length == 0 or (view.data_ptr() % 16 != 0) == (name in self.mis)
        return view

    def inp(self, name, host=None):
        """The input vector `name` (the case's, or `host`), uploaded anew."""
        if name in self.bufs:
            buf, off, length = self.bufs[name]
            view = buf[off:off + length]
        else:
            view = self._alloc(name, self.n, 0.0)
        view.copy_(up(self.eng, self.c.vec(name) if host is None else host))
        return view

    def out(self, name):
        """An output vector filled with the sentinel."""
        if name in self.bufs:
            buf, off, length = self.bufs[name]
            buf.fill_(SENTINEL)
            return buf[off:off + length]
        return self._alloc(name, self.n, SENTINEL)

    def basis(self):
        if self.V is None:
            flat = self._alloc("V", self.rows * self.ld, float("nan"))
            V2 = flat.view(self.rows, self.ld)
            V2[:, :self.n] = up(self.eng, self.c.V[:self.rows])
            self.V = V2[:, :self.n]
            assert self.V.stride(0) == self.ld
            self.snap = self.bufs["V"][0].clone()
        return self.V

    def commit_row(self, j, vec):
        """V[j] = vec (the new basis vector takes its row); the snapshot follows."""
        self.V[j].copy_(vec)
        self.snap = self.bufs["V"][0].clone()

    def check(self):
        """Guards of every allocation untouched, the basis (NaN padding included) bit for bit what was uploaded."""
        for name, (buf, off, length) in self.bufs.items():
            assert bool((buf[:off] == SENTINEL).all()) and bool((buf[off + length:] == SENTINEL).all()), f"guards of {name} overwritten"
        if self.snap is not None:
            assert torch.equal(self.bufs["V"][0].view(torch.int32), self.snap.view(torch.int32)), "the basis was written to"


class Worst(dict):
    """Checks device results against references; keeps the worst error / bound of the general operands per name."""

    def see(self, name, got, R, exact):
        got = np.asarray(got).reshape(-1)
        assert got.shape == R.ref.shape, (name, got.shape, R.ref.shape)
        err = R.error(got)
        if exact:
            bad = np.flatnonzero(~(err == 0))
            assert bad.size == 0, (name, "exact operands", bad.size, bad[:8], got[bad[:8]], R.ref[bad[:8]])
            return
        bad = np.flatnonzero(~(err <= R.bound))
        assert bad.size == 0, (name, bad.size, bad[:8], got[bad[:8]], R.ref[bad[:8]], R.bound[bad[:8]])
        pos = R.bound > 0
        ratio = float(np.max(err[pos].astype(np.float64) / R.bound[pos])) if pos.any() else 0.0
        print(f"{name}: max error / bound {ratio:.3e}")
        self[name] = max(self.get(name, 0.0), ratio)

    def flush(self, tag):
        for name, v in sorted(self.items()):
            bar(f"gemv.entrywise[{name}:{tag}]", v, 1.0)


# ------------------------------------------------------------------------------------------------------------ references (cached)
def row_dots(c, name, wpow=0):
    """V[j] . weighted(vec(name)) for every row of the case, computed once."""
    return c._get(("dots", name, wpow), lambda: C.dots(c.V[:c.k], C.weighted(c.vec(name), c.w, wpow), c.exact))


def dot_refs(c, k, names, wpow=0, xrow=False):
    """The k dots per right-hand side, concatenated [q k + j] (and xrow . r behind them)."""
    R = [row_dots(c, nm, wpow) for nm in names]
    ref, bound = [r.ref[:k] for r in R], [r.bound[:k] for r in R]
    if xrow:
        x = c._get(("xdot", names[0]), lambda: C.dots(c.vec("xrow")[None, :], c.vec(names[0]), c.exact))
        ref.append(x.ref)
        bound.append(x.bound)
    return C.Ref(np.concatenate(ref), np.concatenate(bound))


def partial_sum(P, nb):
    """The nb raw block partials summed (np.longdouble); the rest of the buffer untouched."""
    p = P.values()
    assert 1 <= nb <= CAP and np.all(p[nb:] == SENTINEL)
    return np.array([C.wide(p[:nb]).sum()])


# ------------------------------------------------------------------------------------------------------------ one call per entry point
def run_t(D, k, W, path, wpow=0):
    c, e = D.c, D.eng
    V, H = D.basis(), Scal(D.eng, k)
    if wpow == 0:
        e.gemv_t(V, k, D.inp("r"), H.ref())
    elif wpow == 1:
        e.gemv_t(V, k, D.inp("r"), H.ref(), w2=D.inp("w", c.w))
    else:                                                               # c1 = V (w r), c2 = V (w^2 r) behind trk_wgram's Gram matrix
        G, C1 = Scal(e, k * k), Scal(e, k)
        e.wgram(V, k, D.inp("w", c.w), D.inp("r"), G.ref(), C1.ref(), H.ref())
        W.see(f"t_w1.{path}", C1.values(), dot_refs(c, k, ["r"], 1), c.exact)
    W.see(f"t_w{wpow}.{path}" if wpow else f"t.{path}", H.values(), dot_refs(c, k, ["r"], wpow), c.exact)


def run_t_x(D, k, W, path):
    H = Scal(D.eng, k + 1)
    D.eng.gemv_t_x(D.basis(), k, D.inp("r"), D.inp("xrow"), H.ref(0), H.ref(k))
    W.see(f"t_x.{path}", H.values(), dot_refs(D.c, k, ["r"], xrow=True), D.c.exact)


def run_t2(D, k, W, path):
    H = Scal(D.eng, 2 * k)
    D.eng.gemv_t2(D.basis(), k, D.inp("r"), D.inp("r2"), H.ref())
    W.see(f"t2.{path}", H.values(), dot_refs(D.c, k, ["r", "r2"]), D.c.exact)


RHS = ("r2", "r", "r4", "r3")                 # (an order of its own: a swap of two right-hand sides shows)


def run_tn(D, k, W, path, R):
    H = Scal(D.eng, R * k)
    D.eng.gemv_tn(D.basis(), k, [D.inp(nm) for nm in RHS[:R]], H.ref())
    W.see(f"tn{R}.{path}", H.values(), dot_refs(D.c, k, RHS[:R]), D.c.exact)


def run_n(D, k, W, path, with_base, with_sumsq, alias=False, a=0.5, s=-2.0):
    """trk_gemv_n; returns the output as stored (device tensor)."""
    c, e = D.c, D.eng
    V, y = D.basis(), c.coef("y")[:k]
    Y = Scal(e, k, y)
    if not with_base:
        a, s = 0.0, 1.0
    base = D.inp("base") if with_base else None
    out = base if alias else D.out("out")
    SS = Scal(e, 1) if with_sumsq else None
    e.gemv_n(V, k, Y.ref(), out, a=a, base=base, s=s, sumsq=SS.ref() if SS else None)
    got = out.cpu().numpy()
    name = f"n{'.base' if with_base else ''}.{path}"
    W.see(name, got, C.combination(c.V[:k], y, a, c.vec("base") if with_base else None, s), c.exact)
    if SS:
        W.see(f"n.sumsq.{path}", SS.values(), C.sum_of_squares(got), c.exact)
    return out


def run_n_err(D, k, W, path, hosty=False, with_ref=True):
    """trk_gemv_n_err / trk_gemv_n_hosty; returns the output as stored."""
    c, e = D.c, D.eng
    V, y = D.basis(), np.ascontiguousarray(c.coef("y")[:k])
    out, P = D.out("out"), Scal(e, CAP)
    ref = D.inp("ref") if with_ref else None
    if hosty:
        nb = e.gemv_n_hosty(V, k, y, out, ref, P.ref() if with_ref else None, CAP if with_ref else 0)
    else:
        Y = Scal(e, k, y)
        nb = e.gemv_n_err(V, k, Y.ref(), out, ref, P.ref(), CAP)
    got = out.cpu().numpy()
    name = "n_hosty" if hosty else "n_err"
    if k <= 128:                                                        # (beyond: rounded to float32 between the launches — exact operands only)
        W.see(f"{name}.{path}", got, C.combination(c.V[:k], y), c.exact)
    else:
        assert c.exact
        W.see(f"{name}.{path}", got, C.combination(c.V[:k], y), True)
    if with_ref:
        W.see(f"{name}.err.{path}", partial_sum(P, nb), C.sum_of_squares(got, c.vec("ref")), c.exact)
    else:
        assert nb == 0 and np.all(P.values() == SENTINEL)
    return out


def run_orth(D, k, W, path, with_x, with_ref=False, with_chk=False):
    """trk_gemv_orth_iterate; returns (vn, x_next, the device scalars y_next) as stored."""
    c, e = D.c, D.eng
    V = D.basis()
    cc, y = c.coef("c")[:k], c.coef("y")[:k + 1]
    Cc, R2 = Scal(e, k, cc), Scal(e, 1, [c.rho2])
    Yn = Scal(e, k + 1, y) if with_x else None
    vn, x = D.out("vn"), (D.out("x") if with_x else None)
    ref = D.inp("ref") if with_ref else None
    P, CH = Scal(e, CAP), (Scal(e, 1) if with_chk else None)
    nb = e.gemv_orth_iterate(V, k, D.inp("w_in"), Cc.ref(), R2.ref(), vn, y_next=Yn.ref() if with_x else None, x_next=x, ref=ref,
                             partials=P.ref() if with_ref else None, capacity=CAP if with_ref else 0, chk=CH.ref() if with_chk else None)
    vn_got = vn.cpu().numpy()
    inv = 1.0 / np.sqrt(c.rho2)
    form = "vn" if not with_x else ("x_ref" if with_ref else "x")
    W.see(f"orth.{form}.vn.{path}", vn_got, C.combination(c.V[:k], cc, 1.0, c.vec("w_in"), -1.0, post=inv), c.exact)
    if with_x:
        x_got = x.cpu().numpy()
        W.see(f"orth.{form}.x.{path}", x_got, C.combination(list(c.V[:k]) + [vn_got], y), c.exact)
    if with_ref:
        W.see(f"orth.err.{path}", partial_sum(P, nb), C.sum_of_squares(x_got, c.vec("ref")), c.exact)
    else:
        assert nb == 0 and np.all(P.values() == SENTINEL)
    if with_chk:
        W.see(f"orth.chk.{path}", CH.values(), C.chk_sum(c.V[:k], cc, c.vec("w_in")), c.exact)
    return vn, x, Yn


def run_nt(D, k, W, path, alias=False):
    c, e = D.c, D.eng
    h = c.coef("h")[:k]
    Hc, Gs = Scal(e, k, h), Scal(e, k)
    w_in = D.inp("w_in")
    w_out = w_in if alias else D.out("w_out")
    e.gemv_nt(D.basis(), k, Hc.ref(), w_in, w_out, Gs.ref())
    got = w_out.cpu().numpy()
    W.see(f"nt.w.{path}", got, C.combination(c.V[:k], h, 1.0, c.vec("w_in"), -1.0), c.exact)
    W.see(f"nt.g.{path}", Gs.values(), C.dots(c.V[:k], got, c.exact), c.exact)


def everything(D, k, W, path):
    """Every entry point over the basis once on the layout of D, and the two bit-for-bit promises of the header."""
    run_t(D, k, W, path)
    run_t(D, k, W, path, wpow=1)
    run_t_x(D, k, W, path)
    run_t2(D, k, W, path)
    run_tn(D, k, W, path, 3)
    run_tn(D, k, W, path, 4)
    plain = None
    for with_base in (False, True):
        for with_sumsq in (False, True):
            out = run_n(D, k, W, path, with_base, with_sumsq)
            if not with_base:
                plain = out.clone()
    for hosty, with_ref in ((False, True), (True, True), (True, False)):
        assert torch.equal(run_n_err(D, k, W, path, hosty, with_ref), plain)       # the sum of trk_gemv_n term for term
    run_nt(D, k, W, path)
    run_orth(D, k, W, path, with_x=False)
    run_orth(D, k, W, path, with_x=False, with_chk=True)
    run_orth(D, k, W, path, with_x=True, with_ref=True)
    vn, x, Yn = run_orth(D, k, W, path, with_x=True, with_chk=True)
    D.check()
    # x_next against trk_gemv_n over the k + 1 stored rows, bit for bit (trk.h)
    vn, x = vn.clone(), x.clone()
    D.commit_row(k, vn)
    out = D.out("out")
    D.eng.gemv_n(D.V, k + 1, Yn.ref(), out)
    assert torch.equal(out, x)
    D.check()


# ------------------------------------------------------------------------------------------------------------ row layouts
LAYOUTS = {"ld": (1028, 1028, "vec"), "pad1": (1029, 1032, "vec"), "pad2": (1030, 1032, "vec"), "pad3": (1031, 1032, "vec"),
           "odd": (1031, 1031, "scalar"), "odd_ld": (1030, 1033, "scalar")}


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_row_layouts(eng, layout, exact):
    """Every entry point on ld == n, on padded rows with n % 4 = 1, 2, 3 (body and tail; NaN in the padding) and on leading dimensions
    that are no multiple of 4 (the scalar kernels)."""
    n, ld, path = LAYOUTS[layout]
    assert n in C.LAYOUT_N
    W = Worst()
    everything(Dev(eng, C.case(C.LAYOUT_K, n, exact), ld=ld), C.LAYOUT_K, W, path)
    W.flush(layout)


#: entry point -> (the operands of its launcher's `vec` predicate, the call)
MISALIGNED = {
    "t": (("V", "r"), lambda D, k, W: run_t(D, k, W, "scalar")),
    "t_w1": (("V", "r", "w"), lambda D, k, W: run_t(D, k, W, "scalar", wpow=1)),
    "t_x": (("V", "r", "xrow"), lambda D, k, W: run_t_x(D, k, W, "scalar")),
    "t2": (("V", "r", "r2"), lambda D, k, W: run_t2(D, k, W, "scalar")),
    "tn3": (("V",) + RHS[:3], lambda D, k, W: run_tn(D, k, W, "scalar", 3)),
    "tn4": (("V",) + RHS[:4], lambda D, k, W: run_tn(D, k, W, "scalar", 4)),
    "n": (("V", "out", "base"), lambda D, k, W: run_n(D, k, W, "scalar", True, True)),
    "n_err": (("V", "out", "ref"), lambda D, k, W: run_n_err(D, k, W, "scalar")),
    "n_hosty": (("V", "out", "ref"), lambda D, k, W: run_n_err(D, k, W, "scalar", hosty=True)),
    "orth": (("V", "w_in", "vn", "x", "ref"), lambda D, k, W: run_orth(D, k, W, "scalar", True, True, True)[1]),
    "nt": (("V", "w_in", "w_out"), lambda D, k, W: run_nt(D, k, W, "scalar")),
}


@pytest.mark.parametrize("entry", list(MISALIGNED))
def test_misaligned_operand(eng, entry):
    """ld % 4 == 0 and one operand one float off a 16-byte boundary, each operand of the launcher's predicate in turn: the call takes
    the scalar kernel — the same values (exact operands), the same bits in the entry-wise outputs (general operands)."""
    operands, call = MISALIGNED[entry]
    k, (n, ld, _) = C.LAYOUT_K, LAYOUTS["pad2"]
    W = Worst()
    for exact in (True, False):
        c = C.case(k, n, exact)
        aligned = call(Dev(eng, c, ld=ld), k, Worst())
        for name in operands:
            D = Dev(eng, c, ld=ld, mis=(name,))
            got = call(D, k, W)
            D.check()
            if aligned is not None:                                     # fixed order of the k terms of an entry, whatever the width of the loads
                assert torch.equal(got, aligned), (entry, name)
    W.flush(entry)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
def test_weight_squared_through_wgram(eng, exact):
    """k_gemv_t<2> (and <1> beside it): trk_wgram's c2 = V (w^2 r) for k + 2 > 64, on padded rows, on an odd leading dimension and
    with each operand of the predicate misaligned."""
    k, W = C.WGRAM_K, Worst()
    for n, ld, path, mis in ((1030, 1032, "vec", ()), (1031, 1031, "scalar", ()), (1030, 1032, "scalar", ("V",)),
                             (1030, 1032, "scalar", ("r",)), (1030, 1032, "scalar", ("w",))):
        D = Dev(eng, C.case(k, n, exact, k), ld=ld, mis=mis)
        run_t(D, k, W, path, wpow=2)
        D.check()
    W.flush("wgram")


# ------------------------------------------------------------------------------------------------------------ row tiles, grid shapes
TILED = {"t": run_t, "t_x": run_t_x, "t2": run_t2, "tn3": lambda D, k, W, p: run_tn(D, k, W, p, 3),
         "tn4": lambda D, k, W, p: run_tn(D, k, W, p, 4)}


@pytest.mark.parametrize("entry", list(TILED))
def test_row_tiles(eng, entry):
    """Every k from 1 to 41 (one to six tiles of equal height, the last one short or not; t_x: the extra row inside a tile, and at
    k = 8, 16, 24, 32, 40 opening one) on exact operands: the layout partials[bx][R k] with q k + j0 + j, bit for bit."""
    D = Dev(eng, C.case(C.TILE_KMAX, C.TILE_N, True, C.TILE_KMAX), ld=1032)
    W = Worst()
    for k in range(1, C.TILE_KMAX + 1):
        TILED[entry](D, k, W, "vec")
    D.check()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
@pytest.mark.parametrize("k,n", C.GRID_CASES)
def test_grid_shapes(eng, k, n, exact):
    """The grid of the dot kernels: one and two x-blocks (2048, 2052), the float4s-per-thread switch of tiled_dot_grid_x (2^20, 2^20 + 4),
    four tiles whose workgroups stride more than once (k = 25, n = 1 200 003 in rows of 1 200 004: body and tail)."""
    W = Worst()
    D = Dev(eng, C.case(k, n, exact, k), ld=(n + 3) // 4 * 4)
    for entry in TILED:
        TILED[entry](D, k, W, "vec")
    D.check()
    W.flush(f"k{k}-n{n}")


# ------------------------------------------------------------------------------------------------------------ the combination
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
def test_combination_row_ladder(eng, exact):
    """k_gemv_n's groups of 8, 4 and 1 rows: every k from 1 to 13, 16 and 21, with and without a base and the fused sum of squares;
    trk_gemv_n_err's output is trk_gemv_n's."""
    W = Worst()
    D = Dev(eng, C.case(max(C.LADDER_K), C.LADDER_N, exact), ld=1032)
    for k in C.LADDER_K:
        plain = run_n(D, k, W, "vec", False, True).clone()
        run_n(D, k, W, "vec", True, k % 2 == 0)
        assert torch.equal(run_n_err(D, k, W, "vec"), plain)
        run_orth(D, k, W, "vec", with_x=True)
    D.check()
    W.flush("ladder")


def test_host_coefficients_beyond_one_launch(eng):
    """trk_gemv_n_hosty with k = 130: a second launch of two rows adds to what the first left in `out` (exact operands)."""
    k = 130
    D = Dev(eng, C.case(k, C.LADDER_N, True, k), ld=1032)
    W = Worst()
    run_n_err(D, k, W, "vec", hosty=True, with_ref=True)
    run_n_err(D, k, W, "vec", hosty=True, with_ref=False)
    D.check()


def test_accept_reject_limits(eng):
    """KMAX_LDS = 1024 rows for trk_gemv_n (1025: an error, no launch), k < 1024 for trk_gemv_orth_iterate, k <= 16 for trk_gemv_nt
    (8, 9, 16 computed: both instantiations, the wider one full), 3 or 4 right-hand sides for trk_gemv_tn; trk_gemv_orth_iterate's
    refused aliases."""
    W = Worst()
    D = Dev(eng, C.case(C.KMAX_LDS, C.KMAX_N, True, C.KMAX_LDS + 1))
    V, e, k = D.basis(), eng, C.KMAX_LDS
    run_n(D, k, W, "vec", True, True)
    run_n_err(D, k, W, "vec")
    run_orth(D, k - 1, W, "vec", with_x=True)
    Y, out = Scal(e, k + 1, D.c.coef("y", k + 1)), D.out("out")
    with pytest.raises(ValueError):
        e.gemv_n(V, k + 1, Y.ref(), out)
    with pytest.raises(ValueError):
        e.gemv_n_err(V, k + 1, Y.ref(), out, D.inp("ref"), Scal(e, CAP).ref(), CAP)
    R2, vn, w = Scal(e, 1, [4.0]), D.out("vn"), D.inp("w_in")
    with pytest.raises(ValueError):
        e.gemv_orth_iterate(V, k, w, Y.ref(), R2.ref(), vn)
    with pytest.raises(ValueError):                                     # vn == w
        e.gemv_orth_iterate(V, 5, w, Y.ref(), R2.ref(), w)
    with pytest.raises(ValueError):                                     # x_next == vn
        e.gemv_orth_iterate(V, 5, w, Y.ref(), R2.ref(), vn, y_next=Y.ref(), x_next=vn)
    with pytest.raises(ValueError):                                     # x_next == w
        e.gemv_orth_iterate(V, 5, w, Y.ref(), R2.ref(), vn, y_next=Y.ref(), x_next=w)
    for kk in (8, 9, 16):
        run_nt(D, kk, W, "vec")
    H = Scal(e, 5 * 17)
    with pytest.raises(ValueError):
        e.gemv_nt(V, 17, Y.ref(), w, D.out("w_out"), H.ref())
    for R in (2, 5):
        with pytest.raises(ValueError):
            e.gemv_tn(V, 4, [D.inp("r")] * R, H.ref())
    assert np.all(out.cpu().numpy() == SENTINEL) and np.all(vn.cpu().numpy() == SENTINEL) and np.all(H.values() == SENTINEL)
    D.check()


def test_rows_split_over_the_waves(eng):
    """k_gemv_n_split (trk_gemv_n with a base and no sum of squares, k >= 12, n / 4 <= 64 x 4 x CUs; trk_gemv_orth_iterate's image form
    with 1 / sqrt(*rho2)): unequal quarter shares (k = 12 .. 15, 17), a last workgroup of one column, the longest vector it serves and
    one float4 beyond, where the call is k_gemv_n's again.  Exact operands: the same bits as k_gemv_n (a misaligned base sends the
    call there); general operands: within the bound of an output rounded once."""
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    W = Worst()
    sizes = [(k, C.SPLIT_N) for k in C.SPLIT_K] + [(12, C.split_edge(cus)), (12, C.split_edge(cus) + 4)]
    for k, n in sizes:
        for exact in (True, False):
            c = C.case(k, n, exact)
            path = "split" if n <= C.split_edge(cus) else "vec"
            D = Dev(eng, c)
            out = run_n(D, k, W, path, True, False, a=-1.0, s=1.0).clone()
            vn = run_orth(D, k, W, path, with_x=False)[0].clone()
            D.check()
            if exact:
                D2 = Dev(eng, c, mis=("base", "w_in"))
                assert torch.equal(run_n(D2, k, W, "scalar", True, False, a=-1.0, s=1.0), out)
                assert torch.equal(run_orth(D2, k, W, "scalar", with_x=False)[0], vn)
                D2.check()
    W.flush("split")


# ------------------------------------------------------------------------------------------------------------ aliasing, n = 0
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
def test_aliased_outputs(eng, exact):
    """trk_gemv_n with out == base, trk_gemv_nt with w_out == w_in, on the 16-byte and on the scalar path."""
    W = Worst()
    for layout in ("pad3", "odd"):
        n, ld, path = LAYOUTS[layout]
        c = C.case(C.LAYOUT_K, n, exact)
        for k in (C.LAYOUT_K, 5):                                       # (5: rows 4 + 1 and k_gemv_nt<8>)
            D = Dev(eng, c, ld=ld)
            run_n(D, k, W, path, True, True, alias=True, a=1.0, s=-1.0)
            run_nt(D, k, W, path, alias=True)
            D.check()
    W.flush("alias")


def test_empty_vectors(eng):
    """n = 0 with non-null pointers (zero-length views into live storage): every dot and sum of squares is exactly 0.0, nothing
    around the outputs is touched."""
    import ctypes
    from trips_py_amd import _lib
    lib, st = eng.lib, eng.stream()
    k = 5
    buf = torch.full((64,), SENTINEL, dtype=torch.float32, device=eng.device)
    p = [buf.data_ptr() + 16 * i for i in range(8)]                     # distinct, 16-byte aligned, inside buf
    Cf = Scal(eng, k + 1, np.arange(1, k + 2) / 8.0)
    R2 = Scal(eng, 1, [4.0])
    for ld in (0, 4, 7):
        H = Scal(eng, 4 * k + 1)
        H.S.t[GUARD_D:GUARD_D + 4 * k + 1] = 3.5
        _lib.check(lib.trk_gemv_t(p[0], ld, k, 0, p[1], None, H.ref(), st), "t")
        assert np.all(H.values()[:k] == 0.0) and np.all(H.values()[k:] == 3.5)
        _lib.check(lib.trk_gemv_t(p[0], ld, k, 0, p[1], p[2], H.ref(), st), "t w")
        _lib.check(lib.trk_gemv_t_x(p[0], ld, k, 0, p[1], p[2], H.ref(), H.ref(k), st), "t_x")
        assert np.all(H.values()[:k + 1] == 0.0) and np.all(H.values()[k + 1:] == 3.5)
        _lib.check(lib.trk_gemv_t2(p[0], ld, k, 0, p[1], p[2], H.ref(), st), "t2")
        assert np.all(H.values()[:2 * k] == 0.0) and np.all(H.values()[2 * k:] == 3.5)
        for R in (3, 4):
            arr = (ctypes.c_void_p * R)(*p[1:1 + R])
            _lib.check(lib.trk_gemv_tn(p[0], ld, k, 0, arr, R, H.ref(), st), "tn")
            assert np.all(H.values()[:R * k] == 0.0) and np.all(H.values()[R * k:] == 3.5)
        S = Scal(eng, 2)
        S.S.t[GUARD_D:GUARD_D + 2] = 3.5
        _lib.check(lib.trk_gemv_n(p[0], ld, k, 0, Cf.ref(), 0.5, p[1], -2.0, p[2], None, st), "n")
        _lib.check(lib.trk_gemv_n(p[0], ld, k, 0, Cf.ref(), 0.5, p[1], -2.0, p[2], S.ref(), st), "n sumsq")
        _lib.check(lib.trk_gemv_n(p[0], ld, k, 0, Cf.ref(), 0.0, None, 1.0, p[2], S.ref(1), st), "n sumsq, no base")
        assert np.all(S.values() == 0.0)
        P, nb = Scal(eng, CAP), ctypes.c_int(-1)
        _lib.check(lib.trk_gemv_n_err(p[0], ld, k, 0, Cf.ref(), p[2], p[3], P.ref(), CAP, ctypes.byref(nb), st), "n_err")
        assert nb.value >= 1 and np.all(P.values()[:nb.value] == 0.0) and np.all(P.values()[nb.value:] == SENTINEL)
        yh = np.arange(1, k + 1) / 8.0
        P, nb = Scal(eng, CAP), ctypes.c_int(-1)
        _lib.check(lib.trk_gemv_n_hosty(p[0], ld, k, 0, yh.ctypes.data, p[2], p[3], P.ref(), CAP, ctypes.byref(nb), st), "n_hosty")
        assert nb.value >= 1 and np.all(P.values()[:nb.value] == 0.0) and np.all(P.values()[nb.value:] == SENTINEL)
        P, nb, CH = Scal(eng, CAP), ctypes.c_int(-1), Scal(eng, 1)
        _lib.check(lib.trk_gemv_orth_iterate(p[0], ld, k, 0, p[1], Cf.ref(), R2.ref(), Cf.ref(), p[2], p[3], p[4], P.ref(), CAP,
                                             ctypes.byref(nb), CH.ref(), st), "orth")
        assert nb.value >= 1 and np.all(P.values()[:nb.value] == 0.0) and np.all(P.values()[nb.value:] == SENTINEL)
        assert CH.values()[0] == 0.0
        G = Scal(eng, k + 1)
        G.S.t[GUARD_D:GUARD_D + k + 1] = 3.5
        _lib.check(lib.trk_gemv_nt(p[0], ld, k, 0, Cf.ref(), p[1], p[2], G.ref(), st), "nt")
        assert np.all(G.values()[:k] == 0.0) and G.values()[k] == 3.5
        P, nb, ST = Scal(eng, CAP), ctypes.c_int(-1), Scal(eng, 4)
        _lib.check(lib.trk_lsqr_damped_update(p[0], p[1], None, p[2], 0, p[3], P.ref(), CAP, ctypes.byref(nb), R2.ref(), R2.ref(),
                                              R2.ref(), 0.5, None, ST.ref(), 1, st), "lsqr")
        assert nb.value >= 1 and np.all(P.values()[:nb.value] == 0.0) and np.all(np.isfinite(ST.values()))
    assert bool((buf == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------ damped LSQR
LSQR = dict(alpha_sq=1.7, beta_sq=0.9, beta0_sq=2.3, damp=0.3)


def run_lsqr(D, W, path, first, with_ref, alias=False):
    """One trk_lsqr_damped_update (general operands) against the rotations repeated in float64; returns (w, x) as stored."""
    c, e = D.c, D.eng
    vk, w = D.inp("vk"), D.inp("w_old")
    x_in = None if first else D.inp("x_in")
    x_out = x_in if alias else D.out("x")
    ref = D.inp("ref") if with_ref else None
    _, st_in = C.lsqr_coefficients(3.1, 0.4, LSQR["beta0_sq"], LSQR["damp"], None, True)          # a state a first step leaves
    coefs, st_ref = C.lsqr_coefficients(LSQR["alpha_sq"], LSQR["beta_sq"], LSQR["beta0_sq"], LSQR["damp"], st_in, first)
    SC, SI, SO, P = Scal(e, 3, [LSQR["alpha_sq"], LSQR["beta_sq"], LSQR["beta0_sq"]]), Scal(e, 4, st_in), Scal(e, 4), Scal(e, CAP)
    nb = e.lsqr_damped_update(vk, w, x_in, x_out, SC.ref(0), SC.ref(1), SC.ref(2), LSQR["damp"], None if first else SI.ref(), SO.ref(),
                              first, ref=ref, partials=P.ref() if with_ref else None, capacity=CAP if with_ref else 0)
    w_got, x_got = w.cpu().numpy(), x_out.cpu().numpy()
    form = "first" if first else "later"
    W.see(f"lsqr.{form}.state", SO.values(), C.Ref(C.wide(st_ref), C.LSQR_SLACK * C.U53 * np.abs(st_ref)), False)
    W.see(f"lsqr.{form}.w.{path}", w_got, C.lsqr_w(c.vec("vk"), c.vec("w_old"), coefs, first), False)
    W.see(f"lsqr.{form}.x.{path}", x_got, C.lsqr_x(None if first else c.vec("x_in"), w_got, coefs), False)
    if with_ref:
        W.see(f"lsqr.err.{path}", partial_sum(P, nb), C.sum_of_squares(x_got, c.vec("ref")), False)
    else:
        assert nb == 0 and np.all(P.values() == SENTINEL)
    D.check()
    return w.clone(), x_out.clone()


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
def test_lsqr_damped_update(eng, first):
    """The damped-LSQR step: n % 4 == 0 and n % 4 == 3 (body and tail), with and without ref, in place (x_out == x_in), and each
    operand of the predicate misaligned — the scalar kernel leaves the same bits."""
    W = Worst()
    for n in (1028, 1031):
        c = C.case(1, n, False)
        for with_ref in (False, True):
            w0, x0 = run_lsqr(Dev(eng, c), W, "vec", first, with_ref)
            for name in ("vk", "w_old", "x", "ref") + (() if first else ("x_in",)):
                if name == "ref" and not with_ref:
                    continue
                w1, x1 = run_lsqr(Dev(eng, c, mis=(name,)), W, "scalar", first, with_ref)
                assert torch.equal(w1, w0) and torch.equal(x1, x0), name
        if not first:
            w1, x1 = run_lsqr(Dev(eng, c), W, "vec", first, True, alias=True)
            assert torch.equal(w1, w0) and torch.equal(x1, x0)
    W.flush("first" if first else "later")


# ------------------------------------------------------------------------------------------------------------ non-temporal loads
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "general"])
def test_nontemporal_loads(eng, exact):
    """n = 11 x 2^20 + 4, k = 3: the basis rows are loaded with ld4_nt (stream_nontemporal's bits 64, 128) by k_gemv_t, _t2, _tr<3>,
    k_gemv_n (with the sum of squares) and k_gemv_orth_iter (with x_next).  Exact operands bit for bit, general ones within the bounds.
    The one large case of the file."""
    k, n = C.NT_K, C.NT_N
    assert n >= C.NT_MIN and n % 4 == 0
    W = Worst()
    D = Dev(eng, C.case(k, n, exact, k))
    run_t(D, k, W, "nt")
    run_t2(D, k, W, "nt")
    run_tn(D, k, W, "nt", 3)
    run_n(D, k, W, "nt", False, True)
    run_orth(D, k, W, "nt", with_x=True)
    D.check()
    W.flush("nt")
