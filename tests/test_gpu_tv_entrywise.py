"""The first-difference kernels (csrc/tvops.hip) and k_isotv_weights (csrc/vecops.hip) entry by entry against float64 on the same
float32 operands, on every path N, nt, the capped grids and the time-sharded handles select.  Operands, references, bounds and the
slicing: tests/tv_cases.py (checked on the CPU by tests/test_tv_cases_host.py).  All calls go through HipEngine / engine.lib.

Exact operands (small integers, weights 0.5 / 1 / 2 / 4, lam = 0.25): the device result must EQUAL the reference, sums included.
General operands: within the bounds derived in tv_cases' docstring; the worst deviation of every entry point and path is logged as
a fraction of its bound (conftest.bar, limit 1).  Every device vector lives between guard floats that must be unchanged after the
calls; outputs start as NaN, so a store that was skipped shows.  Time-sharded handles are made in this one process
(trk_spacetime_create(N, nt_local, has_next, has_prev)) and fed their halos by hand from the global vector (trk_tv_halo,
trk_spacetime_set_halo): their outputs must be the bits of the one-handle result.

Which test reaches which instantiation launched from tvops.hip's first-difference entry points (k_d2_adj gathers through
AdjGather<TEMPORAL> of tv_internal.h, which PDHG's fused primal in pdhg_tv.hip shares: tests/test_gpu_pdhg_iso3.py has that table):

  entry point                               kernel<template arguments>             covering test
  trk_op_apply, 2-D, forward                k_d2_fwd<false>                        apply_2d, apply_batched
  ... with sumsq                            k_d2_fwd<true>                         apply_2d, apply_batched, capped_grid_apply[1] (strided batches)
  trk_op_apply, 2-D, transpose              k_d2_adj<false, false>                 apply_2d, apply_batched
  ... with sumsq                            k_d2_adj<true, false>                  apply_2d, apply_batched, capped_grid_apply[1]
  trk_op_apply, space-time, forward         k_d2_fwd<false> + k_time_fwd<false>    apply_spacetime (513: strided), apply_batched, sharded (halo_next)
  ... with sumsq                            k_d2_fwd<true> + k_time_fwd<true>      apply_spacetime, capped_grid_apply[2], sharded
  trk_op_apply, space-time, transpose       k_d2_adj<false, true>                  apply_spacetime, apply_batched, sharded (first_has_prev, last_has_cur)
  ... with sumsq                            k_d2_adj<true, true>                   apply_spacetime, capped_grid_apply[2], sharded
  trk_tv_weights                            k_tv_weights (+ k_tvt_weights, nt > 1  tv_weights (q, eps, flat images), sharded (xnext row, the previous
                                            or a neighbour)                        slice's row)
  trk_tv_grad, w, r_in                      k_tv_grad<true, true, false>           tv_grad, sharded (xprev, xnext, wrow_prev)
  trk_tv_grad, w, no r_in                   k_tv_grad<true, false, false>          tv_grad
  trk_tv_grad, no w, r_in                   k_tv_grad<false, true, false>          tv_grad
  trk_tv_grad, no w, no r_in                k_tv_grad<false, false, false>         tv_grad
  trk_tv_grad_dot, w, r_in                  k_tv_grad<true, true, true>            tv_grad (257: idle threads in the block sum), capped_grid_tv_grad, sharded
  trk_tv_grad_dot, w, no r_in               k_tv_grad<true, false, true>           tv_grad, capped_grid_tv_grad
  trk_tv_grad_dot, no w, r_in               k_tv_grad<false, true, true>           tv_grad, capped_grid_tv_grad
  trk_tv_grad_dot, no w, no r_in            k_tv_grad<false, false, true>          tv_grad, capped_grid_tv_grad
  trk_tv_grad_dot_xsq, the four of them     k_tv_grad<W, RIN, true>, xsq = 1       tv_grad, capped_grid_tv_grad, sharded (no w)
  trk_tv_halo / trk_spacetime_set_halo      (no kernel: the contract)              halo_contract
  trk_isotv_weights                         k_isotv_weights                        isotv_weights
"""
import ctypes

import numpy as np
import pytest
import torch

import tv_cases as C
from conftest import bar

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 8                      # floats on both sides of every device vector
GUARD_D = 4                    # doubles on both sides of every device scalar
TRK_EINVAL = -1
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def eng():
    from trips_py_amd.engine import default_engine
    return default_engine()


class Pool:
    """Device vectors, each in an allocation of its own between guard floats."""

    def __init__(self, eng):
        self.eng, self.bufs = eng, []

    def _alloc(self, n, fill):
        buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.float32, device=self.eng.device)
        buf[:GUARD] = SENTINEL
        buf[GUARD + n:] = SENTINEL
        self.bufs.append((buf, n))
        return buf[GUARD:GUARD + n]

    def inp(self, host):
        host = np.ascontiguousarray(host, dtype=F32).reshape(-1)
        v = self._alloc(host.size, 0.0)
        v.copy_(torch.from_numpy(host))
        return v

    def out(self, n):
        """An output of n floats, all NaN."""
        return self._alloc(int(n), float("nan"))

    def check(self):
        for buf, n in self.bufs:
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), "guard floats overwritten"


class Scal:
    """m device doubles between guards."""

    def __init__(self, eng, m=1):
        self.S, self.m = eng.scalars(m + 2 * GUARD_D), m
        self.S.t[:] = SENTINEL

    def ref(self, i=0):
        return self.S.ref(GUARD_D + i)

    def values(self):
        h = self.S.t.cpu().numpy()
        assert np.all(h[:GUARD_D] == SENTINEL) and np.all(h[GUARD_D + self.m:] == SENTINEL), "guard doubles overwritten"
        return h[GUARD_D:GUARD_D + self.m].copy()


def _p(t):
    return None if t is None else t.data_ptr()


class Handle:
    """A trk_op of the first-difference family, every call returning its code.  nt None: the 2-D operator."""

    def __init__(self, eng, N, nt=None, has_next=False, has_prev=False):
        self.eng, self.lib, self.N, self.nt = eng, eng.lib, N, 1 if nt is None else nt
        self.h = ctypes.c_void_p()
        if nt is None:
            rc = self.lib.trk_deriv2d_create(N, ctypes.byref(self.h))
        else:
            rc = self.lib.trk_spacetime_create(N, nt, int(has_next), int(has_prev), ctypes.byref(self.h))
        assert rc == 0 and self.h
        self.npix, self.ps, self.ntemp, self.rows = C.sizes(N, self.nt, has_next)
        r, c = ctypes.c_int64(), ctypes.c_int64()
        assert self.lib.trk_op_shape(self.h, ctypes.byref(r), ctypes.byref(c)) == 0
        assert (r.value, c.value) == (self.rows, self.nt * self.npix)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.synchronize()
        self.lib.trk_op_destroy(self.h)

    def apply(self, tr, x, y, ss=None, batch=1, ldx=0, ldy=0):
        return self.lib.trk_op_apply(self.h, int(tr), _p(x), int(ldx), _p(y), int(ldy), int(batch), None if ss is None else ss.ref(),
                                     self.eng.stream())

    def set_halo(self, x_next, y_prev):
        return self.lib.trk_spacetime_set_halo(self.h, _p(x_next), _p(y_prev))

    def halo(self, xprev, xnext):
        return self.lib.trk_tv_halo(self.h, _p(xprev), _p(xnext))

    def weights(self, x, eps, q, w):
        return self.lib.trk_tv_weights(self.h, _p(x), float(eps), float(q), _p(w), self.eng.stream())

    def grad(self, x, w, r, lam, out, dotv=None, dot=None, xsq=None):
        s = self.eng.stream()
        if xsq is not None:
            return self.lib.trk_tv_grad_dot_xsq(self.h, _p(x), _p(w), _p(r), float(lam), _p(out), _p(dotv), dot.ref(), xsq.ref(), s)
        if dot is not None:
            return self.lib.trk_tv_grad_dot(self.h, _p(x), _p(w), _p(r), float(lam), _p(out), _p(dotv), dot.ref(), s)
        return self.lib.trk_tv_grad(self.h, _p(x), _p(w), _p(r), float(lam), _p(out), s)


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=F32).view(np.int32), np.asarray(b, dtype=F32).view(np.int32))


class Worst(dict):
    """Checks device results against references; keeps the worst error / bound of the general operands per name."""

    def see(self, name, got, R, exact):
        got = np.asarray(got).reshape(-1)
        assert np.all(np.isfinite(got.astype(F64))), (name, "not finite", int(np.sum(~np.isfinite(got.astype(F64)))))
        bad, ratio = C.compare(got, R, exact)
        assert bad.size == 0, (name, "exact operands" if exact else "bound", bad.size, bad[:8], got[bad[:8]], R.val[bad[:8]],
                               R.bound[bad[:8]])
        if not exact:
            print(f"{name}: max error / bound {ratio:.3e}")
            self[name] = max(self.get(name, 0.0), ratio)

    def flush(self, tag):
        for name, v in sorted(self.items()):
            bar(f"tv.entrywise[{name}:{tag}]", v, 1.0)


KINDS = ("exact", "normal")


# ------------------------------------------------------------------------------------------------------------ L x and L^T y
def apply_checks(eng, W, path, hd, X, y, exact, xnext=None, halo_prev=None):
    """L x and L^T y of one handle, plain and with sumsq; returns the four device results (host arrays, sums as float64)."""
    P = Pool(eng)
    dx, dy = P.inp(X), P.inp(y)
    dxn, dhp = (None if xnext is None else P.inp(xnext)), (None if halo_prev is None else P.inp(halo_prev))
    if hd.nt != 1 or dxn is not None or dhp is not None:
        assert hd.set_halo(dxn, dhp) == 0
    lx, lx_s, at, at_s = P.out(hd.rows), P.out(hd.rows), P.out(hd.nt * hd.npix), P.out(hd.nt * hd.npix)
    s1, s2 = Scal(eng), Scal(eng)
    assert hd.apply(0, dx, lx) == 0 and hd.apply(0, dx, lx_s, ss=s1) == 0
    assert hd.apply(1, dy, at) == 0 and hd.apply(1, dy, at_s, ss=s2) == 0
    lx, lx_s, at, at_s = host(lx), host(lx_s), host(at), host(at_s)
    P.check()
    W.see(f"Lx.{path}", lx, C.lx_ref(X, xnext), exact)
    W.see(f"LTy.{path}", at, C.adj_ref(y, hd.N, hd.nt, xnext is not None, halo_prev), exact)
    assert same_bits(lx, lx_s) and same_bits(at, at_s), "the sumsq variant stores other bits"
    W.see(f"Lx.sumsq.{path}", s1.values(), C.dot_ref(lx, lx), exact)
    W.see(f"LTy.sumsq.{path}", s2.values(), C.dot_ref(at, at), exact)
    return lx, at, s1.values()[0], s2.values()[0]


@pytest.mark.parametrize("N", [2, 3, 4, 5, 6, 255, 256, 257])
def test_apply_2d(eng, N):
    W = Worst()
    with Handle(eng, N) as hd:
        for kind in KINDS:
            apply_checks(eng, W, "2d", hd, C.image(kind, 1, N), C.vector(kind, hd.rows, 1), kind == "exact")
    W.flush(f"N={N}")


@pytest.mark.parametrize("N,nt", [(2, 2), (3, 5), (4, 3), (5, 2), (6, 3), (255, 2), (256, 3), (257, 2), (513, 2), (5, 1), (257, 1)])
def test_apply_spacetime(eng, N, nt):
    """(513: the temporal kernels stride; nt = 1: a space-time handle without temporal rows)"""
    assert C.temporal_strided(513) and not C.temporal_strided(512)
    W = Worst()
    with Handle(eng, N, nt) as hd:
        for kind in KINDS:
            apply_checks(eng, W, "st", hd, C.image(kind, nt, N), C.vector(kind, hd.rows, 1), kind == "exact")
    W.flush(f"N={N},nt={nt}")


@pytest.mark.parametrize("N,nt", [(5, None), (257, None), (5, 2), (6, 3)])
def test_apply_batched(eng, N, nt):
    """An (n, 3) operand with padded leading dimensions (the padding NaN on the input side, untouched on the output side)."""
    W, B = Worst(), 3
    with Handle(eng, N, nt) as hd:
        cols = hd.nt * hd.npix
        ldx, ldy = cols + 5, hd.rows + 3
        for kind in KINDS:
            exact = kind == "exact"
            Xs = [C.image(kind, hd.nt, N, seed=b) for b in range(B)]
            ys = [C.vector(kind, hd.rows, 10 + b) for b in range(B)]
            P = Pool(eng)
            xin, yin = np.full((B, ldx), np.nan, dtype=F32), np.full((B, ldy), np.nan, dtype=F32)
            for b in range(B):
                xin[b, :cols], yin[b, :hd.rows] = Xs[b].reshape(-1), ys[b]
            dx, dy = P.inp(xin), P.inp(yin)
            for with_ss in (False, True):
                lx, at = P.out(B * ldy), P.out(B * ldx)
                s1, s2 = (Scal(eng), Scal(eng)) if with_ss else (None, None)
                assert hd.apply(0, dx, lx, ss=s1, batch=B, ldx=ldx, ldy=ldy) == 0
                assert hd.apply(1, dy, at, ss=s2, batch=B, ldx=ldy, ldy=ldx) == 0
                lx, at = host(lx).reshape(B, ldy), host(at).reshape(B, ldx)
                P.check()
                assert np.all(np.isnan(lx[:, hd.rows:])) and np.all(np.isnan(at[:, cols:])), "the padding was written to"
                for b in range(B):
                    W.see("Lx.batch", lx[b, :hd.rows], C.lx_ref(Xs[b]), exact)
                    W.see("LTy.batch", at[b, :cols], C.adj_ref(ys[b], N, hd.nt), exact)
                if with_ss:                                               # one sum over the whole batch
                    W.see("Lx.sumsq.batch", s1.values(), C.dot_ref(lx[:, :hd.rows], lx[:, :hd.rows]), exact)
                    W.see("LTy.sumsq.batch", s2.values(), C.dot_ref(at[:, :cols], at[:, :cols]), exact)
    W.flush(f"N={N},nt={nt}")


@pytest.mark.parametrize("nt", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_capped_grid_apply(eng, nt, kind):
    """N = 2049: grid2(..., capped = true) strides over the row batches (9 columns of workgroups, 455 of the 513 batches)."""
    N = 2049
    assert C.row_batches_strided(N) and not C.row_batches_strided(N - 1)
    W = Worst()
    with Handle(eng, N, None if nt == 1 else nt) as hd:
        apply_checks(eng, W, "capped", hd, C.image(kind, nt, N), C.vector(kind, hd.rows, 1), kind == "exact")
    W.flush(f"N={N},nt={nt}")


# ------------------------------------------------------------------------------------------------------------ weights
def powf_units(got, R):
    """The worst |got / ref - 1| in units of 2^-24."""
    return float(np.max(np.abs(np.asarray(got, dtype=F64) / R.val - 1.0))) / C.U24


WEIGHT_SHAPES = [(2, 1), (3, 1), (5, 3), (6, 2), (257, 1), (257, 2)]


@pytest.mark.parametrize("q", [1.0, 0.7, 2.0, 0.5])
@pytest.mark.parametrize("eps", [0.1, 1e-3, 1e-16, 1e-20])
def test_tv_weights(eng, q, eps):
    """(eps = 1e-16, 1e-20: eps^2 < 1e-30, q = 1 leaves the hardware reciprocal square root for 1 / sqrtf; 1e-20: eps^2 is a denormal
    float32, and it is all there is of t wherever a flat image's difference is 0)"""
    W, units = Worst(), 0.0
    for N, nt in WEIGHT_SHAPES:
        with Handle(eng, N, None if nt == 1 else nt) as hd:
            for kind in ("normal", "flat"):
                X = C.image(kind, nt, N)
                P = Pool(eng)
                dx, w = P.inp(X), P.out(hd.rows)
                assert hd.weights(dx, eps, q, w) == 0
                w = host(w)
                P.check()
                R = C.tv_weights_ref(X, eps, q)
                if kind == "flat":
                    assert np.count_nonzero(C.st_fwd(X, dtype=F32) == 0) > hd.rows // 4
                if C.is_powf(q):
                    units = max(units, powf_units(w, R))
                W.see(f"weights.{kind}", w, R, False)
    if C.is_powf(q):
        bar(f"tv.entrywise[weights.powf.units:q={q},eps={eps}]", units, C.POWF_CAP)
        assert C.POWF_U <= C.POWF_CAP
    W.flush(f"q={q},eps={eps}")


# ------------------------------------------------------------------------------------------------------------ tv_grad
COMBOS = ((True, True), (True, False), (False, True), (False, False))          # (W, RIN)


def grad_checks(eng, W, path, hd, X, w, r, d, lam, exact, combos=COMBOS, forms=("plain", "dot", "xsq"), xprev=None, xnext=None):
    """Every asked-for instantiation of k_tv_grad on one handle: the entries, the same bits in every form, the dots.  Returns
    {(W, RIN): (out, dot or None, xsq or None)} as host values."""
    P = Pool(eng)
    dx, dw, dr, dd = P.inp(X), P.inp(w), P.inp(r), P.inp(d)
    dxp, dxn = (None if xprev is None else P.inp(xprev)), (None if xnext is None else P.inp(xnext))
    sharded = dxp is not None or dxn is not None
    n = hd.nt * hd.npix
    res = {}
    for cw, cr in combos:
        R = C.tv_grad_ref(X, w if cw else None, r if cr else None, lam, xprev, xnext)
        first, dot_v, xsq_v = None, None, None
        for form in forms:
            out = P.out(n)
            dot, xsq = (Scal(eng) if form != "plain" else None), (Scal(eng) if form == "xsq" else None)
            if sharded:
                assert hd.halo(dxp, dxn) == 0
            assert hd.grad(dx, dw if cw else None, dr if cr else None, lam, out, dd if dot else None, dot, xsq) == 0
            got = host(out)
            name = f"grad.w{int(cw)}r{int(cr)}"
            W.see(f"{name}.{path}", got, R, exact)
            if first is None:
                first = got
            assert same_bits(first, got), (name, form, "other bits than the first form")
            if dot:
                dot_v = dot.values()[0]
                W.see(f"{name}.dot.{path}", dot.values(), C.dot_ref(got, d), exact)
            if xsq:
                xsq_v = xsq.values()[0]
                W.see(f"{name}.xsq.{path}", xsq.values(), C.dot_ref(X, X), exact)
        res[(cw, cr)] = (first, dot_v, xsq_v)
    P.check()
    return res


@pytest.mark.parametrize("N,nt", [(2, 1), (3, 1), (4, 2), (5, 3), (6, 5), (255, 1), (256, 2), (257, 1), (257, 2), (5, -1)])
def test_tv_grad(eng, N, nt):
    """All eight k_tv_grad<W, RIN, DOT> and the xsq form of the four with DOT.  (nt = -1: a space-time handle of one frame)"""
    W = Worst()
    frames = abs(nt)
    with Handle(eng, N, None if nt == 1 else frames) as hd:
        for kind in KINDS:
            grad_checks(eng, W, "one", hd, C.image(kind, frames, N), C.weights(kind, hd.rows), C.vector(kind, frames * N * N, 2, top=31),
                        C.vector(kind, frames * N * N, 3), C.lam_of(kind), kind == "exact")
    W.flush(f"N={N},nt={nt}")


@pytest.mark.parametrize("nt,kind,combos,forms", [
    (1, "exact", ((True, True), (False, False)), ("xsq",)),
    (1, "normal", ((True, False), (False, True)), ("dot",)),
    (1, "normal", ((True, True),), ("plain", "xsq")),
    (2, "exact", ((True, True),), ("xsq",)),
    (2, "normal", ((False, False),), ("plain", "dot")),
])
def test_capped_grid_tv_grad(eng, nt, kind, combos, forms):
    """N = 2049: the reducing forms stride over the row batches; the last of the 9 workgroup columns has one live thread, the
    other 255 stay for the block sum on column N - 1."""
    N = 2049
    assert C.row_batches_strided(N)
    W = Worst()
    with Handle(eng, N, None if nt == 1 else nt) as hd:
        grad_checks(eng, W, "capped", hd, C.image(kind, nt, N), C.weights(kind, hd.rows), C.vector(kind, nt * N * N, 2, top=31),
                    C.vector(kind, nt * N * N, 3), C.lam_of(kind), kind == "exact", combos=combos, forms=forms)
    W.flush(f"N={N},nt={nt},{'+'.join(forms)}")


# ------------------------------------------------------------------------------------------------------------ time-sharded handles
@pytest.mark.parametrize("Wn", [2, 4])
@pytest.mark.parametrize("ntl", [1, 2])
@pytest.mark.parametrize("N", [5, 257])
def test_sharded(eng, Wn, ntl, N):
    """W slices of nt_local frames, each on a handle of its own fed by hand: every output mapped into the global layout is the
    one-handle result bit for bit — the recomputed previous-boundary weight row included (tvops.hip:134) — and within bound of
    float64; the slices' partial sums add up to the global ones."""
    nt = Wn * ntl
    npix = N * N
    W = Worst()
    eps = 1e-3
    for kind in KINDS:
        exact = kind == "exact"
        X, lam = C.image(kind, nt, N), C.lam_of(kind)
        r, d = C.vector(kind, nt * npix, 2, top=31), C.vector(kind, nt * npix, 3)
        with Handle(eng, N, nt) as g:
            y = C.vector(kind, g.rows, 1)
            g_lx, g_at, g_ss_lx, g_ss_at = apply_checks(eng, W, "global", g, X, y, exact)
            P = Pool(eng)
            dx = P.inp(X)
            g_w = {}
            for q in ((1.0, 0.7) if not exact else ()):
                w = P.out(g.rows)
                assert g.weights(dx, eps, q, w) == 0
                g_w[q] = host(w)
                W.see("weights.global", g_w[q], C.tv_weights_ref(X, eps, q), False)
            P.check()
            wg = C.weights(kind, g.rows) if exact else g_w[0.7]
            g_res = grad_checks(eng, W, "global", g, X, wg, r, d, lam, exact, combos=((True, True), (False, False)), forms=("dot", "xsq"))
        sums = {"lx": 0.0, "at": 0.0, "dot": 0.0, "dot0": 0.0, "xsq": 0.0}
        prev_w = None
        for s in C.cut(nt, N, Wn):
            xs, xprev, xnext = C.frames_of(X, s)
            path = f"slice.p{int(s['has_prev'])}n{int(s['has_next'])}"
            with Handle(eng, N, ntl, s["has_next"], s["has_prev"]) as hd:
                assert hd.rows == s["lx_map"].size
                halo = y[s["prev_rows"]] if s["has_prev"] else None
                lx, at, ss_lx, ss_at = apply_checks(eng, W, path, hd, xs, y[s["lx_map"]], exact, xnext, halo)
                assert same_bits(lx, g_lx[s["lx_map"]]) and same_bits(at, g_at[s["out_map"]])
                sums["lx"] += ss_lx
                sums["at"] += ss_at
                P = Pool(eng)
                dxs = P.inp(xs)
                dxp, dxn = (None if xprev is None else P.inp(xprev)), (None if xnext is None else P.inp(xnext))
                this_w = {}
                for q in g_w:
                    w = P.out(s["w_map"].size)
                    assert hd.halo(dxp, dxn) == 0 and hd.weights(dxs, eps, q, w) == 0
                    this_w[q] = host(w)
                    W.see(f"weights.{path}", this_w[q], C.tv_weights_ref(xs, eps, q, xprev, xnext), False)
                    assert same_bits(this_w[q], g_w[q][s["w_map"]])
                    if s["has_prev"]:                                     # the row as its owner wrote it: the owner's last temporal row
                        owner = prev_w[q][ntl * hd.ps + (ntl - 1) * npix:ntl * hd.ps + ntl * npix]
                        assert same_bits(this_w[q][hd.rows:], owner), "the recomputed boundary row differs from its owner's"
                prev_w = this_w
                P.check()
                res = grad_checks(eng, W, path, hd, xs, wg[s["w_map"]], r[s["out_map"]], d[s["out_map"]], lam, exact,
                                  combos=((True, True), (False, False)), forms=("plain", "dot", "xsq"), xprev=xprev, xnext=xnext)
                for key in res:
                    assert same_bits(res[key][0], g_res[key][0][s["out_map"]]), (key, "slice differs from the one-handle result")
                sums["dot"] += res[(True, True)][1]
                sums["dot0"] += res[(False, False)][1]
                sums["xsq"] += res[(True, True)][2]
        W.see("sum.Lx.sumsq", [sums["lx"]], C.dot_ref(g_lx, g_lx), exact)
        W.see("sum.LTy.sumsq", [sums["at"]], C.dot_ref(g_at, g_at), exact)
        W.see("sum.dot.w1r1", [sums["dot"]], C.dot_ref(g_res[(True, True)][0], d), exact)
        W.see("sum.dot.w0r0", [sums["dot0"]], C.dot_ref(g_res[(False, False)][0], d), exact)
        W.see("sum.xsq", [sums["xsq"]], C.dot_ref(X, X), exact)
    W.flush(f"W={Wn},ntl={ntl},N={N}")


def test_halo_contract(eng):
    """The parked halo serves ONE fused call and is consumed on every exit path; a plain apply needs its own halo.  Every check is
    on the return code: a refused call launches nothing (its output keeps its NaNs)."""
    N, ntl = 5, 2
    X = C.image("normal", ntl + 2, N)
    P = Pool(eng)
    dx, dxp, dxn = P.inp(X[1:3]), P.inp(X[0]), P.inp(X[3])
    with Handle(eng, N, ntl, True, True) as hd:
        npix = hd.npix
        w, out, lx, at = P.out(hd.rows + npix), P.out(ntl * npix), P.out(hd.rows), P.out(ntl * npix)
        dot, dd = Scal(eng), P.inp(C.vector("normal", ntl * npix, 3))
        dy, dhp = P.inp(C.vector("normal", hd.rows, 1)), P.inp(C.vector("normal", npix, 4))
        # no halo given
        assert hd.weights(dx, 0.1, 1.0, w) == TRK_EINVAL
        assert hd.grad(dx, None, None, 0.5, out) == TRK_EINVAL
        assert hd.grad(dx, None, None, 0.5, out, dd, dot) == TRK_EINVAL
        assert hd.grad(dx, None, None, 0.5, out, dd, dot, Scal(eng)) == TRK_EINVAL
        # a frame missing for a neighbour that exists
        assert hd.halo(None, dxn) == TRK_EINVAL and hd.halo(dxp, None) == TRK_EINVAL
        # a call that fails its own argument check still consumes the halo
        assert hd.halo(dxp, dxn) == 0
        assert hd.grad(dx, None, None, 0.5, None) == TRK_EINVAL
        assert hd.grad(dx, None, None, 0.5, out) == TRK_EINVAL
        assert hd.halo(dxp, dxn) == 0
        assert hd.weights(dx, 0.1, 1.0, None) == TRK_EINVAL
        assert hd.weights(dx, 0.1, 1.0, w) == TRK_EINVAL
        assert hd.halo(dxp, dxn) == 0
        assert hd.lib.trk_tv_grad_dot(hd.h, _p(dx), None, None, 0.5, _p(out), _p(dd), None, eng.stream()) == TRK_EINVAL
        assert hd.grad(dx, None, None, 0.5, out, dd, dot) == TRK_EINVAL
        assert hd.halo(dxp, dxn) == 0
        assert hd.grad(dx, None, None, 0.5, dx) == TRK_EINVAL               # out aliases x
        assert hd.grad(dx, None, None, 0.5, out) == TRK_EINVAL
        eng.synchronize()
        assert np.all(np.isnan(host(w))) and np.all(np.isnan(host(out))) and dot.values()[0] == SENTINEL
        # the halo serves one call
        assert hd.halo(dxp, dxn) == 0
        assert hd.weights(dx, 0.1, 1.0, w) == 0
        assert hd.weights(dx, 0.1, 1.0, w) == TRK_EINVAL
        assert hd.grad(dx, w, None, 0.5, out) == TRK_EINVAL
        assert hd.halo(dxp, dxn) == 0
        assert hd.grad(dx, w, None, 0.5, out) == 0
        assert hd.grad(dx, w, None, 0.5, out) == TRK_EINVAL
        assert np.all(np.isfinite(host(w))) and np.all(np.isfinite(host(out)))
        # plain applies: forward needs halo_next, transpose halo_prev
        assert hd.apply(0, dx, lx) == TRK_EINVAL and hd.apply(1, dy, at) == TRK_EINVAL
        assert hd.set_halo(dxn, None) == 0
        assert hd.apply(1, dy, at) == TRK_EINVAL
        assert hd.set_halo(None, dhp) == 0
        assert hd.apply(0, dx, lx) == TRK_EINVAL
        eng.synchronize()
        assert np.all(np.isnan(host(lx))) and np.all(np.isnan(host(at)))
        assert hd.set_halo(dxn, dhp) == 0
        assert hd.apply(0, dx, lx) == 0 and hd.apply(1, dy, at) == 0
        assert np.all(np.isfinite(host(lx))) and np.all(np.isfinite(host(at)))
    with Handle(eng, N, ntl) as whole:                                      # no neighbour: no halo asked for
        out2 = P.out(ntl * npix)
        assert whole.grad(dx, None, None, 0.5, out2) == 0 and whole.grad(dx, None, None, 0.5, out2) == 0
    with Handle(eng, N) as flat:
        assert flat.halo(dxp, dxn) == TRK_EINVAL and flat.set_halo(dxn, dhp) == TRK_EINVAL
    P.check()


# ------------------------------------------------------------------------------------------------------------ isotropic weights
@pytest.mark.parametrize("N,nt", [(1, 1), (2, 3), (3, 1), (16, 3), (257, 2)])
def test_isotv_weights(eng, N, nt):
    """q = 2: the constant 1; q = 0: 1 / sqrtf; q = 1: 1 / sqrtf(sqrtf); q = 0.5, 1.3: powf.  Tails: none, 7, one longer than the
    spatial part (the grid is sized by the longer of the two)."""
    W, units = Worst(), 0.0
    ns = N * N * nt
    for q in (1.0, 0.5, 2.0, 0.0, 1.3):
        for eps in (0.05, 1e-3):
            for n_tail in (0, 7, ns + 3):
                x, tail = C.vector("normal", ns, 5), C.vector("normal", n_tail, 6)
                P = Pool(eng)
                dx, out = P.inp(x), P.out(2 * ns + n_tail)
                dt = P.inp(tail) if n_tail else None
                rc = eng.lib.trk_isotv_weights(dx.data_ptr(), N, nt, _p(dt), n_tail, float(eps), float(q), out.data_ptr(), eng.stream())
                assert rc == 0
                got = host(out)
                P.check()
                R = C.isotv_weights_ref(x, N, nt, tail, eps, q)
                W.see(f"isotv.q{q}", got, R, False)
                assert same_bits(got[:ns], got[ns:2 * ns])
                if C.isotv_special(q)[1] == 0:
                    units = max(units, powf_units(got, R))
    bar(f"tv.entrywise[isotv.powf.units:N={N},nt={nt}]", units, C.POWF_CAP)
    W.flush(f"N={N},nt={nt}")
