"""The weighted Gram kernels (csrc/wgram.hip) entry by entry against float64 on the same float32 operands, on every kernel path the
row count, the row layout, the alignment, the length and the arithmetic mode select.  Operands, references, bounds and the launch
plans that name the cases: tests/wgram_cases.py (checked on the CPU by tests/test_wgram_cases_host.py).  All calls go through
HipEngine / the C ABI.

Exact operands (multiples of 1 / 8, weights 0, 0.5, 1, 2): every order of summation, every bf16 split and every arithmetic mode is
exact, the device result must EQUAL the reference.  General operands: trk_wgram within the bounds derived in wgram_cases' docstring
(36 u S on the matrix cores, 4 u S for the tile pairs), the worst deviation of every path logged as a fraction of its bound
(conftest.bar, limit 1); the TV Gram within the contract of include/trk.h per mode.

Every operand lives inside a larger allocation whose guard floats must be unchanged after the call; padding columns (ld > m, ld > N^2)
hold NaN; operands and padding must be bit for bit what was uploaded.  G, c1, c2, h sit between guard doubles; G == G^T to the bit.
Before a case runs, its launch plan on THIS device's compute-unit count must show the branch it is named for.

Which test reaches which instantiation (HAS_W: every case runs weighted and unweighted; HAS_B: every family has cases with and
without b; the host test asserts that the named cases reach every row):

  entry point              kernel<template arguments>                      reached by
  trk_wgram, KA <= 48,     k_wgram_t16<T, HAS_W, HAS_B>, T = 1, 2, 3       row_layouts[KA] (ld == m; padded ld with m % 4 = 1, 2, 3: the 16-byte body and
    16-byte aligned                                                          the scalar tail), groups_per_wave (lone consume, the pair branch, one trip of
                                                                             the two-group loop + either remainder, waves that differ by a group, a ragged
                                                                             tail), ladders, short_rows, twice / after_a_large_one
  trk_wgram, KA <= 32,     k_wgram_mfma<1, HAS_W, HAS_B>                   row_layouts (odd ld; W, w, b1 each one float off), chunks_per_workgroup[mfma1]
    not aligned                                                              (one and two chunks, ragged last chunk), short_rows
  trk_wgram, 33 <= KA      k_wgram_mfma<2, HAS_W, HAS_B>, vec_ok on        ladders (KA = 49, 64 aligned), chunks_per_workgroup[mfma2-aligned] (full chunks,
    <= 64                                                                    then a ragged one)
                           ... vec_ok off                                  row_layouts[33, 48] (odd ld, misaligned), ladders (odd ld), chunks[mfma2-odd]
  trk_wgram, KA > 64       k_wgram<HAS_W, VEC>; c1, c2: k_gemv_t<1>, <2>   ladders (k = 63 with b, 65 without; VEC on and off), short_rows (k = 70), k = 512
  trk_wgram_tv(_z),        k_wgram_tv<T, Z, 3, BF>, BF = 0, 2, 3, 4        tv_register_fed_exact (all four modes, with and without z: one strip, short last
    N < 2048 or k > 32                                                       band, lockstep, lockstep + XCD map, XCD map alone, both sides of ls_pays,
                                                                             two_pass, T = 3 at N = 2048), tv_general, tv_auto_with_verdict_1_is_the_fp32_form
  trk_wgram_tv(_z),        k_wgram_tv_lds<T, Z, BF>, T = 1, 2              tv_lds_exact (every k from 1 to 32 at N = 2048 in every mode, with and without z:
    N >= 2048, k <= 32                                                       every count of staged loads the hand-placed vmcnt waits meet), tv_lds_exact_nine_tiles
"""
import numpy as np
import pytest
import torch

import wgram_cases as C
from conftest import bar
from test_gpu_gemv_entrywise import GUARD, SENTINEL, Dev, Scal, Worst, up

pytestmark = pytest.mark.gpu

REF_CUS = 256                                  # the case NAMES are built at collection time; the sizes follow the device
MIS = {None: (), "W": ("V",), "w": ("w",), "b1": ("b",)}


@pytest.fixture(scope="module")
def eng():
    from trips_py_amd.engine import default_engine
    return default_engine()


@pytest.fixture(scope="module")
def cus(eng):
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


class Bars(Worst):
    def flush(self, tag):
        for name, v in sorted(self.items()):
            bar(f"wgram.entrywise[{name}:{tag}]", v, 1.0)


def addr(D, name):
    """The device address of operand `name` of D (never NULL, whatever its length)."""
    buf, off, _ = D.bufs[name]
    return buf.data_ptr() + 4 * off


def path_of(p):
    return f"{p['kernel']}<{','.join(str(int(a)) for a in p['targs'])}>"


# ------------------------------------------------------------------------------------------------------------ stored rows
def run_rows(eng, cus, c, W, kinds=(True, False), keep=None):
    """One RowCase: exact and general operands, unweighted and weighted, every output against its reference; guards, inputs and NaN
    padding unchanged.  keep: a dict that receives the raw outputs by (exact, has_w)."""
    from trips_py_amd import _lib
    k, m = c.k, c.m
    for exact in kinds:
        d = C.rows_case(k, m, exact)
        D = Dev(eng, d, ld=c.ld, mis=MIS[c.mis], rows=k)
        D.basis()
        D.inp("w", d.w)
        D.inp("b", d.b)
        snap = {nm: D.bufs[nm][0].clone() for nm in ("w", "b")}
        for has_w in (False, True):
            p = c.check(has_w, cus)
            R = C.gram_ref(d.V, k, d.w if has_w else None, d.b if c.has_b else None, m, pair_path=p["kernel"] == "k_wgram", exact=exact)
            G, c1, c2 = Scal(eng, k * k), Scal(eng, k), Scal(eng, k)
            rc = eng.lib.trk_wgram(addr(D, "V"), c.ld, k, m, addr(D, "w") if has_w else None, addr(D, "b") if c.has_b else None,
                                   G.ref(), c1.ref() if c.has_b else None, c2.ref() if c.has_b else None, eng.stream())
            _lib.check(rc, f"trk_wgram {c.name}")
            g, h1, h2 = G.values(), c1.values(), c2.values()
            assert np.array_equal(g.reshape(k, k), g.reshape(k, k).T), (c.name, "G is not symmetric to the bit")
            name = path_of(p)
            W.see(f"{name}.G", g, R["G"], exact)
            if c.has_b:
                W.see(f"{name}.c1", h1, R["c1"], exact)
                W.see(f"{name}.c2", h2, R["c2"], exact)
            else:
                assert np.all(h1 == SENTINEL) and np.all(h2 == SENTINEL)
            D.check()
            for nm, s in snap.items():
                assert torch.equal(D.bufs[nm][0].view(torch.int32), s.view(torch.int32)), f"{nm} was written to"
            if keep is not None:
                keep[(exact, has_w)] = (g, h1, h2)


def by_name(cases):
    return {c.name: c for c in cases}


@pytest.mark.parametrize("KA", C.LAYOUT_KA)
def test_row_layouts(eng, cus, KA):
    """T = 1, 2, 3 at both ends of each tile count: ld == m, padded ld with every m % 4 (16-byte body + scalar tail, NaN behind every
    row), odd ld (k_wgram_mfma), and W, w, b1 in turn one float off a 16-byte boundary."""
    W = Bars()
    for c in C.layout_cases(KA):
        run_rows(eng, cus, c, W)
    W.flush(f"layouts-KA{KA}")


def test_ladders(eng, cus):
    """KA = 48 | 49 and 64 | 65 with b, and 16 | 17, 32 | 33, 48 | 49, 64 | 65 without, aligned and with an odd leading dimension."""
    W = Bars()
    for c in C.ladder_cases():
        run_rows(eng, cus, c, W)
    W.flush("ladders")


@pytest.mark.parametrize("name", [c.name for T in (1, 2, 3) for c in C.group_cases(T, REF_CUS)])
def test_groups_per_wave(eng, cus, name):
    """The software-pipelined loop of k_wgram_t16: m = 32 (j gs + r) + tail on this device's gs waves."""
    T = int(name[1])
    W = Bars()
    run_rows(eng, cus, by_name(C.group_cases(T, cus))[name], W)
    W.flush(name)


@pytest.mark.parametrize("name", [c.name for nt in (1, 2) for c in C.chunk_cases(nt, REF_CUS)])
def test_chunks_per_workgroup(eng, cus, name):
    """k_wgram_mfma's chunk loop: accd carried across chunks, a full chunk followed by a ragged one in the same workgroup."""
    nt = int(name[4])
    W = Bars()
    run_rows(eng, cus, by_name(C.chunk_cases(nt, cus))[name], W)
    W.flush(name)


def test_short_rows_one_row_and_512_rows(eng, cus):
    """m = 0 (all zeros), 1, 31, 33, 127, 129 on every kernel; k = 1; k = 512 (8256 tile pairs)."""
    W = Bars()
    for c in C.edge_cases():
        keep = {}
        run_rows(eng, cus, c, W, keep=keep)
        if c.m == 0:
            for g, h1, h2 in keep.values():
                assert not g.any() and (not c.has_b or (not h1.any() and not h2.any()))
    W.flush("edges")


def test_a_small_problem_after_a_large_one_and_the_same_call_twice(eng, cus):
    """The scratch of the large call is reused by the small one on the same stream; a repeated call leaves the same bits."""
    W = Bars()
    big = by_name(C.group_cases(2, cus))["T2b-j2-pair"]
    small = by_name(C.layout_cases(17))["KA17b-pad1-tail5"]
    for c in (big, small, by_name(C.chunk_cases(1, cus))["mfma1b-odd-j1-r1"], small, by_name(C.ladder_cases())["k63b-odd_ld"], small):
        first, again = {}, {}
        run_rows(eng, cus, c, W, kinds=(True,), keep=first)
        run_rows(eng, cus, c, W, kinds=(False,), keep=first)
        run_rows(eng, cus, c, W, kinds=(False,), keep=again)
        for key, outs in again.items():
            assert all(np.array_equal(a, b) for a, b in zip(outs, first[key])), (c.name, key)
    W.flush("reuse")


def test_argument_contract(eng):
    """k = 0, k = 513, ld < m, b1 with c1 / c2 NULL: an error code, nothing launched, the outputs untouched."""
    d = C.rows_case(3, 260, True)
    D = Dev(eng, d, ld=260, rows=3)
    D.basis()
    D.inp("w", d.w)
    D.inp("b", d.b)
    G, c1, c2 = Scal(eng, 9), Scal(eng, 3), Scal(eng, 3)
    V, w, b, st, f = addr(D, "V"), addr(D, "w"), addr(D, "b"), eng.stream(), eng.lib.trk_wgram
    assert f(V, 260, 0, 260, w, b, G.ref(), c1.ref(), c2.ref(), st) != 0
    assert f(V, 260, 513, 260, w, b, G.ref(), c1.ref(), c2.ref(), st) != 0
    assert f(V, 256, 3, 260, w, b, G.ref(), c1.ref(), c2.ref(), st) != 0
    assert f(V, 260, 3, -1, w, b, G.ref(), c1.ref(), c2.ref(), st) != 0
    assert f(V, 260, 3, 260, w, b, G.ref(), None, c2.ref(), st) != 0
    assert f(V, 260, 3, 260, w, b, G.ref(), c1.ref(), None, st) != 0
    assert f(None, 260, 3, 260, w, b, G.ref(), c1.ref(), c2.ref(), st) != 0
    assert f(V, 260, 3, 260, w, b, None, c1.ref(), c2.ref(), st) != 0
    eng.synchronize()
    assert all(np.all(s.values() == SENTINEL) for s in (G, c1, c2))
    D.check()
    assert f(V, 260, 3, 260, w, b, G.ref(), c1.ref(), c2.ref(), st) == 0          # ... and the legal call still runs
    assert np.array_equal(G.values(), C.gram_ref(d.V, 3, d.w, d.b, 260, exact=True)["G"].ref)


# ------------------------------------------------------------------------------------------------------------ TV Gram
REG_CASES = C.tv_register_cases()
LDS_CASES = C.tv_lds_cases()
KMAX = {}
for _c in REG_CASES + LDS_CASES:
    KMAX[_c.N] = max(KMAX.get(_c.N, 0), _c.k)
HOST_REF_MAX_N = 256
_TV = {}


def _guarded(eng, host, fill=None):
    n = len(host)
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=eng.device)
    buf[GUARD:GUARD + n] = up(eng, host).float() * (fill or 1.0)
    return buf, buf[GUARD:GUARD + n]


class TvDev:
    """The operands of the TV cases of one (N, exact) for the largest k run at that N: V with NaN padding behind every row (ld = N^2 + 4),
    w and z, each between guard floats, and the float64 references G [kmax, kmax], h [kmax], Sh (the absolute terms of h)."""

    def __init__(self, eng, N, exact, kmax):
        self.eng, self.N, self.k, self.exact = eng, N, kmax, exact
        n = N * N
        self.ld = n + 4
        Vh, wh, zh = C.tv_operands(kmax, N, exact, as_int8=exact)
        scale = 0.125 if exact else None
        self.Vbuf = torch.full((GUARD + kmax * self.ld + GUARD,), float("nan"), dtype=torch.float32, device=eng.device)
        self.Vbuf[:GUARD] = SENTINEL
        self.Vbuf[GUARD + kmax * self.ld:] = SENTINEL
        self.V = self.Vbuf[GUARD:GUARD + kmax * self.ld].view(kmax, self.ld)[:, :n]
        for j in range(kmax):
            self.V[j] = up(eng, Vh[j]).float() * (scale or 1.0)
        self.wbuf, self.w = _guarded(eng, wh)
        self.zbuf, self.z = _guarded(eng, zh, scale)
        assert self.V.data_ptr() % 16 == 0 and self.w.data_ptr() % 16 == 0 and self.z.data_ptr() % 16 == 0 and self.V.stride(0) == self.ld
        self.snap = [b.clone() for b in (self.Vbuf, self.wbuf, self.zbuf)]
        if N <= HOST_REF_MAX_N:
            Vf = Vh.astype(np.float32) * np.float32(0.125) if exact else Vh
            zf = zh.astype(np.float32) * np.float32(0.125) if exact else zh
            self.G, self.h = C.tv_ref_host(Vf, N, wh, zf)
            self.Sh = np.abs(Vf).astype(np.float64) @ np.abs(zf).astype(np.float64)
            if N <= 128:
                Go = C.tv_ref_oracle(Vf, N, wh)
                assert np.array_equal(self.G, Go) if exact else C.tv_relative(self.G, Go) < 4 * 2.0 ** -24 * (1 + 2.0 ** -20)
        else:
            self.G = self.device_reference()
            self.h = (self.V.double() @ self.z.double()).cpu().numpy()
            self.Sh = (self.V.abs().double() @ self.z.abs().double()).cpu().numpy()
        assert np.array_equal(self.G, self.G.T)

    def device_reference(self):
        """float64 on the device with plain torch slicing, in row blocks, from d = fl32(fl32(x - x') w)."""
        k, N, w = self.k, self.N, self.w
        X3 = self.Vbuf[GUARD:].as_strided((k, N, N), (self.ld, N, 1))
        wh, wv = w[:N * (N - 1)].reshape(N, N - 1), w[N * (N - 1):].reshape(N - 1, N)
        ref = torch.zeros(k, k, dtype=torch.float64, device=self.eng.device)
        B = 128
        for lo in range(0, N, B):
            hi = min(lo + B, N)
            X = X3[:, lo:min(hi + 1, N), :]
            dh = ((X[:, :hi - lo, :-1] - X[:, :hi - lo, 1:]) * wh[lo:hi]).double().reshape(k, -1)
            ref += dh @ dh.T
            nv = min(hi, N - 1) - lo
            if nv > 0:
                dv = ((X[:, :nv, :] - X[:, 1:nv + 1, :]) * wv[lo:lo + nv]).double().reshape(k, -1)
                ref += dv @ dv.T
        ref = ref.cpu().numpy()
        return np.triu(ref) + np.triu(ref, 1).T

    def check(self):
        for b, s, nm in zip((self.Vbuf, self.wbuf, self.zbuf), self.snap, "Vwz"):
            assert torch.equal(b.view(torch.int32), s.view(torch.int32)), f"{nm} (guards and NaN padding included) was written to"

    def run(self, k, with_z):
        """One call on the leading k vectors: (G [k, k], h [k] or None)."""
        G, H = Scal(self.eng, k * k), Scal(self.eng, k)
        if with_z:
            self.eng.wgram_tv(self.V[:k], k, self.N, self.w, G.ref(), z=self.z, h=H.ref())
        else:
            self.eng.wgram_tv(self.V[:k], k, self.N, self.w, G.ref())
        g, h = G.values().reshape(k, k), H.values()
        assert np.array_equal(g, g.T), "G is not symmetric to the bit"
        if not with_z:
            assert np.all(h == SENTINEL)
        self.check()
        return g, (h if with_z else None)


def tv_dev(eng, N, exact):
    """One TvDev per (N, exact), shared by the tests; those of another N are dropped first (the largest is 0.8 GB)."""
    if (N, exact) not in _TV:
        for key in [key for key in _TV if key[0] != N]:
            del _TV[key]
        _TV[(N, exact)] = TvDev(eng, N, exact, KMAX[N])
    return _TV[(N, exact)]


def tv_exact(eng, cus, F, cases, modes=C.TV_MODES):
    """Every case on exact operands in every mode: G and h EQUAL the leading blocks of the reference."""
    was = eng.wgram_tv_precision()
    try:
        for mode in modes:
            eng.wgram_tv_precision(mode)
            for c in cases:
                c.check(mode, cus)
                g, h = F.run(c.k, c.with_z)
                bad = np.argwhere(g != F.G[:c.k, :c.k])
                assert bad.size == 0, (c.name, mode, len(bad), bad[:6].tolist(), (g - F.G[:c.k, :c.k])[tuple(bad[:6].T)])
                if c.with_z:
                    assert np.array_equal(h, F.h[:c.k]), (c.name, mode, np.flatnonzero(h != F.h[:c.k])[:6])
    finally:
        eng.wgram_tv_precision(was)


REG_NK = sorted({(c.N, c.k) for c in REG_CASES})


@pytest.mark.parametrize("N,k", REG_NK)
def test_tv_register_fed_exact(eng, cus, N, k):
    """k_wgram_tv on exact operands, all four modes, with and without z (the cases of this (N, k): wgram_cases.tv_register_cases)."""
    cases = [c for c in REG_CASES if (c.N, c.k) == (N, k)]
    assert cases
    tv_exact(eng, cus, tv_dev(eng, N, True), cases)


@pytest.mark.parametrize("with_z", [False, True], ids=["plain", "z"])
@pytest.mark.parametrize("mode", C.TV_MODES)
def test_tv_lds_exact(eng, cus, mode, with_z):
    """k_wgram_tv_lds at N = 2048 for EVERY k from 1 to 32 (each a pattern of staged loads and vmcnt waits of its own) against the
    leading blocks of one k = 48 reference."""
    cases = [c for c in LDS_CASES if c.N == 2048 and c.with_z == with_z]
    assert [c.k for c in cases] == list(range(1, 33))
    tv_exact(eng, cus, tv_dev(eng, 2048, True), cases, modes=(mode,))


def test_tv_lds_exact_nine_tiles(eng, cus):
    """k = 20 at N = 2304: nine 256-column tiles, dealt to the workgroups without the XCD map."""
    cases = [c for c in LDS_CASES if c.N == 2304]
    assert len(cases) == 2
    tv_exact(eng, cus, tv_dev(eng, 2304, True), cases)


@pytest.mark.parametrize("N,k", [(96, 32), (1024, 20)])
def test_tv_equals_the_gram_of_the_stored_images_exactly(eng, N, k):
    """trk_wgram_tv == trk_wgram over the stored L v_j (L.apply: pinned by tests/tv_cases.py) on exact operands, to the bit."""
    from trips_py_amd.operators import FirstDerivative2D
    F = tv_dev(eng, N, True)
    L = FirstDerivative2D(N, engine=eng)
    LV = torch.empty(k, 2 * N * (N - 1), device=eng.device)
    for j in range(k):
        L.apply(F.V[j].contiguous(), out=LV[j])
    G = Scal(eng, k * k)
    eng.wgram(LV, k, F.w, None, G.ref())
    g, _ = F.run(k, False)
    assert np.array_equal(G.values().reshape(k, k), g) and np.array_equal(g, F.G[:k, :k])


@pytest.mark.parametrize("N,k", C.TV_GENERAL)
def test_tv_general(eng, cus, N, k):
    """General operands on the register-fed kernel (one shape of each T, and lockstep with the XCD map): the limits of include/trk.h per
    mode relative to sqrt(G_aa G_bb); h within the float64 dot bound; 'auto' on such data IS the two-piece form (verdict 0)."""
    F = tv_dev(eng, N, False)
    Gr, hr = F.G[:k, :k], F.h[:k]
    was = eng.wgram_tv_precision()
    got = {}
    try:
        for mode in C.TV_MODES:
            eng.wgram_tv_precision(mode)
            for z in (False, True):
                p = C.wgram_tv_plan(k, N, z, mode, cus)
                assert p["kernel"] == "k_wgram_tv" and p["targs"][0] == C.ceil_div(k, 16) and p["targs"][-1] == C.TV_BF[mode]
                if N == 1024:
                    assert p["xcd_map"] and p["lock"] == (not z)
                g, h = F.run(k, z)
                got[(mode, z)] = (g, h)
                if mode == "auto":
                    verdict, sampled = eng.wgram_tv_last_probe()
                    assert verdict == 0 and sampled <= 3e-7, (verdict, sampled)
                bar(f"wgram_tv.entrywise[N{N}-k{k}{'-z' if z else ''}-{mode}]", C.tv_relative(g, Gr), C.TV_LIMIT[mode])
                if z:
                    assert np.all(np.abs(h - hr) <= N * N * C.U53 * F.Sh[:k]), (mode, np.max(np.abs(h - hr) / F.Sh[:k]))
    finally:
        eng.wgram_tv_precision(was)
    for z in (False, True):
        assert np.array_equal(got[("auto", z)][0], got[("bf16x2", z)][0])
    assert all(np.array_equal(got[(mode, True)][1], got[("fp32", True)][1]) for mode in C.TV_MODES)      # the dots do not depend on the mode


@pytest.mark.parametrize("N,k", [(2048, 33), (2048, 24)], ids=["register-fed", "lds"])
def test_tv_auto_with_verdict_1_is_the_fp32_form(eng, cus, N, k):
    """'auto' on an image of repeated values (verdict 1) leaves the bits of 'fp32', on one register-fed and one LDS shape."""
    from test_gpu_kernels import _adversarial_basis
    from trips_py_amd.operators import FirstDerivative2D
    assert C.wgram_tv_plan(k, N, False, "auto", cus)["use_lds"] == (k <= 32)
    V = _adversarial_basis("constant_steps", k, N, eng.device)
    w = torch.empty(2 * N * (N - 1), device=eng.device)
    FirstDerivative2D(N, engine=eng).tv_weights(V[0].contiguous(), 0.1, 1.0, w)
    z = V[k - 1].clone()
    was = eng.wgram_tv_precision()
    out = {}
    try:
        for mode in ("auto", "fp32", "bf16x2"):
            eng.wgram_tv_precision(mode)
            for with_z in (False, True):
                G, H = Scal(eng, k * k), Scal(eng, k)
                if with_z:
                    eng.wgram_tv(V, k, N, w, G.ref(), z=z, h=H.ref())
                else:
                    eng.wgram_tv(V, k, N, w, G.ref())
                if mode == "auto":
                    verdict, sampled = eng.wgram_tv_last_probe()
                    assert verdict == 1 and sampled > 3e-7, (verdict, sampled)
                out[(mode, with_z)] = (G.values(), H.values())
    finally:
        eng.wgram_tv_precision(was)
    for with_z in (False, True):
        assert np.array_equal(out[("auto", with_z)][0], out[("fp32", with_z)][0])
        assert np.array_equal(out[("auto", with_z)][1], out[("fp32", with_z)][1])
        assert not np.array_equal(out[("auto", with_z)][0], out[("bf16x2", with_z)][0])
