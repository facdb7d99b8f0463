"""PDHG with isotropic space-time TV on the GPU (k_pdhg_tv_dual<kTriples, .> and k_pdhg_tv_primal<., true> in csrc/pdhg_tv.hip, the
entry points there and in csrc/pdhg.hip, solvers/PDHG.py tv='iso3') against the NumPy restatement of tests/pdhg_iso3_cases.py: one
launch of each dual form against the storage-faithful form, crafted groups, the fused pair against the unfused path (bit for bit), the
one-call C loop against single steps (bit for bit), whole solves against the float64 form, argument checks, and the routing of the
older modes.

The three modes share one dual template k_pdhg_tv_dual<Groups, FUSED> and one primal template k_pdhg_tv_primal<HAS_XT, TEMPORAL>.
Which test of this file reaches which instantiation (the kRows dual and the rest of the 2-D ones: test_gpu_pdhg.py, test_gpu_pdhg_iso.py):

  entry point                               kernel<template arguments>             covering test
  trk_pdhg_st_dual_iso3                     k_pdhg_tv_dual<kTriples, true>         fused_dual_against_the_restatement, crafted_*, fused_equals_unfused,
                                                                                   one_frame_is_the_2d_fused_pair, run_equals_steps, solve_against_float64
  trk_pdhg_dual_q_iso3                      k_pdhg_tv_dual<kTriples, false>        unfused_dual_against_the_restatement, one_frame_is_the_isotropic_dual,
                                                                                   crafted_*, fused_equals_unfused, run_equals_steps (fused=False, csr)
  trk_pdhg_dual_q_iso                       k_pdhg_tv_dual<kPairs, false>          one_frame_is_the_isotropic_dual, fused_equals_unfused (frames in z),
                                                                                   old_routing_is_unchanged
  trk_pdhg_tv_dual_iso                      k_pdhg_tv_dual<kPairs, true>           one_frame_is_the_2d_fused_pair, old_routing_is_unchanged
  trk_pdhg_st_primal, x_true                k_pdhg_tv_primal<true, true>           fused_equals_unfused[True], one_frame_is_the_2d_fused_pair,
                                                                                   run_equals_steps, solve_against_float64
  trk_pdhg_st_primal, no x_true             k_pdhg_tv_primal<false, true>          fused_equals_unfused[False], one_frame_is_the_2d_fused_pair
  trk_pdhg_tv_primal, x_true / none         k_pdhg_tv_primal<true / false, false>  one_frame_is_the_2d_fused_pair, old_routing_is_unchanged (none)
  the argument checks of all of them        (no kernel)                            argument_checks_come_first"""
import numpy as np
import pytest
import torch

import pdhg_cases as C
import pdhg_iso3_cases as T
import pdhg_iso_cases as I
from conftest import bar
from test_gpu_pdhg import CAP, _dev, _sums_match, _ulps

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SIGMA, LAM, TAU, LO, HI = 0.37, 0.1, 0.21, 0.2, 0.8      # |q + sigma u| falls on both sides of lam on random images
NT, RB, MAX_BLOCKS = 256, 4, 4096                        # the kernels' column block, row batch and block cap

# The grid rule: gx = ceil(N / 256) column blocks, gy = ceil(N / 4) row batches, one launch over the frames, and gy cut to
# 4096 // (gx frames) (at least 1) where gx gy frames > 4096.  A block strides over more than one row batch where
# ceil(N / 4) > 4096 // (ceil(N / 256) frames).  With N a multiple of 256 that needs N^2 frames > 4 M unknowns; one column past a
# multiple doubles gx for almost no unknowns: N = 257 has 2 x 65 = 130 blocks per frame, 31 frames fit (4030) and 32 do not (4160 >
# 4096, gy = 4096 // 64 = 64 < 65), at 257^2 x 32 = 2.1 M unknowns: the smallest such shape near 2 M.
CAPPED = (257, 32)
SIZES = [(2, 2), (5, 3), (16, 3), (33, 2), (257, 2), (260, 3), CAPPED]


@pytest.fixture(scope="module")
def eng():
    from trips_py_amd.engine import default_engine
    return default_engine()


def _grid3(N, frames):
    gx, gy = (N + NT - 1) // NT, (N + RB - 1) // RB
    return gx * min(gy, max(MAX_BLOCKS // (gx * frames), 1)) * frames


_inputs, _dual_ref = {}, {}


def _st_inputs(N, frames):
    """Seeded image vectors, a dual inside every ball (|q| <= 0.05 < lam / sqrt 3) and a stored u, computed once per size."""
    if (N, frames) not in _inputs:
        rng = np.random.default_rng(7 * N + frames)
        n, r = N * N * frames, T.rows_of(N, frames)
        _inputs[(N, frames)] = {"xbar": rng.random(n).astype(F32), "q": (0.1 * rng.random(r) - 0.05).astype(F32),
                                "x": rng.random(n).astype(F32), "z": (0.2 * rng.random(n) - 0.1).astype(F32),
                                "xt": rng.random(n).astype(F32), "u": (rng.random(r) - 0.5).astype(F32)}
    return _inputs[(N, frames)]


def _fused_reference(N, frames):
    """(u, (q', s1, s3)) of the restatement on the fused inputs, computed once per size."""
    if (N, frames) not in _dual_ref:
        v = _st_inputs(N, frames)
        u = T.st_fwd_f32(N, frames, v["xbar"])
        _dual_ref[(N, frames)] = (u, T.dual_q_iso3_f32(N, frames, SIGMA, LAM, u, v["q"]))
    return _dual_ref[(N, frames)]


def _check_projection(N, frames, sigma, lam, u, q, qh, both):
    """What the projection promises of q' = qh whatever the rounding: singles inside [-lf, lf] exactly, every group's float64 norm
    <= lf (1 + 8 * 2^-24) (include/trk.h derives 1 + 4.5 * 2^-24 for a triple and 1 + 4 * 2^-24 for a pair), and a group the
    restatement keeps (m <= lf) is t = fmaf(sf, u, q) itself.  both: every kind must have kept and scaled groups — asked of the
    restatement's own mask first, so that a failure of the equalities after it is the kernel's."""
    sf, lf = F32(sigma), F32(lam)
    g = T.groups3(N, frames)
    assert np.all(np.isfinite(qh))
    sg = g["single"]
    assert np.all((qh[sg] >= -lf) & (qh[sg] <= lf))
    norms = T.group_norms(N, frames, qh)
    assert max(v.max(initial=0.0) for v in norms.values()) <= F64(lf) * (1 + 8 * 2.0 ** -24)
    keeps = {}
    for kind in ("hvt", "hv", "ht", "vt"):
        rows = g[kind]
        t = [C.fma32(sf, u[r], q[r]) for r in rows]
        if kind == "hvt":
            m2 = I.fma32_arrays(t[0], t[0], I.fma32_arrays(t[1], t[1], t[2] * t[2]))
        else:
            m2 = I.fma32_arrays(t[0], t[0], t[1] * t[1])
        keeps[kind] = keep = np.sqrt(m2) <= lf
        if both:
            assert 0 < np.count_nonzero(keep) < keep.size, (kind, np.count_nonzero(keep), keep.size)
        for r, tr in zip(rows, t):
            assert np.array_equal(qh[r][keep], tr[keep]), kind                    # a kept group is t itself
    ts = C.fma32(sf, u[sg], q[sg])
    keeps["single"] = keep = np.abs(ts) <= lf
    if both:
        assert 0 < np.count_nonzero(keep) < keep.size
    assert np.array_equal(qh[sg][keep], ts[keep])
    return keeps


def _check_partials(NP, nb, want, tag):
    parts = NP.host().reshape(CAP, 8)
    assert not parts[nb:].any() and not parts[:, [0, 2, 4, 5, 6, 7]].any(), tag    # slots 1 and 3 of the blocks that ran only
    _sums_match(parts.sum(axis=0)[[1, 3]], want, tag)


# ====================================================================== (1) the fused dual, one launch
@pytest.mark.parametrize("N,frames", SIZES)
def test_fused_dual_against_the_restatement(eng, N, frames):
    """(2, 2): one triple; (5, 3): a ragged row batch; (16, 3): Q5's shape; (257, 2): the 256-thread column block crossed; CAPPED:
    the grid cap makes a block stride over two row batches."""
    from trips_py_amd.operators import SpaceTimeDerivative
    L = SpaceTimeDerivative(N, frames, engine=eng)
    v = _st_inputs(N, frames)
    q, NP = eng.to_vec(v["q"]), eng.scalars(8 * CAP)
    nb = eng.pdhg_st_dual_iso3(L._h, SIGMA, LAM, eng.to_vec(v["xbar"]), q, NP.ref(0), CAP)
    assert nb == _grid3(N, frames) == eng.pdhg_blocks_iso3(1, 1, T.rows_of(N, frames), N, frames, L._h)
    gx, batches = (N + NT - 1) // NT, (N + RB - 1) // RB
    if (N, frames) == CAPPED:
        assert nb == 4096 and nb // (gx * frames) == 64 < batches == 65          # the 65th batch is a second one of a block's
    else:
        assert nb == gx * batches * frames
    u, (qn, s1, s3) = _fused_reference(N, frames)
    qh = q.cpu().numpy()
    print((N, frames), "ulps", _ulps(qh, qn))
    assert _ulps(qh, qn) <= 1
    _check_partials(NP, nb, [s1, s3], (N, frames))
    _check_projection(N, frames, SIGMA, LAM, u, v["q"], qh, both=N >= 16)


# ====================================================================== (2) the unfused dual
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("N,frames", SIZES[:-1])
def test_unfused_dual_against_the_restatement(eng, N, frames, offset):
    """u = L xbar in memory (any operator with the row layout); offset1 moves both operands one float off a 16-byte boundary."""
    v = _st_inputs(N, frames)
    u, q0 = v["u"], v["q"]
    ud, q, NP = _dev(eng, u, offset), _dev(eng, q0, offset), eng.scalars(8 * CAP)
    nb = eng.pdhg_dual_q_iso3(N, frames, SIGMA, LAM, ud, q, NP.ref(0), CAP)
    assert nb == _grid3(N, frames) == eng.pdhg_blocks_iso3(1, 1, u.size, N, frames)
    qn, s1, s3 = T.dual_q_iso3_f32(N, frames, SIGMA, LAM, u, q0)
    qh = q.cpu().numpy()
    print((N, frames), "ulps", _ulps(qh, qn))
    assert _ulps(qh, qn) <= 1
    _check_partials(NP, nb, [s1, s3], (N, frames))
    _check_projection(N, frames, SIGMA, LAM, u, q0, qh, both=N >= 16)


@pytest.mark.parametrize("N", [2, 5, 33, 260])
def test_one_frame_is_the_isotropic_dual(eng, N):
    """frames = 1: every group is a pair or a single of tv='iso': the bits of pdhg_dual_q_iso on the same operands."""
    rng = np.random.default_rng(N)
    rows = 2 * N * (N - 1)
    u, q0 = (rng.random(rows) - 0.5).astype(F32), (0.1 * rng.random(rows) - 0.05).astype(F32)
    ud, q3, q2, NP3, NP2 = eng.to_vec(u), eng.to_vec(q0), eng.to_vec(q0), eng.scalars(8 * CAP), eng.scalars(8 * CAP)
    eng.pdhg_dual_q_iso3(N, 1, SIGMA, LAM, ud, q3, NP3.ref(0), CAP)
    eng.pdhg_dual_q_iso(N, 1, SIGMA, LAM, ud, q2, NP2.ref(0), CAP)
    assert torch.equal(q3, q2) and not torch.equal(q3, eng.to_vec(q0))
    c3, c2 = NP3.host().reshape(CAP, 8).sum(axis=0), NP2.host().reshape(CAP, 8).sum(axis=0)
    _sums_match(c3[[1, 3]], c2[[1, 3]], N)


@pytest.mark.parametrize("N", [2, 5, 33, 260])
def test_one_frame_is_the_2d_fused_pair(eng, N):
    """frames = 1: the space-time handle's fused pair leaves the bits of the 2-D handle's fused pair on the same operands — the
    kTriples dual with no temporal member against the kPairs dual, the TEMPORAL primal with both neighbours NULL against the
    plain one.  At one frame grid3 is grid2, so every block's row of partials is compared as it stands.  2: the smallest; 5: an odd
    batch tail; 33: short of a 64-lane wave by half; 260: a second column block."""
    from trips_py_amd.operators import FirstDerivative2D, SpaceTimeDerivative
    L3, L2 = SpaceTimeDerivative(N, 1, engine=eng), FirstDerivative2D(N, engine=eng)
    d = {k: eng.to_vec(a) for k, a in _st_inputs(N, 1).items()}
    q3, q2, NP3, NP2 = d["q"].clone(), d["q"].clone(), eng.scalars(8 * CAP), eng.scalars(8 * CAP)
    nb = eng.pdhg_st_dual_iso3(L3._h, SIGMA, LAM, d["xbar"], q3, NP3.ref(0), CAP)
    assert nb == eng.pdhg_tv_dual_iso(L2._h, SIGMA, LAM, d["xbar"], q2, NP2.ref(0), CAP) == _grid3(N, 1)
    assert torch.equal(q3, q2) and not torch.equal(q3, d["q"])
    p3, p2 = NP3.host().reshape(CAP, 8), NP2.host().reshape(CAP, 8)
    assert np.array_equal(p3[:, [1, 3]], p2[:, [1, 3]]) and p3[:nb, 1].all()
    for xt in (d["xt"], None):
        x3, b3, x2, b2 = (torch.empty_like(d["x"]) for _ in range(4))
        NP3, NP2 = eng.scalars(8 * CAP), eng.scalars(8 * CAP)
        assert eng.pdhg_st_primal(L3._h, TAU, LO, HI, d["x"], d["z"], q3, x3, b3, xt, NP3.ref(0), CAP) == nb
        assert eng.pdhg_tv_primal(L2._h, TAU, LO, HI, d["x"], d["z"], q2, x2, b2, xt, NP2.ref(0), CAP) == nb
        assert torch.equal(x3, x2) and torch.equal(b3, b2) and not torch.equal(x3, d["x"])
        p3, p2 = NP3.host().reshape(CAP, 8), NP2.host().reshape(CAP, 8)
        assert np.array_equal(p3[:, 4:], p2[:, 4:]) and p3[:nb, 4].all() and (xt is None) == (not p3[:, 6].any())


# ====================================================================== (3) crafted groups through both dual forms
# (2, 2): rows [H0: 0 1 | V0: 2 3 | H1: 4 5 | V1: 6 7 | T0: 8 9 10 11]; the triple is (0, 2, 8) of voxel (0, 0, 0), the (h, t) pair
# (1, 10) of voxel (0, 1, 0) on the last image row, the (v, t) pair (3, 9) of voxel (0, 0, 1) on the last image column.
# sigma = 0.5; (lam, q, u) -> q', every number exact in fp32
CRAFTED_TRIPLES = {"kept": (7.0, (1.0, 1.0, 2.0), (2.0, 4.0, 8.0), (2.0, 3.0, 6.0)),                       # t = (2, 3, 6), m = 7 <= 7
                   "scaled": (3.5, (1.0, 1.0, 2.0), (2.0, 4.0, 8.0), (1.0, 1.5, 3.0)),                     # s = 0.5
                   "on_the_ball_pushed_outward": (7.0, (2.0, 3.0, 6.0), (4.0, 6.0, 12.0), (2.0, 3.0, 6.0)),   # t = (4, 6, 12): q' = q
                   "one_member_zero": (2.5, (0.0, 1.0, 2.0), (0.0, 4.0, 4.0), (0.0, 1.5, 2.0)),            # t = (0, 3, 4), s = 0.5
                   "two_members_zero": (2.0, (0.0, 0.0, 2.0), (0.0, 0.0, 4.0), (0.0, 0.0, 2.0)),           # t = (0, 0, 4), s = 0.5
                   "lam_zero_t_zero": (0.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),            # m = 0 <= 0: kept, no 0 / 0
                   "lam_zero_t_nonzero": (0.0, (0.0, 0.0, 0.0), (2.0, 4.0, 8.0), (0.0, 0.0, 0.0)),         # s = 0 / m = 0
                   "lands_on_the_ball": (7.0, (1.0, 1.5, 3.0), (2.0, 3.0, 6.0), (2.0, 3.0, 6.0))}          # q inside, |t| = lam exactly


def _both_forms(eng, lam, img, q0, qn, s1, s3, tag):
    from trips_py_amd.operators import SpaceTimeDerivative
    L = SpaceTimeDerivative(2, 2, engine=eng)
    u = T.st_fwd_f32(2, 2, img)
    for form in ("unfused", "fused"):
        q, NP = eng.to_vec(q0), eng.scalars(8 * CAP)
        if form == "fused":
            nb = eng.pdhg_st_dual_iso3(L._h, 0.5, lam, eng.to_vec(img), q, NP.ref(0), CAP)
        else:
            nb = eng.pdhg_dual_q_iso3(2, 2, 0.5, lam, eng.to_vec(u), q, NP.ref(0), CAP)
        got = q.cpu().numpy()
        assert nb == 2 and np.array_equal(got, qn) and np.all(np.isfinite(got)), (tag, form, got, qn)
        cols = NP.host().reshape(CAP, 8).sum(axis=0)
        _sums_match(cols[[1, 3]], [s1, s3], (tag, form))
        assert np.isfinite(cols).all()


@pytest.mark.parametrize("case", list(CRAFTED_TRIPLES))
def test_crafted_triples(eng, case):
    lam, (qh0, qv0, qt0), (uh, uv, ut), want = CRAFTED_TRIPLES[case]
    a = 32.0
    b, c, e = a - uh, a - uv, a - ut
    img = np.array([a, b, c, c, e, b, c, c], dtype=F32)      # frame 0 [[a, b], [c, c]], frame 1 [[e, b], [c, c]]
    u = T.st_fwd_f32(2, 2, img)
    assert (u[0], u[2], u[8]) == (uh, uv, ut)
    q0 = np.full(12, 0.25, dtype=F32)
    q0[[0, 2, 8]] = (qh0, qv0, qt0)
    qn, s1, s3 = T.dual_q_iso3_f32(2, 2, 0.5, lam, u, q0)
    assert tuple(qn[[0, 2, 8]]) == want                      # the restatement gives the exact values
    _both_forms(eng, lam, img, q0, qn, s1, s3, case)


@pytest.mark.parametrize("lam,want", [(5.0, (3.0, 4.0)), (2.5, (1.5, 2.0))], ids=["kept", "scaled"])
def test_crafted_pairs_with_a_temporal_member(eng, lam, want):
    """t = (3, 4) in the (h, t) pair of the last image row and in the (v, t) pair of the last image column."""
    c = 16.0
    d, g = c - 2.0, c - 4.0                                  # voxel (0, 1, 0): h = c - d = 2, t = c - g = 4
    b = d + 2.0                                              # voxel (0, 0, 1): v = b - d = 2
    f = b - 4.0                                              #                  t = b - f = 4
    img = np.array([c, b, c, d, c, f, g, d], dtype=F32)      # frame 0 [[c, b], [c, d]], frame 1 [[c, f], [g, d]]
    u = T.st_fwd_f32(2, 2, img)
    assert (u[1], u[10]) == (2.0, 4.0) and (u[3], u[9]) == (2.0, 4.0)
    q0 = np.full(12, 0.25, dtype=F32)
    q0[[1, 10, 3, 9]] = 2.0
    qn, s1, s3 = T.dual_q_iso3_f32(2, 2, 0.5, lam, u, q0)
    assert tuple(qn[[1, 10]]) == want and tuple(qn[[3, 9]]) == want
    _both_forms(eng, lam, img, q0, qn, s1, s3, lam)


# ====================================================================== (4) fused = unfused on the space-time handle
@pytest.mark.parametrize("with_xt", [True, False])
@pytest.mark.parametrize("N,frames", SIZES)
def test_fused_equals_unfused(eng, N, frames, with_xt):
    from trips_py_amd.operators import SpaceTimeDerivative
    L = SpaceTimeDerivative(N, frames, engine=eng)
    v = _st_inputs(N, frames)
    d = {k: eng.to_vec(a) for k, a in v.items()}
    xt = d["xt"] if with_xt else None
    qf, qg, NPf, NPg = d["q"].clone(), d["q"].clone(), eng.scalars(8 * CAP), eng.scalars(8 * CAP)
    nbf = eng.pdhg_st_dual_iso3(L._h, SIGMA, LAM, d["xbar"], qf, NPf.ref(0), CAP)
    nbg = eng.pdhg_dual_q_iso3(N, frames, SIGMA, LAM, L.apply(d["xbar"]), qg, NPg.ref(0), CAP)
    assert nbf == nbg and torch.equal(qf, qg) and not torch.equal(qf, d["q"])
    xf, bf, xg, bg = (torch.empty_like(d["x"]) for _ in range(4))
    assert eng.pdhg_st_primal(L._h, TAU, LO, HI, d["x"], d["z"], qf, xf, bf, xt, NPf.ref(0), CAP) == nbf
    eng.pdhg_primal(TAU, LO, HI, d["x"], d["z"], L.apply(qg, transpose=True), xg, bg, xt, NPg.ref(0), CAP)
    assert torch.equal(xf, xg) and torch.equal(bf, bg)
    pf, pg = NPf.host().reshape(CAP, 8), NPg.host().reshape(CAP, 8)
    assert not pf[nbf:].any() and not pf[:, [0, 2]].any()
    cf, cg = pf.sum(axis=0), pg.sum(axis=0)
    _sums_match(cf[[1, 3, 4, 5, 6]], cg[[1, 3, 4, 5, 6]], (N, frames))
    assert cf[7] == cg[7] and (with_xt or cf[6] == 0.0)
    # the fused primal against the restatement, which gathers the device's q'
    xn, xb, tail = T.st_primal_f32(N, frames, TAU, LO, HI, v["x"], v["z"], qf.cpu().numpy(), v["xt"] if with_xt else None)
    xh = xf.cpu().numpy()
    print((N, frames), "ulps", _ulps(xh, xn), _ulps(bf.cpu().numpy(), xb))
    assert _ulps(xh, xn) <= 1 and _ulps(bf.cpu().numpy(), xb) <= 1
    _sums_match(cf[[4, 5, 6]], tail[:3], (N, frames))
    assert cf[7] == tail[3] == np.count_nonzero((xh == F32(LO)) | (xh == F32(HI)))
    if N >= 16:
        assert 0 < cf[7] < xh.size
    if (N, frames) == (260, 3) and with_xt:                  # x_new may be x
        xa, ba = d["x"].clone(), torch.empty_like(d["x"])
        eng.pdhg_st_primal(L._h, TAU, LO, HI, xa, d["z"], qf, xa, ba, xt, eng.scalars(8 * CAP).ref(0), CAP)
        assert torch.equal(xa, xf) and torch.equal(ba, bf)
    # ... and it is not the spatially isotropic, temporally l1 dual (whose grid, capped per frame, needs more rows than CAP at CAPPED)
    if frames > 1 and (N, frames) != CAPPED:
        qi = d["q"].clone()
        eng.pdhg_dual_q_iso(N, frames, SIGMA, LAM, L.apply(d["xbar"]), qi, eng.scalars(8 * CAP).ref(0), CAP)
        assert not torch.equal(qi, qf)


# ====================================================================== (5) the one-call loop against single steps
K = 12


def _run(eng, name, history=True, fused=None, max_iter=K, csr=False):
    from trips_py_amd.solvers import PDHGRun
    P = T.problem(name)
    if csr:
        from oracle import cpu_ref as O
        from trips_py_amd.operators import SparseOp
        L, dims = SparseOp(O.spacetime_derivative(16, 16, 3), engine=eng), T.GEOMETRY[name]
    else:
        L, dims = P.device_L(eng), None
    return PDHGRun(P.device(eng), P.b, L, P.lam, P.sigma, P.tau, P.lo, P.hi, None, max_iter, P.x_true, history=history,
                   fused=fused, tv="iso3", tv_dims=dims)


def _bits(run):
    run.rows()
    return [t.clone() for t in (run.x_cur, run.xbar, run.p, run.q)], run.S.host().view(np.int64).copy()


def _loop_equals_steps(eng, name, history, **kw):
    ref = _run(eng, name, history, **kw)
    for _ in range(K):
        ref.step()
    want_vecs, want_S = _bits(ref)
    assert np.all(np.isfinite(ref.rows())) and ref.rows()[:, 4].min() > 0
    for calls in ([K], [1, K - 1], [3, 5, K - 8]):
        run = _run(eng, name, history, **kw)
        for c in calls:
            run.run(c)
        assert run.k == K
        vecs, Sb = _bits(run)
        for key, a, b in zip(("x", "xbar", "p", "q"), vecs, want_vecs):
            assert torch.equal(a, b), (calls, key)
        assert np.array_equal(Sb, want_S), calls
    if history is True:
        assert all(torch.equal(ref.slot(k), run.slot(k)) for k in range(K))
    return ref, want_vecs


@pytest.mark.parametrize("history", [True, False, 3])
@pytest.mark.parametrize("name", T.NAMES)
def test_run_equals_steps(eng, name, history):
    ref, want_vecs = _loop_equals_steps(eng, name, history)
    assert ref.fused and ref.geo == T.GEOMETRY[name] and ref.tv == "iso3"
    # the unfused path on the same handle: the same bits, the order of the fp64 sums aside
    gen, gen_vecs = _loop_equals_steps(eng, name, history, fused=False)
    assert not gen.fused
    for key, a, b in zip(("x", "xbar", "p", "q"), gen_vecs, want_vecs):
        assert torch.equal(a, b), ("unfused", key)
    assert np.allclose(gen.rows(), ref.rows(), rtol=1e-12, atol=0)
    # the CSR space-time matrix with tv_dims: unfused, loop = steps bit for bit.  Its transposed product sums a voxel's six terms in
    # the order of the matrix's columns, not the gather's, so against the handle it is the same solve up to fp32 rounding.
    with pytest.raises(ValueError):
        _run(eng, name, history, fused=True, csr=True)
    csr, csr_vecs = _loop_equals_steps(eng, name, history, csr=True)
    assert not csr.fused and csr.geo == T.GEOMETRY[name]
    assert torch.linalg.norm(csr_vecs[0] - want_vecs[0]) <= 1e-5 * torch.linalg.norm(want_vecs[0])
    assert np.allclose(csr.rows()[:, :6], ref.rows()[:, :6], rtol=1e-4, atol=0)


# ====================================================================== (6) whole solves against float64
ITERS = 30
# The worst relative 2-norm distance of the storage-faithful restatement (pdhg_iso3_cases.pdhg_iso3_f32, the fused kernels' order)
# from the float64 restatement over 30 iterates, measured in NumPy on a CPU on the oracle's operators — what fp32 storage alone costs
# (tests/test_pdhg_iso3_host.py recomputes them):
CPU_F32_ITERATES = {"Q5": 1.15e-7, "Q5u": 9.06e-8}
# ... and, in the same two runs, the worst relative deviation of ||A xbar - b|| / ||b|| and of the objective:
CPU_F32_RNRM = {"Q5": 7.54e-8, "Q5u": 4.44e-8}
CPU_F32_OBJECTIVE = {"Q5": 9.74e-8, "Q5u": 7.83e-8}


def _limit(cpu_figure):
    """8 x the cost of fp32 storage alone, never below 1e-5 (the rule of test_gpu_pdhg.py's bars)."""
    return max(8 * cpu_figure, 1e-5)


@pytest.mark.parametrize("name", T.NAMES)
def test_solve_against_float64(eng, name):
    from trips_py_amd.solvers import PDHG
    P, geo = T.problem(name), T.GEOMETRY[name]
    A, L = P.device(eng), P.device_L(eng)
    Apair = C.pair(P.oracle())
    ref = T.f64(name, ITERS, x_true=P.x_true)
    x, info = PDHG(A, P.b, L, P.lam, ITERS, 0, x_true=P.x_true, lower=P.lo, upper=P.hi, sigma=P.sigma, tau=P.tau, tv="iso3")
    assert info["its"] == ITERS and len(info["xHistory"]) == ITERS and info["tv"] == "iso3"
    H = [h.reshape(-1) for h in info["xHistory"]]
    assert all(float(h.min()) >= P.lo and float(h.max()) <= P.hi for h in H)
    worst = max(np.linalg.norm(h - xr) / np.linalg.norm(xr) for h, xr in zip(H, ref["X"]))
    bar(f"pdhg_iso3_{name}_iterates_vs_float64", worst, _limit(CPU_F32_ITERATES[name]))
    Sr = ref["S"]
    bar(f"pdhg_iso3_{name}_Rnrm_vs_float64", np.max(np.abs(np.array(info["Rnrm"]) / (np.sqrt(Sr[:, 0]) / np.linalg.norm(P.b)) - 1)),
        _limit(CPU_F32_RNRM[name]))
    bar(f"pdhg_iso3_{name}_objective_vs_float64", np.max(np.abs(np.array(info["objective"]) / (0.5 * Sr[:, 0] + P.lam * Sr[:, 1]) - 1)),
        _limit(CPU_F32_OBJECTIVE[name]))
    assert np.allclose(info["relError"], np.sqrt(Sr[:, 6]) / np.linalg.norm(P.x_true), rtol=1e-4)
    want = T.objective_iso3(Apair, C.pair(P.oracle_L()), P.b, P.lam, x, geo)
    assert abs(info["objectiveFinal"] / want - 1) < 1e-5
    assert info["active"] == [int(np.count_nonzero((h == P.lo) | (h == P.hi))) for h in H]
    if name == "Q5u":
        assert np.count_nonzero(H[-1] == P.hi) > T.Q5U_MIN_AT_UPPER and np.count_nonzero(H[-1] == P.lo) >= 1


# ====================================================================== (7) argument checks
def test_argument_checks_come_first(eng):
    """Bad arguments are refused with trk_last_error's text before anything is launched."""
    import scipy.sparse as sp
    from trips_py_amd.operators import FirstDerivative2D, SpaceTimeDerivative, SparseOp
    rows = T.rows_of(5, 3)                                                            # 195
    u, q, x, z = (torch.zeros(n, dtype=torch.float32, device=eng.device) for n in (rows, rows, 75, 75))
    xn, xb = torch.zeros_like(x), torch.zeros_like(x)
    NP = eng.scalars(8 * CAP)
    L = SpaceTimeDerivative(5, 3, engine=eng)
    r0 = NP.ref(0)
    for geo in ((5, 2), (4, 3), (5, 4)):
        with pytest.raises(ValueError, match="rows"):
            eng.pdhg_dual_q_iso3(*geo, 0.5, 0.1, u, q, r0, CAP)
    with pytest.raises(ValueError, match="rows"):                                     # a surplus tail
        eng.pdhg_dual_q_iso3(5, 3, 0.5, 0.1, torch.zeros(rows + 1, device=eng.device), torch.zeros(rows + 1, device=eng.device), r0, CAP)
    with pytest.raises(ValueError, match="N >= 2"):
        eng.pdhg_dual_q_iso3(1, 3, 0.5, 0.1, u, q, r0, CAP)
    with pytest.raises(ValueError, match="frames"):
        eng.pdhg_dual_q_iso3(5, 0, 0.5, 0.1, u, q, r0, CAP)
    with pytest.raises(ValueError, match="sigma"):
        eng.pdhg_dual_q_iso3(5, 3, float("inf"), 0.1, u, q, r0, CAP)
    with pytest.raises(ValueError, match="lam"):
        eng.pdhg_dual_q_iso3(5, 3, 0.5, float("nan"), u, q, r0, CAP)
    with pytest.raises(ValueError, match="alias"):
        eng.pdhg_dual_q_iso3(5, 3, 0.5, 0.1, q, q, r0, CAP)
    with pytest.raises(ValueError, match="too small"):
        eng.pdhg_dual_q_iso3(5, 3, 0.5, 0.1, u, q, r0, 5)                             # two row batches x three frames: six blocks
    with pytest.raises(ValueError, match="sigma"):
        eng.pdhg_st_dual_iso3(L._h, 0.0, 0.1, x, q, r0, CAP)
    with pytest.raises(ValueError, match="lam"):
        eng.pdhg_st_dual_iso3(L._h, 0.5, -0.1, x, q, r0, CAP)
    with pytest.raises(ValueError, match="alias"):
        eng.pdhg_st_dual_iso3(L._h, 0.5, 0.1, q, q, r0, CAP)
    with pytest.raises(ValueError, match="too small"):
        eng.pdhg_st_dual_iso3(L._h, 0.5, 0.1, x, q, r0, 5)
    with pytest.raises(ValueError, match="tau"):
        eng.pdhg_st_primal(L._h, 0.0, 0.0, 1.0, x, z, q, xn, xb, None, r0, CAP)
    with pytest.raises(ValueError, match="lo <= hi"):
        eng.pdhg_st_primal(L._h, 0.2, 1.0, 0.0, x, z, q, xn, xb, None, r0, CAP)
    with pytest.raises(ValueError, match="alias"):
        eng.pdhg_st_primal(L._h, 0.2, 0.0, 1.0, x, z, q, xn, x, None, r0, CAP)        # xbar aliases x
    with pytest.raises(ValueError, match="alias"):
        eng.pdhg_st_primal(L._h, 0.2, 0.0, 1.0, x, z, q, z, xb, None, r0, CAP)        # x_new may alias x only
    with pytest.raises(ValueError, match="too small"):
        eng.pdhg_st_primal(L._h, 0.2, 0.0, 1.0, x, z, q, xn, xb, None, r0, 5)
    with pytest.raises(ValueError, match="rows"):
        eng.pdhg_blocks_iso3(75, 75, rows + 25, 5, 3)
    for geo in ((5, 2), (4, 3)):                                                      # a geometry that is not the handle's
        with pytest.raises(ValueError, match="geometry"):
            eng.pdhg_blocks_iso3(75, 75, T.rows_of(*geo), *geo, L._h)
    # handles the space-time forms do not take: a CSR handle and a 2-D handle
    Ls, L2 = SparseOp(sp.identity(75, format="csr"), engine=eng), FirstDerivative2D(5, engine=eng)
    for h in (Ls._h, L2._h):
        with pytest.raises(NotImplementedError):
            eng.pdhg_st_dual_iso3(h, 0.5, 0.1, x, q, r0, CAP)
        with pytest.raises(NotImplementedError):
            eng.pdhg_st_primal(h, 0.2, 0.0, 1.0, x, z, q, xn, xb, None, r0, CAP)
        with pytest.raises(NotImplementedError):
            eng.pdhg_blocks_iso3(75, 75, rows, 5, 3, h)
    assert not NP.host().any() and not q.any() and not xn.any() and not xb.any()
    # the loop refuses a geometry that is not L's, fused or not, and a fused call on a CSR handle
    from trips_py_amd.solvers import PDHGRun
    P = T.problem("Q5")
    for fused in (None, False):
        run = PDHGRun(P.device(eng), P.b, P.device_L(eng), P.lam, P.sigma, P.tau, P.lo, P.hi, None, 2, tv="iso3", fused=fused)
        for geo in ((15, 3), (16, 2), (16, 4)):
            run.geo = geo
            with pytest.raises(ValueError):
                run.run(1)
        assert not run.q.any() and not run.p.any()
    run = _run(eng, "Q5", max_iter=2, csr=True)
    run.fused = True                                             # a CSR handle has no fused form
    with pytest.raises(NotImplementedError):
        run.run(1)
    assert not run.q.any() and not run.p.any()


# ====================================================================== (8) the older modes keep their routing
def test_old_routing_is_unchanged(eng):
    from trips_py_amd.operators import SpaceTimeDerivative
    from trips_py_amd.solvers import PDHGRun
    P = C.problem("Q5")
    L = SpaceTimeDerivative(16, 3, engine=eng)
    assert eng.pdhg_fused_caps(L._h) == 0
    for tv in ("aniso", "iso"):
        run = PDHGRun(P.device(eng), P.b, L, P.lam, P.sigma, P.tau, P.lo, P.hi, None, 2, tv=tv)
        assert not run.fused and run.u is not None and run.v is not None
        with pytest.raises(ValueError):
            PDHGRun(P.device(eng), P.b, L, P.lam, P.sigma, P.tau, P.lo, P.hi, None, 2, tv=tv, fused=True)
    run3 = PDHGRun(P.device(eng), P.b, L, P.lam, P.sigma, P.tau, P.lo, P.hi, None, 2, tv="iso3")
    assert run3.fused and run3.u is None and run3.v is None
    # FirstDerivative2D is (N, 1): the unfused dual behind L.apply, the bits of tv='iso'
    Q = C.problem("Q1")
    a = PDHGRun(Q.device(eng), Q.b, Q.device_L(eng), Q.lam, Q.sigma, Q.tau, Q.lo, Q.hi, None, 4, tv="iso3")
    b = PDHGRun(Q.device(eng), Q.b, Q.device_L(eng), Q.lam, Q.sigma, Q.tau, Q.lo, Q.hi, None, 4, tv="iso")
    assert not a.fused and a.geo == (32, 1) and b.fused
    a.run(4)
    b.run(4)
    assert torch.equal(a.x_cur, b.x_cur) and torch.equal(a.q, b.q)
    with pytest.raises(ValueError):
        PDHGRun(Q.device(eng), Q.b, Q.device_L(eng), Q.lam, Q.sigma, Q.tau, Q.lo, Q.hi, None, 4, tv="iso3", fused=True)
