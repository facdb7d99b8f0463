"""The fan-beam pair (csrc/fanbeam2d.hip) entry by entry against the float64 oracle (oracle.FanBeam2D.rows / .cols: the brute-force
ray / pixel clipping of matrix(), one ray or one pixel at a time), at the sizes and geometries that select each of its kernels.

(A) Matrix entries by unit probes: A @ e_p is column p of the kernel's matrix, A^T @ e_i row i — single-term outputs, no
    accumulation error — against the oracle's column / row, with a bound per entry from the kernels' arithmetic; a weight that is
    present on one side and missing on the other fails by itself; the forward and the adjoint (and the gather-march forward and
    the older adjoint gather) give the same floats on every (ray, pixel) pair both probe sets hold.
(B) Accumulation on real inputs, on the probed rows and columns: norm-wise and per entry.
(C) Several columns at once = the columns one by one, to the bit, both directions.

Bounds.  Row-march (source and detector outside the circumscribed circle): a ray's entry in step tt (its marching index: the
pixel's row for a steep ray, its column for a shallow one) is len * w with w = the fraction of the step's segment in the pixel.
  * fp32: w0 from one clamped FMA on (float)(~frac) (2^-24) and 0.25 rcp(|m|) (|m| to float 2^-24, v_rcp_f32 1 ulp = 2^-23),
    its rounding (2^-24): 5 2^-24 relative; w1 = 1 - w0 rounds once more (2^-25 absolute); len is a float (2^-24) and len * w
    rounds (2^-24): |error| <= 7 2^-24 len.
  * fixed point: the position X0 + tt M is exact integer arithmetic on X0 rounded to 2^-30 with its bit 0 cleared (<= 1.5 2^-30)
    and M rounded to 2^-30 (<= 2^-31 per step, and 2^-31 / |M| relative in the split's reciprocal): the position is off by
    <= (4 + tt) 2^-31, and a weight moves by that / |M| (w is 1/|M|-Lipschitz in the position).
  tau = len (7 2^-24 + (4 + tt) 2^-31 / |M|).  The second term GROWS WITH N (through tt) — the 30 fraction bits of M, not the
  weights' arithmetic: at 2048^2 and |M| ~ 0.3 it is 2^-20 of a pixel, near an axis (|M| ~ 1e-4) it is ~1e-3.
General pair (detector inside the circumscribed circle: k_fan_fwd's Siddon traversal, k_fan_adj's slab clipping): differences
of fp32 ray parameters along the source-to-detector segment of length L_ray; see general_tau below.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import bar, relerr

pytestmark = pytest.mark.gpu

CU = 256                 # MI355X compute units: the gather march's band count hangs on it (fan_apply), only the seam probes use it
EPS = 2.0 ** -24


def fb_rows(N):
    return 64 if 64 * (N + 8) * 4 <= 150 * 1024 else 32


def kernel_paths(N, nd, na, pitch, sod, odd):
    """The create-time conditions of trk_fanbeam2d_create and the dispatch of fan_apply, restated: (forward, adjoint, seams) —
    seams: the first rows (columns) of the forward's bands."""
    if not odd > 0.7072 * N:
        return "k_fan_fwd", "k_fan_adj", []
    if N % 64 == 0 and 128 <= N <= 1024:
        rows = fb_rows(N)
        fwd, seams = f"band{rows}x{N // rows}", list(range(rows, N, rows))
    else:
        nrays = na * nd
        nb = max(1, min(4, N // 64, -(-8 * 4 * CU * 64 // nrays)))
        band = ((N + nb - 1) // nb + 7) // 8 * 8
        nb = -(-N // band)
        fwd, seams = ("pad+march+sum%d" % nb if nb > 1 else "pad+march"), list(range(band, N, band))
    tan_max = 0.5 * nd * pitch / (sod + odd)
    reach = float(np.float32(0.7072 / pitch * (1.0 + tan_max * tan_max) * 1.02))
    max_cand = int(np.floor(2.0 * (reach * (sod + odd) / (sod - 0.7072 * N) * 1.001 + 0.01))) + 1
    dense = 2.0 * ((sod + odd) * reach / (sod + 0.7072 * N)) >= 1.0
    if max_cand <= 3 and na * 32 <= 48 * 1024:
        adj = "views_dense" if dense else "views_sparse"
    else:
        adj = "march2" if max_cand <= 3 else "march0"
    return fwd, adj, seams


def _views(n):
    return np.linspace(0, np.pi, n, endpoint=False)


def _full_turn():
    a = np.linspace(0, 2 * np.pi, 90, endpoint=False) + 0.013
    a[::4] -= 2 * np.pi                                  # a quarter of them negative
    return a


# name, N, angles, FanBeam2D keywords (the defaults of Tomography.define_proj_id otherwise)
CASES = [
    ("a", 128, _views(30), {}),
    ("b_bench", 512, _views(180), {}),
    ("c", 576, _views(45), {}),
    ("d640", 640, _views(20), {}),
    ("d1024", 1024, _views(12), {}),
    ("e_demo", 1000, _views(50), {}),
    ("f1088", 1088, _views(8), {}),
    ("f2048", 2048, _views(6), {}),
    ("g_turn", 256, _full_turn(), {}),
    ("h_ties", 500, np.array([0, np.pi / 4, np.pi / 2, 3 * np.pi / 4, np.pi, 3 * np.pi / 2]), {}),
    ("i_pitch2", 512, _views(180), {"det_pitch": 2.0}),
    ("j_pitch05", 256, _views(60), {"det_pitch": 0.5}),
    ("k_1600", 96, _views(1600), {}),
    ("l_general", 512, _views(45), {"origin_detector": 256.0}),
]


def _geometry(N, ang, kw):
    nd = int(kw.get("n_det", int(np.sqrt(2) * N)))
    sod, odd = 3.0 * N, float(kw.get("origin_detector", N))
    pitch = float(kw.get("det_pitch", (sod + odd) / sod))
    return nd, pitch, sod, odd


def _case_id(c):
    name, N, ang, kw = c
    nd, pitch, sod, odd = _geometry(N, ang, kw)
    fwd, adj, _ = kernel_paths(N, nd, len(ang), pitch, sod, odd)
    return f"{name}-{N}x{len(ang)}x{nd}-{fwd}-{adj}"


def _probe_rays(Ao, rng):
    na, nd = len(Ao.angles), Ao.nd
    wrap = lambda t: np.abs(np.angle(np.exp(1j * (Ao.angles - t))))
    views = sorted({int(np.argmin(wrap(t))) for t in (0.0, np.pi / 4, np.pi / 2, 3 * np.pi / 4)})
    rays = [a * nd + d for a in views for d in (0, nd // 2 - 1, nd // 2, nd // 2 + 1, nd - 1)]
    _, _, dx, dy, _ = Ao._rays(np.arange(na * nd))
    steep = (np.abs(dy) >= np.abs(dx)).reshape(na, nd)
    mixed = np.nonzero(steep.any(axis=1) & ~steep.all(axis=1))[0]       # view_cls 2: steep and shallow rays in one view
    if mixed.size:
        a = int(mixed[mixed.size // 2])
        sw = np.nonzero(steep[a, 1:] != steep[a, :-1])[0]
        rays += [a * nd, a * nd + nd - 1] + [a * nd + int(d) for d in sw[:2]] + [a * nd + int(d) + 1 for d in sw[:2]]
    rays += list(rng.integers(0, na, 8) * nd + rng.integers(nd // 4, 3 * nd // 4, 8))
    return np.unique(np.asarray(rays, dtype=np.int64))


def _probe_pixels(N, seams, R, rng):
    px = [0, N - 1, (N - 1) * N, N * N - 1]
    for s in seams[:1] + seams[len(seams) // 2:len(seams) // 2 + 1] + seams[-1:]:
        for t in (s - 1, s):
            px += [t * N + int(rng.integers(N)), int(rng.integers(N)) * N + t]
    for k in range(R.shape[0]):                                           # the support of every probe ray
        row = R.getrow(k)
        idx, w = row.indices, row.data
        if idx.size == 0:
            continue
        px += [int(idx[np.argmin(w)]), int(idx[np.argmax(w)])]
        r, c = np.divmod(idx, N)
        border = idx[(r == 0) | (r == N - 1) | (c == 0) | (c == N - 1)]
        px += [int(border.min()), int(border.max())] if border.size else []
    px += list(rng.integers(0, N * N, 16))
    return np.unique(np.asarray(px, dtype=np.int64))


# General pair (k_fan_fwd traverses, k_fan_adj clips each pixel; both from the fp32 FanAngle fields).  An entry is L_ray times a
# difference of two ray parameters t in [0, 1], each from an fp32 difference and a division: 4 2^-24 L_ray.  The ray's endpoints
# are fp32 coordinates of magnitude <= L_ray (source, detector pixel centre): the ray sits up to 2 2^-24 L_ray sideways, len times
# that along a row (column), and the split of a step moves by that / |M| of the step's length len: 2 2^-24 L_ray len^2 / |M|.
# (Measured before k_fan_fwd computed each crossing parameter afresh: 140 x the first term — repeated adds, up to 2N roundings.)
def general_tau(L, ln, inv_m):
    return EPS * L * (4.0 + 2.0 * ln * ln * inv_m)


def _unit_batch(n, idx, dev):
    E = torch.zeros((idx.size, n), dtype=torch.float32, device=dev)
    E[torch.arange(idx.size, device=dev), torch.from_numpy(idx).to(dev)] = 1.0
    return E


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_fanbeam_entrywise_against_float64_oracle(case, monkeypatch):
    from oracle import cpu_ref as O
    from trips_py_amd.operators import FanBeam2D
    name, N, ang, kw = case
    nd, pitch, sod, odd = _geometry(N, ang, kw)
    fwd_path, adj_path, seams = kernel_paths(N, nd, len(ang), pitch, sod, odd)
    general = fwd_path == "k_fan_fwd"
    monkeypatch.delenv("TRK_FAN_NO_BANDRES", raising=False)
    monkeypatch.delenv("TRK_FAN_ADJ_MARCH2", raising=False)
    A = FanBeam2D(N, angles=ang, **kw)
    Ao = O.FanBeam2D(N, ang, n_det=nd, sod=sod, odd=odd, pitch=pitch)
    assert A.shape == Ao.shape and A.n_det == nd and A.pitch == pitch
    dev, (m, n) = A.engine.device, A.shape
    rng = np.random.default_rng(N + len(ang))
    rays = _probe_rays(Ao, rng)
    R = Ao.rows(rays)                                                        # oracle rows of the probe rays
    pix = _probe_pixels(N, seams, R, rng)
    pr, pc = np.divmod(pix, N)
    C = Ao.cols(pix)                                                         # oracle columns of the probe pixels (m, pixels), CSC

    # per-ray quantities of the bound: the row-march's |M| and len, its class; the general pair's L_ray
    allrays = np.arange(m)
    _, _, dx, dy, Lray = Ao._rays(allrays)
    M = Ao.slope(allrays)
    ln = np.sqrt(1.0 + M * M)
    steep = np.abs(dy) >= np.abs(dx)
    with np.errstate(divide="ignore"):
        inv_m = 1.0 / M

    def tau(ray_i, pr_, pc_):                                                # broadcast over (ray, pixel)
        if general:
            return general_tau(Lray[ray_i], ln[ray_i], inv_m[ray_i])
        tt = np.where(steep[ray_i], pr_, pc_)
        return ln[ray_i] * (7 * EPS + (4 + tt) * 2.0 ** -31 * inv_m[ray_i])

    stats = {}
    fails = []

    def entries(tag, got, want, t):
        err = np.abs(got - want)
        ratio = float(np.max(np.where(err > 0, err / t, 0.0))) if err.size else 0.0
        miss = ((got == 0) != (want == 0)) & (np.maximum(np.abs(got), np.abs(want)) > np.maximum(2.0 ** -20, t))
        stats[tag] = max(stats.get(tag, 0.0), ratio)
        stats[tag + "_max_abs"] = max(stats.get(tag + "_max_abs", 0.0), float(err.max()) if err.size else 0.0)
        stats[tag + "_zero_pattern"] = stats.get(tag + "_zero_pattern", 0) + int(miss.sum())

    # ---- (A) forward: columns by unit images, in chunks of <= 256 MB -----------------------------------------------------------
    chunk = max(1, min(64, (256 << 20) // (4 * n)))
    fwd_at_rays = np.zeros((rays.size, pix.size))
    kcols, krows = [], []                                                    # the kernel's probed columns / rows, sparse
    gather_equal = True
    for s in range(0, pix.size, chunk):
        idx = pix[s:s + chunk]
        E = _unit_batch(n, idx, dev)
        G = A.apply(E)
        if not general and fwd_path.startswith("band"):
            monkeypatch.setenv("TRK_FAN_NO_BANDRES", "1")
            gather_equal &= bool(torch.equal(A.apply(E), G))
            monkeypatch.delenv("TRK_FAN_NO_BANDRES")
        G = G.double().cpu().numpy().T                                       # (m, k): columns of the kernel's matrix
        del E
        W = C[:, s:s + chunk].toarray()
        entries("fwd", G, W, tau(allrays[:, None], pr[None, s:s + chunk], pc[None, s:s + chunk]))
        fwd_at_rays[:, s:s + chunk] = G[rays]
        kcols.append(sp.csc_matrix(G))

    # ---- (A) adjoint: rows by unit sinogram entries, compared on the union of both sides' supports -------------------------
    rchunk = max(1, min(64, (256 << 20) // (4 * n)))
    adj_at_pix = np.zeros((rays.size, pix.size))
    march2_equal = True
    for s in range(0, rays.size, rchunk):
        F = _unit_batch(m, rays[s:s + rchunk], dev)
        H = A.apply(F, transpose=True)
        if not general and adj_path.startswith("views"):
            monkeypatch.setenv("TRK_FAN_ADJ_MARCH2", "1")
            march2_equal &= bool(torch.equal(A.apply(F, transpose=True), H))
            monkeypatch.delenv("TRK_FAN_ADJ_MARCH2")
        del F
        adj_at_pix[s:s + rchunk] = H[:, torch.from_numpy(pix).to(dev)].double().cpu().numpy()
        for k in range(H.shape[0]):
            hk = torch.nonzero(H[k]).reshape(-1).cpu().numpy()
            row = R.getrow(s + k)
            u = np.union1d(hk, row.indices)
            got = H[k, torch.from_numpy(u).to(dev)].double().cpu().numpy()
            krows.append(sp.csr_matrix((got, (np.zeros(u.size, dtype=np.int64), u)), shape=(1, n)))
            want = row.toarray().reshape(-1)[u]
            ur, uc = np.divmod(u, N)
            entries("adj", got, want, tau(np.full(u.size, rays[s + k]), ur, uc))
        del H
    # matched pair: every (probe ray, probe pixel) entry, from the forward's columns and from the adjoint's rows
    shared_nz = int(np.count_nonzero(adj_at_pix))
    matched = bool(np.array_equal(fwd_at_rays, adj_at_pix))

    # ---- (B) accumulation on real inputs, on the probed rows (forward) and columns (adjoint) --------------------------------
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    smooth = np.exp(-((ii - N / 2.5) ** 2 + (jj - N / 1.7) ** 2) / (0.02 * N * N)) + 0.3 * np.cos(jj * 5.0 / N)
    X = np.stack([rng.standard_normal(n), smooth.reshape(-1), rng.random(n)]).astype(np.float32)
    Y = np.stack([rng.standard_normal(m), np.tile(np.hanning(nd) + 0.1, len(ang)), rng.random(m)]).astype(np.float32)
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    AX, ATY = A.apply(Xd), A.apply(Yd, transpose=True)
    # (C) several columns at once = the columns one by one, to the bit
    batch_equal = all(torch.equal(AX[j], A.apply(Xd[j])) and torch.equal(ATY[j], A.apply(Yd[j], transpose=True)) for j in range(3))
    AX, ATY = AX.double().cpu().numpy(), ATY.double().cpu().numpy()
    # the per-entry bounds on the union of the oracle's and the kernel's non-zeros (the kernel's from (A))
    Ur = (abs(R) + abs(sp.vstack(krows).tocsr())).tocoo()
    Tr = sp.csr_matrix((tau(rays[Ur.row], *np.divmod(Ur.col, N)), (Ur.row, Ur.col)), shape=R.shape)
    Uc = (abs(C) + abs(sp.hstack(kcols).tocsc())).tocoo()
    Tc = sp.csc_matrix((tau(Uc.row, pr[Uc.col], pc[Uc.col]), (Uc.row, Uc.col)), shape=C.shape)
    nz_row, nz_col = np.diff(R.indptr), np.diff(C.indptr)
    # the north-star 1e-5; the general pair's entries carry up to 4 2^-24 L_ray = 4.3e-4 of a pixel at 512^2 (L_ray = 3.5 N), and on
    # the ~100 probed pixels its adjoint measured 1.02e-4 (test_fanbeam_vs_bruteforce_oracle's 1e-4 holds the whole vectors at N <= 132)
    norm_bar = 4e-4 if general else 1e-5
    for j in range(3):
        x64, y64 = X[j].astype(np.float64), Y[j].astype(np.float64)
        want_f, got_f = R @ x64, AX[j][rays]
        b_f = (2 * nz_row + 16) * EPS * (abs(R) @ np.abs(x64)) + Tr @ np.abs(x64)
        want_a, got_a = C.T @ y64, ATY[j][pix]
        b_a = (2 * nz_col + 16) * EPS * (abs(C).T @ np.abs(y64)) + Tc.T @ np.abs(y64)
        for tag, got, want, b in (("acc_fwd", got_f, want_f, b_f), ("acc_adj", got_a, want_a, b_a)):
            err = np.abs(got - want)
            stats[tag] = max(stats.get(tag, 0.0), float(np.max(np.where(err > 0, err / np.maximum(b, 1e-300), 0.0))))
            stats[tag + "_norm"] = max(stats.get(tag + "_norm", 0.0), relerr(got, want))

    print(f"\n[fanbeam {_case_id(case)}] probes {rays.size} rays x {pix.size} pixels ({shared_nz} shared non-zeros) | "
          f"entry err/bound fwd {stats['fwd']:.3f} adj {stats['adj']:.3f} (max abs {stats['fwd_max_abs']:.2e} / {stats['adj_max_abs']:.2e}; "
          f"zero-pattern misses {stats['fwd_zero_pattern']} / {stats['adj_zero_pattern']}) | accumulation err/bound fwd {stats['acc_fwd']:.3f} "
          f"adj {stats['acc_adj']:.3f}, relerr {stats['acc_fwd_norm']:.2e} / {stats['acc_adj_norm']:.2e} | "
          f"matched {matched} gather {gather_equal} march2 {march2_equal} batch {batch_equal}")
    for tag, limit in (("fwd", 1.0), ("adj", 1.0), ("acc_fwd", 1.0), ("acc_adj", 1.0), ("acc_fwd_norm", norm_bar), ("acc_adj_norm", norm_bar)):
        try:
            bar(f"fanbeam_accuracy.{name}.{tag}", stats[tag], limit)
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, fails
    assert stats["fwd_zero_pattern"] == 0 and stats["adj_zero_pattern"] == 0, stats
    # the forward and the adjoint weigh by the same floats (the general pair does not: two separate clippings)
    assert general or (matched and shared_nz > rays.size), (matched, shared_nz)
    assert gather_equal and march2_equal and batch_equal
