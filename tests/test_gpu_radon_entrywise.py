"""The parallel-beam pair (csrc/radon2d.hip, radon_fwd.hip, radon_adj.hip) entry by entry against the float64 oracle
(oracle.Radon2D.rows / .cols: the rows and columns of matrix(), to the bit, without the matrix), on the cases of tests/radon_cases.py:
one per forward kernel and adjoint route of the dispatch restated there (checked on the CPU by test_radon_oracle_rows_cols_host.py).

(A) Entries by unit probes.  A e_p is column p of the kernels' matrix, A^T e_r its row r: one term per output, no accumulation.
    Each is compared with the oracle's column / row on the union of both supports against tau below; an entry present on one
    side only and larger than max(2^-20 w scale, tau) is a zero-pattern miss and fails by itself.
(B) The same bits from every kernel of the geometry.  A unit image leaves one non-zero tap per ray, a unit sinogram entry one angle
    per pixel, so the summation order cannot matter: the case's own route must equal, with torch.equal, what the knobs
    TRK_RADON_NO_BANDRES (a second handle), TRK_RADON_NO_QUADF, TRK_RADON_NO_ADJQ, TRK_RADON_ADJ_SIMPLE and a batch of three give.
(C) Matched pair.  On every (probe ray, probe pixel) entry the forward's value and the adjoint's are the same bits where the ray is
    certainly the pixel's nearest (|q - col| < 1/2 - 2^-10 by the oracle), and within 2 u w scale elsewhere.
(D) Accumulation on real inputs (white noise, a smooth image / a Hanning-profile sinogram, uniform [0, 1)) on the probed rows and
    columns: per entry within (2 nnz + 16) u (|A| |x|) + T |x| (T: tau on the union pattern), norm-wise within the project's 1e-5;
    a batch of three = the three one by one to the bit where the dispatch gives both the same kernel, within the bound elsewhere.

Bounds, u = 2^-24, derived from the kernels (w = 1/|cos| or 1/|sin| of the ray's angle, scale = 1/N):
  * Position.  q = (A32[d] + B32[tt]) 2^-24 with both tables rounded once from float64 (radon_create_impl: llrint) and added as
    integers: within 1 u of the float64 q.  The quad members' tables are exact integer images of the base's (negation, flips), and the
    base's are rounded the same way.  The hat weight 1 - |q - col| is 1-Lipschitz in q: the tap weight f or 1 - f moves by <= 1 u.
  * Forward entry.  f 2^32 = (float)(Q << 8) and 2^32 - that are exact in fp32 (24 significant bits); with a unit image the fp32 FMA
    chain and the float64 band sums are exact; the output is wgt * (float)total with wgt = (float)(w scale 2^-32): 1/2 u relative for
    the weight's conversion, 1/2 u for the product.  |error| <= (1 + 1) u w scale; tau_fwd = 3 u w scale holds it with one u to spare.
  * Adjoint entry.  The nearest ray: t_int = A32 + B32 - (col << 24) exactly, w0 = 1 - |t_int| 2^-24 exactly, the record (float)(w
    scale) * S (1/2 u for the conversion, exact for S = 1), one FMA rounding (1/2 u): the forward's bits.  A neighbour: clamp(c1 -+ t0)
    with c1 a 2^-24-grid neighbour of 1 - |inv| (< 1 u off) and t0 on the grid within 1 u: exact FMA, 2 u off; record and product 1 u
    relative.  |error| <= 3 u w scale; tau_adj = 4 u w scale holds it with one u to spare.

What (B) rests on in the adjoint.  Every route forms d0 = rint(fma(col, rinv, C)) from the same fp32 operands (the mirrored-pair kernel
from the base geometry's, whose roundings are the members' mirrored) and the neighbour weights from the c1 the handle gives it.  The
mirrored-pair kernel has ONE c1 per quad; k_radon_adj_tile and k_radon_adj_simple had one per angle from a diffusion of their own, and
on quad1024 / quad2048 every neighbour entry of about half the rays differed between the routes (up to 1.48 u w scale on 318 .. 1005
pixels of a ray) until radon_create_impl gave the members of such a handle their quad's value.  Where two routes ever placed d0
differently at a half-way pixel, the entry would be a centre weight on one side and a neighbour weight on the other, up to 2 u apart:
none of the probes meets that.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import radon_cases as RC
from conftest import bar, relerr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
TAU_FWD, TAU_ADJ = 3 * EPS, 4 * EPS


class _Oracle:
    """oracle.Radon2D over the nt * na angles of a (dynamic) handle: rows / cols / geometry of the block-diagonal operator."""

    def __init__(self, N, ang, nd, nt):
        from oracle import cpu_ref as O
        self.N, self.nd, self.nt, self.na = N, nd, nt, len(ang) // nt
        self.o = O.Radon2D(N, ang, n_det=nd)
        self.angles, self.scale = self.o.angles, self.o.scale
        self.mf, self.nf = self.na * nd, N * N                       # rows, columns of a frame
        self.shape = (nt * self.mf, nt * self.nf)

    def rows(self, rays):
        R = self.o.rows(rays).tocoo()
        return sp.csr_matrix((R.data, (R.row, R.col + (rays // self.mf)[R.row] * self.nf)), shape=(rays.size, self.shape[1]))

    def cols(self, pix):
        C = self.o.cols(pix % self.nf).tocoo()
        keep = C.row // self.mf == (pix // self.nf)[C.col]
        return sp.csc_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=(self.shape[0], pix.size))

    def geometry(self, rays):
        return self.o.geometry(rays)

    def offset(self, rays, pix):
        """q - col of every (ray, pixel) pair, by the oracle's expression; inf across frames."""
        a, d = np.divmod(rays, self.nd)
        i, j = np.divmod(pix % self.nf, self.N)
        out = np.full((rays.size, pix.size), np.inf)
        for r in range(rays.size):
            rows, ct, st, _ = self.o._mode(a[r])
            k, tap = (i, j) if rows else (j, i)
            t = self.o._coord(rows, ct, st, d[r] - (self.nd - 1) / 2.0, k) - tap
            same = pix // self.nf == rays[r] // self.mf
            out[r, same] = t[same]
        return out


def _probe_rays(Ao, rng):
    N, nd, na_all = Ao.N, Ao.nd, len(Ao.angles)
    wrap = lambda t: np.abs(np.angle(np.exp(1j * (Ao.angles - t))))
    views = sorted({int(np.argmin(wrap(t))) for t in (0.0, np.pi / 4, np.pi / 2, 3 * np.pi / 4)})
    dets = sorted({d for d in (0, 1, nd // 2 - 1, nd // 2, nd - 2, nd - 1) if 0 <= d < nd})
    rays = [a * nd + d for a in views for d in dets]
    mode, _ = Ao.geometry(np.arange(na_all) * nd)
    s = np.arange(nd) - (nd - 1) / 2.0
    for a in range(na_all):                                          # the first and the last detector whose ray touches the image
        rows, ct, st, _ = Ao.o._mode(a)
        qa, qb = Ao.o._coord(rows, ct, st, s, 0), Ao.o._coord(rows, ct, st, s, N - 1)
        hit = np.nonzero((np.maximum(qa, qb) > -1.0) & (np.minimum(qa, qb) < N))[0]
        if hit.size:
            rays += [a * nd + int(hit[0]), a * nd + int(hit[-1])]
    fold = np.abs(np.angle(np.exp(4j * Ao.angles)) / 4)              # distance from the nearest axis, in [0, pi/4]
    for m in (0, 1):                                                 # a generic view of each marching mode
        cand = np.nonzero(mode == m)[0]
        if cand.size:
            a = int(cand[np.argmin(np.abs(fold[cand] - np.pi / 8))])
            rays += [a * nd + nd // 3, a * nd + (2 * nd) // 3]
    rays += list(rng.integers(0, na_all, 8) * nd + rng.integers(0, nd, 8))
    return np.unique(np.asarray(rays, dtype=np.int64))


def _seam_picks(seams):
    return sorted(set(seams[:1] + seams[len(seams) // 2:len(seams) // 2 + 1] + seams[-1:]))


def _probe_pixels(Ao, band, R, rng):
    N, nt = Ao.N, Ao.nt
    px = [0, N - 1, (N - 1) * N, N * N - 1]                          # corners; one pixel on each border
    px += [int(rng.integers(1, N - 1)), (N - 1) * N + int(rng.integers(1, N - 1)), int(rng.integers(1, N - 1)) * N,
           int(rng.integers(1, N - 1)) * N + N - 1]
    edges = [band] + [T for T in (16, 32, 64) if T < N]              # forward band seams; adjoint tile seams
    for e in edges:
        for s in _seam_picks(list(range(e, N, e))):
            for t in (s - 1, s):                                     # as a row (mode 0 marches rows) and as a column (mode 1)
                px += [t * N + int(rng.integers(N)), int(rng.integers(N)) * N + t]
        last = (N - 1) // e * e                                      # inside the last (ragged) tile / band
        t = int(rng.integers(last, N))
        px += [t * N + int(rng.integers(last, N)), t * N + int(rng.integers(N)), int(rng.integers(N)) * N + t]
    px = [p + int(rng.integers(nt)) * N * N for p in px]
    for k in range(R.shape[0]):                                      # the smallest and the largest weight of every probe ray
        row = R.getrow(k)
        if row.indices.size:
            px += [int(row.indices[np.argmin(row.data)]), int(row.indices[np.argmax(row.data)])]
    px += list(rng.integers(0, nt * N * N, 16))
    return np.unique(np.asarray(px, dtype=np.int64))


def _unit_batch(n, idx, dev):
    E = torch.zeros((idx.size, n), dtype=torch.float32, device=dev)
    E[torch.arange(idx.size, device=dev), torch.from_numpy(idx).to(dev)] = 1.0
    return E


def _make(case, monkeypatch, env):
    from trips_py_amd.operators import BlockDiagOp, Radon2DParallel
    name, N, ang, nd, nt, _ = case
    for k in ("TRK_RADON_NO_BANDRES", "TRK_RADON_ADJQ_MIN", "TRK_RADON_NO_QUADF", "TRK_RADON_NO_ADJQ", "TRK_RADON_ADJ_SIMPLE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    na = len(ang) // nt
    ops = [Radon2DParallel(N, ang[f * na:(f + 1) * na], n_det=nd) for f in range(nt)]
    A = ops[0] if nt == 1 else BlockDiagOp(ops)
    for k in env:
        monkeypatch.delenv(k)
    return A


@pytest.mark.parametrize("case", RC.CASES, ids=[RC.case_id(c) for c in RC.CASES])
def test_radon_entrywise_against_float64_oracle(case, monkeypatch):
    name, N, ang, nd, nt, env = case
    na = len(ang) // nt
    fwd_path, (band, nb), adj_kind, nsplit, prep = RC.case_paths(case)
    A = _make(case, monkeypatch, env)
    Ao = _Oracle(N, ang, nd, nt)
    assert A.shape == Ao.shape
    dev, (m, n) = A.engine.device, A.shape
    rng = np.random.default_rng(N + na + nd)
    rays = _probe_rays(Ao, rng)
    R = Ao.rows(rays)
    pix = _probe_pixels(Ao, band, R, rng)
    C = Ao.cols(pix)
    allrays = np.arange(m)
    _, w_all = Ao.geometry(allrays)
    ws = w_all * Ao.scale                                            # w scale per ray
    stats, fails, unequal = {}, [], []

    def entries(tag, got, want, t, wsc):
        err = np.abs(got - want)
        ratio = float(np.max(np.where(err > 0, err / t, 0.0))) if err.size else 0.0
        miss = ((got == 0) != (want == 0)) & (np.maximum(np.abs(got), np.abs(want)) > np.maximum(2.0 ** -20 * wsc, t))
        stats[tag] = max(stats.get(tag, 0.0), ratio)
        stats[tag + "_zero_pattern"] = stats.get(tag + "_zero_pattern", 0) + int(np.sum(miss))

    def differs(tag, a, b, wsc=None):
        """(B): record where two kernels' outputs are not the same bits — how many entries, the largest difference in u w scale."""
        if not torch.equal(a, b):
            d = (a.double() - b.double()).abs().cpu().numpy()
            unequal.append((tag, int(np.count_nonzero(d)), float(np.max(d / (EPS * wsc))) if wsc is not None else float(d.max())))

    # ---- (A), (B) forward: columns by unit images, in chunks of <= 256 MB ----------------------------------------------------
    band_geo = N % 64 == 0 and 128 <= N <= 1024
    A2 = None
    if band_geo:                                                     # the other forward of this geometry, on a second handle
        env2 = {k: v for k, v in env.items() if k != "TRK_RADON_NO_BANDRES"}
        if "TRK_RADON_NO_BANDRES" not in env:
            env2["TRK_RADON_NO_BANDRES"] = "1"
        A2 = _make(case, monkeypatch, env2)
    chunk = max(1, min(64, (256 << 20) // (4 * n)))
    fwd_at_rays = np.zeros((rays.size, pix.size))
    kcols, krows = [], []
    ws_dev = torch.from_numpy(ws).to(dev)
    for s in range(0, pix.size, chunk):
        E = _unit_batch(n, pix[s:s + chunk], dev)
        G = A.apply(E)
        if A2 is not None:
            differs("fwd_other_bandres", A2.apply(E), G, ws[None, :])
        if fwd_path == "k_radon_fwd_quadf+quad":
            monkeypatch.setenv("TRK_RADON_NO_QUADF", "1")
            differs("fwd_no_quadf", A.apply(E), G, ws[None, :])
            monkeypatch.delenv("TRK_RADON_NO_QUADF")
        del E
        G = G.double().cpu().numpy().T                               # (m, k): columns of the kernels' matrix
        entries("fwd", G, C[:, s:s + chunk].toarray(), TAU_FWD * ws[:, None], ws[:, None])
        fwd_at_rays[:, s:s + chunk] = G[rays]
        kcols.append(sp.csc_matrix(G))
    del A2

    # ---- (A), (B) adjoint: rows by unit sinogram entries, ONE AT A TIME (a batch takes another route) --------------------------
    adj_at_pix = np.zeros((rays.size, pix.size))
    pix_dev = torch.from_numpy(pix).to(dev)
    held = []
    for k, r in enumerate(rays):
        F = torch.zeros(m, dtype=torch.float32, device=dev)
        F[int(r)] = 1.0
        H = A.apply(F, transpose=True)
        if adj_kind == "quad":
            monkeypatch.setenv("TRK_RADON_NO_ADJQ", "1")
            differs("adj_no_adjq", A.apply(F, transpose=True), H, ws[r])
            monkeypatch.delenv("TRK_RADON_NO_ADJQ")
        if adj_kind != "simple":
            monkeypatch.setenv("TRK_RADON_ADJ_SIMPLE", "1")
            differs("adj_simple", A.apply(F, transpose=True), H, ws[r])
            monkeypatch.delenv("TRK_RADON_ADJ_SIMPLE")
        held.append((F, H, ws[r]))
        if len(held) == 3 or k == rays.size - 1:                     # the same probes as a batch: the batch route
            while len(held) < 3:
                held.append(held[0])
            HB = A.apply(torch.stack([h[0] for h in held]), transpose=True)
            for b in range(3):
                differs("adj_batch3", HB[b], held[b][1], held[b][2])
            held = []
        adj_at_pix[k] = H[pix_dev].double().cpu().numpy()
        hk = torch.nonzero(H).reshape(-1).cpu().numpy()
        row = R.getrow(k)
        u = np.union1d(hk, row.indices)
        got = H[torch.from_numpy(u).to(dev)].double().cpu().numpy()
        krows.append(sp.csr_matrix((got, (np.zeros(u.size, dtype=np.int64), u)), shape=(1, n)))
        entries("adj", got, row.toarray().reshape(-1)[u], TAU_ADJ * ws[r], ws[r])

    # ---- (C) matched pair ------------------------------------------------------------------------------------------------------
    shared_nz = int(np.count_nonzero((fwd_at_rays != 0) & (adj_at_pix != 0)))
    off = Ao.offset(rays, pix)
    nearest = np.abs(off) < 0.5 - 2.0 ** -10
    pair = np.abs(fwd_at_rays - adj_at_pix) / (EPS * ws[rays])[:, None]
    stats["pair_nearest"] = float(np.max(np.where(nearest, pair, 0.0)))         # must be 0: the same bits
    stats["pair_neighbour"] = float(np.max(np.where(nearest, 0.0, pair))) / 2.0   # <= 1: within 2 u w scale

    # ---- (D) accumulation on real inputs ---------------------------------------------------------------------------------------
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    smooth = np.exp(-((ii - N / 2.5) ** 2 + (jj - N / 1.7) ** 2) / (0.02 * N * N)) + 0.3 * np.cos(jj * 5.0 / N)
    X = np.stack([rng.standard_normal(n), np.tile(smooth.reshape(-1), nt), rng.random(n)]).astype(np.float32)
    Y = np.stack([rng.standard_normal(m), np.tile(np.hanning(nd) + 0.1, nt * na), rng.random(m)]).astype(np.float32)
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    AX3, ATY3 = A.apply(Xd), A.apply(Yd, transpose=True)
    AX1 = torch.stack([A.apply(Xd[j]) for j in range(3)])
    ATY1 = torch.stack([A.apply(Yd[j], transpose=True) for j in range(3)])
    same_adj = RC.case_paths(case, 3)[2:] == (adj_kind, nsplit, prep)
    batch_equal = torch.equal(AX3, AX1) and (not same_adj or torch.equal(ATY3, ATY1))
    # the same apply again = the same bits (k_radon_adj_quad once let records land in registers it had given away: 2048^2 with two
    # quads returned ~100 other pixels per apply, which is how the batch of three above came to differ from the three one by one)
    batch_equal = batch_equal and torch.equal(A.apply(Yd[0], transpose=True), ATY1[0]) and torch.equal(A.apply(Xd[0]), AX1[0])
    Ur = (abs(R) + abs(sp.vstack(krows).tocsr())).tocoo()
    Tr = sp.csr_matrix((TAU_FWD * ws[rays[Ur.row]], (Ur.row, Ur.col)), shape=R.shape)
    Uc = (abs(C) + abs(sp.hstack(kcols).tocsc())).tocoo()
    Tc = sp.csc_matrix((TAU_ADJ * ws[Uc.row], (Uc.row, Uc.col)), shape=C.shape)
    nz_row, nz_col = np.diff(R.indptr), np.diff(C.indptr)
    for j in range(3):
        x64, y64 = X[j].astype(np.float64), Y[j].astype(np.float64)
        want_f = R @ x64
        b_f = (2 * nz_row + 16) * EPS * (abs(R) @ np.abs(x64)) + Tr @ np.abs(x64)
        want_a = C.T @ y64
        b_a = (2 * nz_col + 16) * EPS * (abs(C).T @ np.abs(y64)) + Tc.T @ np.abs(y64)
        sets = [("acc_fwd", AX1[j][torch.from_numpy(rays).to(dev)], want_f, b_f), ("acc_adj", ATY1[j][pix_dev], want_a, b_a)]
        if not same_adj:
            sets.append(("acc_adj_batch3", ATY3[j][pix_dev], want_a, b_a))
        for tag, got, want, b in sets:
            got = got.double().cpu().numpy()
            err = np.abs(got - want)
            stats[tag] = max(stats.get(tag, 0.0), float(np.max(np.where(err > 0, err / np.maximum(b, 1e-300), 0.0))))
            stats[tag + "_norm"] = max(stats.get(tag + "_norm", 0.0), relerr(got, want))

    print(f"\n[radon {RC.case_id(case)}] probes {rays.size} rays x {pix.size} pixels ({shared_nz} shared non-zeros, "
          f"{int(nearest.sum())} certainly nearest) | " + " ".join(f"{k} {v:.3g}" for k, v in sorted(stats.items()))
          + f" | batch_equal {batch_equal} (same adjoint kernel {same_adj}) | unequal {unequal}")
    for tag, limit in [(t, 1.0) for t in ("fwd", "adj", "pair_neighbour", "acc_fwd", "acc_adj")] + \
                      [(t, 1e-5) for t in ("acc_fwd_norm", "acc_adj_norm")] + \
                      ([("acc_adj_batch3", 1.0), ("acc_adj_batch3_norm", 1e-5)] if not same_adj else []):
        try:
            bar(f"radon_entrywise.{name}.{tag}", stats[tag], limit)
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, fails
    assert stats["fwd_zero_pattern"] == 0 and stats["adj_zero_pattern"] == 0, stats
    assert not unequal, unequal                                      # (B)
    assert stats["pair_nearest"] == 0.0 and shared_nz >= rays.size, (stats["pair_nearest"], shared_nz, rays.size)   # (C)
    assert batch_equal
