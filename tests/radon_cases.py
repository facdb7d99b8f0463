"""Cases of the parallel-beam projector's entry-wise tests (tests/test_gpu_radon_entrywise.py) and the projector's dispatch restated
in Python, importable without a GPU: tests/test_radon_oracle_rows_cols_host.py asserts on the CPU that the table still reaches
every forward kernel and every adjoint route, so a case that a later dispatch change moves to another kernel fails there.

kernel_paths restates, with CU = 256 compute units (MI355X):
  * radon_create_impl (csrc/radon2d.hip): the band height (128; 64 when 128-row bands give fewer than 64 workgroups; 256 from
    2048^2 on; br_rows(N) = 64 or 32 for the band-resident kernel), the band-resident condition, the quads of a frame and adjq_ok;
  * fwd_path / radon_forward (csrc/radon_fwd.hip): k_radon_fwd or k_radon_fwd_lds, written at once (one band) or as band
    partials that k_radon_bands_post adds up; k_radon_fwd_band; the quad kernels;
  * adj_path (csrc/radon_adj.hip): simple, tile16_b16, tile16_b4, tile32_b8 with nsplit 1, 4 or 8, groups, quad, and prep.
"""
import numpy as np

CU = 256
RADON_BAND, BR_ROWS, BR_PAD, BR_NMAX, QD_R, QD_MAXCH = 128, 64, 4, 1024, 8, 32

ADJ_KINDS = ("quad", "groups", "tile32_b8", "tile16_b16", "tile16_b4", "simple")      # AdjKind (csrc/radon_internal.h)


def _ceil_div(a, b):
    return -(-a // b)


def br_rows(N):
    return BR_ROWS if BR_ROWS * (N + 2 * BR_PAD) * 4 <= 150 * 1024 else BR_ROWS // 2


def quads_of_frame(angles):
    """The quads radon_create_impl makes of one frame's angles: the member count of each (angles that are images of one base angle
    in [0, 45 deg] under the grid's symmetries share a quad, one per slot; a slot met twice opens another quad of that base)."""
    cand = []
    for th in angles:
        ct, st = np.cos(th), np.sin(th)
        if abs(ct) >= abs(st):
            t = abs(st) / abs(ct)
            slot = 0 if (ct > 0) == (st >= 0) else 1
        else:
            t = abs(ct) / abs(st)
            slot = 2 + (0 if (st > 0) == (ct >= 0) else 1)
        cand.append((np.arctan2(t, 1.0), slot))
    cand.sort(key=lambda c: c[0])                      # stable, like std::stable_sort
    quads, i = [], 0
    while i < len(cand):
        j = i
        while j < len(cand) and cand[j][0] - cand[i][0] <= 1e-12:
            j += 1
        left = [c[1] for c in cand[i:j]]
        while left:
            taken, rest = set(), []
            for s in left:
                (rest.append(s) if s in taken else taken.add(s))
            quads.append(len(taken))
            left = rest
        i = j
    return quads


def kernel_paths(N, nd, na, nt, batch, env, angles=None):
    """(forward, (band height, bands), adjoint, nsplit, prep) of a handle of nt frames of N x N pixels, na angles per frame and nd
    detectors, for an apply of `batch` vectors.  env: the TRK_RADON_* variables that are set (a mapping; those read when the handle
    is made and those read per call alike).  angles: the nt * na angles, frame-major (only the mirrored-pair adjoint's condition
    looks at them); None: na equally spaced views of [0, pi) in every frame."""
    if angles is None:
        angles = np.tile(np.linspace(0, np.pi, na, endpoint=False), nt)
    angles = np.asarray(angles, dtype=np.float64).reshape(nt, na)
    # ---- radon_create_impl
    band = RADON_BAND
    wgs128 = _ceil_div(nd, 64) * _ceil_div(na, 4) * _ceil_div(N, RADON_BAND)
    if wgs128 < 64 and N > 64:
        band = 64
    if N >= 2048 and N % QD_R == 0:
        band = 2 * RADON_BAND
    band_res = N % BR_ROWS == 0 and 2 * BR_ROWS <= N <= BR_NMAX and "TRK_RADON_NO_BANDRES" not in env
    if band_res:
        band = br_rows(N)
    nb = _ceil_div(N, band)
    per_frame = [quads_of_frame(angles[f]) for f in range(nt)]
    nq = max(len(q) for q in per_frame)
    members = sum(sum(q) for q in per_frame)
    adjq_min = int(env.get("TRK_RADON_ADJQ_MIN", 2048))
    adjq_ok = nq > 0 and N % 64 == 0 and N >= adjq_min and 4 * members >= 3 * 4 * nt * nq
    # ---- fwd_path / radon_forward (torch's allocations and the rows of a [batch, N * N] block are 16-byte aligned when N % 4 == 0)
    lds = N % 4 == 0
    win = nb > 1 and N >= 1024 and lds and band <= QD_R * QD_MAXCH and not band_res
    if band_res and lds:
        fwd = "k_radon_fwd_band"
    elif win:
        fwd = "k_radon_fwd_quad" if "TRK_RADON_NO_QUADF" in env else "k_radon_fwd_quadf+quad"
    else:
        fwd = "k_radon_fwd_lds" if lds else "k_radon_fwd"
    # ---- adj_path
    if "TRK_RADON_ADJ_SIMPLE" in env or N < 16:
        return fwd, (band, nb), "simple", 1, True
    kind, prep, nsplit = "tile32_b8", na > 32, 1
    tiles32 = _ceil_div(N, 32) ** 2 * nt
    if batch == 1 and tiles32 < 1024 and na > 32 and N >= 64:
        nsplit = 8 if tiles32 <= 128 else 4
    T = 32 if (tiles32 >= 1024 or nsplit > 1) else 16
    wgs = _ceil_div(N, T) ** 2 * nt
    if T == 32:
        if nsplit == 1 and adjq_ok and "TRK_RADON_NO_ADJQ" not in env:
            kind, prep = "quad", True
        elif nsplit == 4 and wgs <= CU and wgs * 4 >= 3 * CU:
            kind = "groups"
    elif na > 32 or wgs <= 4 * CU:
        kind = "tile16_b16"
    else:
        kind = "tile16_b4"
    return fwd, (band, nb), kind, nsplit, prep


def views(na, offset=0.0):
    return np.linspace(0, np.pi, na, endpoint=False) + offset


def _deg(*d):
    return np.deg2rad(np.asarray(d, dtype=np.float64))


TIES = np.array([0, np.pi / 4, np.pi / 2, 3 * np.pi / 4, np.pi, 3 * np.pi / 2, -np.pi / 4])
# every sign case of (cos, sin), angles outside [0, pi): the "signs" set of test_radon_shared_window_forward_vs_oracle
SIGNS = _deg(20.0, 160.0, -20.0, 200.0, 70.0, 110.0, -70.0, 250.0, 290.0, 340.0, -160.0, 21.0)
# a complete quad, one of three, a complete one, and 30 deg given twice (the second opens a quad of its own): 16 members in 5 quads,
# mostly full; the second group of four quads holds one
QUADS_MIXED = _deg(10.0, 80.0, 100.0, 170.0, 11.0, 79.0, 101.0, 12.0, 78.0, 102.0, 168.0, 30.0, 30.0, 150.0, 60.0, 120.0)
QUADS_TWO = _deg(15.0, 75.0, 105.0, 165.0, 40.0, 50.0, 130.0, 140.0)

# name, N, angles (nt * na, frame-major), n_det, frames, variables set while the handle is made
CASES = [
    ("tiny", 12, views(5, 0.1), 12, 1, {}),
    ("odd50", 50, views(12), 75, 1, {}),
    ("odd257", 257, views(33, 0.013), 301, 1, {}),
    ("odd257few", 257, views(7, 0.2), 257, 1, {}),
    ("lds64", 64, views(40), 40, 1, {}),
    ("lds132", 132, views(12, 0.05), 190, 1, {}),
    ("band128", 128, views(30), 128, 1, {}),
    ("band640", 640, views(45, 0.013), 905, 1, {}),
    ("groups448", 448, views(36), 448, 1, {}),
    ("b4_520", 520, views(8, 0.3), 520, 1, {}),
    ("tile1000", 1000, views(40), 1000, 1, {}),
    ("tile1000few", 1000, views(8, 0.11), 1000, 1, {}),
    ("quad1028", 1028, SIGNS, 1028, 1, {}),
    ("quad1024", 1024, QUADS_MIXED, 1024, 1, {"TRK_RADON_NO_BANDRES": "1", "TRK_RADON_ADJQ_MIN": "1024"}),
    ("quad2048", 2048, QUADS_TWO, 2048, 1, {}),
    ("dynamic", 256, np.concatenate([views(15, 0.21 * f) for f in range(5)]), 364, 5, {}),
    ("ties96", 96, TIES, 96, 1, {}),
    ("ties97", 96, TIES, 97, 1, {}),
]


def case_paths(case, batch=1, extra_env=()):
    name, N, ang, nd, nt, env = case
    e = dict(env)
    e.update({k: "1" for k in extra_env})
    return kernel_paths(N, nd, len(ang) // nt, nt, batch, e, ang)


def case_id(case):
    name, N, ang, nd, nt, env = case
    fwd, (band, nb), adj, nsplit, prep = case_paths(case)
    return f"{name}-{N}x{len(ang) // nt}x{nd}" + (f"x{nt}f" if nt > 1 else "") + f"-{fwd}-{band}x{nb}-{adj}" + (f"/{nsplit}" if nsplit > 1 else "") + ("-prep" if prep else "")
