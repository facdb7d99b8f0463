"""Operands, references and bounds of the first-difference tests (csrc/tvops.hip: k_d2_fwd, k_d2_adj, k_time_fwd, k_tv_weights,
k_tvt_weights, k_tv_grad; csrc/vecops.hip: k_isotv_weights), built from sizes and seeds alone and with NumPy alone:
tests/test_tv_cases_host.py checks the cases themselves on the CPU, tests/test_gpu_tv_entrywise.py runs them through the kernels.

Layout (tvops.hip:4-6).  An image sequence is an array X[f][i][j] of shape (nt, N, N), frame-major.  With ps = 2 N (N - 1) and
npix = N^2 the rows of the space-time operator are
  [ frame 0: H (N x (N-1), H[i][j] = x[i][j] - x[i][j+1]) ; V ((N-1) x N, V[i][j] = x[i][j] - x[i+1][j]) | frame 1 ... |
    temporal row 0: x_0 - x_1 | ... | temporal row nt-2 ]
and the 2-D operator is the case nt = 1.  A time slice (a rank's share) owns whole frames; with a next slice it also owns the row
(its last frame) - (the next slice's first frame), and the weights of a slice with a previous slice carry one more row behind its
own: the weight of the previous slice's boundary row, recomputed.  Every reference below is index arithmetic on such arrays in
float64 (the same functions evaluate in float32 with dtype=np.float32: the kernels' own steps), none goes through a sparse matrix.

Two kinds of operands.

Exact operands make every intermediate exact in float32, in any order, so a device result must EQUAL its reference:
  images, y, dotv        non-zero integers in [-15, 15]
  r_in                   non-zero integers in [-31, 31]
  weights                one of 0.5, 1, 2, 4
  lam                    0.25
A difference is an integer of at most 30, a weighted one a multiple of 1/2 of at most 120, a sum of six of them at most 720, lam
times it a multiple of 1/8, and with r_in below 2^10: far inside the 24 bits of a float32 (`fits_float32` checks the values).  The
float64 sums are exact while the sum of the absolute terms stays below 2^53 units (`sum_is_exact`).  One term dropped, doubled or
taken from a neighbouring pixel changes an entry by at least 1/8.

General operands are standard normals (weights: uniform in [0.5, 2)); `flat` images are piecewise constant — blocks of equal
values in space and pairs of equal frames, so that many differences are exactly 0 — for the weights.

Bounds, from the kernels' arithmetic (u = 2^-24), not measured:
  L x                    one subtraction per entry:  |got - ref| <= u |ref|
  L2^T y, L^T y          k_d2_adj adds the k <= 6 terms present at a pixel one after the other in float32, starting from 0: the first
                         addition is exact, each later one rounds once, |got - ref| <= (k - 1) u S + O(u^2); taken as  k u S,  S the sum
                         of the absolute terms of the pixel
  tv_grad                k_tv_grad: every term w (a - b) carries two roundings (the difference, __fmul_rn), the sum of k terms k - 1,
                         lam * one more, r_in + one more of the result:  |got - ref| <= (k + 3) u (|r_in| + lam S),  S the sum of the
                         absolute terms w |a - b| of the pixel
  dots, sums of squares  float64 accumulation of exact products of the float32 values AS STORED:  n 2^-53 sum |t_i|
  weights                the reference repeats the kernel's float32 steps up to t — v = fl32(a - b), eps2 = fl32(eps^2), t = fmaf(v, v, eps2)
                         rounded once (`fma32`) — and evaluates t^e in float64;  |got - ref| <= (|e| + U + 1) u |ref|,  U the error of the
                         function in units of u: 1 for the hardware reciprocal square root (q = 1, eps2 >= 1e-30), 2 for 1 / sqrtf
                         (two correctly rounded operations) and for 1 / sqrtf(sqrtf) of the isotropic kernel (2.5 u by the same count,
                         within |e| + U + 1 = 3.25), 0 and a bound of 0 where the weight is the constant 1.
  powf                   nothing in the project gives a figure.  POWF_U is twice the worst deviation from the float64 reference measured
                         on the MI355X over the cases of test_tv_weights and test_isotv_weights (tests/test_gpu_tv_entrywise.py; the
                         `powf.units` lines of profiles/tv_entrywise/bars.txt), in units of u, and never above POWF_CAP = 16 (the OpenCL
                         full-profile limit for pow, taken in the smaller unit u <= 1 ulp): the cap is a condition those tests assert
                         on what they measure, not a measurement.
"""
import numpy as np

NT = 256                       # threads of a workgroup: one per image column
RB = 4                         # image rows per thread and batch
TV_MAX_BLOCKS = 4096           # cap on the blocks per frame of the reducing 2-D forms (kTvMaxBlocks)
TIME_MAX_BLOCKS = 1024         # cap on the blocks per row of the temporal kernels (kMaxPartialBlocks)
U24, U53, DENORM = 2.0 ** -24, 2.0 ** -53, 2.0 ** -149
POWF_CAP = 16.0
POWF_MEASURED = 2.327          # worst |got / ref - 1| / u of a powf weight on the MI355X: the *.powf.units lines of profiles/tv_entrywise/bars.txt
POWF_U = min(2.0 * POWF_MEASURED, POWF_CAP)
LAM_EXACT = 0.25
LAM_GENERAL = float(np.float32(0.37))          # the kernels take lam as a float32

WIDE = np.longdouble
assert np.finfo(WIDE).nmant >= 63, "the references of the sums need a significand wider than float64's"
F32, F64 = np.float32, np.float64


def _rng(*key):
    return np.random.default_rng([int(v) for v in key])


def _nonzero_ints(rng, shape, top):
    m = rng.integers(0, 2 * top, shape, dtype=np.int16) - np.int16(top)
    m[m >= 0] += 1
    return m.astype(F32)


# ----------------------------------------------------------------------------------------------------------- sizes
def sizes(N, nt=1, has_next=False):
    """(npix, ps, ntemp, rows) of a handle over nt frames."""
    npix, ps = N * N, 2 * N * (N - 1)
    ntemp = nt - 1 + (1 if has_next else 0)
    return npix, ps, ntemp, nt * ps + ntemp * npix


def row_batches_strided(N):
    """Whether the capped grid of the reducing 2-D forms (grid2(..., capped = true)) strides over the row batches."""
    gx = -(-N // NT)
    return -(-N // RB) > TV_MAX_BLOCKS // gx


def temporal_strided(N):
    return -(-N * N // NT) > TIME_MAX_BLOCKS


# ----------------------------------------------------------------------------------------------------------- operands
def image(kind, nt, N, seed=0):
    """A float32 sequence (nt, N, N): 'exact' (non-zero integers), 'normal', 'flat' (piecewise constant).  Do not modify."""
    rng = _rng(11, ("exact", "normal", "flat").index(kind), nt, N, seed)
    if kind == "exact":
        return _nonzero_ints(rng, (nt, N, N), 15)
    if kind == "normal":
        return rng.standard_normal((nt, N, N)).astype(F32)
    b = max(2, N // 3)
    base = rng.standard_normal(((nt + 1) // 2, -(-N // b), -(-N // b))).astype(F32)
    return np.ascontiguousarray(np.repeat(np.repeat(np.repeat(base, 2, 0), b, 1), b, 2)[:nt, :N, :N])


def vector(kind, n, seed, top=15):
    """A float32 vector of n entries: non-zero integers in [-top, top] ('exact') or standard normals."""
    rng = _rng(12, kind == "exact", n, seed)
    return _nonzero_ints(rng, n, top) if kind == "exact" else rng.standard_normal(n).astype(F32)


def weights(kind, n, seed=0):
    rng = _rng(13, kind == "exact", n, seed)
    if kind == "exact":
        return rng.choice(np.array([0.5, 1.0, 2.0, 4.0], dtype=F32), n)
    return rng.uniform(0.5, 2.0, n).astype(F32)


def lam_of(kind):
    return LAM_EXACT if kind == "exact" else LAM_GENERAL


# ----------------------------------------------------------------------------------------------------------- references
class Ref:
    """A reference per entry (float64, flat), its bound, and for the gather forms the sum S of the absolute terms and their count k."""

    def __init__(self, val, bound, S=None, k=None):
        self.val, self.bound, self.S, self.k = np.asarray(val).reshape(-1), np.asarray(bound).reshape(-1), S, k

    def take(self, idx):
        return Ref(self.val[idx], self.bound[idx])


def compare(got, R, exact):
    """(indices of the entries that fail, worst error / bound): equality on exact operands, the bound otherwise; a NaN fails."""
    got = np.asarray(got).reshape(-1)
    assert got.shape == R.val.shape, (got.shape, R.val.shape)
    err = np.abs(got.astype(WIDE) - R.val.astype(WIDE)).astype(F64) if R.val.dtype == WIDE else np.abs(got.astype(F64) - R.val)
    if exact:
        return np.flatnonzero(~(err == 0)), 0.0
    bad = np.flatnonzero(~(err <= R.bound))
    pos = R.bound > 0
    ratio = float(np.max(err[pos] / R.bound[pos])) if pos.any() else 0.0
    return bad, ratio


def d2_fwd(X, dtype=F64):
    """[H ; V] of every leading index of X (..., N, N): shape (..., 2 N (N - 1))."""
    X = np.asarray(X, dtype=dtype)
    lead = X.shape[:-2]
    H = X[..., :, :-1] - X[..., :, 1:]
    V = X[..., :-1, :] - X[..., 1:, :]
    return np.concatenate((H.reshape(lead + (-1,)), V.reshape(lead + (-1,))), axis=-1)


def st_fwd(X, xnext=None, dtype=F64):
    """The rows of the space-time operator over the frames X (nt, N, N), flat; xnext: the first frame of the next slice."""
    X = np.asarray(X, dtype=dtype)
    after = X[1:] if xnext is None else np.concatenate((X[1:], np.asarray(xnext, dtype=dtype)[None]), axis=0)
    T = X[:after.shape[0]] - after
    return np.concatenate((d2_fwd(X, dtype).reshape(-1), T.reshape(-1)))


def lx_ref(X, xnext=None):
    v = st_fwd(X, xnext)
    return Ref(v, U24 * np.abs(v) + DENORM)


def split_rows(y, N, nt, ntemp):
    """The blocks of a vector laid out as the rows of L: H (nt, N, N-1), V (nt, N-1, N), T (ntemp, N, N)."""
    npix, ps = N * N, 2 * N * (N - 1)
    sp = y[:nt * ps].reshape(nt, ps)
    return (sp[:, :N * (N - 1)].reshape(nt, N, N - 1), sp[:, N * (N - 1):].reshape(nt, N - 1, N),
            y[nt * ps:nt * ps + ntemp * npix].reshape(ntemp, N, N))


MUTANTS = ("predicate", "column", "frame0", "wrow")


def gather(H, V, T, Tprev=None, dtype=F64, mutant=None):
    """(L^T y) per pixel from the blocks of y, the terms added one after the other in k_d2_adj's / k_tv_grad's order
         + H[i][j] (j < N-1)  - H[i][j-1] (j > 0)  + V[i][j] (i < N-1)  - V[i-1][j] (i > 0)  + T[f] (row f exists)  - T[f-1]
    where the row before frame 0 is Tprev, the previous slice's (None: there is none).  dtype float64: the reference;
    dtype float32: every addition rounds as the kernels' does — their restatement.  Returns (sum, S, k) of shape (nt, N, N).
    mutant: a subtly wrong restatement — 'predicate': the V[i][j] term needs i < N - 2; 'column': V[i-1] is read from column j + 1
    (the last column from itself); 'frame0': frame 0 drops its + T[0]."""
    nt, N = H.shape[0], H.shape[1]
    acc = np.zeros((nt, N, N), dtype=dtype)
    S = np.zeros((nt, N, N))
    k = np.zeros((nt, N, N), dtype=np.int32)

    def add(where, term, sign):
        term = np.asarray(term, dtype=dtype)
        acc[where] = acc[where] + term if sign > 0 else acc[where] - term
        S[where] += np.abs(term.astype(F64))
        k[where] += 1

    add(np.s_[:, :, :N - 1], H, +1)
    add(np.s_[:, :, 1:], H, -1)
    if mutant == "predicate":
        add(np.s_[:, :N - 2, :], V[:, :N - 2], +1)
    else:
        add(np.s_[:, :N - 1, :], V, +1)
    if mutant == "column":
        add(np.s_[:, 1:, :], np.concatenate((V[:, :, 1:], V[:, :, N - 1:]), axis=2), -1)
    else:
        add(np.s_[:, 1:, :], V, -1)
    ntemp = T.shape[0]                                   # nt - 1, or nt with a next slice
    if mutant == "frame0":
        add(np.s_[1:ntemp], T[1:], +1)
    else:
        add(np.s_[:ntemp], T, +1)
    add(np.s_[1:], T[:nt - 1], -1)
    if Tprev is not None:
        add(np.s_[:1], np.asarray(Tprev).reshape(1, N, N), -1)
    return acc, S, k


def adj_ref(y, N, nt, has_next=False, halo_prev=None, dtype=F64, mutant=None):
    """L^T y of a slice of nt frames; halo_prev: the previous slice's last temporal block (N^2)."""
    ntemp = nt - 1 + (1 if has_next else 0)
    H, V, T = split_rows(np.asarray(y, dtype=dtype), N, nt, ntemp)
    acc, S, k = gather(H, V, T, None if halo_prev is None else np.asarray(halo_prev, dtype=dtype), dtype, mutant)
    return Ref(acc.astype(F64), k * U24 * S + DENORM, S.reshape(-1), k.reshape(-1))


def tv_grad_ref(X, w, r, lam, xprev=None, xnext=None, dtype=F64, mutant=None):
    """r + lam L^T (w .* L x) over the frames X of a slice (w None: unit weights; r None: 0); xprev / xnext: the neighbour slices'
    boundary frames; w as k_tv_weights / k_tvt_weights lay it out (the previous slice's boundary row last).  dtype float32: the
    kernel's own steps — differences, products, the sequential sum, lam *, r + each rounded once.  mutant 'wrow': the previous
    slice's weight row is read from row ntemp - 1 instead of ntemp."""
    X = np.asarray(X, dtype=dtype)
    nt, N = X.shape[0], X.shape[1]
    npix, ps, ntemp, rows = sizes(N, nt, xnext is not None)
    H, V, T = split_rows(st_fwd(X, xnext, dtype), N, nt, ntemp)
    Tp = None if xprev is None else np.asarray(xprev, dtype=dtype).reshape(N, N) - X[0]
    if w is not None:
        w = np.asarray(w, dtype=dtype)
        wH, wV, wT = split_rows(w, N, nt, ntemp)
        H, V, T = wH * H, wV * V, wT * T
        if Tp is not None:
            at = rows - npix if mutant == "wrow" else rows
            Tp = w[at:at + npix].reshape(N, N) * Tp
    acc, S, k = gather(H, V, T, Tp, dtype, mutant)
    lam = dtype(lam)
    out = lam * acc
    mag = float(lam) * S
    if r is not None:
        r = np.asarray(r, dtype=dtype).reshape(nt, N, N)
        out = r + out
        mag = mag + np.abs(r.astype(F64))
    return Ref(out.astype(F64), (k + 3) * U24 * mag + DENORM, S.reshape(-1), k.reshape(-1))


def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays: the exact product (48 bits, a float64), added in float64 with the rounding error recovered
    (Knuth) and folded back as a sticky bit — rounding to odd — so that the second rounding to float32 is that of the exact value."""
    p = np.asarray(a, dtype=F32).astype(F64) * np.asarray(b, dtype=F32).astype(F64)
    c = np.broadcast_to(np.asarray(c, dtype=F32).astype(F64), p.shape)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def _power_ref(t, ed, special):
    """(t^e in float64, U) of the float32 values t.  special: 1 the constant 1, 2 the reciprocal square root (U given by the caller:
    negative here), 3 1 / sqrt(sqrt), 0 powf with e = fl32(ed)."""
    t64 = t.astype(F64)
    if special == 1:
        return np.ones_like(t64), 0.0, 0.0
    if special == 2:
        return 1.0 / np.sqrt(t64), 0.5, -1.0
    if special == 3:
        return 1.0 / np.sqrt(np.sqrt(t64)), 0.25, 2.0
    e = float(F32(ed))
    with np.errstate(over="ignore", divide="ignore"):
        return np.power(t64, e), abs(e), POWF_U


def mm_w_ref(v, eps, q):
    """mm_w (trk_internal.h) of the float32 differences v: ((v^2 + eps^2))^(q/2 - 1)."""
    eps2 = F32(eps * eps)
    t = fma32(v, v, eps2)
    special = 1 if q == 2.0 else 2 if q == 1.0 else 0
    val, ae, U = _power_ref(t, q / 2.0 - 1.0, special)
    if special == 2:
        U = 1.0 if eps2 >= F32(1e-30) else 2.0
    return Ref(val, (0.0 if special == 1 else (ae + U + 1.0) * U24) * np.abs(val))


def is_powf(q):
    return q not in (1.0, 2.0)


def tv_weights_ref(X, eps, q, xprev=None, xnext=None):
    """The weights of every row of L over a slice and, with a previous slice, of that slice's boundary row behind them."""
    X = np.asarray(X, dtype=F32)
    v = st_fwd(X, xnext, F32)
    if xprev is not None:
        v = np.concatenate((v, (np.asarray(xprev, dtype=F32).reshape(X.shape[1:]) - X[0]).reshape(-1)))
    return mm_w_ref(v, eps, q)


def isotv_special(q):
    ed = (q - 2.0) / 4.0
    return ed, (1 if ed == 0.0 else 2 if ed == -0.5 else 3 if ed == -0.25 else 0)


def isotv_weights_ref(x, N, nt, tail, eps, q):
    """k_isotv_weights (vecops.hip:207-213): x viewed as X[i][j][t], centred differences (0 on the first and last row / column),
    w = (g1^2 + g2^2 + eps^2)^((q - 2) / 4) twice, then the weights of the tail."""
    X = np.asarray(x, dtype=F32).reshape(N, N, nt)
    half = F32(0.5)
    g1, g2 = np.zeros_like(X), np.zeros_like(X)
    g1[:, 1:-1, :] = half * X[:, 2:, :] - half * X[:, :-2, :]
    g2[1:-1, :, :] = half * X[2:, :, :] - half * X[:-2, :, :]
    eps2 = F32(eps * eps)
    ed, special = isotv_special(q)
    t = fma32(g1, g1, fma32(g2, g2, eps2)).reshape(-1)
    tt = fma32(tail, tail, eps2) if len(tail) else np.zeros(0, dtype=F32)
    val, ae, U = _power_ref(np.concatenate((t, t, tt)), ed, special)
    if special == 2:
        U = 2.0                                         # 1 / sqrtf on every eps
    return Ref(val, (0.0 if special == 1 else (ae + U + 1.0) * U24) * np.abs(val))


def dot_ref(a, b):
    """sum a_i b_i of float32 vectors as stored (np.longdouble), with the bound n 2^-53 sum |a_i b_i|.  Beyond 2^16 terms the
    products are added in float64 in runs of 4096 (NumPy's pairwise sum: within 12 2^-53 of a run's absolute sum, less than 2^-12
    of the bound) and the runs in np.longdouble."""
    p = np.asarray(a, dtype=F64).reshape(-1) * np.asarray(b, dtype=F64).reshape(-1)        # exact: 24 + 24 bits
    n, run = p.size, 4096
    if n <= 1 << 16:
        s = p.astype(WIDE).sum() if n else WIDE(0)
    else:
        body = n - n % run
        s = p[:body].reshape(-1, run).sum(axis=1).astype(WIDE).sum() + p[body:].astype(WIDE).sum()
    return Ref(np.array([s], dtype=WIDE), np.array([n * U53 * float(np.abs(p).sum())]))


def sum_is_exact(a, b, unit):
    """Whether sum a_i b_i is exact in float64 in any order: every product a multiple of `unit`, their absolute sum below 2^53 units."""
    p = np.asarray(a, dtype=F64).reshape(-1) * np.asarray(b, dtype=F64).reshape(-1)
    q = p / unit
    return bool(np.all(q == np.rint(q))) and float(np.abs(q).sum()) < 2.0 ** 53


def fits_float32(val, unit):
    """Whether every value is a multiple of `unit` (a power of two) below 2^24 units: it is a float32, and so is every partial sum."""
    q = np.asarray(val, dtype=F64) / unit
    return bool(np.all(q == np.rint(q))) and bool(np.all(np.abs(q) < 2.0 ** 24))


# ----------------------------------------------------------------------------------------------------------- slicing
def cut(nt, N, W):
    """A global problem of nt frames cut into W contiguous slices of nt / W frames.  Per slice a dict:
      nt_local, has_prev, has_next, f0 (its first frame)
      lx_map    global row index of every entry of the slice's L x (its spatial rows, its temporal rows — with a next slice the
                boundary row too)
      w_map     the same for its weights: lx_map, then (has_prev) the previous slice's boundary row
      out_map   global pixel index of every entry of the slice's L^T y / tv_grad
      prev_rows global row indices of the previous slice's last temporal block (the halo of the transpose), or None"""
    assert nt % W == 0
    ntl = nt // W
    npix, ps = N * N, 2 * N * (N - 1)
    out = []
    for s in range(W):
        f0, has_prev, has_next = s * ntl, s > 0, s < W - 1
        ntemp = ntl - 1 + (1 if has_next else 0)
        lx_map = np.concatenate((np.arange(f0 * ps, (f0 + ntl) * ps), nt * ps + np.arange(f0 * npix, (f0 + ntemp) * npix)))
        prev_rows = nt * ps + np.arange((f0 - 1) * npix, f0 * npix) if has_prev else None
        out.append(dict(nt_local=ntl, has_prev=has_prev, has_next=has_next, f0=f0, lx_map=lx_map,
                        w_map=np.concatenate((lx_map, prev_rows)) if has_prev else lx_map,
                        out_map=np.arange(f0 * npix, (f0 + ntl) * npix), prev_rows=prev_rows))
    return out


def frames_of(X, s):
    """(the slice's frames, the previous slice's last frame or None, the next slice's first frame or None) of the global X."""
    f0, f1 = s["f0"], s["f0"] + s["nt_local"]
    return X[f0:f1], (X[f0 - 1] if s["has_prev"] else None), (X[f1] if s["has_next"] else None)
