"""Operands, references, restatements and bounds of the projected k x k solves (csrc/projected.hip), built from sizes and seeds
alone, on the CPU: tests/test_projected_cases_host.py checks the cases themselves, tests/test_gpu_projected_entrywise.py runs them
through the kernels.

Reference arithmetic: the stdlib `decimal` module at PREC = 60 significant digits (round-half-even), on the float64 operands exactly
as the device receives them (Decimal(float) converts exactly).  Sums and products are formed in that arithmetic; a solution y* of
M y = c is reached by refinement — the residual c - M y in the reference arithmetic, a correction from a float64 LU factorisation,
the update in the reference arithmetic — until the residual is below 1e-45 of ||M|| ||y|| (`ref_solve` raises otherwise), so y*
carries more than 40 digits whatever cond(M) <= 1e13.  trk_bidiag_tikhonov receives the SQUARES, so its reference starts from
them (alpha_j = sqrt(alpha_sq[j]) in the reference arithmetic).

EXACT operands: nothing rounds, in any order of summation, so the device must EQUAL the reference bit for bit.
  cgs_coeffs, cgs_coeffs_rho,   G, h, a, c, rhs: integers in [-2, 2] (G symmetric; at k > 258 cgs' G keeps 4 % of its entries, +-1), rho2 = 4 (rho = 2: the quotients of the row are
  gram_row_from_sweep           halves, of the diagonal entry quarters), rr, s, tb integers.  `exact_headroom` adds up the ABSOLUTE
                                terms of every sum the kernels form — an upper bound of every partial sum in every order — and
                                the host test asserts that all stay below 2^53 (2^51 for the quotients' numerators) at every size
                                used, 2048 included.
  Cholesky paths                M = C C^T, C an integer lower triangle of bandwidth 3 with entries in {-1, 0, 1} below a diagonal of
                                4 or 8 (strictly diagonally dominant: cond(M) stays below 1e3 at every k): the pivots are 16 or 64,
                                their roots and every quotient by them exact, every Schur update an integer.  M = GA + 0.5 GL with GL
                                a random even symmetric integer matrix and GA = M - GL / 2.  c = M y for an integer y, so both
                                triangular solves pass through integers (C^T y) and multiples of 1 / 8.
  bordered paths                M = C C^T, C UNIT lower bidiagonal with off-diagonals p_j = +-1: the new row of M is (0 .. 0, p_j, 2),
                                every Schur complement is 1, and M^-1[a][b] = q_a q_b (k - max(a, b)) with q_j = prod_{l <= j} (-p_l):
                                integers of size at most k, at any k.  Split and right-hand side as above.
  hess_tikhonov                 an integer upper Hessenberg matrix (entries in [-3, 3], the sub-diagonal 1 .. 4 and its square in
                                nrm2_sq), every column split as integer coef + coef2: the stored column and the row of G = H^T H are
                                exact.  Mode 0 also runs on H = [C^T; 0] (C of the Cholesky paths, lam = 0): then G = C C^T and
                                y = (beta0 / C[0][0]) e_1 exactly.  With lam > 0, G + lam I = C C^T has no integer Hessenberg root
                                at large k (the smallest eigenvalue of a unit-bidiagonal C C^T falls as 1 / k^2), so the solves of
                                modes 1 and 2 on integer H are held to the bounds below, not to equality; mode 2 at k = 1 with
                                lam = 0 and a diagonal entry that is a power of two is exact.

GENERAL operands
  Krylov Gram data              A: the 256 x 256 matrix of a 7 x 7 Gaussian blur (sigma 1.5, zero boundary) of a 16 x 16 image, L: the
                                2-D first-difference matrix (480 x 256), b = A x_true + noise.  V: Golub-Kahan on (A, b) with full
                                reorthogonalisation (128 vectors: cond(GA) 1e7, cond(GA + lam GL) up to 2e3) and by the plain
                                three-term recurrence, which loses orthogonality near step 25 (cond(GA + lam GL) 1e8 .. 1e11, as
                                the solvers' fp32 bases give), in NumPy float64; GA = (AV)^T AV, GL = (LV)^T LV, c = (AV)^T b, lam
                                in {1e-4, 1e-1, 10}, the depth cut per lam by the condition cap below (`krylov_depth`).
  Hessenberg                    Arnoldi (modified Gram-Schmidt, float64) on that blur, started from b.
  bidiagonals                   alpha, beta of that Golub-Kahan run (they decay with the blur's singular values), as squares,
                                mu in {0, 1e-6, 1e-2, 0.5}; a random set (entries in [0.05, 1.05)) at the large sizes.
  random                        W W^T of Gaussian W (k x (2k + 5), k x 3k), a random upper Hessenberg matrix: cond ~ 1e2.
Condition cap, asserted on the CPU for every solve case: k cond_2(M) 2^-53 <= 1e-3 — no pivot of the Cholesky factorisation and
no Schur complement of the bordering comes near zero, so the 1e-300 lifts are never taken on general operands.

BOUNDS of the general operands, u = 2^-53, gamma_n = n u / (1 - n u).
  sums of products              A sum of n products formed in ANY order (symv4's four chains per row and two lane exchanges, a
                                thread's strided partial, wave_sum and the four wave totals; sequentially in k_hess_tikhonov) rounds
                                every product once and sends every term through at most n - 1 additions (additions of zero are
                                exact): |computed - exact| <= gamma_{n+1} sum |terms|  (Higham, Accuracy and Stability of Numerical
                                Algorithms, section 4.2; one unit of slack).  Carried through the recurrences as running errors:
    cgs_coeffs                  pass 1: c = h (0 + h: exact, e = 0).  Pass p + 1: t = fl(h - fl(G c)), c' = fl(c + t):
                                e' = e + [gamma_{k+1} |G| (|c| + e) + |G| e] + u |t~| + u |c'~|  per entry (`ref_cgs`).
    rho2                        v = fl(fl(rr - 2 ch) + cgc), ch = c . h, cgc = c . (G c), each a sum of k products of computed values:
                                |dv| <= 2 d_ch + d_cgc + 2 u (|rr| + 2 |ch| + |cgc| + 2 d_ch + d_cgc).
    gram_row_from_sweep         rho = fl(sqrt(rho2)): row_i = fl(fl(a_i - fl((G c)_i)) / rho):
                                [gamma_{k+1} (|G| |c|)_i + u |a_i - (G c)_i|] / rho + 3 u |row_i|;  the diagonal entry divides by
                                fl(rho rho): two roundings more, 5 u; rhs_k as the row with c . rhs in the place of (G c)_i.
    hess_tikhonov, row of G     g_i = sum_{r <= i+1} H[r][i] hc[r], sequential: gamma_{i+3} sum |terms| (hc is the STORED column
                                fl(coef + coef2), fl(sqrt(nrm2_sq)) — one IEEE operation each, restated bit for bit in NumPy).
  Cholesky solves               normwise backward error of the device's y in the reference arithmetic,
                                eta = ||c - M y||_2 / (||M||_2 ||y||_2 + ||c||_2) <= k gamma_{3k+1} + d_M / ||M||_2 :
                                Higham, Theorems 10.3 and 10.4: (M + dM) y = c with |dM| <= gamma_{3k+1} |R^T| |R| and
                                || |R^T| |R| ||_2 <= k ||M||_2.  d_M is the error of the operand the factorisation starts from:
                                2 u || |GA| + lam |GL| ||_F for fl(GA + fl(lam GL)) (two roundings per entry); for
                                k_hess_tikhonov mode 0 the Frobenius norm of the running-error bounds of G's entries plus u (lam on
                                the diagonal) plus u ||c|| for c = fl(beta0 H[0][:]) (`chol_bound`, `hess_chol_bound`).
  bidiag_tikhonov               residual of the normal equations in the reference arithmetic: T = B^T B + mu^2 I (tridiagonal),
                                d = beta0 alpha_1 e_1:  ||T y - d||_2 <= 32 k u (a^2 ||y||_2 + a beta0), a = the largest column norm of
                                [B; mu I] (a lower bound of its 2-norm: no looser than the norm itself).  Givens QR is backward stable
                                (Higham, Theorem 19.10): y solves the least-squares problem of A + dA, b + db with ||dA|| <= eps ||A||,
                                ||db|| <= eps ||b||, hence ||A^T (A y - b)|| <= eps (||A||^2 ||y|| + 2 ||A|| ||b||) to first order.  The
                                right-hand side passes through all 2k rotations, gamma_6 each (Higham, Lemma 19.8): 12 k u; the
                                square roots of the operands, the stored 1 / rho and the back substitution add a few u: eps = 16 k u,
                                doubled for the factor 2 of the second term.  y_over_alpha: y'_j fl(alpha_j) = y_j to 4 u.
  bordered inverse              An explicit inverse is not backward stable: its y is held to a FORWARD error,
                                    ||y - y*||_2 / (cond_2(M) u ||y*||_2)   and   max |Minv M - I| / (cond_2(M) u),
                                against a bar MEASURED on the NumPy float64 restatement of the same recurrence (`np_border`: u = Minv g
                                row sums, s = g_j - g . u, Minv += u u^T / s, the border -u / s, 1 / s) over the whole list of general
                                bordered cases (`border_cases`, `hess_cases`: random, Krylov and Hessenberg chains, grown one row at
                                a time, several at a time and from nothing).  cond_2 comes from NumPy's SVD; Minv M - I is formed in
                                np.longdouble (64-bit significand: its own error is 2^-11 of the quantity measured).
                                One constant does not fit the three families of cases, so each has its own, (forward, inverse):
                                    "well"  tikhonov_border_body (trk_gram_tikhonov with Minv, trk_gks_rows_solve) on the random and
                                            the reorthogonalised Krylov cases, cond <= 2e3: measured 1.15, 2.06   recorded 1.2, 2.1
                                    "ill"   the same on the plain-recurrence Krylov cases, cond 5e9 .. 2.5e11:
                                                                                        measured 71.5, 1.66e4  recorded 72, 17000
                                            (the Cholesky form reaches 0.4 there: the bordered inverse loses about cond^1.3 u, not
                                            cond u — a relative error of 3e-4 in y at cond 2.5e11, still below the fp32 basis)
                                    "hess"  k_hess_tikhonov's chain (mode 2 at k <= 2, then mode 1; its G rows carry k roundings
                                            of their own into every later step): measured 39.9, 20.3            recorded 40, 21
                                The bar of a case is 8 x the recorded constant of its family (BORDER[family]; three bits: the kernel
                                sums in symv4's four chains per row where NumPy sums pairwise — both are draws under the same bound):
                                    well 9.6, 16.8     ill 576, 136000     hess 320, 168
                                One common bar, 8 x the largest of all, would leave the well-conditioned cases 1e4 times more room.
                                The "ill" inverse bar is 136000 cond u, about 3.8 at cond 2.5e11 (the restatement reaches 0.46):
                                it admits max |Minv M - I| above 1 and so constrains nothing there — on those cases only the
                                forward bar on y holds the inverse.  The host test recomputes the maxima and asserts that none
                                exceeds its recorded constant.
"""
import decimal
import functools
from decimal import Decimal

import numpy as np

PREC = 60
U = 2.0 ** -53
CAP = 1e-3
BORDER = {"well": (1.2, 2.1), "ill": (72.0, 1.7e4), "hess": (40.0, 21.0)}     # measured (forward, inverse) ratios: docstring
BAR_FACTOR = 8.0


def border_family(name):
    return "hess" if name.startswith("hess") else ("ill" if "plain" in name else "well")


def border_bars(name):
    f, i = BORDER[border_family(name)]
    return BAR_FACTOR * f, BAR_FACTOR * i
BIDIAG_C = 32.0

SIZES = list(range(1, 18)) + [63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257, 258]
CHOL_SIZES = [k for k in SIZES if k <= 139] + [87, 88, 89, 90, 139]          # 64 KB of LDS ends at 89 (gram), 87 (hess mode 0)
BIG_SIZES = [1024, 2048]
LAMS = (1e-4, 1e-1, 10.0)
MUS = (0.0, 1e-6, 1e-2, 0.5)

_CTX = decimal.Context(prec=PREC, rounding=decimal.ROUND_HALF_EVEN, Emin=-999999, Emax=999999)


def reference_digits():
    return _CTX.prec


def ctx():
    return decimal.localcontext(_CTX)


def gamma(n):
    return n * U / (1.0 - n * U)


def _rng(*key):
    return np.random.default_rng([int(v) for v in key])


def dec(a):
    """The float64 array as an object array of Decimals: exact."""
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    flat = out.reshape(-1)
    for i, v in enumerate(a.reshape(-1).tolist()):
        flat[i] = Decimal(v)
    return out


def fl(a):
    """Decimals rounded to float64 (correctly rounded)."""
    a = np.asarray(a, dtype=object)
    return np.array([float(v) for v in a.reshape(-1)], dtype=np.float64).reshape(a.shape)


def dnorm(v):
    """2-norm of a Decimal vector, as a float."""
    with ctx():
        return float(sum((x * x for x in np.asarray(v, dtype=object).reshape(-1)), Decimal(0)).sqrt())


# ------------------------------------------------------------------------------------------------------------ exact operands
def small_ints(rng, shape, m=2):
    return rng.integers(-m, m + 1, shape).astype(np.float64)


def exact_sym(rng, k, m=2):
    a = np.tril(small_ints(rng, (k, k), m))
    return a + np.tril(a, -1).T


def exact_cgs(k, seed=0):
    """G (symmetric), h, g_new (= the last row of G), rr: integers."""
    rng = _rng(11, k, seed)
    G, h = exact_sym(rng, k), small_ints(rng, k)
    if k > 258:                                                # 4 % of the entries, +-1: three passes stay below 2^53 at 2048
        keep = np.tril(rng.random((k, k)) < 0.04)
        G, h = np.sign(G) * (keep | keep.T), np.sign(h)
    return {"G": G, "h": h, "g_new": G[k - 1].copy(), "rr": float(rng.integers(1, 9)) * 2.0 ** 40}


def int_cgs(G, h, passes):
    """c after `passes` sweeps and G c, in Python integers (object arrays): exact at any size."""
    Gi, hi = G.astype(np.int64).astype(object), h.astype(np.int64).astype(object)
    c = np.zeros(len(h), dtype=object)
    for p in range(passes):
        c = c + (hi - Gi.dot(c)) if p else hi.copy()
    return c, Gi.dot(c)


def float_cgs(G, h, passes):
    """int_cgs in float64 (BLAS sums): the same integers wherever exact_headroom stays below 2^53 — for the large sizes."""
    c = np.zeros(len(h))
    for p in range(passes):
        c = c + (h - G @ c) if p else h.copy()
    return c, G @ c


def exact_headroom(G, h, passes, a=None, rhs=None):
    """The largest sum of absolute terms any of the kernels' sums can meet on these operands (all are integers): cgs through `passes`,
    c . h, c . G c, and with `a` the products of gram_row_from_sweep with this c."""
    Ga, c = np.abs(G), np.zeros(len(h))
    worst = 0.0
    for p in range(passes):
        if p:
            s = Ga @ np.abs(c)
            worst = max(worst, float(s.max()))
            c = np.abs(c) + np.abs(h) + s
        else:
            c = np.abs(h)
    s = Ga @ c
    worst = max(worst, float(s.max()), float(c @ np.abs(h)), float(c @ s))
    if a is not None:
        worst = max(worst, float(c @ np.abs(a)), float((np.abs(a) + s).max()))
    if rhs is not None:
        worst = max(worst, float(c @ np.abs(rhs)))
    return worst


def exact_gram_row(k, seed=0):
    """gram_row_from_sweep on integers with rho2 = 4: G (k x k), a, c, s, tb, rhs — c, a are the sweep's, not related to G."""
    rng = _rng(12, k, seed)
    return {"G": exact_sym(rng, k), "a": small_ints(rng, k), "c": small_ints(rng, k), "s": float(rng.integers(-9, 10)),
            "rho2": 4.0, "rhs": small_ints(rng, k), "tb": float(rng.integers(-9, 10))}


def int_gram_row(G, a, c, s, rho2, rhs=None, tb=None):
    """(row, diagonal entry, rhs_k) of gram_row_from_sweep from integer operands with rho2 = 4: exact float64 values."""
    assert rho2 == 4.0
    Gi, ai, ci = (np.asarray(x).astype(np.int64).astype(object) for x in (G, a, c))
    gc = Gi.dot(ci)
    row = np.array([float(v) / 2.0 for v in ai - gc])
    diag = float(int(s) - 2 * int(ci.dot(ai)) + int(ci.dot(gc))) / 4.0
    rk = None if rhs is None else float(int(tb) - int(ci.dot(np.asarray(rhs).astype(np.int64).astype(object)))) / 2.0
    return row, diag, rk


def exact_split(rng, M, lam=0.5):
    """M = GA + lam GL with GL a random even symmetric integer matrix."""
    GL = 2.0 * exact_sym(rng, M.shape[0], 3)
    return M - lam * GL, GL


def exact_chol(k, seed=0):
    """The Cholesky paths' exact operands: C, M = C C^T = GA + 0.5 GL, an integer y and c = M y."""
    rng = _rng(13, k, seed)
    C = np.zeros((k, k))
    for d in (1, 2, 3):
        if k > d:
            C += np.diag(small_ints(rng, k - d, 1), -d)
    C += np.diag(rng.choice([4.0, 8.0], k))
    M = C @ C.T
    GA, GL = exact_split(rng, M)
    y = small_ints(rng, k, 3)
    return {"C": C, "M": M, "GA": GA, "GL": GL, "lam": 0.5, "y": y, "c": M @ y}


def exact_border(k, seed=0):
    """The bordered paths' exact operands: p (off-diagonals of the unit bidiagonal C), M = C C^T = GA + 0.5 GL, integer c,
    the inverse in closed form (`exact_border_inverse`) and y = M^-1 c."""
    rng = _rng(14, k, seed)
    p = rng.choice([-1.0, 1.0], k)
    p[0] = 0.0                                                 # (row 0 has no sub-diagonal entry)
    M = np.diag(np.full(k, 2.0)) + np.diag(p[1:], -1) + np.diag(p[1:], 1)
    M[0, 0] = 1.0
    GA, GL = exact_split(rng, M)
    c = small_ints(rng, k)
    return {"p": p, "M": M, "GA": GA, "GL": GL, "lam": 0.5, "c": c}


def exact_border_inverse(p, k):
    """M^-1 of the leading k x k block of the bordered exact operand: q_a q_b (k - max(a, b)), q_j = prod_{l<=j} (-p_l)."""
    q = np.cumprod(np.where(np.arange(k) == 0, 1.0, -p[:k]))
    idx = np.arange(k)
    return np.outer(q, q) * (k - np.maximum.outer(idx, idx))


def exact_hess(kmax, seed=0):
    """An integer upper Hessenberg matrix, (kmax + 1) x kmax, and an integer split of every column."""
    rng = _rng(15, kmax, seed)
    H = np.triu(small_ints(rng, (kmax + 1, kmax), 3), -1)
    H[np.arange(1, kmax + 1), np.arange(kmax)] = rng.integers(1, 5, kmax).astype(np.float64)
    half = np.triu(small_ints(rng, (kmax + 1, kmax), 3))
    return {"H": H, "coef": half, "coef2": H - half, "beta0": 3.0}


# ------------------------------------------------------------------------------------------------------------ general operands
@functools.lru_cache(maxsize=None)
def blur_problem():
    """A (256 x 256 Gaussian blur of a 16 x 16 image, zero boundary), L (2-D first differences), b (noisy), in float64."""
    N = 16
    t = np.arange(N)
    T = np.exp(-((t[:, None] - t[None, :]) ** 2) / (2 * 1.5 ** 2)) * (np.abs(t[:, None] - t[None, :]) <= 3)
    T /= T[N // 2].sum()
    A = np.kron(T, T)
    D = np.eye(N)[1:] - np.eye(N)[:-1]
    L = np.vstack((np.kron(np.eye(N), D), np.kron(D, np.eye(N))))
    yy, xx = np.mgrid[0:N, 0:N]
    x_true = np.exp(-((yy - 6.0) ** 2 + (xx - 9.0) ** 2) / 8.0) + ((yy > 9) & (xx < 6))
    rng = _rng(21)
    b = A @ x_true.reshape(-1)
    b = b + 1e-2 * np.linalg.norm(b) / np.sqrt(b.size) * rng.standard_normal(b.size)
    return A, L, b


@functools.lru_cache(maxsize=None)
def golub_kahan(reorth=True, kmax=128):
    """V (n x kmax), alpha, beta (kmax each: B[j][j], B[j+1][j]), beta0 of Golub-Kahan on the blur; reorth: every new vector is
    orthogonalised twice against all earlier ones, else the plain three-term recurrence (it loses orthogonality near step 25)."""
    A, _, b = blur_problem()
    beta0 = np.linalg.norm(b)
    Us, Vs, al, be = [b / beta0], [], [], []
    for j in range(kmax):
        v = A.T @ Us[-1] - (be[-1] * Vs[-1] if j else 0.0)
        for w in (Vs + Vs if reorth else []):
            v = v - (w @ v) * w
        al.append(np.linalg.norm(v))
        Vs.append(v / al[-1])
        u = A @ Vs[-1] - al[-1] * Us[-1]
        for w in (Us + Us if reorth else []):
            u = u - (w @ u) * w
        be.append(np.linalg.norm(u))
        Us.append(u / be[-1])
    return np.array(Vs).T.copy(), np.array(al), np.array(be), float(beta0)


@functools.lru_cache(maxsize=None)
def krylov_gram(reorth=True):
    A, L, b = blur_problem()
    V = golub_kahan(reorth)[0]
    AV, LV = A @ V, L @ V
    return AV.T @ AV, LV.T @ LV, AV.T @ b


def cap_value(M):
    return M.shape[0] * np.linalg.cond(M) * U


@functools.lru_cache(maxsize=None)
def krylov_depth(lam, reorth=True):
    """The deepest basis (at most 128 vectors; 40 of the plain recurrence) at which the Krylov Gram data meet the condition cap."""
    GA, GL, _ = krylov_gram(reorth)
    k = 128 if reorth else 40
    while k > 3 and cap_value(GA[:k, :k] + lam * GL[:k, :k]) > CAP:
        k -= 1
    return k


def krylov_case(lam, reorth=True, k=None):
    GA, GL, c = krylov_gram(reorth)
    k = krylov_depth(lam, reorth) if k is None else k
    return {"GA": GA[:k, :k].copy(), "GL": GL[:k, :k].copy(), "c": c[:k].copy(), "lam": lam, "k": k}


def krylov_cases():
    """(name, case): the reorthogonalised basis at full depth and the plain recurrence cut where the cap bites, per lam."""
    return [(f"krylov-{'reorth' if r else 'plain'}-lam{lam:g}", krylov_case(lam, r)) for r in (True, False) for lam in LAMS]


def random_gram(k, seed=0):
    rng = _rng(31, k, seed)
    Wa, Wl = rng.standard_normal((k, 2 * k + 5)), rng.standard_normal((k, 3 * k))
    return {"GA": Wa @ Wa.T, "GL": Wl @ Wl.T, "c": rng.standard_normal(k), "lam": 1e-2, "k": k}


@functools.lru_cache(maxsize=None)
def arnoldi_hess(kmax=40):
    """H ((kmax + 1) x kmax) of Arnoldi on the blur from b (modified Gram-Schmidt twice), and beta0."""
    A, _, b = blur_problem()
    beta0 = np.linalg.norm(b)
    Vs, H = [b / beta0], np.zeros((kmax + 1, kmax))
    for k in range(kmax):
        w = A @ Vs[-1]
        for _ in range(2):
            for j, v in enumerate(Vs):
                hj = v @ w
                H[j, k] += hj
                w = w - hj * v
        H[k + 1, k] = np.linalg.norm(w)
        Vs.append(w / H[k + 1, k])
    return H, float(beta0)


EXACT_HESS_KMAX, EXACT_HESS_LAM = 258, 0.5                       # the integer chain of the GPU test
HESS_CHECK_K = (1, 2, 3, 16, 17, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257, 258)


def hess_split(H, seed=0):
    """coef, coef2, nrm2_sq (as k_hess_tikhonov receives a column) and the column it STORES: fl(coef + coef2) over fl(sqrt(nrm2_sq))."""
    rng = _rng(32, H.shape[1], seed)
    coef = np.triu(H * rng.random(H.shape))
    coef2 = np.triu(H) - coef
    nrm2 = np.diagonal(H, -1) ** 2
    stored = np.triu(coef + coef2)
    stored[np.arange(1, H.shape[0]), np.arange(H.shape[1])] = np.sqrt(nrm2)
    return coef, coef2, nrm2, stored


def random_hess(kmax, seed=0):
    rng = _rng(33, kmax, seed)
    H = np.triu(rng.standard_normal((kmax + 1, kmax)), -1)
    H[np.arange(1, kmax + 1), np.arange(kmax)] = np.abs(H[np.arange(1, kmax + 1), np.arange(kmax)]) + 0.5
    return H, 2.7


def hess_cases():
    """(name, H, beta0, lam, kmax): the general Hessenberg chains (mode 2 at k <= 2, mode 1 beyond; mode 0 where k <= 139)."""
    Ha, b0 = arnoldi_hess()
    out = []
    for lam in (1e-1, 10.0):
        k = Ha.shape[1]
        while k > 3 and cap_value(Ha[:k + 1, :k].T @ Ha[:k + 1, :k] + lam * np.eye(k)) > CAP:
            k -= 1
        out.append((f"arnoldi-lam{lam:g}", Ha[:k + 1, :k].copy(), b0, lam, k))
    for kmax, lam in ((17, 0.3), (66, 1e-2), (139, 1e-2), (258, 1e-2)):
        H, b0 = random_hess(kmax)
        out.append((f"random-{kmax}", H, b0, lam, kmax))
    return out


def border_cases():
    """(name, case, schedule): general operands of the bordered form; schedule = the (k_from, k) calls, in order."""
    out = []
    for name, cs in krylov_cases():
        k = cs["k"]
        out.append((name + "-rows", cs, [(0, 3)] + [(j - 1, j) for j in range(4, k + 1)]))
        out.append((name + "-from0", cs, [(0, k)]))
    for k in (1, 2, 5, 17, 66, 130, 258):
        cs = random_gram(k)
        sched = [(0, min(3, k))] + [(j - 1, j) for j in range(4, k - 2)] + ([(max(3, k - 3), k)] if k > 3 else []) + [(k, k)]
        out.append((f"random-{k}", cs, sched))
    return out


def gk_bidiag(k):
    """alpha^2, beta^2 (k each), beta0^2 of the blur's Golub-Kahan run."""
    _, al, be, b0 = golub_kahan(True)
    return al[:k] ** 2, be[:k] ** 2, b0 ** 2


def random_bidiag(k, seed=0):
    rng = _rng(34, k, seed)
    return (rng.random(k) + 0.05) ** 2, (rng.random(k) + 0.05) ** 2, 1.7 ** 2


# ------------------------------------------------------------------------------------------------------------ references and bounds
def ref_cgs(G, h, passes, rr=None):
    """c after `passes` sweeps in the reference arithmetic, its running-error bound per entry, and with rr: (rho2, its bound)."""
    G, h = np.asarray(G, dtype=np.float64), np.asarray(h, dtype=np.float64)
    k = len(h)
    Ga = np.abs(G)
    with ctx():
        Gd, hd = dec(G), dec(h)
        c, e = np.full(k, Decimal(0), dtype=object), np.zeros(k)
        for p in range(passes):
            if p == 0:
                c = hd.copy()
                continue
            t = hd - Gd.dot(c)
            cn = c + t
            e_gc = gamma(k + 1) * (Ga @ (np.abs(fl(c)) + e)) + Ga @ e
            e = e + e_gc + U * (np.abs(fl(t)) + e_gc) + U * (np.abs(fl(cn)) + e + e_gc)
            c = cn
        if rr is None:
            return c, e
        gc = Gd.dot(c)
        ch, cgc = c.dot(hd), c.dot(gc)
        v = Decimal(float(rr)) - 2 * ch + cgc
        ca, gca = np.abs(fl(c)) + e, np.abs(fl(gc))
        e_gc = gamma(k + 1) * (Ga @ ca) + Ga @ e
        d_ch = e @ np.abs(h) + gamma(k + 1) * (ca @ np.abs(h))
        d_cgc = e @ (gca + e_gc) + ca @ e_gc + gamma(k + 1) * (ca @ (gca + e_gc))
        bound = 2 * d_ch + d_cgc + 2 * U * (abs(float(rr)) + 2 * abs(float(ch)) + abs(float(cgc)) + 2 * d_ch + d_cgc)
        return c, e, v, bound


def ref_gram_row(G, a, c, s, rho2, rhs=None, tb=None):
    """((row, bound), (diagonal entry, bound), (rhs_k, bound) or None) of gram_row_from_sweep in the reference arithmetic."""
    G, a, c = (np.asarray(x, dtype=np.float64) for x in (G, a, c))
    k = len(a)
    Ga, ca = np.abs(G), np.abs(c)
    with ctx():
        Gd, ad, cd = dec(G), dec(a), dec(c)
        rho = Decimal(float(rho2)).sqrt()
        gc = Gd.dot(cd)
        row = (ad - gc) / rho
        e_gc = gamma(k + 1) * (Ga @ ca)
        rho_f = float(rho)
        row_b = (e_gc + U * (np.abs(fl(ad - gc)) + e_gc)) / rho_f + 3 * U * np.abs(fl(row))
        ca_, cgc = cd.dot(ad), cd.dot(gc)
        num = Decimal(float(s)) - 2 * ca_ + cgc
        diag = num / (rho * rho)
        d_ca = gamma(k + 1) * (ca @ np.abs(a))
        d_cgc = ca @ e_gc + gamma(k + 1) * (ca @ (np.abs(fl(gc)) + e_gc))
        d_num = 2 * d_ca + d_cgc + 2 * U * (abs(float(s)) + 2 * abs(float(ca_)) + abs(float(cgc)) + 2 * d_ca + d_cgc)
        diag_b = d_num / rho_f ** 2 + 5 * U * (abs(float(diag)) + d_num / rho_f ** 2)
        out = [(row, row_b), (diag, diag_b), None]
        if rhs is not None:
            rhs = np.asarray(rhs, dtype=np.float64)
            cr = cd.dot(dec(rhs[:k]))
            rk = (Decimal(float(tb)) - cr) / rho
            d_cr = gamma(k + 1) * (ca @ np.abs(rhs[:k]))
            rk_b = (d_cr + U * (abs(float(tb)) + abs(float(cr)) + d_cr)) / rho_f + 3 * U * abs(float(rk))
            out[2] = (rk, rk_b)
        return out


def ref_hess_row(Hs, k):
    """Row k-1 of G = H^T H from the STORED float64 columns 0 .. k-1 of H ((k+1) x >= k), in the reference arithmetic, and the
    bound of the kernel's sequential sums."""
    with ctx():
        Hd = dec(np.triu(Hs[:k + 1, :k], -1))
        g = Hd.T.dot(Hd[:, k - 1])
    terms = np.abs(Hs[:k + 1, :k]).T @ np.abs(Hs[:k + 1, k - 1])
    return g, np.array([gamma(min(i + 1, k) + 3) for i in range(k)]) * terms


class HessOp:
    """M = H^T H + lam I of the stored columns as an operator of the reference arithmetic: y -> H^T (H y) + lam y (forming M itself
    would cost k^3 reference operations); .f is M in float64, for norms, cond and the LU factorisation of the refinement."""

    def __init__(self, Hs, lam, k):
        H = np.triu(np.asarray(Hs[:k + 1, :k], dtype=np.float64), -1)
        self.H, self.lam = dec(H), Decimal(float(lam))
        self.f = H.T @ H + lam * np.eye(k)

    def dot(self, y):
        return self.H.T.dot(self.H.dot(y)) + self.lam * y


def mat_float(M):
    return M.f if isinstance(M, HessOp) else fl(M)


def ref_solve(M, c):
    """y* with M y* = c to more than 40 digits (M: a Decimal array or a HessOp, c: Decimals): refinement on a float64 LU factorisation."""
    import scipy.linalg as sla
    with ctx():
        lu = sla.lu_factor(mat_float(M))
        y = np.full(len(c), Decimal(0), dtype=object)
        nM = float(np.linalg.norm(mat_float(M), 2))
        for _ in range(60):
            r = c - M.dot(y)
            if dnorm(r) <= 1e-45 * (nM * dnorm(y) + 1e-300):
                return y
            y = y + dec(sla.lu_solve(lu, fl(r)))
    raise ArithmeticError("ref_solve: the refinement did not converge")


def gram_matrix(GA, GL, lam):
    """GA + lam GL in the reference arithmetic."""
    with ctx():
        return dec(GA) + Decimal(float(lam)) * dec(GL)


def backward_error(M, c, y):
    """||c - M y||_2 / (||M||_2 ||y||_2 + ||c||_2), the residual in the reference arithmetic (M, c Decimal; y float64)."""
    with ctx():
        r = c - M.dot(dec(y))
    return dnorm(r) / (float(np.linalg.norm(mat_float(M), 2)) * float(np.linalg.norm(y)) + dnorm(c))


def chol_bound(GA, GL, lam):
    k = GA.shape[0]
    M = GA + lam * GL
    return k * gamma(3 * k + 1) + 2 * U * np.linalg.norm(np.abs(GA) + abs(lam) * np.abs(GL)) / np.linalg.norm(M, 2)


def hess_chol_bound(Hs, lam, k):
    H = Hs[:k + 1, :k]
    terms = np.abs(H).T @ np.abs(H)
    M = H.T @ H + lam * np.eye(k)
    return k * gamma(3 * k + 1) + (gamma(k + 3) * np.linalg.norm(terms) + U * np.linalg.norm(M)) / np.linalg.norm(M, 2) + U


def hess_system(Hs, beta0, lam, k):
    """M = H^T H + lam I and c = beta0 H[0][:] in the reference arithmetic from the stored columns."""
    with ctx():
        return HessOp(Hs, lam, k), Decimal(float(beta0)) * dec(Hs[0, :k])


def diff(dev, ref):
    """device float64 values minus Decimal references, as float64."""
    with ctx():
        return fl(dec(np.atleast_1d(dev)) - np.atleast_1d(np.asarray(ref, dtype=object)))


def frac(d, bound):
    """max |d| / bound; a zero difference counts as 0 whatever the bound."""
    d, bound = np.abs(np.atleast_1d(d)), np.atleast_1d(bound) * np.ones(np.shape(np.atleast_1d(d)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(d == 0.0, 0.0, d / bound)))


def forward_ratio(y, ystar, cond):
    """||y - y*||_2 / (cond u ||y*||_2); y float64, y* Decimal."""
    with ctx():
        d = dec(y) - ystar
    return dnorm(d) / (cond * U * dnorm(ystar))


def inverse_ratio(Minv, M, cond):
    """max |Minv M - I| / (cond u), the product in np.longdouble."""
    W = np.longdouble
    R = np.asarray(Minv, dtype=W) @ np.asarray(M, dtype=W) - np.eye(M.shape[0], dtype=W)
    return float(np.max(np.abs(R))) / (cond * U)


def long_matrix(GA, GL, lam):
    W = np.longdouble
    return np.asarray(GA, dtype=W) + W(lam) * np.asarray(GL, dtype=W)


def long_hess_matrix(Hs, lam, k):
    W = np.longdouble
    H = np.asarray(Hs[:k + 1, :k], dtype=W)
    return H.T @ H + W(lam) * np.eye(k, dtype=W)


def bidiag_residual(alpha_sq, beta_sq, beta0_sq, mu, y):
    """(||T y - d||_2, bound): T = B^T B + mu^2 I, d = beta0 alpha_1 e_1 in the reference arithmetic from the squares."""
    k = len(y)
    with ctx():
        a2, b2 = dec(alpha_sq[:k]), dec(beta_sq[:k])
        al = np.array([v.sqrt() for v in a2], dtype=object)
        be = np.array([v.sqrt() for v in b2], dtype=object)
        b0, m2 = Decimal(float(beta0_sq)).sqrt(), Decimal(float(mu)) ** 2
        yd = dec(y)
        r = (a2 + b2 + m2) * yd
        if k > 1:
            off = al[1:] * be[:-1]                              # T[j][j+1] = alpha_{j+1} beta_{j+1} (B[j+1][j+1] B[j+1][j])
            r[:-1] = r[:-1] + off * yd[1:]
            r[1:] = r[1:] + off * yd[:-1]
        r[0] = r[0] - b0 * al[0]
        res = dnorm(r)
    a = float(np.sqrt(np.max(np.asarray(alpha_sq[:k]) + np.asarray(beta_sq[:k]) + mu * mu)))
    return res, BIDIAG_C * k * U * (a * a * float(np.linalg.norm(y)) + a * float(np.sqrt(beta0_sq)))


# ------------------------------------------------------------------------------------------------------------ NumPy restatements
def np_cgs(G, h, passes, rr=None):
    k = len(h)
    c = np.zeros(k)
    for p in range(passes):
        t = h.copy() if p == 0 else h - (G[:k, :k] * c[None, :]).sum(axis=1)
        c = c + t
    if rr is None:
        return c
    gc = (G[:k, :k] * c[None, :]).sum(axis=1)
    v = rr - 2.0 * np.sum(c * h) + np.sum(c * gc)
    return c, (v if v > 0.0 else 1e-300)


def np_gram_row(G, a, c, s, rho2, rhs=None, tb=None):
    k = len(a)
    rho = np.sqrt(rho2)
    gc = (G[:k, :k] * c[None, :]).sum(axis=1)
    row = (a - gc) / rho
    diag = (s - 2.0 * np.sum(c * a) + np.sum(c * gc)) / (rho * rho)
    rk = None if rhs is None else (tb - np.sum(c * rhs[:k])) / rho
    return row, diag, rk


def np_border(GA, GL, lam, c, k, k_from, Minv):
    """tikhonov_border_body: Minv (>= k x k, updated in place) bordered by rows k_from .. k-1, then y = Minv c."""
    for j in range(k_from, k):
        g = GA[j, :j + 1] + lam * GL[j, :j + 1]
        u = (Minv[:j, :j] * g[None, :j]).sum(axis=1)
        sinv = 1.0 / (g[j] - np.sum(u * g[:j]))
        Minv[:j, :j] += np.outer(u, u) * sinv
        Minv[:j, j] = -u * sinv
        Minv[j, :j] = -u * sinv
        Minv[j, j] = sinv
    return (Minv[:k, :k] * c[None, :k]).sum(axis=1)


def np_chol_solve(M, c):
    """chol_solve_lds: right-looking Cholesky of the lower triangle with the 1e-300 lift, then the two triangular solves."""
    M, z = np.array(M, dtype=np.float64), np.array(c, dtype=np.float64)
    k = len(z)
    for j in range(k):
        d = M[j, j]
        M[j, j] = np.sqrt(d if d > 0.0 else 1e-300)
        M[j + 1:, j] /= M[j, j]
        M[j + 1:, j + 1:] -= np.tril(np.outer(M[j + 1:, j], M[j + 1:, j]))
    for j in range(k):
        z[j] /= M[j, j]
        z[j + 1:] -= M[j + 1:, j] * z[j]
    for j in range(k - 1, -1, -1):
        z[j] /= M[j, j]
        z[:j] -= M[j, :j] * z[j]
    return z


def np_hess(H, G, Minv, coef, coef2, nrm2_sq, beta0, k, lam, mode):
    """k_hess_tikhonov: H ((>= k+1) x >= k, column k-1 written), G, Minv (>= k x k, updated in place); returns y."""
    hc = np.empty(k + 1)
    hc[:k] = coef[:k] + (coef2[:k] if coef2 is not None else 0.0)
    hc[k] = np.sqrt(nrm2_sq)
    H[:k + 1, k - 1] = hc
    Hk = np.triu(H[:k + 1, :k], -1)                            # (what lies below the sub-diagonal is never read)
    g = np.zeros(k)
    for r in range(k + 1):                                     # every g_i sequentially in r, as the kernel's threads do
        g[max(r - 1, 0):] += Hk[r, max(r - 1, 0):] * hc[r]
    G[:k, k - 1] = g
    G[k - 1, :k] = g
    cv = beta0 * H[0, :k]
    if mode == 0:
        return np_chol_solve(G[:k, :k] + lam * np.eye(k), cv)
    gamma_ = g[k - 1] + lam
    if mode == 2:
        if k == 1:
            Minv[0, 0] = 1.0 / gamma_
        else:
            a, b = G[0, 0] + lam, g[0]
            det = a * gamma_ - b * b
            Minv[0, 0], Minv[0, 1], Minv[1, 0], Minv[1, 1] = gamma_ / det, -b / det, -b / det, a / det
    else:
        m = k - 1
        u = (Minv[:m, :m] * g[None, :m]).sum(axis=1)
        sinv = 1.0 / (gamma_ - np.sum(u * g[:m]))
        Minv[:m, :m] += np.outer(u, u) * sinv
        Minv[:m, m] = -u * sinv
        Minv[m, :m] = -u * sinv
        Minv[m, m] = sinv
    return (Minv[:k, :k] * cv[None, :]).sum(axis=1)


def np_bidiag(alpha_sq, beta_sq, k, mu, beta0_sq, y_over_alpha=False, state=None):
    """k_bidiag_tikhonov in Python floats (no fused multiply-add).  state: a dict kept between calls = the `work` array; the resume
    rule is the kernel's (same mu, 1 <= columns done < k)."""
    al = np.sqrt(np.asarray(alpha_sq[:k], dtype=np.float64))
    st = state if state is not None else {}
    j0 = int(st["done"]) if st.get("mu") == mu and 1 <= st.get("done", 0) < k else 0
    if j0 == 0:
        st["ir"], st["th"], st["ph"] = {}, {}, {}
        abar, phibar = float(al[0]), float(np.sqrt(beta0_sq))
    else:
        abar, phibar = st["abar"] * float(al[j0]), st["phibar"]
        st["th"][j0] = st["th"][j0] * float(al[j0])
    mu2 = mu * mu
    for j in range(j0, k):
        bj2 = float(beta_sq[j])
        rhat2 = abar * abar + mu2
        r2 = rhat2 + bj2
        rhat, r, bj = np.sqrt(rhat2), np.sqrt(r2), np.sqrt(bj2)
        ir = 1.0 / r
        phihat = (abar / rhat) * phibar
        c2, s2 = rhat * ir, bj * ir
        st["ir"][j], st["ph"][j] = ir, c2 * phihat
        if j + 1 < k:
            st["th"][j + 1] = s2 * float(al[j + 1])
            abar = -c2 * float(al[j + 1])
        else:
            st["th"][j + 1] = s2
            abar = -c2
        phibar = s2 * phihat
    st.update(done=k, mu=mu, abar=abar, phibar=phibar)
    y = np.empty(k)
    yn = st["ph"][k - 1] * st["ir"][k - 1]
    y[k - 1] = yn
    for j in range(k - 2, -1, -1):
        yn = (st["ph"][j] - st["th"][j + 1] * yn) * st["ir"][j]
        y[j] = yn
    return y / al if y_over_alpha else y


def measure_border_bar():
    """The largest forward-error and inverse ratios of the NumPy restatements over border_cases() and hess_cases()."""
    worst = {}
    for name, cs, sched in border_cases():
        kmax = cs["k"]
        Minv = np.full((kmax, kmax), np.nan)
        for k_from, k in sched:
            y = np_border(cs["GA"], cs["GL"], cs["lam"], cs["c"], k, k_from, Minv)
        M = cs["GA"][:k, :k] + cs["lam"] * cs["GL"][:k, :k]
        cond = np.linalg.cond(M)
        Md = gram_matrix(cs["GA"][:k, :k], cs["GL"][:k, :k], cs["lam"])
        worst[name] = (forward_ratio(y, ref_solve(Md, dec(cs["c"][:k])), cond),
                       inverse_ratio(Minv[:k, :k], long_matrix(cs["GA"][:k, :k], cs["GL"][:k, :k], cs["lam"]), cond))
    for name, H, beta0, lam, kmax in hess_cases():
        coef, coef2, nrm2, Hs = hess_split(H)
        Hd, G, Minv = (np.full((kmax + 1, kmax + 1), np.nan) for _ in range(3))
        for k in range(1, kmax + 1):
            y = np_hess(Hd, G, Minv, coef[:, k - 1], coef2[:, k - 1], nrm2[k - 1], beta0, k, lam, 2 if k <= 2 else 1)
        Md, cd = hess_system(Hs, beta0, lam, kmax)
        cond = np.linalg.cond(mat_float(Md))
        worst["hess-" + name] = (forward_ratio(y, ref_solve(Md, cd), cond), inverse_ratio(Minv[:kmax, :kmax], long_hess_matrix(Hs, lam, kmax), cond))
    return worst
