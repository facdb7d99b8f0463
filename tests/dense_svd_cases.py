"""Matrices and checks for the tests of the dense float64 Jacobi SVD (csrc/dense_svd.hip) and of trk_dense_gemv_f64.  NumPy alone:
tests/test_dense_svd_cases_host.py runs every check on LAPACK's factors, tests/test_gpu_dense_svd.py on the device's.

Factors are passed as np.linalg.svd(full_matrices=False) returns them: U (m x k), S (k,), Vh (k x n), k = min(m, n).

The contract (`check_contract`).  One-sided Jacobi works on G = A V and stops after a sweep that found, for every column pair,
    |g_i . g_j| <= tol ||g_i|| ||g_j||   or   |g_i . g_j| <= tol max(||g_i||, ||g_j||)^2,      tol = max(m, 64) eps,
of which the second is the weaker.  That sweep rotated nothing, so the test held on the returned G, up to the rounding of the
kernel's chunked Gram sums (at most gamma_m ||g_i|| ||g_j|| <= tol max^2) and of forming g_j = S_j U_j again from the
returned factors (less than that again).  Hence, for every pair i != j of the returned factors,
    |g_i . g_j| <= 3 tol max(||g_i||, ||g_j||)^2,
which for the unit columns reads |u_i . u_j| <= 3 tol sigma_big / sigma_small: U is orthonormal to tol times the ratio of the
two singular values, not to eps.  `jacobi_model` is that iteration in scalar NumPy; it reaches 0.97 of tol sigma_big /
sigma_small on matrices of every grading (the host test prints it), so the bound has no slack to give away.
A wide matrix runs on its transpose: the columns that the iteration orthogonalises are then the rows of S Vh."""
import numpy as np

EPS = np.finfo(np.float64).eps
LD = np.longdouble

# column blocks of 16 (block count padded to an even number), Gram row chunks of 128, apply workgroups of 256 rows
EDGE_N = (15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65)
EDGE_M = (127, 128, 129, 255, 256, 257)
EDGE_SHAPES = [(m, n) for n in EDGE_N for m in (n,) + EDGE_M]
WIDE_SHAPES = [(16, 127), (33, 128), (48, 129), (49, 257), (65, 256)]          # transposes of five of the above


# ------------------------------------------------------------------------------------------------------------ builders
def gaussian(m, n, seed=None):
    return np.random.default_rng(m * 1000 + n if seed is None else seed).standard_normal((m, n))


def graded(m, n, seed, smallest):
    """Q1 diag(geomspace(1, smallest, n)) Q2^T with Q1 (m x n) and Q2 (n x n) orthonormal: rank n, condition number 1 / smallest.
    For m == n this is `_graded` of tests/test_gpu_direct.py, entry for entry."""
    rng = np.random.default_rng(seed)
    Q1 = np.linalg.qr(rng.standard_normal((m, n)))[0]
    Q2 = np.linalg.qr(rng.standard_normal((n, n)))[0]
    return (Q1 * np.geomspace(1.0, smallest, n)) @ Q2.T


def scaled(A, k):
    """2^k A, exactly."""
    return np.ldexp(A, k)


def zero(m=40, n=33):
    return np.zeros((m, n))


def rank_one(m=64, n=48, seed=11):
    rng = np.random.default_rng(seed)
    return np.outer(rng.standard_normal(m), rng.standard_normal(n))


DIAG_SHAPE = (50, 33)


def diag_entries():
    """33 values, unsorted: one negative, one zero, one repeated; the others distinct."""
    d = ((np.arange(33) * 7) % 33 + 1) * 0.37
    d[4] = -d[4]
    d[10] = 0.0
    d[20] = d[7]
    return d


def diag_top():
    A = np.zeros(DIAG_SHAPE)
    A[:33, :33] = np.diag(diag_entries())
    return A


REPEATED_SIGMA = np.array([3.0, 3.0, 3.0, 2.0, 2.0] + [1.0] * 43)


def repeated(m=64, n=48, seed=12):
    """Q1 diag(3, 3, 3, 2, 2, 1, ..., 1) Q2^T: every singular value is a repeated one, so no vector is determined."""
    rng = np.random.default_rng(seed)
    Q1 = np.linalg.qr(rng.standard_normal((m, n)))[0]
    Q2 = np.linalg.qr(rng.standard_normal((n, n)))[0]
    return (Q1 * REPEATED_SIGMA) @ Q2.T


def blur576():
    import direct_cases as dc
    return dc.blur2d_dense(24, (9, 9), (3.0, 3.0))


# name -> (builder, whether cond <= 1e6 (U^T U - I is then bounded too), whether the vectors are compared with LAPACK's)
NAMED = {
    "gauss257x100": (lambda: gaussian(257, 100), True, True),
    "gauss100x257": (lambda: gaussian(100, 257), True, True),
    "graded300_1e-6": (lambda: graded(300, 300, 9, 1e-6), True, True),
    "graded300_1e-10": (lambda: graded(300, 300, 9, 1e-10), False, True),
    "graded300_1e-14": (lambda: graded(300, 300, 9, 1e-14), False, True),
    "blur576": (blur576, False, True),
    "rank_one": (rank_one, False, False),
    "repeated": (repeated, True, False),
    "zero": (zero, False, False),
    "diag_top": (diag_top, False, False),
}
SCALE_CASES = ("gauss257x100", "graded300_1e-10")
_BUILT = {}


def named(name):
    """The matrix of a named case, built once; callers do not write to it."""
    if name not in _BUILT:
        _BUILT[name] = NAMED[name][0]()
        _BUILT[name].setflags(write=False)
    return _BUILT[name]


# -------------------------------------------------------------------------------------------------------------- checks
def pow2_exponent(A):
    """e with max |A| in [2^e, 2^(e + 1)); 0 for the zero matrix."""
    amax = float(np.max(np.abs(A))) if A.size else 0.0
    return int(np.frexp(amax)[1]) - 1 if amax > 0 else 0


def unit_scale(A, S):
    """(2^-e A, 2^-e S) with e = pow2_exponent(A): exact, and the checks below, all relative, then square nothing that could leave
    the float64 range (np.linalg.norm of a matrix near 2^600 is Inf, and Inf <= Inf would pass)."""
    e = pow2_exponent(A)
    return np.ldexp(A, -e), np.ldexp(S, -e)


def lapack_factors(A):
    """np.linalg.svd's thin factors in this project's convention: where a singular value is exactly zero, the vector on the side
    that the iteration normalises (U for a tall matrix, Vh for a wide one) is zero."""
    U, S, Vh = np.linalg.svd(A, full_matrices=False)
    if A.shape[0] >= A.shape[1]:
        U = U * (S > 0)
    else:
        Vh = Vh * (S > 0).reshape(-1, 1)
    return U, S, Vh


def check_reconstruction(A, U, S, Vh):
    """||A - U S Vh||_F <= 1e-13 sqrt(n) ||A||_F (tests/test_gpu_direct.py); returns measured / bound."""
    A, S = unit_scale(A, S)
    bound = 1e-13 * np.sqrt(A.shape[1]) * np.linalg.norm(A)
    err = np.linalg.norm(A - (U * S) @ Vh)
    assert err <= bound, (err, bound)
    return err / bound if bound > 0 else 0.0


def check_rotation_orthogonal(A, U, Vh):
    """The accumulated rotation (V for a tall matrix, U for a wide one) is orthogonal to 1e-13 sqrt(n), whatever the sweep count."""
    R = Vh.T if A.shape[0] >= A.shape[1] else U
    k = R.shape[1]
    bound = 1e-13 * np.sqrt(max(A.shape[1], 1))
    err = np.max(np.abs(R.T @ R - np.eye(k)))
    assert err <= bound, (err, bound)
    return err / bound


def check_against_lapack(A, U, S, Vh, vectors=True):
    """`_check_against_lapack` of tests/test_gpu_direct.py on given factors, every bound relative to sigma_1."""
    m, n = A.shape
    k = min(m, n)
    assert U.shape == (m, k) and S.shape == (k,) and Vh.shape == (k, n)
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(S)) and np.all(np.isfinite(Vh))
    Sn = unit_scale(A, S)[1]
    if vectors:
        _, Sl, Vhl = np.linalg.svd(A, full_matrices=False)
    else:
        Sl = np.linalg.svd(A, compute_uv=False)
    Sl = np.ldexp(Sl, -pow2_exponent(A))
    assert np.all(np.diff(S) <= 0) and np.all(S >= 0)
    es = np.max(np.abs(Sn - Sl))
    assert es <= 8 * max(m, n) * EPS * Sl[0], (es, 8 * max(m, n) * EPS * Sl[0])
    check_reconstruction(A, U, S, Vh)
    V = Vh.T
    assert np.max(np.abs(V.T @ V - np.eye(k))) <= 1e-13 * np.sqrt(n)
    if vectors and k > 1:
        gap = np.full(k, np.inf)
        gap[1:] = np.minimum(gap[1:], Sl[:-1] - Sl[1:])
        gap[:-1] = np.minimum(gap[:-1], Sl[:-1] - Sl[1:])
        sel = gap >= 1e-6 * Sl[0]
        dots = np.abs(np.sum(Vh[sel] * Vhl[sel], axis=1))
        assert np.all(dots >= 1 - 1e-9), dots.min()


def iteration_side(A, U, Vh):
    """(the unit columns that the iteration orthogonalises, its row count): U and m for a tall matrix, Vh^T and n for a wide one."""
    m, n = A.shape
    return (U, m) if m >= n else (Vh.T, n)


def check_contract(A, U, S, Vh, bound_utu):
    """The contract of the module docstring on the returned factors, Gram matrices in np.longdouble:
        |g_i . g_j| <= 3 tol max(||g_i||, ||g_j||)^2 for i != j, g_j = S_j u_j;
        | ||u_j||^2 - 1 | <= tol where S_j > 0, and u_j exactly zero where S_j = 0;
        with bound_utu (cases of cond <= 1e6 only, asserted): max |U^T U - I| <= 3 tol cond, cond = sigma_1 / sigma_k by LAPACK.
    Returns the three measured / bound ratios (the last None without bound_utu)."""
    Q, rows = iteration_side(A, U, Vh)
    tol = max(rows, 64) * EPS
    Sn = unit_scale(A, S)[1]
    k = S.size
    Ql = Q.astype(LD)
    gram_u = Ql.T @ Ql
    live = S > 0
    assert not np.any(Q[:, ~live]), "a singular value is 0 and its vector is not"
    r_diag = float(np.max(np.abs(np.diag(gram_u)[live] - 1), initial=0.0) / tol)
    assert r_diag <= 1.0, r_diag
    G = Ql * Sn.astype(LD)
    gram = G.T @ G
    n2 = np.diag(gram)
    big = np.maximum.outer(n2, n2)
    off = np.abs(gram - np.diag(n2))
    assert not np.any(off[big == 0])
    r_g = float(np.max(np.where(big > 0, off / np.where(big > 0, 3 * tol * big, 1), 0), initial=0.0))
    assert r_g <= 1.0, r_g
    r_utu = None
    if bound_utu:
        Sl = np.linalg.svd(A, compute_uv=False)
        cond = Sl[0] / Sl[-1]
        assert 3 * tol * cond < 1e-6, cond                      # cond <= 1e6 to rounding: the bound says something
        r_utu = float(np.max(np.abs(gram_u - np.eye(k))) / (3 * tol * cond))
        assert r_utu <= 1.0, r_utu
    return r_g, r_diag, r_utu


def check_diag_top(U, S, Vh):
    """The 50 x 33 matrix whose top block is diag(d): nothing rotates, so S is sorted |d| exactly (sqrt(fl(d^2)) == |d| in binary
    floating point), V exactly a permutation matrix, and the sign of a negative d sits in U."""
    d = diag_entries()
    assert np.array_equal(S, np.sort(np.abs(d))[::-1])
    assert np.all((Vh == 0) | (Vh == 1)) and np.array_equal(Vh @ Vh.T, np.eye(33)) and np.array_equal(Vh.T @ Vh, np.eye(33))
    col = np.argmax(Vh, axis=1)                                   # S[j] is |d[col[j]]|
    assert np.array_equal(np.abs(d[col]), S)
    for j in range(33):
        want = np.zeros(50)
        if S[j] > 0:
            want[col[j]] = np.sign(d[col[j]])
        assert np.max(np.abs(U[:, j] - want)) <= 2 * EPS and np.count_nonzero(U[:, j]) == (S[j] > 0)
        assert S[j] == 0 or np.sign(U[col[j], j]) == np.sign(d[col[j]])
    assert np.sum(U < 0) == 1


# ------------------------------------------------------------------------------------------- the scalar model of the kernel
def jacobi_model(A, tol, max_sweeps=60):
    """Cyclic one-sided Jacobi in scalar float64 with the acceptance rule of k_svd_jacobi, the columns ordered by decreasing norm
    before every sweep -> (G = A V with the columns in their last order, sweeps).  The last sweep rotates nothing."""
    G = np.array(A, dtype=np.float64)
    n = G.shape[1]
    for sweep in range(1, max_sweeps + 1):
        G = G[:, np.argsort(-np.linalg.norm(G, axis=0), kind="stable")]
        rotated = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                gi, gj = G[:, i].copy(), G[:, j].copy()
                aii, ajj, aij = gi @ gi, gj @ gj, gi @ gj
                if abs(aij) > tol * (np.sqrt(aii) * np.sqrt(ajj)) and abs(aij) > tol * max(aii, ajj):
                    tau = (ajj - aii) / (2.0 * aij)
                    t = (1.0 if tau >= 0 else -1.0) / (abs(tau) + np.sqrt(1.0 + tau * tau))
                    c = 1.0 / np.sqrt(1.0 + t * t)
                    G[:, i], G[:, j] = c * gi - t * c * gj, t * c * gi + c * gj
                    rotated = True
        if not rotated:
            return G, sweep
    raise AssertionError(f"the model did not converge in {max_sweeps} sweeps")


def model_ratio(A):
    """max over column pairs of |u_i . u_j| / (tol sigma_big / sigma_small) for the model's factors, and its sweep count."""
    m = A.shape[0]
    tol = max(m, 64) * EPS
    G, sweeps = jacobi_model(A, tol)
    Gl = G.astype(LD)
    s = np.sqrt(np.sum(Gl * Gl, axis=0))
    Ul = Gl / s
    gram = np.abs(Ul.T @ Ul - np.eye(G.shape[1]))
    ratio = np.maximum.outer(s, s) / np.minimum.outer(s, s)
    return float(np.max(gram / (tol * ratio))), sweeps


# --------------------------------------------------------------------------------------------------- trk_dense_gemv_f64
GEMV_SHAPES = [(1, 1), (255, 3), (256, 17), (257, 40), (1000, 300), (3, 700)]
GEMV_COEFFS = [(1.0, 0.0), (-0.5, 2.0), (0.0, 1.0)]


def gemv_operands(m, n, trans, seed):
    """(A (m x n), x, d, y0) for y = beta y0 + alpha op(A) (d .* x)."""
    rng = np.random.default_rng(seed)
    nin, nout = (m, n) if trans else (n, m)
    return rng.standard_normal((m, n)), rng.standard_normal(nin), rng.uniform(0.5, 2.0, nin) * rng.choice([-1.0, 1.0], nin), \
        rng.standard_normal(nout)


def gemv_reference(trans, A, x, d, alpha, beta, y0):
    """(the product in np.longdouble, the entry-wise bound (L + 3) eps |alpha| sum |A| |d| |x| + 2 eps |beta y0|): L the length of
    the sums; the worst case of the arithmetic in any summation order.  beta = 0 does not read y0."""
    Al = (A.T if trans else A).astype(LD)
    v = x.astype(LD) * (1 if d is None else d.astype(LD))
    L = Al.shape[1]
    base = np.zeros(Al.shape[0], dtype=LD) if beta == 0 else LD(beta) * y0.astype(LD)
    ref = base + LD(alpha) * (Al @ v)
    bound = (L + 3) * EPS * abs(alpha) * (np.abs(Al) @ np.abs(v)) + 2 * EPS * np.abs(base)
    return ref, bound
