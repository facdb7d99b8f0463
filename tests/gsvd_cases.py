"""Matrix pairs (A, L) of the GSVD tests and `gsvd_numpy`, the float64 NumPy restatement of the device algorithm's
stages (docs/kernels/dense_svd.md, "GSVD") that tests/test_gpu_gsvd.py compares the device against and tests/test_gsvd_host.py
compares with the reference's answers (tests/golden/direct_tgsvd_deblur1d.npz, tools/make_gsvd_goldens.py).

A case states what it is built to exercise: `J`, the number of columns with c > 1/sqrt(2) (the device's third stage runs on
them), and `zero_s`, the number of columns with s <= n eps (their V columns are zero by convention)."""
import functools

import numpy as np

import direct_cases as dc
from conftest import load_golden

EPS = np.finfo(np.float64).eps


def gsvd_numpy(A, L):
    """M = [A; L] = Q diag(sigma) Vm^T (LAPACK), Q1 = Q[:m] = U diag(c) W^T (LAPACK), c ascending; on the columns J with
    c > 1/sqrt(2), W_J <- W_J Z with Q2 W_J = V diag(s) Z^T (LAPACK): there the c lie within (1 - c) of one another and LAPACK's
    W_J carries angles of order eps / gap(c), while the s are apart (with L = 0.01 x Gaussian, 1.6e-9 against 1.6e-13 in X).
    Returns a dict with c, s (n), G = Q1 W = U diag(c) (m x n), H = Q2 W = V diag(s) (p x n), X = Vm diag(sigma) W,
    Y = X^-T = Vm diag(1 / sigma) W (n x n), so that A = G X^T and L = H X^T, and sigma (descending)."""
    A, L = np.asarray(A, dtype=np.float64), np.asarray(L, dtype=np.float64)
    m = A.shape[0]
    Q, sig, VmT = np.linalg.svd(np.vstack((A, L)), full_matrices=False)
    W = np.linalg.svd(Q[:m], full_matrices=False)[2].T[:, ::-1]
    J = np.linalg.norm(Q[:m] @ W, axis=0) > np.sqrt(0.5)
    if J.any():
        W[:, J] = W[:, J] @ np.linalg.svd(Q[m:] @ W[:, J], full_matrices=False)[2].T
    W = W[:, np.argsort(np.linalg.norm(Q[:m] @ W, axis=0), kind="stable")]
    G, H = Q[:m] @ W, Q[m:] @ W
    return dict(c=np.linalg.norm(G, axis=0), s=np.linalg.norm(H, axis=0), G=G, H=H, X=(VmT.T * sig) @ W, Y=(VmT.T / sig) @ W,
                sigma=sig)


def tgsvd_numpy(f, b, k):
    """The reference's filter on gsvd_numpy's factors: x = Y (keep .* (G^T b)), keep = 1 except keep[:k] = 0."""
    keep = np.ones(f["c"].size)
    keep[:k] = 0
    return f["Y"] @ (keep * (f["G"].T @ np.asarray(b, dtype=np.float64).reshape(-1)))


def residuals(A, L, G, H, X):
    """(||A - G X^T||_F, ||L - H X^T||_F) / ||[A; L]||_F"""
    nM = np.sqrt(np.linalg.norm(A) ** 2 + np.linalg.norm(L) ** 2)
    return np.linalg.norm(A - G @ X.T) / nM, np.linalg.norm(L - H @ X.T) / nM


def _gauss(m, p, n):
    rng = np.random.default_rng(10000 * m + 100 * p + n)
    return rng.standard_normal((m, n)), rng.standard_normal((p, n))


def _from_c(m, p, c, seed):
    """A = U1 diag(c) X^T, L = U2 diag(sqrt(1 - c^2)) X^T with orthonormal U1, U2 and a well-conditioned X."""
    rng = np.random.default_rng(seed)
    n = c.size
    U1 = np.linalg.qr(rng.standard_normal((m, n)))[0]
    U2 = np.linalg.qr(rng.standard_normal((p, n)))[0]
    X = np.linalg.qr(rng.standard_normal((n, n)))[0] * rng.uniform(1.0, 3.0, n)
    return (U1 * c) @ X.T, (U2 * np.sqrt(1.0 - c * c)) @ X.T


def deblur1d_pair():
    """The 1-D deblurring demo's pair: the n = 200 Gauss (sigma 30) blur and the (n - 1) x n first difference with a zero row."""
    n = 200
    return dc.blur1d_dense(n, 30.0), np.vstack((dc.first_difference(n).toarray(), np.zeros((1, n))))


def blur2d_pair():
    """The 24^2 blur of tests/golden/direct_blur2d.npz and its 1104 x 576 difference operator (a null vector: the constants)."""
    g = load_golden("direct_blur2d")
    N = int(g["N"])
    return dc.build(g), dc.first_difference_2d(N, N).toarray()


# name -> (builder, J, zero_s)
CASES = {
    "g1x1x1": (lambda: _gauss(1, 1, 1), 0, 0),
    "g2x2x2": (lambda: _gauss(2, 2, 2), 0, 0),
    "g17x17x17": (lambda: _gauss(17, 17, 17), 10, 0),
    "g40x40x17": (lambda: _gauss(40, 40, 17), 10, 0),
    "g257x300x100": (lambda: _gauss(257, 300, 100), 44, 0),
    "g300x257x100": (lambda: _gauss(300, 257, 100), 55, 0),
    "J_empty": (lambda: (0.01 * _gauss(40, 40, 17)[0], _gauss(40, 40, 17)[1]), 0, 0),
    "J_all": (lambda: (_gauss(40, 40, 17)[0], 0.01 * _gauss(40, 40, 17)[1]), 17, 0),
    "J_one": (lambda: _from_c(40, 33, np.append(np.linspace(0.05, 0.65, 16), 0.9), 3), 1, 0),
    "deblur1d": (deblur1d_pair, 5, 1),
    "blur2d": (blur2d_pair, 17, 1),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(A, L, factors of gsvd_numpy, cond([A; L])) — built once and shared; treat as read-only."""
    A, L = CASES[name][0]()
    f = gsvd_numpy(A, L)
    for v in (A, L, *f.values()):
        v.setflags(write=False)
    return A, L, f, float(f["sigma"][0] / f["sigma"][-1])


def separated(c, gap=1e-6):
    """Columns whose c is at least `gap` away from both neighbours (c sorted): there X's column is defined up to sign."""
    d = np.diff(c)
    g = np.full(c.size, np.inf)
    g[1:] = np.minimum(g[1:], d)
    g[:-1] = np.minimum(g[:-1], d)
    return g >= gap
