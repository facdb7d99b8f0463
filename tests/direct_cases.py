"""Problems of the direct-solver fixtures (tests/golden/direct_*.npz), rebuilt from the sizes and seeds the fixtures hold: the
blurs from the engine's PSF formulas (trips_py_amd.problems) with scipy.ndimage, the regularisers with scipy.sparse, the tall
system from its formula.  The fixtures hold b, the reference's answers and the singular values of the reference's A, which
tests/test_direct_host.py compares with the rebuilt matrices."""
import numpy as np
import scipy.sparse as sps
from scipy.ndimage import convolve, convolve1d

from trips_py_amd.problems import gauss_psf, gauss_psf_1d


def blur1d_dense(n, sigma):
    """Deblurring1D.forward_Op_1D(sigma, n).todense(): convolve1d with the normalised Gaussian, mode 'reflect'."""
    return convolve1d(np.eye(n), gauss_psf_1d(n, sigma), axis=0, mode="reflect")


def blur2d_dense(N, dim, spread):
    """Deblurring2D.forward_Op(dim, spread, N, N).todense(): convolve on the row-major N x N image, mode 'reflect'."""
    psf, _ = gauss_psf(dim, spread)
    A = np.empty((N * N, N * N))
    e = np.zeros(N * N)
    for j in range(N * N):
        e[j] = 1.0
        A[:, j] = convolve(e.reshape(N, N), psf, mode="reflect").reshape(-1)
        e[j] = 0.0
    return A


def parallel_beam_dense(N, n_angles, n_det, shift):
    """A small parallel-beam system (n_angles * n_det rows, N^2 columns): pixel (i, j) at its centre (x, y) contributes
    max(0, 1 - |x cos t + y sin t - s|) to the ray of angle t and detector offset s (linear interpolation onto the detector).
    An odd angle count and a detector shifted off the centre leave no symmetry of the grid, so no two singular values tie."""
    c = np.arange(N) - (N - 1) / 2.0
    X, Y = np.meshgrid(c, -c)
    s = np.arange(n_det) - (n_det - 1) / 2.0 + shift
    rows = []
    for t in np.linspace(0.0, np.pi, n_angles, endpoint=False):
        proj = X * np.cos(t) + Y * np.sin(t)
        rows.append(np.maximum(0.0, 1.0 - np.abs(proj.reshape(1, -1) - s.reshape(-1, 1))))
    return np.vstack(rows)


def first_difference(n):
    """(n - 1) x n, rows e_i - e_{i+1} (operators.py gen_first_derivative_operator), scipy.sparse."""
    return (sps.identity(n) - sps.diags(np.ones(n - 1), 1))[:-1, :].tocsr()


def first_difference_2d(nx, ny):
    """[I kron D_x; D_y kron I] (operators.py:30 gen_first_derivative_operator_2D), scipy.sparse."""
    return sps.vstack((sps.kron(sps.identity(nx), first_difference(nx)), sps.kron(first_difference(ny), sps.identity(ny)))).tocsr()


def test_image(N, seed):
    rng = np.random.default_rng(seed)
    img = np.zeros((N, N))
    for _ in range(4):
        a, b = np.sort(rng.integers(0, N, 2))
        c, d = np.sort(rng.integers(0, N, 2))
        img[a:b + 1, c:d + 1] += rng.uniform(0.3, 1.0)
    yy, xx = np.mgrid[0:N, 0:N] / N
    return (img + 0.5 * np.exp(-((xx - 0.6) ** 2 + (yy - 0.4) ** 2) / 0.02)).reshape(-1, 1)


def noise(shape, level, norm_b, seed):
    e = np.random.default_rng(seed).standard_normal(shape)
    return e * (level * norm_b / np.linalg.norm(e))


def build(g):
    """A of a fixture, from its 'kind' and parameters."""
    kind = str(g["kind"])
    if kind == "blur1d":
        return blur1d_dense(int(g["n"]), float(g["sigma"]))
    if kind == "blur2d":
        return blur2d_dense(int(g["N"]), tuple(int(v) for v in g["dim"]), tuple(float(v) for v in g["spread"]))
    if kind == "parallel_beam":
        return parallel_beam_dense(int(g["N"]), int(g["n_angles"]), int(g["n_det"]), float(g["det_shift"]))
    raise ValueError(kind)


def regulariser(g):
    """The L the fixture's 'tikh_L' runs used: the demo's (n-1) x n difference, or the 2-D one for a blur2d case."""
    return first_difference(int(g["n"])) if str(g["kind"]) == "blur1d" else first_difference_2d(int(g["N"]), int(g["N"]))
