"""Problem builders: the operator constructors of the reference's test problems plus seeded synthetic data
(the reference's own generators are unseeded: Deblurring2D.py:143, Tomography.py:206).

  gauss_psf(dim, spread)              <- Deblurring2D.Gauss            trips/test_problems/Deblurring2D.py:48-64
  gauss_psf_1d(n, sigma)              <- Deblurring1D.Gauss1D          trips/test_problems/Deblurring1D.py:63-69
  Deblurring1D().Defocus1D(n, r)      <- Deblurring1D.Defocus1D        trips/test_problems/Deblurring1D.py:70-82
  defocus_psf(dim, radius)            out-of-focus blur: a uniform disc (an extension; on gauss_psf's grid)
  motion_psf(dim, length, angle_deg)  linear motion blur: a line segment, bilinear deposits (an extension)
  Deblurring2D().forward_Op(...)      <- Deblurring2D.forward_Op       :66-73   (returns a trips_py_amd Blur2D)
  synthetic_image / add_noise         seeded versions of the data recipe (:141-146): what bench.py / smoke() / the tests use

In scope here: the PSF and the operator constructors.  The demos' host-side data preparation — gen_xtrue,
gen_data, the classes' unseeded add_noise (OUT OF SCOPE) — is not part of the package: tools/demo_helpers.py
holds it as mixins (`demo_classes()`), for a notebook that wants the reference's whole class surface.
"""
import numpy as np

from .operators import Blur1D, Blur2D, BlockDiagOp, FanBeam2D, Radon2DParallel, normalize_boundary


def gauss_psf(dim, spread):
    """PSF = exp(-(X^2/s1^2 + Y^2/s2^2)/2) on X = arange(-fix(n/2), ceil(n/2)), normalised; centre = argmax."""
    m, n = int(dim[0]), int(dim[1])
    if isinstance(spread, (int, float)):
        s1 = s2 = float(spread)
    else:
        s1, s2 = float(spread[0]), float(spread[1])
    xs = np.arange(-np.fix(n / 2), np.ceil(n / 2))
    ys = np.arange(-np.fix(m / 2), np.ceil(m / 2))
    X, Y = np.meshgrid(xs, ys)
    psf = np.exp(-0.5 * ((X ** 2) / (s1 ** 2) + (Y ** 2) / (s2 ** 2)))
    psf /= psf.sum()
    mm, nn = np.where(psf == psf.max())
    return psf, np.array([mm[0], nn[0]]).astype(int)


def gauss_psf_1d(n, sigma):
    x = np.arange(-np.fix(n / 2), np.ceil(n / 2))
    psf = np.exp(-0.5 * ((x ** 2) / (sigma ** 2)))
    return psf / psf.sum()


def defocus_psf(dim, radius):
    """Out-of-focus blur: 1 where X^2 + Y^2 <= radius^2 on gauss_psf's grid (arange(-fix(k/2), ceil(k/2)) per axis), 0 elsewhere,
    normalised to sum 1.  Returns (psf, center) with center = [fix(m/2), fix(n/2)], the grid's origin."""
    m, n = int(dim[0]), int(dim[1])
    radius = float(radius)
    if radius < 0:
        raise ValueError(f"defocus_psf: radius must be >= 0, got {radius!r}")
    xs = np.arange(-np.fix(n / 2), np.ceil(n / 2))
    ys = np.arange(-np.fix(m / 2), np.ceil(m / 2))
    X, Y = np.meshgrid(xs, ys)
    psf = (X ** 2 + Y ** 2 <= radius ** 2).astype(np.float64)
    psf /= psf.sum()
    return psf, np.array([int(np.fix(m / 2)), int(np.fix(n / 2))])


def motion_psf(dim, length, angle_deg):
    """Linear motion blur: a segment of `length` pixels through the centre [fix(m/2), fix(n/2)], at `angle_deg` counter-clockwise
    from the column axis (rows go down).  S = max(2, 4 ceil(length) + 1) points t uniform on [-length/2, length/2] sit at
    (c0 - t sin(a), c1 + t cos(a)); each deposits its bilinear weights on its four neighbours; float64 throughout, normalised to
    sum 1.  A point with a neighbour outside the array raises ValueError (the PSF array is too small for the segment).
    Returns (psf, center)."""
    m, n = int(dim[0]), int(dim[1])
    length = float(length)
    if length < 0:
        raise ValueError(f"motion_psf: length must be >= 0, got {length!r}")
    c0, c1 = int(np.fix(m / 2)), int(np.fix(n / 2))
    a = np.deg2rad(float(angle_deg))
    t = np.linspace(-length / 2, length / 2, max(2, 4 * int(np.ceil(length)) + 1))
    rows, cols = c0 - t * np.sin(a), c1 + t * np.cos(a)
    i0, j0 = np.floor(rows).astype(int), np.floor(cols).astype(int)
    fi, fj = rows - i0, cols - j0
    psf = np.zeros((m, n), dtype=np.float64)
    for di, dj, wgt in ((0, 0, (1 - fi) * (1 - fj)), (0, 1, (1 - fi) * fj), (1, 0, fi * (1 - fj)), (1, 1, fi * fj)):
        ii, jj = i0 + di, j0 + dj
        if ii.min() < 0 or jj.min() < 0 or ii.max() >= m or jj.max() >= n:
            raise ValueError(f"motion_psf: a {length} pixel segment at {angle_deg} degrees does not fit a {m}x{n} PSF")
        np.add.at(psf, (ii, jj), wgt)
    psf /= psf.sum()
    return psf, np.array([c0, c1])


class Deblurring2D:
    """Operator-constructor subset of trips.test_problems.Deblurring2D (same method names), with two PSFs beside the reference's
    Gaussian: Defocus and Motion."""

    def __init__(self, **kwargs):
        self.nx = self.ny = None
        self.CommitCrime = kwargs.get("CommitCrime", False)

    def Gauss(self, PSFdim, PSFspread):
        self.dim, self.spread = PSFdim, PSFspread
        return gauss_psf(PSFdim, PSFspread)

    def Defocus(self, PSFdim, radius):
        self.dim, self.spread = PSFdim, radius
        return defocus_psf(PSFdim, radius)

    def Motion(self, PSFdim, length, angle):
        self.dim, self.spread = PSFdim, (length, angle)
        return motion_psf(PSFdim, length, angle)

    def forward_Op(self, dim, spread, nx, ny, engine=None, boundary_condition="reflect", psf_type="gauss"):
        """boundary_condition (an extension: the reference's 2-D blur is always 'reflect'): any mode Blur2D accepts.
        psf_type (an extension): 'gauss' (the reference's PSF, the default), 'defocus' (spread is the radius), 'motion' (spread
        is (length, angle in degrees)), or a 2-D array taken as the PSF itself (dim and spread are then not used)."""
        self.nx, self.ny = nx, ny
        if isinstance(psf_type, str):
            if psf_type == "gauss":
                psf, _ = self.Gauss(dim, spread)
            elif psf_type == "defocus":
                psf, _ = self.Defocus(dim, spread)
            elif psf_type == "motion":
                psf, _ = self.Motion(dim, spread[0], spread[1])
            else:
                raise ValueError(f"forward_Op: psf_type must be 'gauss', 'defocus', 'motion' or a 2-D array, got {psf_type!r}")
        else:
            psf = np.asarray(psf_type, dtype=np.float64)
            if psf.ndim != 2:
                raise ValueError("forward_Op: a PSF given as an array must be 2-D")
        return Blur2D(psf, nx, ny, engine=engine, boundary=boundary_condition)


class Deblurring1D:
    """trips.test_problems.Deblurring1D: the operator constructor on the engine (Deblurring1D.py:63-69, 93-102) — BASELINE config C1
    (n = 256, sigma = 3)."""

    def __init__(self, **kwargs):
        self.grid_points = self.ny = self.parameter = self.boundary_condition = None
        self.CommitCrime = kwargs.get("CommitCrime", False)

    def Gauss1D(self, grid_points, parameter):
        self.grid_points = grid_points
        psf = gauss_psf_1d(grid_points, parameter)
        return psf, int(np.where(psf == psf.max())[0][0])

    def Defocus1D(self, grid_points, parameter):
        """The reference's 1-D out-of-focus PSF (Deblurring1D.py:70-82), quirk included: the array RETURNED is the un-normalised
        one, 1 / (pi parameter^2) where (i + 1 - center)^2 <= parameter^2; the normalised PSF is stored in self.PSF."""
        self.grid_points = grid_points
        center = np.intp(np.fix(int(grid_points / 2)))
        if parameter == 0:
            PSF = np.zeros(grid_points)
            PSF[center] = 1
            self.PSF = PSF
        else:
            PSF = np.ones(grid_points) / (np.pi * parameter ** 2)
            PSF[(np.arange(1, grid_points + 1) - center) ** 2 > parameter ** 2] = 0
            self.PSF = PSF / PSF.sum()
        return PSF, center

    def forward_Op_1D(self, parameter, nx, boundary_condition="reflect", engine=None):
        """boundary_condition: the scipy.ndimage mode of the forward convolve1d and of the flipped-PSF "transpose" (:56-62) —
        'reflect', 'constant' (0), 'nearest', 'mirror', 'wrap' or a 'grid-*' alias of them; stored as given, as the reference
        does.  The "transpose" is not the exact adjoint for 'nearest' / 'mirror' (nor, in any mode, for an even n)."""
        normalize_boundary(boundary_condition)
        self.parameter, self.boundary_condition = parameter, boundary_condition
        self.PSF, self.center = self.Gauss1D(nx, parameter)
        return Blur1D(self.PSF, nx, engine=engine, boundary=boundary_condition)


class Tomography:
    """Operator-constructor subset of trips.test_problems.Tomography (same method name and return convention)."""

    def __init__(self, **kwargs):
        self.nx = self.ny = None
        self.CommitCrime = kwargs.get("CommitCrime", False)

    def forward_Op(self, nx, ny, views, engine=None):
        """Fan-beam operator of Tomography.py:78-88.  With CommitCrime=False the reference also returns a second operator
        whose angles are shifted by 1e-8 (:61-65); the same triple / pair is returned here."""
        self.nx, self.ny, self.q = nx, ny, views
        self.p = int(np.sqrt(2) * nx)
        A = FanBeam2D(nx, views=views, engine=engine)
        if not self.CommitCrime:
            A_mis = FanBeam2D(nx, angles=A.angles + 1e-8, engine=engine)
            return A, A, A_mis
        return A, A


def parallel_beam_frames(N, angle_sets, engine=None):
    """One Radon2DParallel per time frame (io.py:391-420), combined frame-major with BlockDiagOp."""
    ops = [Radon2DParallel(N, ang, engine=engine) for ang in angle_sets]
    return BlockDiagOp(ops, engine=engine), ops


# ---------------------------------------------------------------------------- seeded synthetic data
def synthetic_image(N, seed=0):
    """N x N float32 test image: piecewise-constant rectangles + 0.1*U(0,1) texture."""
    rng = np.random.default_rng(seed)
    img = np.zeros((N, N), dtype=np.float64)
    for _ in range(8):
        i0, j0 = rng.integers(0, max(1, N - N // 8), size=2)
        h, w = rng.integers(max(1, N // 16), max(2, N // 3), size=2)
        img[i0:i0 + h, j0:j0 + w] += rng.uniform(0.2, 1.0)
    img += 0.1 * rng.random((N, N))
    return img


def add_noise(b_true, level, seed=1):
    """b = b_true + e, e ~ N(0,1) scaled to ||e|| = level*||b_true||; returns (b, delta=||e||)."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(b_true.shape)
    e *= level * np.linalg.norm(b_true) / np.linalg.norm(e)
    return b_true + e, float(np.linalg.norm(e))


def poisson_noise(b_true, peak=None, background=0.0, seed=1):
    """Seeded Poisson counts (float64, the shape of b_true) with mean peak * b_true / max(b_true) + background; peak=None: the mean is
    b_true + background.  b_true and background must be >= 0.  The data of solvers.MLEM and of PDHG(..., data='kl')."""
    mean = np.asarray(b_true, dtype=np.float64)
    if peak is not None:
        mean = float(peak) * mean / mean.max()
    mean = mean + np.asarray(background, dtype=np.float64)
    if not np.all(np.isfinite(mean)) or np.any(mean < 0):
        raise ValueError("poisson_noise: the mean b_true + background must be finite and >= 0")
    return np.random.default_rng(seed).poisson(mean).astype(np.float64)
