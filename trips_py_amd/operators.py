"""Linear operators with the PyLops `LinearOperator` surface the reference's solvers rely on
(`A.shape`, `A @ x`, `A * x`, `A.T @ y`, operands (n,), (n,1), (n,k)), backed by libtrk.so.

  Blur2D(psf, nx, ny)                <- Deblurring2D.forward_Op            trips/test_problems/Deblurring2D.py:66-73
  Blur1D(psf)                        <- Deblurring1D.forward_Op_1D         trips/test_problems/Deblurring1D.py:93-102
  Radon2DParallel(N, angles, ...)    <- parallel-beam OpTomo wrapper       trips/utilities/io.py:392-400
  BlockDiagOp([A_0, ..])             <- pylops.BlockDiag / frame slicing    trips/utilities/io.py:420, :223-225
  FirstDerivative2D(N)               <- gen_first_derivative_operator_2D   trips/utilities/operators.py:30-36
  SpaceTimeDerivative(N, nt)         <- gen_spacetime_derivative_operator  trips/utilities/operators.py:39-45
  Identity(n)                        <- pylops.Identity                    trips/solvers/Hybrid_LSQR.py:76
  first_derivative_operator(_2d), spatial_/time_derivative_operator, VStack
                                     <- the PyLops-built regularisers      trips/utilities/operators_old.py:22-61

NumPy in -> NumPy (float64) out, so the unmodified reference solvers can be handed one of these; torch device
tensors in -> torch device tensors out.  The engine's own solvers use `apply()` on fp32 device vectors and
row-per-vector bases and never leave the GPU.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .engine import default_engine


class LinearOperator:
    """Base class: subclasses provide `_apply(x2d, y2d, transpose, sumsq)` on [batch, n] fp32 device tensors."""

    dtype = np.dtype("float32")
    # True when one apply moves about as many bytes as reading two or three vectors (stencils): the projection solvers
    # then form A x / L x directly instead of (AV) y / (LV) y, which reads k basis vectors
    streaming = False

    def __init__(self, shape, engine=None):
        self.shape = (int(shape[0]), int(shape[1]))
        self.engine = engine if engine is not None else default_engine()

    # ---- engine-native entry point -----------------------------------------------------------
    def apply(self, x, out=None, transpose=False, sumsq=None):
        """y = A x (or A^T x) for a 1-D fp32 device vector, or a [batch, n] row-per-vector block.
        `sumsq` (1-element float64 device view) receives the LOCAL sum(y*y) fused into the kernel."""
        nin = self.shape[0] if transpose else self.shape[1]
        nout = self.shape[1] if transpose else self.shape[0]
        one = x.dim() == 1
        x2 = x.reshape(1, -1) if one else x
        if x2.shape[1] != nin:
            raise ValueError(f"dimension mismatch: operator expects {nin}, got {x2.shape[1]}")
        if out is None:
            out = torch.empty((x2.shape[0], nout), dtype=torch.float32, device=x.device)
        o2 = out.reshape(1, -1) if out.dim() == 1 else out
        if x2.stride(1) != 1 or o2.stride(1) != 1:
            raise ValueError("apply() needs unit-stride vectors")
        self._apply(x2, o2, bool(transpose), sumsq)
        return o2[0] if one else o2

    def _apply(self, x2, y2, transpose, sumsq):
        raise NotImplementedError

    # ---- PyLops-style surface ----------------------------------------------------------------
    def _dot(self, x, transpose):
        nin = self.shape[0] if transpose else self.shape[1]
        is_np = not isinstance(x, torch.Tensor)
        if is_np:
            xa = np.asarray(x)
            if xa.ndim not in (1, 2) or xa.shape[0] != nin:
                raise ValueError(f"dimension mismatch: operator is {self.shape}, operand is {xa.shape}")
            t = torch.from_numpy(np.ascontiguousarray(xa.reshape(nin, -1).T, dtype=np.float32)).to(self.engine.device)
            y = self.apply(t, transpose=transpose)                       # [k, nout]
            out = y.T.to("cpu").numpy().astype(np.float64)
            return out.reshape(-1) if xa.ndim == 1 else out
        if x.dim() not in (1, 2) or x.shape[0] != nin:
            raise ValueError(f"dimension mismatch: operator is {self.shape}, operand is {tuple(x.shape)}")
        t = x.to(device=self.engine.device, dtype=torch.float32)
        rows = t.reshape(nin, -1).T.contiguous()                         # (n,k) column view -> row-per-vector
        y = self.apply(rows, transpose=transpose).T
        return y.reshape(-1) if x.dim() == 1 else y

    def matvec(self, x):
        return self._dot(x, False)

    def rmatvec(self, y):
        return self._dot(y, True)

    matmat = matvec
    rmatmat = rmatvec

    def dot(self, x):
        return self._dot(x, False)

    def __matmul__(self, x):
        return self._dot(x, False)

    def __mul__(self, x):          # `L * v` means matvec in the reference (GKS.py:95, MMGKS.py:127)
        return self._dot(x, False)

    def __call__(self, x):
        return self._dot(x, False)

    @property
    def T(self):
        return _Transposed(self)

    H = T

    def adjoint(self):
        return _Transposed(self)

    transpose = adjoint

    def __array__(self, *args, **kwargs):
        # NumPy asking for an array means a caller took this operator for a matrix — in the reference that is
        # utils.is_identity's `np.allclose(A, np.eye(n))` on any SQUARE operand that is not a pylops LinearOperator
        # (utils.py:55; an n x n eye).  Fail with the remedy instead of an obscure ufunc error.
        raise TypeError(f"{type(self).__name__} is a matrix-free operator, not an array; to hand it to code that tests "
                        "`isinstance(op, pylops.LinearOperator)` (trips/utilities/utils.py:55) pass op.to_pylops()")

    def to_pylops(self):
        """This operator as a `pylops.FunctionOperator(matvec, rmatvec, nr, nc)` — the wrapper the reference's own test
        problems build around their callables (Deblurring2D.py:72, Tomography.py:83, io.py:400).  Use it to hand an engine
        operator to the UNMODIFIED reference solvers: it then passes their `isinstance(.., pylops.LinearOperator)` tests
        (utils.py:55, gcv.py:33) like the operators it replaces.  Needs PyLops (a dependency of the reference)."""
        import pylops
        return pylops.FunctionOperator(self.matvec, self.rmatvec, self.shape[0], self.shape[1])

    def todense(self):
        """Dense float64 matrix (small operators only; Tikhonov.py:20, demo_1D_deblurring)."""
        n = self.shape[1]
        if n > 1 << 14:
            raise MemoryError("todense() is for small operators")
        return self._dot(np.eye(n), False)

    def __repr__(self):
        return f"<{self.shape[0]}x{self.shape[1]} {type(self).__name__} on {self.engine.device}>"


class _Transposed(LinearOperator):
    def __init__(self, op):
        self.op = op
        self.shape = (op.shape[1], op.shape[0])
        self.engine = op.engine

    def apply(self, x, out=None, transpose=False, sumsq=None):
        return self.op.apply(x, out, not transpose, sumsq)

    def _dot(self, x, transpose):
        return self.op._dot(x, not transpose)

    @property
    def T(self):
        return self.op

    H = T


class _HandleOperator(LinearOperator):
    """An operator that owns a trk_op handle."""

    def __init__(self, handle, engine):
        self._h = handle
        rows, cols = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(engine.lib.trk_op_shape(handle, ctypes.byref(rows), ctypes.byref(cols)), "trk_op_shape")
        super().__init__((rows.value, cols.value), engine)

    def _apply(self, x2, y2, transpose, sumsq):
        self.engine.op_apply(self._h, transpose, x2, y2, batch=x2.shape[0], ldx=x2.stride(0), ldy=y2.stride(0), sumsq=sumsq)

    #: hints of apply_axpby (trk.h TRK_HINT_*)
    OUT_FEEDS_OPPOSITE, INPUT_FROM_OPPOSITE, SUMSQ_DEFERRED = 1, 2, 4

    def apply_axpby(self, x, a, b, z, out, transpose=False, sumsq=None, hints=0):
        """out = a * Op(x) + b * z and ||out||^2 in the operator's own output pass (trk_op_apply_axpby: one Golub-Kahan half
        step; a, b: float or engine.Coef; z may be None).  Operators without a native form run apply + axpby in C."""
        self.engine.op_apply_axpby(self._h, transpose, x, a, b, z, out, sumsq, hints)

    def flush_deferred(self):
        """Finish a norm an apply_axpby(..., hints=SUMSQ_DEFERRED) left as block partials (trk_op_flush)."""
        _lib.check(self.engine.lib.trk_op_flush(self._h, self.engine.stream()), "trk_op_flush")

    @property
    def native_axpby(self):
        n = ctypes.c_int(0)
        _lib.check(self.engine.lib.trk_op_axpby_caps(self._h, ctypes.byref(n)), "trk_op_axpby_caps")
        return bool(n.value)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self.engine.lib.trk_op_destroy(h)
            except Exception:
                pass


def _dbl_array(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


# scipy.ndimage boundary modes the blur serves, by their trk.h codes (TRK_BOUNDARY_*), and scipy's aliases of them
BOUNDARY_MODES = {"reflect": 0, "constant": 1, "nearest": 2, "mirror": 3, "wrap": 4}
_BOUNDARY_ALIASES = {"grid-mirror": "reflect", "grid-constant": "constant", "grid-wrap": "wrap"}


def normalize_boundary(mode, cval=0.0):
    """The canonical name of a scipy.ndimage boundary mode for the blur ('grid-*' aliases resolved).  Raises ValueError for
    a mode the blur does not serve and for a non-zero fill value (constant mode pads with 0 only)."""
    if not isinstance(mode, str):
        raise ValueError(f"boundary mode must be a string, got {mode!r}")
    name = _BOUNDARY_ALIASES.get(mode, mode)
    if name not in BOUNDARY_MODES:
        raise ValueError(f"unknown boundary mode {mode!r}: expected one of {sorted(BOUNDARY_MODES) + sorted(_BOUNDARY_ALIASES)}")
    if cval != 0:
        raise ValueError(f"only the fill value 0 is supported (got cval={cval!r})")
    return name


class Blur2D(_HandleOperator):
    """y = scipy.ndimage.convolve(x.reshape(nx,ny), psf, mode=boundary); `.T` = the same with the flipped PSF, in the same
    mode (the reference's "transpose", Deblurring2D.py:70-71, Deblurring1D.py:59-62).

    boundary: 'reflect' (default), 'constant' (zero fill), 'nearest', 'mirror', 'wrap', or scipy's aliases 'grid-mirror',
    'grid-constant', 'grid-wrap'; `self.boundary` holds the canonical name.  The flipped-PSF "transpose" is the exact adjoint
    only for an odd-sized point-symmetric PSF under 'reflect', 'constant' or 'wrap'.  Under 'nearest' / 'mirror', or with an
    even-sized PSF in any mode, it differs from A^T in entries next to the border, as the reference's does.

    `path` names the kernel a plain apply runs on: 'slide' (separable odd PSFs up to 9x9), 'strip' (odd square PSFs up to 15x15),
    'tile' (every other PSF up to 64x64: even, rectangular, wide Gaussians, defocus, motion, measured) or 'generic' (a side above
    64); `set_path` forces 'tile' or 'generic' for tests and rate measurements.

    `streaming` stays `max(psf.shape) <= 15`, whatever the path: it makes GKS / MMGKS re-apply A instead of storing A V, which
    pays for the memory-bound slide and strip kernels only — a tile-path blur is bound by its multiply-adds, not by its bytes."""

    PATHS = {"auto": 0, "slide": 1, "strip": 2, "tile": 3, "generic": 4}          # trk.h TRK_BLUR_PATH_*

    def __init__(self, psf, nx, ny, engine=None, boundary="reflect"):
        self.boundary = normalize_boundary(boundary)       # (a bad name fails before any device is touched)
        engine = engine if engine is not None else default_engine()
        psf = np.asarray(psf, dtype=np.float64)
        if psf.ndim != 2:
            raise ValueError("psf must be 2-D")
        self.psf, self.nx, self.ny = psf, int(nx), int(ny)
        arr, p = _dbl_array(psf)
        h = ctypes.c_void_p()
        _lib.check(engine.lib.trk_blur2d_create_bc(p, psf.shape[0], psf.shape[1], self.nx, self.ny, BOUNDARY_MODES[self.boundary],
                                                   ctypes.byref(h)), "trk_blur2d_create_bc")
        super().__init__(h, engine)
        self.streaming = max(psf.shape) <= 15          # the sliding-window / LDS-strip kernels (csrc/blur2d.hip)

    @property
    def path(self):
        """'slide' | 'strip' | 'tile' | 'generic': the kernel of a contiguous, 16-byte-aligned one-vector apply (trk_blur2d_path)."""
        path, sep = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(self.engine.lib.trk_blur2d_path(self._h, ctypes.byref(path), ctypes.byref(sep)), "trk_blur2d_path")
        return {v: k for k, v in self.PATHS.items()}[path.value]

    def set_path(self, name):
        """Force the kernel: 'tile' (any PSF up to 64x64; NotImplementedError above), 'generic', or 'auto' for the rule again.  A
        forced operator has no fused / epilogue / recompute forms: the solvers take their plain loops (trk_blur2d_set_path)."""
        if name not in ("auto", "tile", "generic"):
            raise ValueError(f"set_path: expected 'auto', 'tile' or 'generic', got {name!r}")
        _lib.check(self.engine.lib.trk_blur2d_set_path(self._h, self.PATHS[name]), "trk_blur2d_set_path")
        return self


class Blur1D(Blur2D):
    """1-D blur with a (possibly length-n) PSF: an n x 1 image and a k x 1 PSF; scipy.ndimage.convolve1d(x, psf, mode=boundary)
    (modes and the "transpose" as Blur2D)."""

    def __init__(self, psf, n=None, engine=None, boundary="reflect"):
        psf = np.asarray(psf, dtype=np.float64).reshape(-1)
        n = len(psf) if n is None else int(n)
        super().__init__(psf.reshape(-1, 1), n, 1, engine, boundary=boundary)


class Radon2DParallel(_HandleOperator):
    """Parallel-beam Joseph projector; sinogram (n_ang, n_det) row-major; scale defaults to 1/N (io.py:397-399)."""

    def __init__(self, N, angles, n_det=None, scale=None, engine=None):
        engine = engine if engine is not None else default_engine()
        self.N = int(N)
        self.angles = np.asarray(angles, dtype=np.float64).reshape(-1)
        self.n_det = self.N if n_det is None else int(n_det)
        self.scale = 1.0 / self.N if scale is None else float(scale)
        arr, p = _dbl_array(self.angles)
        h = ctypes.c_void_p()
        _lib.check(engine.lib.trk_radon2d_create(self.N, self.n_det, p, len(self.angles), self.scale, ctypes.byref(h)), "trk_radon2d_create")
        super().__init__(h, engine)

    # ---- the float64 instrument (csrc/ref64.hip; diagnostics, not a fast path) ----
    ARITHMETIC = {"product": 0, "float64": 1, "tables64": 2}

    def set_ref_sums(self, chunk_fwd=0, chunk_adj=0):
        """The instrument's kernels with emulated fp32 partial sums (trk_radon2d_set_ref_sums): fp32 running sums moved to a float64
        total every chunk_fwd marching steps (forward) / chunk_adj angles (adjoint); 0 = float64 sums."""
        _lib.check(self.engine.lib.trk_radon2d_set_ref_sums(self._h, int(chunk_fwd), int(chunk_adj)), "trk_radon2d_set_ref_sums")
        return self

    def set_arithmetic(self, mode):
        """The arithmetic every apply of this operator runs in (trk_radon2d_set_arithmetic): 'product' — the fast kernels;
        'float64' — interpolation weights from the geometry in float64, float64 sums; 'tables64' — the fast kernels' fixed-point
        weights, float64 sums.  Vectors stay fp32; solvers work unchanged (fused riders run in launches of their own)."""
        _lib.check(self.engine.lib.trk_radon2d_set_arithmetic(self._h, self.ARITHMETIC[mode]), "trk_radon2d_set_arithmetic")
        return self

    def apply_ref(self, x, transpose=False, weights="float64"):
        """Op(x) by the float64-arithmetic kernels on a float32 OR float64 device vector (trk_radon2d_apply_ref)."""
        if x.dtype not in (torch.float32, torch.float64) or not x.is_contiguous():
            raise ValueError("apply_ref: contiguous float32 / float64 device vector expected")
        nin, nout = (self.shape[0], self.shape[1]) if transpose else (self.shape[1], self.shape[0])
        if x.numel() != nin:
            raise ValueError(f"dimension mismatch: operator expects {nin}, got {x.numel()}")
        y = torch.empty(nout, dtype=x.dtype, device=x.device)
        _lib.check(self.engine.lib.trk_radon2d_apply_ref(self._h, int(bool(transpose)), x.element_size(), {"float64": 0, "tables64": 1}[weights],
                                                         x.data_ptr(), y.data_ptr(), self.engine.stream()), "trk_radon2d_apply_ref")
        return y


class FanBeam2D(_HandleOperator):
    """Fan-beam flat-detector line projector with the geometry defaults of Tomography.define_proj_id
    (trips/test_problems/Tomography.py:48-67): p = int(sqrt(2) N) detector pixels, source-origin 3N, origin-detector N,
    detector pitch (SOD+ODD)/SOD, theta = linspace(0, pi, views, endpoint=False)."""

    def __init__(self, N, views=None, angles=None, n_det=None, source_origin=None, origin_detector=None, det_pitch=None,
                 engine=None):
        engine = engine if engine is not None else default_engine()
        self.N = int(N)
        self.angles = (np.linspace(0, np.pi, int(views), endpoint=False) if angles is None
                       else np.asarray(angles, dtype=np.float64).reshape(-1))
        self.n_det = int(np.sqrt(2) * self.N) if n_det is None else int(n_det)
        self.sod = 3.0 * self.N if source_origin is None else float(source_origin)
        self.odd = 1.0 * self.N if origin_detector is None else float(origin_detector)
        self.pitch = (self.sod + self.odd) / self.sod if det_pitch is None else float(det_pitch)
        arr, p = _dbl_array(self.angles)
        h = ctypes.c_void_p()
        _lib.check(engine.lib.trk_fanbeam2d_create(self.N, self.n_det, self.pitch, self.sod, self.odd, p, len(self.angles),
                                                   ctypes.byref(h)), "trk_fanbeam2d_create")
        super().__init__(h, engine)


class _FusedTV:
    """Fused forms of a first-difference regulariser for the re-weighted solvers (trk_tv_weights / trk_tv_grad): no vector of
    the length of L x in between.  `fused_tv` says whether this operator instance has them."""
    fused_tv = True

    def tv_weights(self, x, eps, q, out):
        """out = ((L x)^2 + eps^2)^(q/2-1) (MMGKS.py:60,93)."""
        _lib.check(self.engine.lib.trk_tv_weights(self._h, x.data_ptr(), float(eps), float(q), out.data_ptr(),
                                                  self.engine.stream()), "trk_tv_weights")

    def tv_grad(self, x, w, r_in, lam, out, dot_with=None, dot_out=None, xsq_out=None):
        """out = r_in + lam * L^T (w .* (L x)) (MMGKS.py:116-118); w None: unit weights (GKS.py:81-84); r_in None: 0.
        dot_with / dot_out: also <out, dot_with> into the device scalar dot_out, from the same pass (trk_tv_grad_dot);
        xsq_out (with them): and <x, x> (trk_tv_grad_dot_xsq)."""
        if dot_with is not None and xsq_out is not None:
            rc = self.engine.lib.trk_tv_grad_dot_xsq(self._h, x.data_ptr(), None if w is None else w.data_ptr(),
                                                     None if r_in is None else r_in.data_ptr(), float(lam), out.data_ptr(),
                                                     dot_with.data_ptr(), dot_out if isinstance(dot_out, int) else dot_out.data_ptr(),
                                                     xsq_out if isinstance(xsq_out, int) else xsq_out.data_ptr(), self.engine.stream())
            _lib.check(rc, "trk_tv_grad_dot_xsq")
            return
        if dot_with is not None:
            rc = self.engine.lib.trk_tv_grad_dot(self._h, x.data_ptr(), None if w is None else w.data_ptr(),
                                                 None if r_in is None else r_in.data_ptr(), float(lam), out.data_ptr(),
                                                 dot_with.data_ptr(), dot_out if isinstance(dot_out, int) else dot_out.data_ptr(),
                                                 self.engine.stream())
            _lib.check(rc, "trk_tv_grad_dot")
            return
        rc = self.engine.lib.trk_tv_grad(self._h, x.data_ptr(), None if w is None else w.data_ptr(),
                                         None if r_in is None else r_in.data_ptr(), float(lam), out.data_ptr(),
                                         self.engine.stream())
        _lib.check(rc, "trk_tv_grad")


class FirstDerivative2D(_FusedTV, _HandleOperator):
    def __init__(self, N, engine=None):
        engine = engine if engine is not None else default_engine()
        self.N = int(N)
        h = ctypes.c_void_p()
        _lib.check(engine.lib.trk_deriv2d_create(self.N, ctypes.byref(h)), "trk_deriv2d_create")
        super().__init__(h, engine)
        self.streaming = True


class SpaceTimeDerivative(_FusedTV, _HandleOperator):
    """Space-time first differences over this rank's `nt_local` frames (trips/utilities/operators.py:39-45).

    Time-sharded (engine.world > 1), two ways to meet the rows x_t - x_{t+1} that cross a rank boundary:
      * the fused forms `tv_weights` / `tv_grad` (what GKS / MMGKS use; the kernels one rank runs): the operand's two boundary
        frames of the neighbour ranks — `halo_frames(x)`, ONE two-sided exchange — and the rank forms its own pixels of
        L^T (w .* L x) completely.  `halo=` takes frames the caller already has (GKS derives them for x = V y and v_new from the
        basis vectors' halos: one exchange per iteration);
      * plain `L @ x` / `L.T @ y`: one frame moves to the neighbour before each apply (forward: first frame of the next rank;
        transpose: last temporal block of the previous rank)."""

    def __init__(self, N, nt, engine=None):
        engine = engine if engine is not None else default_engine()
        self.N, self.nt_global = int(N), int(nt)
        w, r = engine.world, engine.rank
        if self.nt_global % w:
            raise ValueError(f"{nt} frames do not shard evenly over {w} ranks")
        self.nt_local = self.nt_global // w
        self.has_next, self.has_prev = r < w - 1, r > 0
        h = ctypes.c_void_p()
        _lib.check(engine.lib.trk_spacetime_create(self.N, self.nt_local, int(self.has_next), int(self.has_prev), ctypes.byref(h)),
                   "trk_spacetime_create")
        super().__init__(h, engine)
        npix = self.N * self.N
        self.npix = npix
        self._halo_next = engine.empty(npix) if self.has_next else None
        self._halo_prev = engine.empty(npix) if self.has_prev else None
        self._xh = engine.empty(2 * npix) if w > 1 else None       # [previous rank's last frame | next rank's first frame]
        self._ps = 2 * self.N * (self.N - 1)
        self.sharded = w > 1
        self.streaming = True
        self.fused_tv = True
        # weights of the fused forms: the rows of L, plus (has_prev) the previous rank's boundary row recomputed here
        self.tv_weights_len = self.shape[0] + (npix if self.has_prev else 0)

    # ---- fused forms over a time-sharded vector
    def halo_frames(self, x, out=None):
        """The neighbour ranks' boundary frames of the time-sharded vector x, [prev's last | next's first] (2 N^2 floats; a half
        without a neighbour is left as it is): ONE two-sided exchange."""
        eng, npix = self.engine, self.npix
        out = self._xh if out is None else out
        eng.halo_exchanges += 1
        if eng.world > 1:
            eng.comm.exchange2(x[:npix], out[:npix], x[(self.nt_local - 1) * npix:self.nt_local * npix], out[npix:2 * npix])
        return out

    def _give_halo(self, x, halo):
        if not self.sharded:
            return
        hf = self.halo_frames(x) if halo is None else halo
        _lib.check(self.engine.lib.trk_tv_halo(self._h, hf.data_ptr() if self.has_prev else None,
                                               hf[self.npix:].data_ptr() if self.has_next else None), "trk_tv_halo")

    def tv_weights(self, x, eps, q, out, halo=None):
        if out.numel() < self.tv_weights_len:
            # (a rank with a previous neighbour also writes that neighbour's boundary row: N^2 more than L has rows)
            raise ValueError(f"tv_weights: out holds {out.numel()} floats, this operator writes tv_weights_len = {self.tv_weights_len}")
        self._give_halo(x, halo)
        super().tv_weights(x, eps, q, out)

    def tv_grad(self, x, w, r_in, lam, out, dot_with=None, dot_out=None, halo=None, xsq_out=None):
        if w is not None and w.numel() < self.tv_weights_len:
            raise ValueError(f"tv_grad: w holds {w.numel()} floats, this operator reads tv_weights_len = {self.tv_weights_len}")
        self._give_halo(x, halo)
        super().tv_grad(x, w, r_in, lam, out, dot_with=dot_with, dot_out=dot_out, xsq_out=xsq_out)

    def _apply(self, x2, y2, transpose, sumsq):
        eng = self.engine
        if eng.world > 1:
            if x2.shape[0] != 1:
                raise NotImplementedError("sharded space-time operator applies one vector at a time")
            eng.halo_exchanges += 1
            spacetime_halo_exchange(eng, x2[0], transpose, self.N, self.nt_local, self._halo_next, self._halo_prev)
            _lib.check(eng.lib.trk_spacetime_set_halo(self._h, None if self._halo_next is None else self._halo_next.data_ptr(),
                                                      None if self._halo_prev is None else self._halo_prev.data_ptr()),
                       "trk_spacetime_set_halo")
        super()._apply(x2, y2, transpose, sumsq)


def spacetime_halo_exchange(eng, x, transpose, N, nt_local, halo_next, halo_prev):
    """The one-frame neighbour exchange of the time-sharded space-time regulariser (operators.py:39-45 of the reference
    couples frame t with t+1 through the rows x_t - x_{t+1}).

    forward  : every rank but the first sends its FIRST frame to the previous rank (which owns the row coupling its
               last frame to it) and receives the next rank's first frame into `halo_next`.
    transpose: every rank but the last sends its LAST temporal block (the row it owns on behalf of the boundary) to the
               next rank and receives the previous rank's into `halo_prev`.
    x is the rank-local operand (frame-major image block for forward; [spatial rows | temporal rows] for transpose)."""
    npix, ps = N * N, 2 * N * (N - 1)
    has_next, has_prev = eng.rank < eng.world - 1, eng.rank > 0
    if not transpose:
        eng.comm.shift(send=x[:npix] if has_prev else None, send_to=eng.rank - 1,
                       recv=halo_next, recv_from=eng.rank + 1 if has_next else None)
    else:
        last = x[nt_local * ps + (nt_local - 1) * npix:nt_local * ps + nt_local * npix] if has_next else None
        eng.comm.shift(send=last, send_to=eng.rank + 1,
                       recv=halo_prev, recv_from=eng.rank - 1 if has_prev else None)


class BlockDiagOp(_HandleOperator):
    """F = blkdiag(A_0 .. A_{T-1}) over THIS RANK's frames; x and b are frame-major."""

    def __init__(self, ops, engine=None):
        engine = engine if engine is not None else ops[0].engine
        self.ops = list(ops)
        h = ctypes.c_void_p()
        first = self.ops[0]
        same_radon = all(isinstance(o, Radon2DParallel) and o.N == first.N and o.n_det == first.n_det
                         and o.scale == first.scale and len(o.angles) == len(first.angles) for o in self.ops)
        if len(self.ops) > 1 and all(type(o) is SparseOp for o in self.ops):
            # frames given as sparse matrices (the blocks io.py:223-225 cuts out of the real data's forward matrix): ONE CSR of the
            # block-diagonal matrix, one launch per apply whatever the number of frames
            import scipy.sparse as sp
            merged = SparseOp(sp.block_diag([o.matrix for o in self.ops], format="csr"), engine=engine)
            self.matrix = merged.matrix
            h, merged._h = merged._h, None
        elif same_radon and len(self.ops) > 1:
            # frames of one dynamic tomography problem: a single handle runs all frames per launch
            ang = np.concatenate([o.angles for o in self.ops])
            arr, p = _dbl_array(ang)
            _lib.check(engine.lib.trk_radon2d_dynamic_create(first.N, first.n_det, p, len(self.ops), len(first.angles),
                                                             first.scale, ctypes.byref(h)), "trk_radon2d_dynamic_create")
        else:
            arr = (ctypes.c_void_p * len(self.ops))(*[o._h for o in self.ops])
            _lib.check(engine.lib.trk_blockdiag_create(arr, len(self.ops), ctypes.byref(h)), "trk_blockdiag_create")
        super().__init__(h, engine)


class SparseOp(_HandleOperator):
    """An operator given as a (scipy.sparse or small dense) matrix: CSR SpMV on the device, both directions as gathers.
    This is what a reference-built regulariser (`gen_first_derivative_operator_2D`, `gen_spacetime_derivative_operator`,
    the framelet analysis matrices: trips/utilities/operators.py) or a precomputed sparse forward matrix
    (io.py:197-229) becomes when handed to the engine's solvers."""

    def __init__(self, M, engine=None):
        import scipy.sparse as sp
        engine = engine if engine is not None else default_engine()
        A = sp.csr_matrix(M)
        A.sum_duplicates()
        At = A.T.tocsr()
        At.sum_duplicates()
        self.matrix = A

        def arrs(C):
            return (np.ascontiguousarray(C.indptr, dtype=np.int64), np.ascontiguousarray(C.indices, dtype=np.int32),
                    np.ascontiguousarray(C.data, dtype=np.float32))
        ip, ix, dv = arrs(A)
        tp, tx, tv = arrs(At)
        h = ctypes.c_void_p()
        _lib.check(engine.lib.trk_csr_create(A.shape[0], A.shape[1], A.nnz, ip.ctypes.data, ix.ctypes.data, dv.ctypes.data,
                                             tp.ctypes.data, tx.ctypes.data, tv.ctypes.data, ctypes.byref(h)), "trk_csr_create")
        super().__init__(h, engine)


def slice_dynamic_frames(A, b, nt, rows_per_frame, cols_per_frame):
    """The per-frame blocks of a dynamic problem's forward matrix and data, exactly as the reference's loaders cut them
    (trips/utilities/io.py:223-225, generate_crossPhantom: `AA[ii] = A_small[700*ii:700*(ii+1), 16384*ii:16384*(ii+1)]`,
    `B[ii] = b[700*ii:700*(ii+1)]`; io.py:160-162 does the same for the emoji data): frame ii owns rows
    [ii rows_per_frame, (ii+1) rows_per_frame) and columns [ii cols_per_frame, (ii+1) cols_per_frame); whatever the matrix
    holds outside those blocks is dropped.  Returns (list of scipy.sparse CSR blocks, list of data blocks)."""
    import scipy.sparse as sp
    A = sp.csr_matrix(A)
    nt, rpf, cpf = int(nt), int(rows_per_frame), int(cols_per_frame)
    if A.shape[0] < nt * rpf or A.shape[1] < nt * cpf:
        raise ValueError(f"slice_dynamic_frames: a {A.shape[0]} x {A.shape[1]} matrix has no {nt} blocks of {rpf} x {cpf}")
    bb = None if b is None else np.asarray(b).reshape(-1)
    AA = [A[rpf * ii:rpf * (ii + 1), cpf * ii:cpf * (ii + 1)].tocsr() for ii in range(nt)]
    B = None if bb is None else [bb[rpf * ii:rpf * (ii + 1)] for ii in range(nt)]
    return AA, B


class SparseBlockDiag(SparseOp):
    """F = blkdiag(A_0 .. A_{T-1}) of sparse frame matrices as ONE CSR operator on the device: x and b frame-major, one launch per
    apply (pylops.BlockDiag over per-frame matrices, io.py:420, for the sparse real-data problems of io.py:197-229).  On several
    ranks every rank holds the blocks of its own frames (dist.frame_range)."""

    def __init__(self, blocks, engine=None):
        import scipy.sparse as sp
        self.blocks = [sp.csr_matrix(B) for B in blocks]
        super().__init__(sp.block_diag(self.blocks, format="csr"), engine=engine)

    @classmethod
    def from_matrix(cls, A, nt, rows_per_frame, cols_per_frame, engine=None):
        """From the whole forward matrix, sliced as the reference slices it (slice_dynamic_frames); with engine.world > 1 only this
        rank's frames are kept."""
        from .dist import frame_range
        engine = engine if engine is not None else default_engine()
        AA, _ = slice_dynamic_frames(A, None, nt, rows_per_frame, cols_per_frame)
        lo, hi = frame_range(int(nt), getattr(engine, "world", 1), getattr(engine, "rank", 0))
        return cls(AA[lo:hi], engine=engine)


def framelet_analysis_matrix(n, l):
    """The reference's 1-D framelet analysis matrix W_n of level l as a scipy CSR matrix, (2l+1) n x n
    (trips/utilities/operators.py:50-103, recursion as written there: the deepest level comes back without the low-pass product)."""
    import scipy.sparse as sp

    def construct_H(lev, nn):                       # operators.py:50-85
        e = np.ones((nn,))
        H0 = (sp.spdiags(e, -lev, nn, nn) + sp.spdiags(2 * e, 0, nn, nn) + sp.spdiags(e, lev, nn, nn)).tolil()
        H1 = (sp.spdiags(-e, -lev, nn, nn) + sp.spdiags(e, lev, nn, nn)).tolil()
        H2 = (sp.spdiags(-e, -lev, nn, nn) + sp.spdiags(2 * e, 0, nn, nn) + sp.spdiags(-e, lev, nn, nn)).tolil()
        for jj in range(lev):
            H0[jj, lev - jj - 1] += 1
            H0[-jj - 1, -lev + jj] += 1
            H1[jj, lev - jj - 1] -= 1
            H1[-jj - 1, -lev + jj] += 1
            H2[jj, lev - jj - 1] -= 1
            H2[-jj - 1, -lev + jj] -= 1
        return H0.tocsr() / 4, H1.tocsr() * (np.sqrt(2) / 4), H2.tocsr() / 4

    def analysis(nn, level, w):                     # operators.py:88-103
        if level == l:
            return sp.vstack(construct_H(level, nn))
        H0, H1, H2 = construct_H(level, nn)
        return sp.vstack((analysis(nn, level + 1, H0), H1, H2)) * w

    return sp.csr_matrix(analysis(n, 1, 1))


def band_tables(W, n, half=None):
    """A 1-D analysis matrix W (blocks n x n, dense or scipy.sparse) as the band tables of trk_framelet2d_create:
    (blocks, half, band) with band[b, i, t] = W[b n + i, i - half + t], 0 where that column lies outside [0, n), float64.
    half=None: the largest |column - (row mod n)| over W's non-zeros.  Pure NumPy.  ValueError: W has not n columns, its row count is
    no multiple of n, a non-zero lies outside the band of a given `half`, or an interior row of a block (half <= i <= n - 1 - half)
    is not the block's stencil shifted (compared as float32, the precision of the kernels): no separable band operator of this kind."""
    n = int(n)
    if hasattr(W, "tocoo"):
        C = W.tocoo()
        shape, r, c, v = C.shape, np.asarray(C.row, dtype=np.int64), np.asarray(C.col, dtype=np.int64), np.asarray(C.data, dtype=np.float64)
    else:
        D = np.asarray(W, dtype=np.float64)
        if D.ndim != 2:
            raise ValueError("band_tables: a 2-D matrix expected")
        shape = D.shape
        r, c = np.nonzero(D)
        v = D[r, c]
    if n < 1 or shape[1] != n or shape[0] % n or shape[0] == 0:
        raise ValueError(f"band_tables: a {shape[0]} x {shape[1]} matrix is not (blocks * {n}) x {n}")
    keep = v != 0
    r, c, v = r[keep], c[keep], v[keep]
    blocks = shape[0] // n
    i = r % n
    reach = int(np.abs(c - i).max()) if v.size else 0
    if half is None:
        half = reach
    elif reach > int(half):
        k = int(np.argmax(np.abs(c - i)))
        raise ValueError(f"band_tables: W[{r[k]}, {c[k]}] is non-zero, {reach} off the diagonal of its block: outside the band of half-width {half}")
    half = int(half)
    band = np.zeros((blocks, n, 2 * half + 1))
    np.add.at(band, (r // n, i, c - i + half), v)
    return blocks, half, _check_band(band, n, half)


def _check_band(band, n, half):
    """band_tables' structure checks on the finished table (the library repeats them on what it is handed)."""
    blocks, w = band.shape[0], 2 * half + 1
    if band.shape != (blocks, n, w):
        raise ValueError(f"band table of shape {band.shape}, expected {(blocks, n, w)}")
    cols = np.arange(n)[:, None] - half + np.arange(w)[None, :]
    if np.any(band[:, (cols < 0) | (cols >= n)] != 0):
        raise ValueError("band table: a non-zero entry lies outside the band's part inside the matrix")
    if n > 2 * half:
        inner = band[:, half:n - half, :].astype(np.float32)
        if np.any(inner != inner[:, :1, :]):
            raise ValueError("band table: the interior rows of a block are not one shifted stencil")
    return band


class Framelet2D(_HandleOperator):
    """A separable band operator: y = vec_F(W_n X W_m^T) for X = x.reshape(n, m, order='F'), `.T` its exact transpose, applied
    matrix-free by the stencil kernels of csrc/framelet2d.hip; rows blocks_n n * blocks_m m, columns n m, the layout of the CSR form
    of kron(W_m, W_n).  Framelet2D(n, m, l) is the reference's framelet analysis operator of level l
    (trips/utilities/operators.py:50-113, create_framelet_operator); Framelet2D.from_analysis takes any pair of 1-D matrices whose
    blocks are band matrices with one stencil in their interior rows (boundary rows are free).  Levels 1 .. 4 (half-width <= 7)."""

    MAX_HALF = 7            # csrc/framelet2d.hip: kMaxHalf
    streaming = True

    def __init__(self, n, m, l, engine=None):
        n, m, l = int(n), int(m), int(l)
        if l < 1:
            raise ValueError("Framelet2D: level l >= 1 expected")
        self._setup(framelet_analysis_matrix(n, l), framelet_analysis_matrix(m, l) if m != n else None, n, m, engine, l)

    @classmethod
    def from_analysis(cls, W_n, W_m, n, m, engine=None):
        """From 1-D analysis matrices W_n ((blocks_n n) x n) and W_m ((blocks_m m) x m), dense or scipy.sparse."""
        self = cls.__new__(cls)
        self._setup(W_n, W_m, int(n), int(m), engine, None)
        return self

    def _setup(self, W_n, W_m, n, m, engine, l):
        tn = band_tables(W_n, n)
        tm = tn if W_m is None else band_tables(W_m, m)
        self.n, self.m, self.l = n, m, l
        self.blocks_n, self.half_n, self.blocks_m, self.half_m = tn[0], tn[1], tm[0], tm[1]
        if max(tn[1], tm[1]) > self.MAX_HALF:
            raise ValueError(f"Framelet2D: half-widths {tn[1]}, {tm[1]} of the 1-D factors exceed the stencil kernels' limit of {self.MAX_HALF} "
                             f"(framelet levels 1 .. 4); use create_framelet_operator(..., matrix_free=False) for the CSR form")
        engine = engine if engine is not None else default_engine()
        h = self._create(engine, n, m, tn, tm)
        super().__init__(h, engine)

    @staticmethod
    def _create(engine, n, m, tn, tm):
        """trk_framelet2d_create on (blocks, half, band) triples; the library's own checks raise ValueError / NotImplementedError."""
        an, pn = _dbl_array(tn[2])
        am, pm = _dbl_array(tm[2])
        h = ctypes.c_void_p()
        _lib.check(engine.lib.trk_framelet2d_create(n, m, int(tn[0]), int(tn[1]), pn, int(tm[0]), int(tm[1]), pm, ctypes.byref(h)),
                   "trk_framelet2d_create")
        return h


def create_framelet_operator(n, m, l, engine=None, matrix_free=False):
    """The reference's framelet analysis operator (trips/utilities/operators.py:50-113): vec_F(W_n X W_m^H) = kron(W_m, W_n) vec_F(X)
    for the reference's column-major reshapes (:106-108); rows n(2l+1) * m(2l+1), columns n*m.
    matrix_free=False: ONE sparse matrix on the device (SparseOp; 169 non-zeros per pixel at l = 2, 1764 at l = 3).
    matrix_free=True: Framelet2D, the two 1-D band matrices applied by stencil kernels — the form for images beyond ~1024^2."""
    if matrix_free:
        return Framelet2D(n, m, l, engine=engine)
    import scipy.sparse as sp
    W_n, W_m = framelet_analysis_matrix(n, l), framelet_analysis_matrix(m, l)
    return SparseOp(sp.kron(W_m, W_n, format="csr"), engine=engine)


# --------------------------------------------------------------------------------------------------------------------
# The PyLops-built regularisers of trips/utilities/operators_old.py:22-61 (what MMGKS's isoTV branch expects of `L`,
# MMGKS.py:61-77).  PyLops is an un-pinned, absent dependency of the reference: `pylops.FirstDerivative(n)` is restated
# here from its published default (kind="centered", 3-point, edge=False): row i = (x[i+1] - x[i-1]) / 2 for
# 1 <= i <= n-2, first and last row zero — PARITY UNPINNED for that stencil.
def _centered_first_derivative_matrix(n):
    import scipy.sparse as sp
    i = np.arange(1, n - 1)
    return sp.csr_matrix((np.concatenate((np.full(i.size, -0.5), np.full(i.size, 0.5))),
                          (np.concatenate((i, i)), np.concatenate((i - 1, i + 1)))), shape=(n, n))


def _first_derivative_2d_matrix(nx, ny):
    import scipy.sparse as sp
    if nx != ny:      # the reference's VStack of an nx^2- and an ny^2-column operator fails as well (operators_old.py:43)
        raise ValueError("first_derivative_operator_2d: the reference's operator exists for nx == ny only")
    return sp.vstack((sp.kron(sp.identity(nx), _centered_first_derivative_matrix(nx)),
                      sp.kron(_centered_first_derivative_matrix(ny), sp.identity(ny)))).tocsr()


def first_derivative_operator(n, engine=None):
    """operators_old.py:22-33 (`pylops.FirstDerivative(n)`): n x n, centered, zero first/last row."""
    return SparseOp(_centered_first_derivative_matrix(n), engine=engine)


def first_derivative_operator_2d(nx, ny, engine=None):
    """operators_old.py:35-45: VStack(Kronecker(I_nx, D_nx), Kronecker(D_ny, I_ny)), 2 nx^2 x nx^2."""
    return SparseOp(_first_derivative_2d_matrix(nx, ny), engine=engine)


def spatial_derivative_operator(nx, ny, nt, engine=None):
    """operators_old.py:47-53: Kronecker(I_nt, first_derivative_operator_2d) on a frame-major vector."""
    import scipy.sparse as sp
    return SparseOp(sp.kron(sp.identity(nt), _first_derivative_2d_matrix(nx, ny)).tocsr(), engine=engine)


def time_derivative_operator(nx, ny, nt, engine=None):
    """operators_old.py:55-61: Kronecker(D_nt, I_{nx^2})."""
    import scipy.sparse as sp
    return SparseOp(sp.kron(_centered_first_derivative_matrix(nt), sp.identity(nx ** 2)).tocsr(), engine=engine)


class VStack(LinearOperator):
    """pylops.VStack(ops): operators stacked by rows (the way the dynamic demos assemble space + time regularisers).
    Sparse-matrix operators are merged into one CSR operator; anything else is applied block by block."""

    def __new__(cls, ops, engine=None):
        ops = list(ops)
        if ops and all(isinstance(o, SparseOp) for o in ops):
            import scipy.sparse as sp
            return SparseOp(sp.vstack([o.matrix for o in ops]).tocsr(), engine=engine if engine is not None else ops[0].engine)
        return super().__new__(cls)

    def __init__(self, ops, engine=None):
        self.ops = list(ops)
        if not self.ops or any(o.shape[1] != self.ops[0].shape[1] for o in self.ops):
            raise ValueError("VStack: operators must share their column count")
        super().__init__((sum(o.shape[0] for o in self.ops), self.ops[0].shape[1]),
                         engine if engine is not None else self.ops[0].engine)
        self._ro = np.cumsum([0] + [o.shape[0] for o in self.ops])
        self._tmp = None

    def _apply(self, x2, y2, transpose, sumsq):
        eng = self.engine
        for j in range(x2.shape[0]):
            if not transpose:
                for i, o in enumerate(self.ops):
                    o.apply(x2[j], out=y2[j, self._ro[i]:self._ro[i + 1]])
            else:
                if self._tmp is None:
                    self._tmp = eng.empty(self.shape[1])
                for i, o in enumerate(self.ops):
                    seg = x2[j, self._ro[i]:self._ro[i + 1]]
                    if i == 0:
                        o.apply(seg, out=y2[j], transpose=True)
                    else:
                        o.apply(seg, out=self._tmp, transpose=True)
                        eng.axpby(1.0, y2[j], 1.0, self._tmp, y2[j])
        if sumsq is not None:
            if x2.shape[0] != 1:
                raise ValueError("VStack: fused sum of squares for single vectors only")
            eng.nrm2sq(y2[0], sumsq)


def bit_reversed_order(S):
    """The subsets 0 .. S-1 sorted by the bit-reversed value of their number in ceil(log2 S) bits: consecutive sub-steps then see
    views far apart.  S = 6: 0, 4, 2, 1, 5, 3."""
    bits = max(1, (int(S) - 1).bit_length())
    return sorted(range(int(S)), key=lambda s: int(format(s, f"0{bits}b")[::-1], 2))


class RowSubsets(LinearOperator):
    """An operator cut into S row subsets, each an operator of the engine of its own: what the ordered-subsets solvers (solvers.OSEM,
    solvers.SIRT / SART) iterate over.

        ops      S operators; ops[s] maps the same x to the rows `rows[s]` of A
        rows     S index arrays into A's rows, together a partition of range(m)
        perm     the concatenation of `rows` in subset order: data are held on the device SUBSET-MAJOR, b[perm]
        offsets  S + 1 row offsets into that order
        order    the order in which a pass visits the subsets

    Radon2DParallel and FanBeam2D: subset s holds the views s, s + S, s + 2S, ... — a new handle made from angles[s::S] with the same
    detector, scale and geometry; 1 <= S <= n_ang, S need not divide n_ang.  SparseOp: S an int (rows s::S) or a list of index arrays
    that partition the rows; each subset is a SparseOp of matrix[rows].  Any other operator (blur, block-diagonal and dynamic
    operators, framelets, first differences) has no views to deal out and raises ValueError for S > 1; S = 1 wraps A itself.

    order: "bitrev" (bit_reversed_order), "sequential", or a permutation of range(S).

    THE SUBSET HANDLES ARE NOT SLICES OF THE FULL OPERATOR'S BITS.  A parallel-beam handle chooses its adjoint's neighbour constants by
    error diffusion over the angles it was made with, and its forward groups symmetric angles: ops[s] agrees with the rows of A to
    rounding, not bit for bit.  Tests therefore compare each subset handle with the float64 operator of ITS angles.

    As a LinearOperator this is the subset-major stack A[perm] (the subsets applied one after the other)."""

    def __init__(self, A, S, order="bitrev"):
        m = A.shape[0]
        if not isinstance(S, (int, np.integer)):
            if type(A) is not SparseOp:
                raise ValueError("RowSubsets: subsets given as index arrays need a SparseOp")
            rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in S]
        elif S == 1:
            self._setup([A], [np.arange(m)], m, order, A)
            return
        elif isinstance(A, (Radon2DParallel, FanBeam2D)):
            n_ang = len(A.angles)
            if not 1 <= S <= n_ang:
                raise ValueError(f"RowSubsets: need 1 <= S <= the {n_ang} views of the operator, got S = {S}")
            if isinstance(A, Radon2DParallel):
                ops = [Radon2DParallel(A.N, A.angles[s::S], n_det=A.n_det, scale=A.scale, engine=A.engine) for s in range(S)]
            else:
                ops = [FanBeam2D(A.N, angles=A.angles[s::S], n_det=A.n_det, source_origin=A.sod, origin_detector=A.odd, det_pitch=A.pitch,
                                 engine=A.engine) for s in range(S)]
            views = np.arange(m).reshape(n_ang, A.n_det)
            self._setup(ops, [views[s::S].reshape(-1) for s in range(S)], m, order, A)
            return
        elif type(A) is SparseOp:
            if not 1 <= S <= m:
                raise ValueError(f"RowSubsets: need 1 <= S <= the {m} rows of the matrix, got S = {S}")
            rows = [np.arange(s, m, S) for s in range(S)]
        else:
            raise ValueError(f"RowSubsets: a {type(A).__name__} has no views or rows to deal out into S = {S} subsets (built for "
                             "Radon2DParallel, FanBeam2D and SparseOp; S = 1 works for every operator)")
        self._partition(rows, m)                                  # before matrix[rows] trips over a bad index
        self._setup([SparseOp(A.matrix[r], engine=A.engine) for r in rows], rows, m, order, A)

    @classmethod
    def from_ops(cls, ops, rows, m, order="bitrev"):
        """From subset operators the caller made: ops[s] stands for the rows `rows[s]` of an m-row operator."""
        self = cls.__new__(cls)
        self._setup(list(ops), [np.asarray(r, dtype=np.int64).reshape(-1) for r in rows], int(m), order, None)
        return self

    @staticmethod
    def _partition(rows, m):
        perm = np.concatenate(rows) if len(rows) else np.empty(0, dtype=np.int64)
        if perm.size != m or not np.array_equal(np.sort(perm), np.arange(m)):
            raise ValueError(f"RowSubsets: the index arrays do not partition the {m} rows")
        return perm

    def _setup(self, ops, rows, m, order, A):
        S = len(ops)
        if S < 1 or len(rows) != S:
            raise ValueError("RowSubsets: need one index array per subset operator, and at least one subset")
        perm = self._partition(rows, m)
        if any(o.shape != (len(r), ops[0].shape[1]) or len(r) == 0 for o, r in zip(ops, rows)):
            raise ValueError("RowSubsets: every subset operator needs the rows of its index array (at least one) and the same columns")
        if isinstance(order, str):
            if order not in ("bitrev", "sequential"):
                raise ValueError(f"RowSubsets: order is 'bitrev', 'sequential' or a permutation, got {order!r}")
            order = bit_reversed_order(S) if order == "bitrev" else range(S)
        self.order = [int(s) for s in order]
        if sorted(self.order) != list(range(S)):
            raise ValueError(f"RowSubsets: order is not a permutation of range({S})")
        self.A, self.ops, self.rows, self.perm = A, ops, rows, perm
        self.offsets = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
        self._ro, self._tmp = self.offsets, None                  # what VStack._apply works with
        super().__init__((m, ops[0].shape[1]), ops[0].engine)

    _apply = VStack._apply

    def split(self, b):
        """A host m-vector in subset-major order, b[perm]."""
        return np.asarray(b).reshape(-1)[self.perm]

    def join(self, y):
        """The inverse of split."""
        out = np.empty_like(np.asarray(y).reshape(-1))
        out[self.perm] = np.asarray(y).reshape(-1)
        return out


class Identity(LinearOperator):
    def __init__(self, n, engine=None):
        super().__init__((n, n), engine)

    def _apply(self, x2, y2, transpose, sumsq):
        y2.copy_(x2)
        if sumsq is not None:
            self.engine.nrm2sq(y2.reshape(-1), sumsq)


def operator_norm_sq(ops, iters=30, seed=0):
    """An estimate of ||K||^2 for K = the operators of `ops` stacked by rows: the largest eigenvalue of sum_O O^T O, by `iters` steps
    of power iteration from `default_rng(seed).standard_normal(n)` rounded to fp32.  Step j normalises v, forms y = sum_O O^T (O v)
    with the engine's apply / axpby / norm kernels and takes the Rayleigh quotient sum_O ||O v||^2 / ||v||^2; the next v is y.
    Returns the last quotient — it approaches ||K||^2 FROM BELOW (PDHG's default steps leave room for that: solvers/PDHG.py).
    One read-back, after the last step."""
    from .engine import Coef
    ops = [ops] if isinstance(ops, LinearOperator) else list(ops)
    if not ops or any(o.shape[1] != ops[0].shape[1] for o in ops):
        raise ValueError("operator_norm_sq: the operators must share their column count")
    iters = int(iters)
    if iters < 1:
        raise ValueError("operator_norm_sq needs iters >= 1")
    eng, n = ops[0].engine, ops[0].shape[1]
    y = eng.to_vec(np.random.default_rng(seed).standard_normal(n).astype(np.float32))
    v, t = eng.empty(n), eng.empty(n)
    outs = [eng.empty(o.shape[0]) for o in ops]
    T = eng.scalars(2 + len(ops))                       # ||y||^2, ||v||^2, ||O v||^2 per operator
    for _ in range(iters):
        eng.nrm2sq(y, T.ref(0))
        eng.scale(Coef(1.0, den=T.ref(0), sqrt_den=True), y, v, sumsq=T.ref(1))
        for i, (o, w) in enumerate(zip(ops, outs)):
            o.apply(v, out=w, sumsq=T.ref(2 + i))
            if i == 0:
                o.apply(w, out=y, transpose=True)
            else:
                o.apply(w, out=t, transpose=True)
                eng.axpby(1.0, y, 1.0, t, y)
    Th = T.host()
    return float(Th[2:].sum() / Th[1])


def is_identity(A):
    """Host predicate selecting the L = I branch (trips/utilities/utils.py:47-62)."""
    if isinstance(A, Identity):
        return True
    if isinstance(A, LinearOperator):
        return False
    if hasattr(A, "shape") and len(A.shape) == 2 and A.shape[0] == A.shape[1]:
        try:
            import scipy.sparse as sp
            if sp.issparse(A):
                return abs((A - sp.eye(A.shape[0])).sum()) < 1e-6
            return bool(np.allclose(np.asarray(A), np.eye(A.shape[0])))
        except Exception:
            return False
    return False
