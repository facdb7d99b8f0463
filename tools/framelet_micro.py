"""The framelet analysis operator alone, matrix-free (csrc/framelet2d.hip) next to its CSR form (csrc/spmv.hip): kernel time per apply
warm and cold, GB/s of the operator's own (1 + (2l+1)^2) n m 4 bytes, and that rate as a fraction of the chip's best cold copy
(6.88 TB/s, profiles/r06/copy_sweep.txt); then one MMGKS solve with either form as the regulariser.

warm: one pair of vectors back to back.  cold: sets of vectors in rotation, >= 1 GB in all, so that nothing an apply touches is
left in the 256 MB memory-side cache from the apply before (the CSR form's matrix, 350 MB per direction at 512^2, never is).

    python tools/framelet_micro.py            # everything
    python tools/framelet_micro.py quick      # 512^2 both forms only (a rehearsal)
    python tools/framelet_micro.py stencil 512 2048   # the stencil form alone at these sizes, l = 2
"""
import ctypes
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
from trips_py_amd.operators import Blur2D, create_framelet_operator  # noqa: E402
from trips_py_amd.problems import add_noise, gauss_psf, synthetic_image  # noqa: E402

COPY_RATE = 6.88e12          # bytes / s, the best cold 1:1 copy (profiles/r06/copy_sweep.txt)
ROTATION_BYTES = 1 << 30
REPS = 20


class KernelTimer:
    """hipEvent pairs the library records around the operator's main kernel (trk_timer_*, include/trk.h)."""

    def __init__(self, op, capacity):
        self.lib, self.op, self.cap = op.engine.lib, op, capacity
        self.h = ctypes.c_void_p()
        assert self.lib.trk_timer_create(capacity, ctypes.byref(self.h)) == 0, self.lib.trk_last_error()

    def __enter__(self):
        self.lib.trk_timer_reset(self.h)
        assert self.lib.trk_op_set_timer(self.op._h, self.h, 2) == 0
        return self

    def __exit__(self, *exc):
        self.lib.trk_op_set_timer(self.op._h, None, 0)

    def median_us(self):
        buf, n = (ctypes.c_float * self.cap)(), ctypes.c_int()
        assert self.lib.trk_timer_read(self.h, buf, self.cap, ctypes.byref(n)) == 0, self.lib.trk_last_error()
        return float(np.median(np.array(buf[:n.value], dtype=np.float64))) * 1e3


def timed(W, fns):
    """(call, kernel) in us of the applies in `fns`, run in order after one untimed pass over them.  call: the mean between two
    stream events around the whole run - what a loop of Python-level applies gets; kernel: the median of the event pairs the library
    puts around each apply's kernel, in a second run.  The two are different statistics of different runs: back to back, a launch
    overlaps the tail of the one before, and an event pair adds its own ~2 us, so `call` can come out below `kernel`."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for fn in fns:
        fn()
    e1.record()
    torch.cuda.synchronize()
    tm = KernelTimer(W, len(fns))
    with tm:
        for fn in fns:
            fn()
        torch.cuda.synchronize()
        kernel = tm.median_us()
    W.engine.lib.trk_timer_destroy(tm.h)
    return e0.elapsed_time(e1) / len(fns) * 1e3, kernel


def time_op(form, n, m, l, W):
    dev = W.engine.device
    rows, cols = W.shape
    alg = 4.0 * (rows + cols)
    sets = max(2, int(np.ceil(ROTATION_BYTES / alg)))
    xs = [torch.rand(cols, device=dev) for _ in range(sets)]
    ys = [torch.empty(rows, device=dev) for _ in range(sets)]
    zs = [torch.empty(cols, device=dev) for _ in range(sets)]
    for k in range(sets):                                       # (the transpose reads what the forward wrote)
        W.apply(xs[k], out=ys[k])
    out = {}
    for tag, warm, cold in (("fwd", [lambda: W.apply(xs[0], out=ys[0])] * REPS,
                             [(lambda k=k: W.apply(xs[k % sets], out=ys[k % sets])) for k in range(max(REPS, sets))]),
                            ("adj", [lambda: W.apply(ys[0], out=zs[0], transpose=True)] * REPS,
                             [(lambda k=k: W.apply(ys[k % sets], out=zs[k % sets], transpose=True)) for k in range(max(REPS, sets))])):
        for temp, fns in (("warm", warm), ("cold", cold)):
            call, us = timed(W, fns)
            out[tag, temp] = us
            rate = alg / (us * 1e-6)
            note = f"   ({sets} sets in rotation)" if temp == "cold" else ""
            print(f"{form:>7} {n:5d} x {m:5d} l={l}  {tag} {temp}  kernel {us:9.1f} us  {rate * 1e-9:8.1f} GB/s  {rate / COPY_RATE:6.3f} of the copy rate"
                  f"   per call {call:9.1f} us{note}", flush=True)
    return out


def both_forms(N, l):
    t0 = time.time()
    F = create_framelet_operator(N, N, l, matrix_free=True)
    t1 = time.time()
    A = create_framelet_operator(N, N, l)
    t2 = time.time()
    print(f"# {N}^2 l={l}: set-up on the host {t1 - t0:.2f} s matrix-free, {t2 - t1:.2f} s CSR ({A.matrix.nnz} non-zeros)", flush=True)
    tf, ta = time_op("stencil", N, N, l, F), time_op("csr", N, N, l, A)
    for key in (("fwd", "warm"), ("fwd", "cold"), ("adj", "warm"), ("adj", "cold")):
        print(f"# {N}^2 l={l} {key[0]} {key[1]}: kernel time CSR / stencil = {ta[key] / tf[key]:.2f} x", flush=True)
    return F, A


def mmgks_rate(N, forms):
    from trips_py_amd.solvers import MMGKS
    psf, _ = gauss_psf((9, 9), (3, 3))
    xt = synthetic_image(N, 0).reshape(-1, 1)
    A = Blur2D(psf, N, N)
    b, _ = add_noise(A @ xt, 0.01, 1)
    for name, L in forms:
        for rep in range(2):                                    # (the first solve warms up code objects and allocations)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x, info = MMGKS(A, b, L, 2, 1, 3, 10, 1e-2, xt)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        print(f"MMGKS {N}^2 blur 9x9, L = framelets l=2 as {name}: projection_dim=3, n_iter=10: {info['its'] / dt:8.2f} iterations/s "
              f"({dt * 1e3:.1f} ms), relError[-1] {info['relError'][-1]:.6f}", flush=True)


def main():
    quick = len(sys.argv) > 1 and sys.argv[1] == "quick"
    if len(sys.argv) > 2 and sys.argv[1] == "stencil":
        for N in sys.argv[2:]:
            time_op("stencil", int(N), int(N), 2, create_framelet_operator(int(N), int(N), 2, matrix_free=True))
            torch.cuda.empty_cache()
        return
    print(f"# device {torch.cuda.get_device_name(0)}; bytes of an apply = (1 + (2l+1)^2) n m 4; copy rate {COPY_RATE * 1e-12:.2f} TB/s", flush=True)
    both_forms(512, 2)
    if quick:
        return
    F, A = both_forms(1024, 2)
    mmgks_rate(1024, (("stencil", F), ("csr", A)))
    del F, A
    torch.cuda.empty_cache()
    for N, l in ((2048, 2), (4096, 2), (1024, 3)):
        time_op("stencil", N, N, l, create_framelet_operator(N, N, l, matrix_free=True))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
