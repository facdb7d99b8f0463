"""Forming the iterates of the hybrid solvers: x_i = V y_i written into its row of the history, ||x_i - x_true||^2 left as raw block
partials of the kernel that forms x_i and summed once after the loop."""
import numpy as np

CAPACITY = 1024          # places for block partials per iterate


class Iterates:
    """Owns the history, the basis V (a krylov.DeviceBasis), E (E[0] = ||x_true||^2, E[i] = ||x_i - x_true||^2), the partials EP and
    their count per iterate `n_ep`, the newest iterate `x_dev` and the number formed `done`; one method per way an iterate's coefficients
    arrive.  `fixed_stride`: the iterates come from kernels with different partial counts (Hybrid_LSQR's recurrence: the adjoint's tiles
    or the update's own grid), so each owns all CAPACITY zero-initialised places and all of them are summed."""

    def __init__(self, eng, hist, basis, xt, rows, fixed_stride=False):
        self.eng, self.hist, self.V, self.xt, self.fixed_stride = eng, hist, basis, xt, fixed_stride
        self.E = eng.scalars(rows + 1)
        if xt is not None:
            eng.nrm2sq(xt, self.E.ref(0))
            eng.allreduce(self.E, 0, 1)
        self.err_fused = xt is not None and hasattr(eng, "gemv_n_err")
        self.EP = eng.scalars(CAPACITY * rows) if self.err_fused else None
        self.n_ep, self.done, self.x_dev = 0, 0, None

    def row(self):
        """The device vector the next iterate is to be written into."""
        return self.hist.row(self.done)

    def partials(self):
        """Where the kernel that writes the next iterate leaves its partials of ||x - x_true||^2 (None where none are kept)."""
        return self.EP.ref((CAPACITY if self.fixed_stride else self.n_ep) * self.done) if self.err_fused else None

    def wrote(self, x, got):
        """A kernel already wrote the next iterate into `x` (= row()) and left `got` partials in partials()."""
        if self.err_fused:
            self.n_ep = got
        self.x_dev = x
        self.hist.pushed(self.done)
        self.done += 1

    def from_device_y(self, k, y):
        """x = V[:k]^T y with y on the device (a scalars ref)."""
        eng, x = self.eng, self.row()
        if self.err_fused:
            return self.wrote(x, eng.gemv_n_err(self.V.data, k, y, x, self.xt, self.partials(), CAPACITY))
        eng.gemv_n(self.V.data, k, y, x)
        self.wrote(x, 0)
        if self.xt is not None:
            eng.diff_nrm2sq(x, self.xt, self.E.ref(self.done))

    def from_host_y(self, k, yk):
        """The same with y on the host (a contiguous float64 array): the coefficients ride in the launch's arguments."""
        x = self.row()
        xt = (self.xt, self.partials(), CAPACITY) if self.xt is not None else ()
        self.wrote(x, self.eng.gemv_n_hosty(self.V.data, k, yk, x, *xt))

    def relError(self):
        """info['relError'] of the iterates formed."""
        eng, E = self.eng, self.E
        if self.err_fused:
            eng.finalize_batched(self.EP.ref(0), CAPACITY if self.fixed_stride else self.n_ep, 1, self.done, E.ref(1), 1)
        eng.allreduce(E, 1, self.done + 1)
        e = E.host(0, self.done + 1)
        return list(np.sqrt(e[1:] / e[0]))
