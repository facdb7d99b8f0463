"""What the iteration runs of CGLS, MRNSD and PDHG share: the operands on the device, the history of the iterates, and the two ways
of driving the recurrence — `step()` by `step()` from Python, or `run(n)` as one library call per stretch."""
from .._io import History, as_operator


class _ShiftedRows:
    """A [rows, n] device block seen `shift` rows further on: what the C iteration loops take when iterate j is to land in
    ring slot (j + shift) instead of row j (they only ask for the base address and the row stride)."""

    def __init__(self, t, shift):
        self.t, self.shift = t, int(shift)

    def data_ptr(self):
        return self.t.data_ptr() + self.shift * self.t.stride(0) * self.t.element_size()

    def stride(self, dim):
        return self.t.stride(dim)


class IterationRun:
    """A recurrence as an object.  A solver's run sets `x_cur` to its start and gives `_step()`, one iteration enqueued from Python
    that writes iterate k - 1 (0-based) into `hist.row(k - 1)` and leaves it in `x_cur`, and, where the library has the loop in C,
    `_c_loop()`."""

    def __init__(self, A, b, max_iter, x_true, history, what):
        self.A = A = as_operator(A)
        self.eng = eng = A.engine
        m, n = A.shape
        self.max_iter = max_iter = int(max_iter)
        self.bv = eng.to_vec(b, m)
        self.xt = None if x_true is None else eng.to_vec(x_true, n)
        self.hist = History(eng, history, max_iter, n, what)       # True / False / stride / 'host' / '<file>.npy'
        self.X = self.hist.X
        self.k = 0

    def slot(self, k):
        """The device row holding iterate k (0-based)."""
        return self.X[self.hist.slot(k)]

    def step(self):
        self._step()
        self.hist.pushed(self.k - 1)

    def _c_loop(self):
        """`call(k_first, n, X, keep)` that enqueues iterations k_first .. k_first + n - 1 (1-based) in one library call, starting
        from `x_cur` and writing iterate j to row j - 1 of X (keep) or to row (j - 1) & 1 (not keep) — or None where this run can
        only be stepped."""
        return None

    def run(self, n_steps):
        """Enqueue `n_steps` iterations (at most what is left of max_iter): through `_c_loop()` where there is one, else `step()` by
        `step()`."""
        n_steps = min(int(n_steps), self.max_iter - self.k)
        if n_steps <= 0:
            return
        call = self._c_loop()
        if call is None:
            for _ in range(n_steps):
                self.step()
        else:
            self._run_c_loop(n_steps, call)

    def _run_c_loop(self, n_steps, call):
        """All at once, or, when the history is streamed through a ring of device slots, in chunks that stay inside one half of the
        ring (the copies of one half drain while the other half is being written) and do not cross its end."""
        h = self.hist
        while n_steps > 0:
            k0 = self.k
            if h.mode != "stream":
                c = n_steps
                call(k0 + 1, c, self.X, 1 if h.mode == "device" else 0)
            else:
                c = min(n_steps, h.R // 2, h.R - k0 % h.R)
                for j in range(c):
                    h.row(k0 + j)                                  # the slots' previous copies must be out
                call(k0 + 1, c, _ShiftedRows(self.X, k0 % h.R - k0), 1)
                for j in range(c):
                    h.pushed(k0 + j)
            self.k += c
            n_steps -= c
            self.x_cur = self.slot(self.k - 1)                     # what the next chunk starts from
