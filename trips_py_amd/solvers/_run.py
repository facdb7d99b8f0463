"""What the iteration runs of CGLS, MRNSD and PDHG share: the operands on the device, the history of the iterates, and the two ways
of driving the recurrence — `step()` by `step()` from Python, or `run(n)` as one library call per stretch."""
import numpy as np
import torch

from .._io import History, _host, as_operator


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


class SubsetRun(IterationRun):
    """What the ordered-subsets runs (OSEMRun, SIRTRun) share.  An iteration is a PASS over the S row subsets of an
    operators.RowSubsets in its visiting order; sub-step `pos` of pass k is w = A_s x, the run's data kernel on the subset's slice of
    the subset-major data (rho over w), t = A_s^T rho, and the run's update kernel.  The first sub-step reads the pass's start iterate
    and writes the scratch xw, the middle ones update xw in place, the last one writes the history slot with x_ref = the start iterate
    and with x_true (include/trk.h).  A run gives `_data(s, w, lo, hi, part)` and `_update(s, x_in, x_ref, x_true, x_out, part)`.

    Sub-step j = (k - 1) S + pos owns the rows of partials at NP + 8 cap j.  Row k of the PASS: slots 0 and 1 are the sums of the S
    sub-steps' slots, added on the host in visiting order — RUNNING values, each subset's term taken at the sub-iterate that subset
    saw, not at one common point; slots 4 to 7 are the last sub-step's (||x_k||^2, ||x_k - x_{k-1}||^2 over the whole pass,
    ||x_k - x_true||^2, the run's count)."""

    def __init__(self, A, b, max_iter, x_true, history, what, subsets, order):
        from ..operators import RowSubsets
        sub = subsets if isinstance(subsets, RowSubsets) else RowSubsets(as_operator(A), subsets, order)
        if A is not None and tuple(A.shape) != sub.shape:
            raise ValueError(f"the subsets stand for a {sub.shape[0]} x {sub.shape[1]} operator, A is {A.shape[0]} x {A.shape[1]}")
        if sub.engine.world > 1:
            raise NotImplementedError(f"{what.split()[0]} is not built for unknowns spread over ranks (eng.world > 1)")
        bh = _host(b).reshape(-1)
        if bh.size != sub.shape[0]:
            raise ValueError(f"b has {bh.size} entries, expected {sub.shape[0]}")
        super().__init__(sub, sub.split(bh), max_iter, x_true, history, what)        # bv: subset-major
        eng, self.sub, self.nS = self.eng, sub, len(sub.ops)
        m_max, n = max(len(r) for r in sub.rows), sub.shape[1]
        self.w, self.t = eng.empty(m_max), eng.empty(n)
        self.xw = eng.empty(n) if self.nS > 1 else None
        self.cap = eng.subsets_blocks(m_max, n)
        self.NP = eng.scalars(8 * self.cap * self.max_iter * self.nS)    # zeroed: a kernel writes only its slots of its blocks' rows
        self.SS = eng.scalars(8 * self.max_iter * self.nS)               # the sub-step rows
        self.B = eng.scalars(1)                                          # ||b||^2
        eng.nrm2sq(self.bv, self.B.ref(0))
        self._final = 0

    def subset_sums(self, transpose):
        """A_s 1 for every subset, subset-major in one m-vector — or, transposed, A_s^T 1 as the rows of an [S, n] block."""
        eng, sub = self.eng, self.sub
        if transpose:
            out = eng.empty_basis(self.nS, sub.shape[1])
            for s, op in enumerate(sub.ops):
                op.apply(eng.to_vec(np.ones(op.shape[0], dtype=np.float32)), out=out[s], transpose=True)
            return out
        ones = eng.to_vec(np.ones(sub.shape[1], dtype=np.float32))
        return torch.cat([op.apply(ones) for op in sub.ops])

    def _step(self):
        sub, S = self.sub, self.nS
        self.k += 1
        for pos, s in enumerate(sub.order):
            first, last = pos == 0, pos == S - 1
            x_in = self.x_cur if first else self.xw
            x_out = self.hist.row(self.k - 1) if last else self.xw
            part = self.NP.ref(8 * self.cap * ((self.k - 1) * S + pos))
            lo, hi = int(sub.offsets[s]), int(sub.offsets[s + 1])
            w = self.w[:hi - lo]
            sub.ops[s].apply(x_in, out=w)
            self._data(s, w, lo, hi, part)                                            # rho over w
            sub.ops[s].apply(w, out=self.t, transpose=True)
            self._update(s, x_in, self.x_cur if last and not first else None, self.xt if last else None, x_out, part)
        self.x_cur = x_out

    def _subset_args(self):
        """(handles, order, row offsets) for the one-call loops, or None where a subset has no handle."""
        if not all(hasattr(o, "_h") for o in self.sub.ops):
            return None
        return [o._h for o in self.sub.ops], self.sub.order, self.sub.offsets

    def _finish(self):
        """The block partials of the passes not summed yet into their sub-step rows."""
        if self._final == self.k:
            return
        f, S = self._final, self.nS
        self.eng.finalize_batched(self.NP.ref(8 * self.cap * f * S), self.cap, 8, (self.k - f) * S, self.SS.ref(8 * f * S), 8)
        self._final = self.k

    def substep_rows(self, k_from=1):
        """[k - k_from + 1, S, 8] on the host: the rows of the sub-steps of passes k_from .. k, in visiting order (host sync)."""
        self._finish()
        return self.SS.host(8 * (k_from - 1) * self.nS, 8 * self.k * self.nS).reshape(-1, self.nS, 8)

    def rows(self, k_from=1):
        """The rows of passes k_from .. k on the host."""
        sr = self.substep_rows(k_from)
        out = sr[:, -1, :].copy()
        out[:, :4] = 0.0
        for pos in range(self.nS):                                                    # in visiting order, always the same association
            out[:, :2] += sr[:, pos, :2]
        return out

    def row(self, k):
        """Pass row k, 1-based (host sync); k = self.k reads back that pass alone."""
        return self.rows(k)[0]

    def b_norm(self):
        return float(np.sqrt(self.B.host(0, 1)[0]))
