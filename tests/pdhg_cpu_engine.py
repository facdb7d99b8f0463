"""TEST-ONLY: tests/cpu_engine.py's engine with the PDHG entry points of the HIP engine (pdhg_blocks, pdhg_dual_p, pdhg_dual_q,
pdhg_primal) restated through tests/pdhg_cases.py, so that PDHG()'s host logic runs without a GPU.  One "block": every kernel writes
its slots of ONE row of 8 partials.  It has no fused forms and no pdhg_iterate, so PDHGRun takes the generic path and run() steps
from Python."""
import numpy as np
import torch

import pdhg_cases as C
from cpu_engine import CpuEngine


def _set(t, a):
    t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))


def _slots(ref, slots, vals):
    s, i = ref
    for j, v in zip(slots, vals):
        s.a[i + j] = v


class PdhgCpuEngine(CpuEngine):
    def pdhg_blocks(self, m, n, rows, fused_handle=None):
        return 1

    def pdhg_dual_p(self, sigma, w, b, p, partials, capacity):
        pn, s0, s2 = C.dual_p_f32(sigma, w.numpy(), b.numpy(), p.numpy().copy())
        _set(p, pn)
        _slots(partials, (0, 2), (s0, s2))
        return 1

    def pdhg_dual_q(self, sigma, lam, u, q, partials, capacity):
        qn, s1, s3 = C.dual_q_f32(sigma, lam, u.numpy(), q.numpy().copy())
        _set(q, qn)
        _slots(partials, (1, 3), (s1, s3))
        return 1

    def pdhg_primal(self, tau, lo, hi, x, z, v, x_new, xbar, x_true, partials, capacity):
        xn, xb, tail = C.primal_f32(tau, lo, hi, x.numpy().copy(), z.numpy(), None if v is None else v.numpy(),
                                    None if x_true is None else x_true.numpy())
        _set(x_new, xn)
        _set(xbar, xb)
        _slots(partials, (4, 5, 6, 7), tail)
        return 1
