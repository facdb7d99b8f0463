"""TEST-ONLY: tests/pdhg_cpu_engine.py's engine with the unfused isotropic dual (pdhg_blocks_iso, pdhg_dual_q_iso) restated through
tests/pdhg_iso_cases.py, so that PDHG(tv='iso')'s host logic runs without a GPU.  No fused form and no pdhg_iterate_iso: PDHGRun
takes the generic path and run() steps from Python."""
import pdhg_iso_cases as I
from pdhg_cpu_engine import PdhgCpuEngine, _set, _slots


class PdhgIsoCpuEngine(PdhgCpuEngine):
    def pdhg_blocks_iso(self, m, n, rows, N, frames, fused_handle=None):
        return 1

    def pdhg_dual_q_iso(self, N, frames, sigma, lam, u, q, partials, capacity):
        qn, s1, s3 = I.dual_q_iso_f32(N, frames, sigma, lam, u.numpy(), q.numpy().copy())
        _set(q, qn)
        _slots(partials, (1, 3), (s1, s3))
        return 1
