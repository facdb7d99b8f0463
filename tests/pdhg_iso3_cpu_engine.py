"""TEST-ONLY: tests/pdhg_iso_cpu_engine.py's engine with the unfused space-time isotropic dual (pdhg_blocks_iso3, pdhg_dual_q_iso3)
restated through tests/pdhg_iso3_cases.py, so that PDHG(tv='iso3')'s host logic runs without a GPU.  No fused form and no
pdhg_iterate_iso3: PDHGRun takes the unfused path and run() steps from Python."""
import pdhg_iso3_cases as T
from pdhg_cpu_engine import _set, _slots
from pdhg_iso_cpu_engine import PdhgIsoCpuEngine


class PdhgIso3CpuEngine(PdhgIsoCpuEngine):
    def pdhg_blocks_iso3(self, m, n, rows, N, frames, fused_handle=None):
        return 1

    def pdhg_dual_q_iso3(self, N, frames, sigma, lam, u, q, partials, capacity):
        qn, s1, s3 = T.dual_q_iso3_f32(N, frames, sigma, lam, u.numpy(), q.numpy().copy())
        _set(q, qn)
        _slots(partials, (1, 3), (s1, s3))
        return 1
