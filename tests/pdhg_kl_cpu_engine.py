"""TEST-ONLY: tests/pdhg_iso3_cpu_engine.py's engine with the Kullback-Leibler dual of p (pdhg_dual_p_kl) restated through
tests/pdhg_kl_cases.py, so that PDHG(data='kl')'s host logic runs without a GPU for every tv.  No fused form and no
pdhg_iterate_data: PDHGRun takes the unfused path and run() steps from Python."""
import torch

import pdhg_kl_cases as K
from pdhg_cpu_engine import _set, _slots
from pdhg_iso3_cpu_engine import PdhgIso3CpuEngine


class PdhgKlCpuEngine(PdhgIso3CpuEngine):
    def pdhg_dual_p_kl(self, sigma, bg, w, b, p, partials, capacity):
        pn, s0, s2 = K.dual_p_kl_f32(sigma, bg.numpy() if isinstance(bg, torch.Tensor) else bg, w.numpy(), b.numpy(), p.numpy().copy())
        _set(p, pn)
        _slots(partials, (0, 2), (s0, s2))
        return 1
