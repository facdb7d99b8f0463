"""TEST-ONLY: tests/mlem_cpu_engine.py's engine with the ordered-subsets entry points of the HIP engine (subsets_blocks, osem_update,
sirt_residual, sirt_update) restated through tests/os_cases.py, so that the host logic of OSEM() and SIRT() runs without a GPU.
One "block": every row of partials is one row of 8.  It has no osem_iterate / sirt_iterate, so the runs step from Python."""
import os_cases as C
from cpu_engine import _put
from mlem_cpu_engine import MlemCpuEngine, _at, _f32, _set


def _opt(t):
    return None if t is None else _f32(t)


class OsCpuEngine(MlemCpuEngine):
    def subsets_blocks(self, m_max, n):
        return 1

    def osem_update(self, x, t, sinv, x_ref, x_true, x_new, partials, capacity):
        u = C.osem_update_f32(_f32(x).copy(), _f32(t), _f32(sinv), _opt(x_ref), _opt(x_true))
        _set(x_new, u["x"])
        _put(_at(partials, 4), [u["xx"], u["dd"], u["ee"], float(u["count"])])
        return 1

    def sirt_residual(self, rinv, w, b, rho, partials, capacity):
        r = C.sirt_residual_f32(_f32(w).copy(), _f32(b), _opt(rinv))
        _set(rho, r["rho"])
        _put(partials, [r["dd"], r["wd"]])
        return 1

    def sirt_update(self, omega, lo, hi, x, t, cinv, x_ref, x_true, x_new, partials, capacity):
        u = C.sirt_update_f32(omega, lo, hi, _f32(x).copy(), _f32(t), _opt(cinv), _opt(x_ref), _opt(x_true))
        _set(x_new, u["x"])
        _put(_at(partials, 4), [u["xx"], u["dd"], u["ee"], float(u["count"])])
        return 1
