"""TEST-ONLY: tests/cpu_engine.py's engine with the MLEM entry points of the HIP engine (mlem_blocks, mlem_sinv, mlem_ratio,
mlem_update) restated through tests/mlem_cases.py, so that MLEM()'s host logic runs without a GPU.  One "block": every row of
partials is one row of 8.  It has no mlem_iterate, so MLEMRun.run() steps from Python."""
import numpy as np
import torch

import mlem_cases as C
from cpu_engine import CpuEngine, _put


def _f32(t):
    return t.numpy()


def _set(t, a):
    t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))


def _at(ref, off):
    return (ref[0], ref[1] + off)


class MlemCpuEngine(CpuEngine):
    def mlem_blocks(self, m, n):
        return 1

    def mlem_sinv(self, s, sinv):
        _set(sinv, C.sinv_f32(_f32(s).copy()))

    def mlem_ratio(self, bg, w, b, rho, partials, capacity):
        r = C.ratio_f32(_f32(w).copy(), _f32(bg) if isinstance(bg, torch.Tensor) else bg, _f32(b))
        _set(rho, r["rho"])
        _put(partials, [r["kl"], r["rr"]])
        return 1

    def mlem_update(self, x, t, sinv, x_true, x_new, partials, capacity):
        u = C.update_f32(_f32(x).copy(), _f32(t), _f32(sinv), None if x_true is None else _f32(x_true))
        _set(x_new, u["x"])
        _put(_at(partials, 4), [u["xx"], u["dd"], u["ee"], float(u["zeros"])])
        return 1
