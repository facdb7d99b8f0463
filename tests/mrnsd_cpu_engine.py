"""TEST-ONLY: tests/cpu_engine.py's engine with the three MRNSD entry points of the HIP engine (mrnsd_init, mrnsd_update,
mrnsd_finish) restated through tests/mrnsd_cases.py, so that MRNSD()'s host logic runs without a GPU.  One "block": every set of
partials has one entry.  It has no mrnsd_iterate, so MRNSDRun.run() steps from Python."""
import numpy as np
import torch

import mrnsd_cases as C
from cpu_engine import CpuEngine, _get, _put


def _f32(t):
    return t.numpy()


def _set(t, a):
    t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))


def _src_sum(ref, n):
    return float(np.sum(np.atleast_1d(_get(ref, n))))


def _src_min(ref, n):
    return float(np.min(np.atleast_1d(_get(ref, n))))


def _at(ref, off):
    return (ref[0], ref[1] + off)


class MrnsdCpuEngine(CpuEngine):
    def mrnsd_init(self, x0, g, r, s, gb_out, gb_capacity, S0):
        x, gv, rv = _f32(x0), _f32(g), _f32(r)
        sv = -(x * gv)
        _set(s, sv)
        gamma = float(-np.dot(gv.astype(np.float64), sv.astype(np.float64)))
        bound = C.bound_of(x, sv)
        _put(gb_out, gamma)
        _put(_at(gb_out, gb_capacity), bound)
        _put(S0, [gamma, bound, float(np.dot(rv.astype(np.float64), rv.astype(np.float64)))])
        return 1

    def mrnsd_update(self, gamma, gamma_n, bound, bound_n, unorm, unorm_n, x, x_new, g, s, z, r, u, x_true, gb_out, gb_capacity, row,
                     pub_gb, partials, capacity):
        ga, bd, uu = _src_sum(gamma, gamma_n), _src_min(bound, bound_n), _src_sum(unorm, unorm_n)
        st = C.update_f32(ga, bd, uu, _f32(x).copy(), _f32(g).copy(), _f32(s).copy(), _f32(z), _f32(r).copy(), _f32(u),
                          None if x_true is None else _f32(x_true))
        _set(x_new, st["x"])
        _set(g, st["g"])
        _set(s, st["s"])
        _set(r, st["r"])
        _put(gb_out, st["gamma"])
        _put(_at(gb_out, gb_capacity), st["bound"])
        _put(row, [uu, st["alpha"]])
        if pub_gb is not None:
            _put(pub_gb, [ga, bd])
        _put(partials, [st["xx"], st["dd"], st["ee"], st["rr"]])
        return 1

    def mrnsd_finish(self, gamma, gamma_n, bound, bound_n, out):
        _put(out, [_src_sum(gamma, gamma_n), _src_min(bound, bound_n)])
