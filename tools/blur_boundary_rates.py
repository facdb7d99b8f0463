"""Kernel time of the 4096^2 9x9 blur (the sliding kernel, k_blur_slide) for every boundary mode, forward and "transpose".

    python tools/blur_boundary_rates.py [out.json] [--reps R] [--rounds M]

Times come from the events libtrk records around the blur's own kernel (trk_timer_*, include/trk.h).  The modes are measured in
interleaved rounds (reflect, constant, nearest, mirror, wrap, reflect, ...) so that drift of the shared machine spreads over
all of them, and every apply reads and writes a different buffer pair out of 4 (512 MB, twice the memory-side cache) so that no
mode finds its operand cached.  Prints one line per mode and writes the table as JSON.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from trips_py_amd.operators import BOUNDARY_MODES, Blur2D  # noqa: E402
from trips_py_amd.problems import gauss_psf  # noqa: E402

N, K, NBUF = 4096, 9, 4


class Timer:
    def __init__(self, op, cap, which):
        self.lib, self.op, self.cap, self.which = op.engine.lib, op, cap, which
        self.h = ctypes.c_void_p()
        assert self.lib.trk_timer_create(cap, ctypes.byref(self.h)) == 0, self.lib.trk_last_error()

    def __enter__(self):
        self.lib.trk_timer_reset(self.h)
        assert self.lib.trk_op_set_timer(self.op._h, self.h, self.which) == 0
        return self

    def __exit__(self, *exc):
        self.lib.trk_op_set_timer(self.op._h, None, 0)

    def read(self):
        buf = (ctypes.c_float * self.cap)()
        n = ctypes.c_int()
        assert self.lib.trk_timer_read(self.h, buf, self.cap, ctypes.byref(n)) == 0, self.lib.trk_last_error()
        return [float(v) for v in buf[:n.value]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--reps", type=int, default=20, help="applies per mode, direction and round")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    psf, _ = gauss_psf((K, K), (3, 3))
    modes = list(BOUNDARY_MODES)
    ops = {m: Blur2D(psf, N, N, boundary=m) for m in modes}
    eng = ops["reflect"].engine
    g = torch.Generator(device="cpu").manual_seed(0)
    X = [torch.randn(N * N, generator=g).to(eng.device) for _ in range(NBUF)]
    Y = [torch.empty(N * N, device=eng.device) for _ in range(NBUF)]
    timers = {(m, tr): Timer(ops[m], a.reps, int(tr)) for m in modes for tr in (False, True)}
    for m in modes:                                             # warm-up: code objects, every buffer touched
        for tr in (False, True):
            for i in range(NBUF):
                ops[m].apply(X[i], out=Y[i], transpose=tr)
    torch.cuda.synchronize()
    ms = {(m, tr): [] for m in modes for tr in (False, True)}
    for _ in range(a.rounds):
        for m in modes:
            for tr in (False, True):
                with timers[(m, tr)] as t:
                    for r in range(a.reps):
                        ops[m].apply(X[r % NBUF], out=Y[(r + 1) % NBUF], transpose=tr)
                ms[(m, tr)] += t.read()
    bytes_per_apply = 8.0 * N * N
    rows = []
    ref = {tr: float(np.median(ms[("reflect", tr)])) for tr in (False, True)}
    for m in modes:
        row = {"mode": m}
        for tr, key in ((False, "fwd"), (True, "adj")):
            v = np.array(ms[(m, tr)]) * 1e3
            med = float(np.median(v))
            row[key + "_us_median"] = round(med, 2)
            row[key + "_us_p10_p90"] = [round(float(np.percentile(v, 10)), 2), round(float(np.percentile(v, 90)), 2)]
            row[key + "_vs_reflect"] = round(med / (ref[tr] * 1e3), 3)
            row[key + "_TBps"] = round(bytes_per_apply / (med * 1e-6) / 1e12, 2)
        rows.append(row)
        print(f"{m:9s} fwd {row['fwd_us_median']:7.2f} us ({row['fwd_vs_reflect']:.3f}x reflect, {row['fwd_TBps']:.2f} TB/s)   "
              f"adj {row['adj_us_median']:7.2f} us ({row['adj_vs_reflect']:.3f}x)")
    res = {"what": f"k_blur_slide kernel time, {N}^2 fp32, {K}x{K} Gaussian, per boundary mode (trk_timer events around the kernel)",
           "device": torch.cuda.get_device_name(0), "reps_per_round": a.reps, "rounds": a.rounds, "buffers": NBUF,
           "bytes_per_apply": bytes_per_apply, "modes": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
