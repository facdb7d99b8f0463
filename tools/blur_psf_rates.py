"""Kernel time of the blur for PSFs beyond the slide / strip shapes (the LDS tile kernel, csrc/blur_tile.hip), against another
build of the package — the parent commit, where every such PSF ran on k_blur_generic.

    python tools/blur_psf_rates.py [out.json] [--baseline-root DIR] [--rounds M] [--reps R] [--sizes 1024 4096]

Cases: 10x10 Gaussian, 21x21 defocus (reflect and constant), 31x31 Gaussian, 31x31 motion at 30 degrees, 63x63 defocus, 64x40
random; forward and "transpose"; N^2 images.  Times come from the events libtrk records around the blur's own kernel (trk_timer_*,
include/trk.h).  Every build is measured in worker processes of its own (`--worker`, one at a time: this process never opens the
GPU), and the rounds ALTERNATE between the builds, so that drift of a shared machine spreads over both.  A slow case (the
generic kernel at 63x63 on 4096^2 takes seconds per apply) gets as many repeats as fit a per-case time budget, at least two.

Each entry carries the algorithmic FLOPs (2 kh kw n, or 2 (kh + kw) n for the separable form), the bytes (8 n), the floor
max(FLOPs / 157.3e12, bytes / 8e12) with the bound that binds, the medians and p10 / p90 of both builds, and whether this build
is faster than the baseline by more than the baseline's own p10-p90 spread.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NBUF = 4
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8e12
PATH_NAMES = {0: "auto", 1: "slide", 2: "strip", 3: "tile", 4: "generic"}


def cases():
    sys.path.insert(0, REPO)
    from trips_py_amd.problems import defocus_psf, gauss_psf, motion_psf
    rng = np.random.default_rng(6440)
    r = rng.random((64, 40))
    return [("gauss10x10", "reflect", gauss_psf((10, 10), 2.0)[0]),
            ("defocus21x21", "reflect", defocus_psf((21, 21), 9)[0]),
            ("defocus21x21", "constant", defocus_psf((21, 21), 9)[0]),
            ("gauss31x31", "reflect", gauss_psf((31, 31), 5.0)[0]),
            ("motion31x31_30deg", "reflect", motion_psf((31, 31), 24, 30)[0]),
            ("defocus63x63", "reflect", defocus_psf((63, 63), 28)[0]),
            ("random64x40", "reflect", r / r.sum())]


# ------------------------------------------------------------------------------------------------ worker (one build, one round)
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

    def close(self):
        self.lib.trk_timer_destroy(self.h)


def worker(a):
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from trips_py_amd.operators import Blur2D
    data = np.load(a.cases)
    names = [str(s) for s in data["names"]]
    modes = [str(s) for s in data["modes"]]
    out = {"root": os.path.abspath(a.root), "device": None, "times_ms": {}, "path": {}, "separable": {}}
    for N in a.sizes:
        n = N * N
        X = Y = None
        for i, (name, mode) in enumerate(zip(names, modes)):
            A = Blur2D(data[f"psf{i}"], N, N, boundary=mode)
            eng = A.engine
            out["device"] = torch.cuda.get_device_name(0)
            if X is None:
                g = torch.Generator(device="cpu").manual_seed(0)
                X = [torch.randn(n, generator=g).to(eng.device) for _ in range(NBUF)]
                Y = [torch.empty(n, device=eng.device) for _ in range(NBUF)]
            if hasattr(A, "path"):
                path, sep = ctypes.c_int(), ctypes.c_int()
                assert eng.lib.trk_blur2d_path(A._h, ctypes.byref(path), ctypes.byref(sep)) == 0
                out["path"][f"{name}|{mode}|{N}"] = PATH_NAMES[path.value]
                out["separable"][f"{name}|{mode}|{N}"] = bool(sep.value)
            for tr in (False, True):
                with Timer(A, 1, int(tr)) as t:                       # warm-up: the code object, and what one apply costs
                    A.apply(X[0], out=Y[0], transpose=tr)
                    first = t.read()[0]
                t.close()
                reps = int(max(2, min(a.reps, a.budget_ms / max(first, 1e-3))))
                with Timer(A, reps, int(tr)) as t:
                    for r in range(reps):
                        A.apply(X[r % NBUF], out=Y[(r + 1) % NBUF], transpose=tr)
                    ms = t.read()
                t.close()
                assert len(ms) == reps
                out["times_ms"][f"{name}|{mode}|{N}|{'adj' if tr else 'fwd'}"] = ms
            del A
        del X, Y
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out), flush=True)


# ------------------------------------------------------------------------------------------------ driver
def run_worker(root, cases_file, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--cases", cases_file, "--reps", str(a.reps),
           "--budget-ms", str(a.budget_ms), "--sizes"] + [str(s) for s in a.sizes]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.worker_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"worker for {root} ended with status {r.returncode}: nothing further is run")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def stats(ms):
    v = np.asarray(ms, dtype=np.float64) * 1e3
    return {"us_median": round(float(np.median(v)), 2), "us_p10": round(float(np.percentile(v, 10)), 2),
            "us_p90": round(float(np.percentile(v, 90)), 2), "samples": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--baseline-root", default=None, help="a tree with another build of trips_py_amd (the parent commit)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20, help="applies per case, direction and round, at most")
    ap.add_argument("--budget-ms", type=float, default=400.0, help="kernel time per case, direction and round (at least 2 applies)")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--worker-timeout", type=float, default=420.0)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=REPO)
    ap.add_argument("--cases", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cs = cases()
    with tempfile.TemporaryDirectory() as tmp:
        cases_file = os.path.join(tmp, "cases.npz")
        np.savez(cases_file, names=np.array([c[0] for c in cs]), modes=np.array([c[1] for c in cs]),
                 **{f"psf{i}": c[2] for i, c in enumerate(cs)})
        roots = [("this", REPO)] + ([("baseline", a.baseline_root)] if a.baseline_root else [])
        times = {k: {} for k, _ in roots}
        meta = {}
        for rnd in range(a.rounds):
            for key, root in roots:
                res = run_worker(root, cases_file, a)
                meta[key] = res
                for case, ms in res["times_ms"].items():
                    times[key].setdefault(case, []).extend(ms)
                print(f"round {rnd + 1}/{a.rounds}: {key} done", flush=True)
    entries = []
    for name, mode, psf in cs:
        kh, kw = psf.shape
        for N in a.sizes:
            ck = f"{name}|{mode}|{N}"
            sep = meta["this"]["separable"][ck]
            n = float(N) * N
            flops = 2.0 * (kh + kw if sep else kh * kw) * n
            byts = 8.0 * n
            tf, tb = flops / PEAK_FLOPS, byts / PEAK_BYTES
            for d in ("fwd", "adj"):
                e = {"case": name, "psf": [kh, kw], "mode": mode, "N": N, "direction": d, "path": meta["this"]["path"][ck],
                     "separable": sep, "flops": flops, "bytes": byts, "floor_us": round(max(tf, tb) * 1e6, 2),
                     "bound": "compute" if tf >= tb else "memory", "this": stats(times["this"][f"{ck}|{d}"])}
                e["fraction_of_floor"] = round(e["floor_us"] / e["this"]["us_median"], 3)
                line = f"{name:18s} {mode:8s} {N:5d} {d} {e['path']:7s} {e['this']['us_median']:11.1f} us (floor {e['floor_us']:8.1f}, {e['bound']})"
                if a.baseline_root:
                    b = stats(times["baseline"][f"{ck}|{d}"])
                    e["baseline"] = b
                    e["speedup"] = round(b["us_median"] / e["this"]["us_median"], 2)
                    e["faster_by_more_than_baseline_spread"] = bool(b["us_median"] - e["this"]["us_median"] > b["us_p90"] - b["us_p10"])
                    line += f"   baseline {b['us_median']:12.1f} us [{b['us_p10']:.1f}, {b['us_p90']:.1f}]  x{e['speedup']:.1f}"
                print(line)
                entries.append(e)
    res = {"what": "blur kernel time per PSF beyond the slide / strip shapes (trk_timer events around the kernel), this build against a "
                   "baseline build in alternating rounds of separate processes",
           "device": meta["this"]["device"], "rounds": a.rounds, "reps_at_most": a.reps, "budget_ms": a.budget_ms, "buffers": NBUF,
           "peak_flops": PEAK_FLOPS, "peak_bytes_per_s": PEAK_BYTES, "baseline": "the parent commit" if a.baseline_root else None,
           "entries": entries}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
