"""MRNSD iteration rates on the device: a record, not a gate.

    python tools/mrnsd_rate.py [--out profiles/mrnsd/mrnsd_rates.json] [--steps K] [--warmup W]

Seeded data; per case W warm-up iterations, then K iterations between two device events, the window closed by a synchronise;
the median of three windows.  Cases: the 9x9 reflect Gaussian blur at 4096^2 and 512^2, the parallel-beam projector 512^2 x 180.
Reported per case: iterations/s of MRNSDRun.run (one library call), the model bytes of an iteration (28n + 12m for the update
kernel, 8 max(n, m) per product: 56n when square) over the measured time, the update kernel alone (trk_mrnsd_update, 28n + 12m
bytes) and, as the yardstick on the same device, k_cgls_xp_update alone (trk_cgls_xp_update, 20n bytes: the same kind of streaming
kernel) and CGLSRun.run under the same protocol."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _window(fn, sync):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    sync()
    return a.elapsed_time(b) * 1e-3


def _case(name):
    from trips_py_amd.operators import Blur2D, Radon2DParallel
    from trips_py_amd.problems import gauss_psf
    rng = np.random.default_rng(5)
    if name.startswith("blur"):
        N = int(name[4:])
        A = Blur2D(gauss_psf((9, 9), 1.5)[0], N, N, boundary="reflect")
    else:
        N = 512
        A = Radon2DParallel(N, np.linspace(0, np.pi, 180, endpoint=False))
    img = np.zeros((N, N), dtype=np.float32)
    img[N // 4: N // 2, N // 3: 2 * N // 3] = 1.0
    img[rng.integers(0, N, 200), rng.integers(0, N, 200)] += 3.0
    xt = A.engine.to_vec(img)
    b = A.apply(xt)
    b = b + 0.01 * float(b.norm()) / np.sqrt(b.numel()) * torch.from_numpy(rng.standard_normal(b.numel()).astype(np.float32)).to(b.device)
    return A, b


def measure(name, steps, warmup):
    from trips_py_amd.solvers import CGLSRun, MRNSDRun
    A, b = _case(name)
    eng = A.engine
    m, n = A.shape
    out = {"case": name, "m": m, "n": n, "steps": steps, "warmup": warmup}
    total = warmup + 3 * steps
    run = MRNSDRun(A, b, None, total, history=False)
    run.run(warmup)
    eng.synchronize()
    t = statistics.median(_window(lambda: run.run(steps), eng.synchronize) for _ in range(3))
    model = 28 * n + 12 * m + 16 * max(n, m)
    out["mrnsd"] = {"raw_partials": run.raw, "iterations_per_s": steps / t, "model_bytes_per_iteration": model,
                    "model_bytes_per_s": model * steps / t}
    s0, rows = run.rows()
    out["mrnsd"]["finite"] = bool(np.all(np.isfinite(rows[:, [0, 1, 2, 4, 5, 7]])))

    # the update kernel alone, on the run's own vectors (finished scalars; the state drifts, the traffic does not)
    S = eng.scalars(16)
    S.set(0, [1.0, 0.5, 1e30])
    GB, NP = eng.scalars(4 * 1024), eng.scalars(4 * 1024)

    def updates():
        for _ in range(steps):
            eng.mrnsd_update(S.ref(0), 1, S.ref(1), 1, S.ref(2), 1, run.X[0], run.X[1], run.g, run.s, run.z, run.r, run.u, None,
                             GB.ref(0), 1024, S.ref(8), None, NP.ref(0), 1024)
    updates()
    eng.synchronize()
    t = statistics.median(_window(updates, eng.synchronize) for _ in range(3))
    out["mrnsd_update_kernel"] = {"us": 1e6 * t / steps, "bytes": 28 * n + 12 * m, "bytes_per_s": (28 * n + 12 * m) * steps / t}

    # the yardstick: k_cgls_xp_update alone, and CGLS under the same protocol
    G = eng.scalars(8)
    G.set(0, [1.0, 1e30, 1.0])

    def xp():
        for _ in range(steps):
            eng.cgls_xp_update(G.ref(0), G.ref(1), G.ref(2), 1, run.X[0], run.g, run.z, run.X[1], None, G.ref(4), NP.ref(0), 1024)
    xp()
    eng.synchronize()
    t = statistics.median(_window(xp, eng.synchronize) for _ in range(3))
    out["cgls_xp_update_kernel"] = {"us": 1e6 * t / steps, "bytes": 20 * n, "bytes_per_s": 20 * n * steps / t}
    del run
    cg = CGLSRun(A, b, np.zeros(n, dtype=np.float32), total, history=False, defer_norms=True)
    cg.run(warmup)
    eng.synchronize()
    t = statistics.median(_window(lambda: cg.run(steps), eng.synchronize) for _ in range(3))
    out["cgls"] = {"iterations_per_s": steps / t}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "mrnsd", "mrnsd_rates.json"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cases", default="blur4096,blur512,radon512x180")
    a = ap.parse_args()
    res = {"what": "MRNSD iterations/s (MRNSDRun.run, history off), model bytes over measured time, and the streaming kernels alone",
           "device": torch.cuda.get_device_name(0), "protocol": "device events, warm-up, window closed by a synchronise, median of 3",
           "entries": [measure(c, a.steps, a.warmup) for c in a.cases.split(",")]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
