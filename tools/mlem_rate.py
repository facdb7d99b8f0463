"""MLEM iteration rates on the device beside MRNSD and CGLS in the same run: a record, not a gate.

    python tools/mlem_rate.py [--out profiles/mlem/mlem_rates.json] [--steps K] [--warmup W]

Seeded Poisson data; per case W warm-up iterations, then K iterations between two device events, the window closed by a synchronise;
the median of three windows.  Cases: the 9x9 reflect Gaussian blur at 4096^2 and 512^2, the parallel-beam projector 512^2 x 180.
Reported per case: iterations/s of MLEMRun.run (one library call, history off), the model bytes of an iteration (12m for the ratio
kernel, 16n for the update kernel, 8 max(n, m) per product: 44n when square) over the measured time, MRNSDRun.run and CGLSRun.run
under the same protocol, and the streaming kernels alone: k_mlem_ratio (12m bytes, one fp64 log per entry) beside k_pdhg_dual_p
(the same 12m bytes, no log) and k_pdhg_dual_p_kl (12m bytes, log and sqrt) on the same vectors — what the logarithm costs — and
k_mlem_update (16n bytes)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.mrnsd_rate import _window  # noqa: E402

BACKGROUND = 5.0


def _case(name):
    """(A, b): the operators of tools/mrnsd_rate.py with photon counts b = poisson(A x + 5), x a 200-count plateau and points."""
    from trips_py_amd.operators import Blur2D, Radon2DParallel
    from trips_py_amd.problems import gauss_psf, poisson_noise
    rng = np.random.default_rng(5)
    if name.startswith("blur"):
        N = int(name[4:])
        A = Blur2D(gauss_psf((9, 9), 1.5)[0], N, N, boundary="reflect")
    else:
        N = 512
        A = Radon2DParallel(N, np.linspace(0, np.pi, 180, endpoint=False))
    img = np.zeros((N, N), dtype=np.float32)
    img[N // 4: N // 2, N // 3: 2 * N // 3] = 200.0
    img[rng.integers(0, N, 200), rng.integers(0, N, 200)] += 600.0
    mean = A.apply(A.engine.to_vec(img)).cpu().numpy().astype(np.float64)
    b = poisson_noise(np.maximum(mean, 0.0), background=BACKGROUND, seed=5)
    return A, A.engine.to_vec(b)


def _kernel(fn, steps, eng):
    def loop():
        for _ in range(steps):
            fn()
    loop()
    eng.synchronize()
    return statistics.median(_window(loop, eng.synchronize) for _ in range(3)) / steps


def measure(name, steps, warmup):
    from trips_py_amd.solvers import CGLSRun, MLEMRun, MRNSDRun
    A, b = _case(name)
    eng = A.engine
    m, n = A.shape
    out = {"case": name, "m": m, "n": n, "steps": steps, "warmup": warmup}
    total = warmup + 3 * steps
    run = MLEMRun(A, b, None, total, history=False, background=BACKGROUND)
    run.run(warmup)
    eng.synchronize()
    t = statistics.median(_window(lambda: run.run(steps), eng.synchronize) for _ in range(3))
    model = 12 * m + 16 * n + 16 * max(n, m)
    rows = run.rows()
    out["mlem"] = {"iterations_per_s": steps / t, "model_bytes_per_iteration": model, "model_bytes_per_s": model * steps / t,
                   "finite": bool(np.all(np.isfinite(rows))), "KL_first": float(rows[0, 0]), "KL_last": float(rows[-1, 0])}

    # the streaming kernels alone, on vectors of the run's sizes (rho beside w, so that the inputs stay what they are)
    w = A.apply(run.x_cur)
    rho, p = eng.empty(m), eng.zeros(m)
    NP = eng.scalars(8 * 1024)
    t = _kernel(lambda: eng.mlem_ratio(BACKGROUND, w, b, rho, NP.ref(0), 1024), steps, eng)
    out["mlem_ratio_kernel"] = {"us": 1e6 * t, "bytes": 12 * m, "bytes_per_s": 12 * m / t}
    t = _kernel(lambda: eng.pdhg_dual_p(0.5, w, b, p, NP.ref(0), 1024), steps, eng)
    out["pdhg_dual_p_kernel"] = {"us": 1e6 * t, "bytes": 12 * m, "bytes_per_s": 12 * m / t}
    p.zero_()
    t = _kernel(lambda: eng.pdhg_dual_p_kl(0.5, BACKGROUND, w, b, p, NP.ref(0), 1024), steps, eng)
    out["pdhg_dual_p_kl_kernel"] = {"us": 1e6 * t, "bytes": 12 * m, "bytes_per_s": 12 * m / t}
    x_new = eng.empty(n)
    t = _kernel(lambda: eng.mlem_update(run.x_cur, run.t, run.sinv, None, x_new, NP.ref(0), 1024), steps, eng)
    out["mlem_update_kernel"] = {"us": 1e6 * t, "bytes": 16 * n, "bytes_per_s": 16 * n / t}
    del run, w, rho, p, x_new

    # the yardsticks: MRNSD and CGLS on the same operator and data under the same protocol
    mr = MRNSDRun(A, b, None, total, history=False)
    mr.run(warmup)
    eng.synchronize()
    t = statistics.median(_window(lambda: mr.run(steps), eng.synchronize) for _ in range(3))
    out["mrnsd"] = {"iterations_per_s": steps / t}
    del mr
    cg = CGLSRun(A, b, np.zeros(n, dtype=np.float32), total, history=False, defer_norms=True)
    cg.run(warmup)
    eng.synchronize()
    t = statistics.median(_window(lambda: cg.run(steps), eng.synchronize) for _ in range(3))
    out["cgls"] = {"iterations_per_s": steps / t}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "mlem", "mlem_rates.json"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cases", default="blur4096,blur512,radon512x180")
    a = ap.parse_args()
    res = {"what": "MLEM iterations/s (MLEMRun.run, history off) beside MRNSD and CGLS, model bytes over measured time, and the "
                   "streaming kernels alone (the ratio kernel's fp64 log beside k_pdhg_dual_p on the same 12m bytes)",
           "device": torch.cuda.get_device_name(0), "protocol": "device events, warm-up, window closed by a synchronise, median of 3",
           "entries": [measure(c, a.steps, a.warmup) for c in a.cases.split(",")]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
