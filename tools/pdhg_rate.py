"""PDHG iteration rates on the device: a record, not a gate.

    python tools/pdhg_rate.py [--tv iso] [--out profiles/pdhg/pdhg_rates.json] [--steps K] [--warmup W]

Seeded data; per case W warm-up iterations, then K iterations between two device events, the window closed by a synchronise;
the median of three windows.  Cases: the 9x9 reflect Gaussian blur at 4096^2 and 512^2 with the 2-D first differences (anisotropic
TV), box [0, inf).  Reported per case: iterations/s of PDHGRun.run (one library call) on the fused path (5 launches, 76n model bytes)
and on the generic path (7 launches, 100n), the model bytes over the measured time, each new kernel alone with its own byte count,
and, for scale from the same run, MRNSDRun.run and MMGKS (projection_dim 3, 30 iterations, lambda fixed) iterations/s.
Model bytes, square problem, rows of L = 2n: A and A^T 8n each, L and L^T 12n each, dual p 16n, dual q 24n, primal 20n, fused dual
20n, fused primal 24n.
--tv iso adds, in the same run and ahead of the anisotropic cases, PDHGRun(tv='iso') fused and unfused (the same model bytes and launch
counts: only the arithmetic of the dual differs) and the two isotropic dual kernels alone; it writes profiles/pdhg/pdhg_iso_rates.json."""
import argparse
import json
import os
import statistics
import sys
import time

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


def _case(N):
    from trips_py_amd.operators import Blur2D, FirstDerivative2D
    from trips_py_amd.problems import gauss_psf
    rng = np.random.default_rng(5)
    A = Blur2D(gauss_psf((9, 9), 1.5)[0], N, N, boundary="reflect")
    img = np.zeros((N, N), dtype=np.float32)
    img[N // 4: N // 2, N // 3: 2 * N // 3] = 1.0
    img[rng.integers(0, N, 200), rng.integers(0, N, 200)] += 3.0
    b = A.apply(A.engine.to_vec(img))
    b = b + 0.01 * float(b.norm()) / np.sqrt(b.numel()) * torch.from_numpy(rng.standard_normal(b.numel()).astype(np.float32)).to(b.device)
    return A, FirstDerivative2D(N, engine=A.engine), b


def measure(N, steps, warmup, tv="aniso"):
    from trips_py_amd.operators import operator_norm_sq
    from trips_py_amd.solvers import MMGKS, MRNSDRun, PDHGRun
    from trips_py_amd.solvers.PDHG import pdhg_steps
    A, L, b = _case(N)
    eng = A.engine
    n, rows = A.shape[1], L.shape[0]
    normK2 = operator_norm_sq([A, L], iters=30, seed=0)
    sigma, tau = pdhg_steps(normK2)
    lam = 0.01
    out = {"case": f"blur{N}_tv", "n": n, "rows_L": rows, "steps": steps, "warmup": warmup, "normK2_estimate": normK2}
    total = warmup + 3 * steps
    cases = [("pdhg_fused", True, 76 * n, "aniso"), ("pdhg_generic", False, 100 * n, "aniso")]
    if tv == "iso":                                     # the same bytes and launches: only the arithmetic of the dual differs
        cases = [("pdhg_iso_fused", True, 76 * n, "iso"), ("pdhg_iso_unfused", False, 100 * n, "iso")] + cases
    for name, fused, model, term in cases:
        run = PDHGRun(A, b, L, lam, sigma, tau, 0.0, np.inf, None, total, history=False, fused=fused, tv=term)
        run.run(warmup)
        eng.synchronize()
        t = statistics.median(_window(lambda: run.run(steps), eng.synchronize) for _ in range(3))
        S = run.rows()
        out[name] = {"launches_per_iteration": 5 if fused else 7, "iterations_per_s": steps / t, "model_bytes_per_iteration": model,
                     "model_bytes_per_s": model * steps / t, "finite": bool(np.all(np.isfinite(S))),
                     "objective_first_last": [float(0.5 * S[k, 0] + lam * S[k, 1]) for k in (0, -1)]}
        if fused:
            del run
    # each new kernel alone, on the generic run's vectors (the state drifts, the traffic does not)
    cap = eng.pdhg_blocks(n, n, rows, L._h)
    NP = eng.scalars(8 * cap)
    X0, X1 = run.X[0], run.X[1]
    kernels = {
        "k_pdhg_dual_p": (16 * n, lambda: eng.pdhg_dual_p(sigma, run.w, run.bv, run.p, NP.ref(0), cap)),
        "k_pdhg_dual_q": (12 * rows, lambda: eng.pdhg_dual_q(sigma, lam, run.u, run.q, NP.ref(0), cap)),
        "k_pdhg_primal": (20 * n, lambda: eng.pdhg_primal(tau, 0.0, np.inf, X0, run.z, run.v, X1, run.xbar, None, NP.ref(0), cap)),
        "k_pdhg_tv_dual<kRows, true>": (4 * n + 8 * rows, lambda: eng.pdhg_tv_dual(L._h, sigma, lam, run.xbar, run.q, NP.ref(0), cap)),
        "k_pdhg_tv_primal<false, false>": (16 * n + 4 * rows, lambda: eng.pdhg_tv_primal(L._h, tau, 0.0, np.inf, X0, run.z, run.q, X1, run.xbar, None,
                                                                        NP.ref(0), cap)),
    }
    if tv == "iso":
        kernels["k_pdhg_tv_dual<kPairs, true>"] = (4 * n + 8 * rows, lambda: eng.pdhg_tv_dual_iso(L._h, sigma, lam, run.xbar, run.q, NP.ref(0), cap))
        kernels["k_pdhg_tv_dual<kPairs, false>"] = (12 * rows, lambda: eng.pdhg_dual_q_iso(N, 1, sigma, lam, run.u, run.q, NP.ref(0), cap))
    for name, (nbytes, call) in kernels.items():
        def many():
            for _ in range(steps):
                call()
        many()
        eng.synchronize()
        t = statistics.median(_window(many, eng.synchronize) for _ in range(3))
        out[name] = {"us": 1e6 * t / steps, "bytes": nbytes, "bytes_per_s": nbytes * steps / t}
    del run
    # for scale: MRNSD under the same protocol, MMGKS as a whole solve (host clock around a synchronise)
    mr = MRNSDRun(A, b, None, total, history=False)
    mr.run(warmup)
    eng.synchronize()
    t = statistics.median(_window(lambda: mr.run(steps), eng.synchronize) for _ in range(3))
    out["mrnsd"] = {"iterations_per_s": steps / t}
    del mr
    MMGKS(A, b, L, 2, 1, 3, 4, 1e-2, history=False)
    eng.synchronize()
    rates = []
    for _ in range(3):
        t0 = time.perf_counter()
        MMGKS(A, b, L, 2, 1, 3, 30, 1e-2, history=False)
        eng.synchronize()
        rates.append(30 / (time.perf_counter() - t0))
    out["mmgks"] = {"iterations_per_s": statistics.median(rates), "projection_dim": 3, "n_iter": 30}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tv", choices=("aniso", "iso"), default="aniso")
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="4096,512")
    a = ap.parse_args()
    a.out = a.out or os.path.join("profiles", "pdhg", "pdhg_iso_rates.json" if a.tv == "iso" else "pdhg_rates.json")
    res = {"what": "PDHG iterations/s (PDHGRun.run, history off) fused and generic, model bytes over measured time, the new kernels alone, "
                   "MRNSD and MMGKS for scale" + ("; isotropic TV fused and unfused and its two dual kernels from the same run"
                                                   if a.tv == "iso" else ""),
           "device": torch.cuda.get_device_name(0), "protocol": "device events, warm-up, window closed by a synchronise, median of 3",
           "entries": [measure(int(s), a.steps, a.warmup, a.tv) for s in a.sizes.split(",")]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
