"""PDHG with isotropic space-time TV (tv='iso3'): iteration rates on the device.  A record, not a gate.

    python tools/pdhg_iso3_rate.py [--out profiles/pdhg/pdhg_iso3_rates.json] [--steps K] [--warmup W] [--cases 256x32x16,1024x16x8]

A case N x frames x angles is the dynamic Radon problem: BlockDiagOp of `frames` Radon2DParallel(N, angles per frame, shifted from frame
to frame) with SpaceTimeDerivative(N, frames), box [0, inf), seeded data.  Per case, in ONE run: PDHGRun.run (one library call,
history off) with tv='iso3' fused (5 launches), tv='iso3' unfused (8 launches) and tv='iso' (the generic path, 9 launches: its dual is
two kernels), W warm-up iterations and then K iterations between two device events, the window closed by a synchronise, the median
of three windows.  Then each new kernel alone under the same protocol, and the two products and the streaming primal of the unfused
L side for comparison.  Model bytes with n = frames N^2 unknowns and `rows` ~ 3n rows of L (docs/kernels/pdhg.md):
  fused dual 4n + 8 rows (8n + 8 rows if the next frame's re-read misses cache), fused primal 16n + 4 rows, unfused dual 12 rows,
  L xbar 12n + 4 rows (k_time_fwd reads both frames again), L^T q 4 rows + 4n, streaming primal 20n: with rows = 3n the L side is
  96n unfused and 56n fused.
A's two products are outside the L side and the same in every mode; their time is in every iterations/s figure.  The file is written
after every case."""
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


def _case(N, frames, angles):
    from trips_py_amd.operators import BlockDiagOp, Radon2DParallel, SpaceTimeDerivative
    rng = np.random.default_rng(5)
    A = BlockDiagOp([Radon2DParallel(N, np.linspace(0, np.pi, angles, endpoint=False) + 0.1 * t) for t in range(frames)])
    eng = A.engine
    vol = np.zeros((frames, N, N), dtype=np.float32)
    for t in range(frames):                                   # a block that drifts and a few bright points
        vol[t, N // 4 + t: N // 2 + t, N // 3: 2 * N // 3] = 1.0
    vol[rng.integers(0, frames, 200), rng.integers(0, N, 200), rng.integers(0, N, 200)] += 3.0
    b = A.apply(eng.to_vec(vol.reshape(-1)))
    b = b + 0.01 * float(b.norm()) / np.sqrt(b.numel()) * torch.from_numpy(rng.standard_normal(b.numel()).astype(np.float32)).to(b.device)
    return A, SpaceTimeDerivative(N, frames, engine=eng), b


def measure(N, frames, angles, steps, warmup):
    from trips_py_amd.operators import operator_norm_sq
    from trips_py_amd.solvers import PDHGRun
    from trips_py_amd.solvers.PDHG import pdhg_steps
    A, L, b = _case(N, frames, angles)
    eng = A.engine
    n, rows = A.shape[1], L.shape[0]
    normK2 = operator_norm_sq([A, L], iters=30, seed=0)
    sigma, tau = pdhg_steps(normK2)
    lam = 0.01
    out = {"case": f"radon{N}x{frames}_angles{angles}", "N": N, "frames": frames, "n": n, "m": A.shape[0], "rows_L": rows, "steps": steps,
           "warmup": warmup, "normK2_estimate": normK2}
    total = warmup + 3 * steps
    modes = [("pdhg_iso3_fused", "iso3", True, 5, 20 * n + 12 * rows), ("pdhg_iso_generic", "iso", False, 9, 36 * n + 20 * rows),
             ("pdhg_iso3_unfused", "iso3", False, 8, 36 * n + 20 * rows)]          # (the last run's vectors serve the kernels below)
    for name, tv, fused, launches, model_L in modes:
        run = PDHGRun(A, b, L, lam, sigma, tau, 0.0, np.inf, None, total, history=False, fused=fused, tv=tv)
        assert run.fused == fused
        run.run(warmup)
        eng.synchronize()
        t = statistics.median(_window(lambda: run.run(steps), eng.synchronize) for _ in range(3))
        S = run.rows()
        out[name] = {"launches_per_iteration": launches, "iterations_per_s": steps / t, "ms_per_iteration": 1e3 * t / steps,
                     "model_bytes_L_side_per_iteration": model_L, "finite": bool(np.all(np.isfinite(S))),
                     "objective_first_last": [float(0.5 * S[k, 0] + lam * S[k, 1]) for k in (0, -1)]}
        if fused or tv == "iso":
            del run
    # each new kernel alone, on the unfused run's vectors (the state drifts, the traffic does not), and the unfused L side's pieces
    cap = eng.pdhg_blocks_iso3(A.shape[0], n, rows, N, frames, L._h)
    NP = eng.scalars(8 * cap)
    X0, X1 = run.X[0], run.X[1]
    kernels = {
        "k_pdhg_tv_dual<kTriples, true>": (4 * n + 8 * rows, lambda: eng.pdhg_st_dual_iso3(L._h, sigma, lam, run.xbar, run.q, NP.ref(0), cap)),
        "k_pdhg_tv_primal<false, true>": (16 * n + 4 * rows, lambda: eng.pdhg_st_primal(L._h, tau, 0.0, np.inf, X0, run.z, run.q, X1, run.xbar, None,
                                                                        NP.ref(0), cap)),
        "k_pdhg_tv_dual<kTriples, false>": (12 * rows, lambda: eng.pdhg_dual_q_iso3(N, frames, sigma, lam, run.u, run.q, NP.ref(0), cap)),
        "L_apply (k_d2_fwd + k_time_fwd)": (12 * n + 4 * rows, lambda: L.apply(run.xbar, out=run.u)),
        "L_apply_transpose (k_d2_adj)": (4 * rows + 4 * n, lambda: L.apply(run.q, out=run.v, transpose=True)),
        "k_pdhg_primal": (20 * n, lambda: eng.pdhg_primal(tau, 0.0, np.inf, X0, run.z, run.v, X1, run.xbar, None, NP.ref(0), cap)),
        "A_apply": (None, lambda: A.apply(run.xbar, out=run.w)),
        "A_apply_transpose": (None, lambda: A.apply(run.p, out=run.z, transpose=True)),
    }
    for name, (nbytes, call) in kernels.items():
        def many():
            for _ in range(steps):
                call()
        many()
        eng.synchronize()
        t = statistics.median(_window(many, eng.synchronize) for _ in range(3))
        out[name] = {"us": 1e6 * t / steps}
        if nbytes is not None:
            out[name].update({"model_bytes": nbytes, "model_bytes_per_s": nbytes * steps / t})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "pdhg", "pdhg_iso3_rates.json"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cases", default="256x32x16,1024x16x8", help="N x frames x angles per frame, comma separated")
    a = ap.parse_args()
    res = {"what": "PDHG iterations/s (PDHGRun.run, history off) on the dynamic Radon problem: tv='iso3' fused and unfused and tv='iso' on the "
                   "generic path from the same run, the model bytes of the L side, each new kernel alone and the unfused L side's pieces",
           "device": torch.cuda.get_device_name(0), "protocol": "device events, warm-up, window closed by a synchronise, median of 3",
           "entries": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for case in a.cases.split(","):
        res["entries"].append(measure(*(int(v) for v in case.split("x")), a.steps, a.warmup))
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
