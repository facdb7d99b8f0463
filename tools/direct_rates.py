#!/usr/bin/env python
"""Rates of the dense direct path: the float64 device SVD (csrc/dense_svd.hip) and the direct solvers (tSVD_sol, Tikhonov with
L = I, regparam='gcv') on n x n blur matrices (sqrt(n)^2 images, Gauss 9 x 9, spread 3), beside NumPy's float64 SVD of the same
matrix on the host (its BLAS threads as the environment sets them; the tool reports the count).

    python tools/direct_rates.py [--sizes 1024,2500,4096] [--reps 2] [--out FILE]

One line per size: device SVD seconds (best of --reps, synchronised), Jacobi sweeps, tSVD and Tikhonov seconds (each includes its
own SVD and the host<->device copies), host SVD seconds (one run)."""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def best(fn, reps):
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return min(t), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,2500,4096")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import direct_cases as dc
    from trips_py_amd import _dense
    from trips_py_amd.solvers import Tikhonov, tSVD_sol
    try:
        from threadpoolctl import threadpool_info
        blas = ", ".join(f"{d['internal_api']} {d['num_threads']} threads" for d in threadpool_info() if d["user_api"] == "blas")
    except Exception:
        blas = "threadpoolctl not available; OMP_NUM_THREADS=" + os.environ.get("OMP_NUM_THREADS", "?")
    lines = [f"# device {torch.cuda.get_device_name(0)}; host BLAS: {blas}",
             "# n      dev_svd_s  sweeps  tsvd_gcv_s  tikh_gcv_s  host_svd_s  host/dev"]
    print(lines[0], flush=True)
    for n in [int(s) for s in a.sizes.split(",")]:
        N = int(round(np.sqrt(n)))
        A = dc.blur2d_dense(N, (9, 9), (3.0, 3.0))
        bt = A @ dc.test_image(N, 1)
        b = bt + dc.noise(bt.shape, 0.01, np.linalg.norm(bt), 2)
        At, m, nn = _dense.to_device_t(A)
        _dense.svd_device_t(At, m, nn)                               # warm-up (module load, allocator)
        t_svd, out = best(lambda: _dense.svd_device_t(At, m, nn), a.reps)
        sweeps = out[3]
        t_tsvd, _ = best(lambda: tSVD_sol(A, b, "gcv"), 1)
        t_tikh, _ = best(lambda: Tikhonov(A, b, np.eye(n), None, "gcv"), 1)
        if a.no_host:
            t_host = float("nan")
        else:
            t0 = time.perf_counter()
            np.linalg.svd(A)
            t_host = time.perf_counter() - t0
        line = f"{n:6d}  {t_svd:9.3f}  {sweeps:6d}  {t_tsvd:10.3f}  {t_tikh:10.3f}  {t_host:10.3f}  {t_host / t_svd:8.1f}"
        lines.append(line)
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
