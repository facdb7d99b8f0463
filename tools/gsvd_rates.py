#!/usr/bin/env python
"""Rates of the device GSVD (trips_py_amd._dense.gsvd_device: three runs of the one-sided Jacobi of csrc/dense_svd.hip) beside
its float64 NumPy restatement on the host (tests/gsvd_cases.py gsvd_numpy: two LAPACK SVDs and four products).

    python tools/gsvd_rates.py [--sizes 200,576,1024,2500] [--reps 2] [--out FILE]

n = 200 is the 1-D deblurring demo's pair (Gauss sigma 30 and the first difference with a zero row); every other n is the blur of a
sqrt(n)^2 image (Gauss 9 x 9, spread 3; n = 576 the pair of tests/golden/direct_blur2d.npz) with its 2-D first difference, which
has 2 sqrt(n) (sqrt(n) - 1) rows.  One line per size: device seconds (best of --reps, synchronised, operands already on the
device), the Jacobi sweeps of the three stages, the number of columns with c > 1/sqrt(2) (the third stage's), host seconds."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200,576,1024,2500")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import direct_cases as dc
    import gsvd_cases as gc
    from trips_py_amd import _dense
    lines = [f"# device {torch.cuda.get_device_name(0)}; OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', '?')}",
             "# n     m     p     dev_gsvd_s  sweeps(M, Q1, Q2_J)  |J|   svd_of_A_s  host_numpy_s  host/dev"]
    print("\n".join(lines), flush=True)
    for n in [int(s) for s in a.sizes.split(",")]:
        if n == 200:
            A, L = gc.deblur1d_pair()
        elif n == 576:
            A, L = gc.blur2d_pair()
        else:
            N = int(round(np.sqrt(n)))
            A, L = dc.blur2d_dense(N, (9, 9), (3.0, 3.0)), dc.first_difference_2d(N, N).toarray()
        At, Lt = torch.from_numpy(A).cuda(), torch.from_numpy(L).cuda()
        _dense.gsvd_device(At, Lt)                                   # warm-up (module load, allocator)
        t_dev, t_svd = [], []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f = _dense.gsvd_device(At, Lt)
            torch.cuda.synchronize()
            t_dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            _dense.svd_device(At)
            torch.cuda.synchronize()
            t_svd.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        gc.gsvd_numpy(A, L)
        t_host = time.perf_counter() - t0
        J = int(torch.sum(f.c > np.sqrt(0.5)))
        line = (f"{n:5d} {A.shape[0]:5d} {L.shape[0]:5d}  {min(t_dev):10.3f}  {str(f.sweeps):19s}  {J:4d}  {min(t_svd):10.3f}  "
                f"{t_host:12.3f}  {t_host / min(t_dev):8.2f}")
        lines.append(line)
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
