"""Pass rates of OSEM and SIRT on the device at S = 1, 6 and 18 subsets: a record, not a gate.

    python tools/os_rate.py [--out profiles/os/os_rates.json] [--steps K] [--warmup W]

The parallel-beam projector 512^2 x 180 of tools/mlem_rate.py with its seeded photon counts (SIRT fits the same counts by least
squares).  Per solver and S: W warm-up passes, then K passes between two device events, the window closed by a synchronise; the
median of three windows.  A pass is S sub-steps of four launches each on 1 / S of the views, so on this launch-bound problem the
question is whether a pass of S sub-steps beats S plain iterations: reported are passes/s, sub-steps/s = S x passes/s, and the
ratio of sub-steps/s to the S = 1 rate of the same solver (1 = a pass costs what S plain iterations cost, S = a pass costs what
one costs)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.mlem_rate import BACKGROUND, _case  # noqa: E402
from tools.mrnsd_rate import _window  # noqa: E402


def measure(steps, warmup, subsets):
    from trips_py_amd.operators import RowSubsets
    from trips_py_amd.solvers import OSEMRun, SIRTRun
    A, b = _case("radon512x180")
    eng = A.engine
    bh = b.cpu().numpy()
    total = warmup + 3 * steps
    out = []
    for S in subsets:
        sub = RowSubsets(A, S)
        for name, make in (("osem", lambda: OSEMRun(A, bh, None, total, history=False, background=BACKGROUND, subsets=sub)),
                           ("sirt", lambda: SIRTRun(A, bh, None, total, history=False, subsets=sub, lower=0.0))):
            run = make()
            run.run(warmup)
            eng.synchronize()
            t = statistics.median(_window(lambda: run.run(steps), eng.synchronize) for _ in range(3))
            rows = run.rows()
            out.append({"solver": name, "S": S, "passes_per_s": steps / t, "substeps_per_s": S * steps / t,
                        "finite": bool(np.all(np.isfinite(rows))), "slot0_first": float(rows[0, 0]), "slot0_last": float(rows[-1, 0])})
            del run
    plain = {e["solver"]: e["passes_per_s"] for e in out if e["S"] == 1}
    for e in out:
        e["substeps_per_s_over_S1_rate"] = e["substeps_per_s"] / plain[e["solver"]] if e["solver"] in plain else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "os", "os_rates.json"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--subsets", default="1,6,18")
    a = ap.parse_args()
    res = {"what": "OSEM and SIRT passes/s on 512^2 x 180 parallel beam (OSEMRun.run / SIRTRun.run, one library call, history off)",
           "device": torch.cuda.get_device_name(0), "protocol": "device events, warm-up, window closed by a synchronise, median of 3",
           "steps": a.steps, "warmup": a.warmup, "entries": measure(a.steps, a.warmup, [int(s) for s in a.subsets.split(",")])}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
