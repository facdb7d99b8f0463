"""Per-launch times of the recomputing CGLS loop from a rocprofv3 kernel trace, forward and adjoint apart.

usage: python tools/rc_trace_split.py <dir holding *_kernel_trace.csv> [skip]

The forward and the adjoint launches of `k_blur_slide<…RC_NORM>` / `<…RC_RATIO>` carry the same kernel name, so the per-kernel
statistics of `--stats` merge them.  In dispatch order the loop issues F0, F1, (x update), A0, A1 per iteration: the norm-only
launches alternate forward / adjoint, and so do the ratio launches.  `skip` leading launches of each kind are left out
(run-in and warm-up; default: the first half).
"""
import csv
import glob
import os
import statistics
import sys


def main():
    root = sys.argv[1]
    files = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {root}"
    rows = []
    for f in files:
        with open(f) as fh:
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows.sort()
    # the last template argument of k_blur_slide: 1 RC_NORM, 3 RC_NORM_LEAN, 2 RC_RATIO
    kinds = {"norm": (", 1>(", ", 3>("), "ratio": (", 2>(",), "x update": ("k_cgls_xs_update",)}
    for label, keys in kinds.items():
        d = [e - s for s, e, k in rows if any(key in k for key in keys) and ("k_blur_slide" in k or label == "x update")]
        if not d:
            continue
        skip = int(sys.argv[2]) if len(sys.argv) > 2 else len(d) // 2
        d = d[skip - skip % 2:]
        # the forward / adjoint labels rest on dispatch parity alone: an extra launch of either kind (a warm-up apply, an odd count)
        # would swap them without a trace
        assert label == "x update" or len(d) % 2 == 0, f"odd number of {label} launches after the skip: {len(d)}"
        groups = {"": d} if label == "x update" else {" forward": d[0::2], " adjoint": d[1::2]}
        for g, v in groups.items():
            q = statistics.quantiles(v, n=4)
            print(f"{label + g:16s} n={len(v):5d}  mean {statistics.fmean(v) / 1e3:7.2f} us  median {statistics.median(v) / 1e3:7.2f}"
                  f"  quartiles {q[0] / 1e3:.2f}-{q[2] / 1e3:.2f}")


if __name__ == "__main__":
    main()
