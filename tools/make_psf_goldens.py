#!/usr/bin/env python
"""Generate tests/golden/psf_defocus1d.npz by RUNNING THE REFERENCE's Deblurring1D.Defocus1D(grid_points, parameter)
(Deblurring1D.py:70-82) for grid_points 16, 17, 64 and parameter 0, 3, 7.5.

TEST TOOLING, NOT PRODUCT.  Run only where the reference exists (the build container), with the same shim as
tools/make_goldens.py (whose path setup and helpers are imported from it):

    python tools/make_psf_goldens.py

Per (grid_points, parameter): the array the method returns (`ret_<n>_<p>`: un-normalised unless parameter == 0), the one it
stores in self.PSF (`psf_<n>_<p>`: normalised) and the centre it returns (`center_<n>_<p>`).  Only numeric arrays are stored.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import Deblurring1D, np, save  # noqa: E402

GRID_POINTS = (16, 17, 64)
PARAMETERS = (0, 3, 7.5)


def key(n, p):
    return f"{n}_{str(p).replace('.', 'p')}"


def defocus1d():
    out = {"grid_points": np.array(GRID_POINTS), "parameters": np.array(PARAMETERS, dtype=np.float64)}
    for n in GRID_POINTS:
        for p in PARAMETERS:
            D1 = Deblurring1D()
            ret, center = D1.Defocus1D(n, p)
            out["ret_" + key(n, p)] = np.array(ret, dtype=np.float64)
            out["psf_" + key(n, p)] = np.array(D1.PSF, dtype=np.float64)
            out["center_" + key(n, p)] = np.array(int(center))
    save("psf_defocus1d", **out)


if __name__ == "__main__":
    defocus1d()
