"""The fan-beam demo fixture against the reference notebook's stored outputs, from data kept under tests/golden alone.

INTEGRATION.md §1 (unmodified reference solvers + engine operators) runs the reference's own solver sources, which are not
part of this repository: tools/check_dropin.py checks it wherever a reference tree is at hand."""
import os
import sys

import numpy as np

from conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_fanbeam_demo_fixture_regenerates_from_the_reference_notebook():
    """tests/golden/fanbeam_demo_image.npz is what tools/make_fanbeam_demo_golden.py decodes from the notebook's stored outputs
    (their PNG bytes: tests/golden/fanbeam_demo_notebook_png.npz), and its phantom is the image the notebook drew of x_true."""
    from make_fanbeam_demo_golden import decode
    pngs = load_golden("fanbeam_demo_notebook_png")
    got = decode({k: v.tobytes() for k, v in pngs.items()})
    g = load_golden("fanbeam_demo_image")
    assert sorted(list(got) + ["phantom"]) == sorted(g)
    for k in got:
        assert np.array_equal(got[k], g[k]), k
    # imshow's grey map of the phantom (vmin / vmax = its min / max; 256 levels, the top one clipped into 255)
    ph = g["phantom"]
    assert ph.shape == (int(g["nx"]), int(g["nx"]))
    u = (ph - ph.min()) / (ph.max() - ph.min())
    assert np.array_equal(g["xtrue_grey"], np.minimum(np.floor(u * 256), 255).astype(np.uint8))
