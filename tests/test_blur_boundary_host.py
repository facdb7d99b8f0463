"""CPU-side checks of the blur's boundary modes: mode-name normalisation (no GPU), the C ABI declaring the new entry point
and mode constants, and the reference-made 1-D goldens (tools/make_boundary_goldens.py) reproducing scipy on their own data."""
import os
import re

import numpy as np
import pytest
from scipy.ndimage import convolve1d

from conftest import load_golden, relerr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_MODES = ["constant", "nearest", "mirror", "wrap"]


@pytest.mark.parametrize("mode,canon", [("reflect", "reflect"), ("constant", "constant"), ("nearest", "nearest"),
                                        ("mirror", "mirror"), ("wrap", "wrap"), ("grid-mirror", "reflect"),
                                        ("grid-constant", "constant"), ("grid-wrap", "wrap")])
def test_boundary_names_normalise(mode, canon):
    from trips_py_amd.operators import BOUNDARY_MODES, normalize_boundary
    assert normalize_boundary(mode) == canon
    assert canon in BOUNDARY_MODES


@pytest.mark.parametrize("mode", ["periodic", "zero", "Reflect", "", "grid-nearest", None, 0])
def test_unknown_boundary_raises_value_error(mode):
    from trips_py_amd.operators import normalize_boundary
    with pytest.raises(ValueError):
        normalize_boundary(mode)


def test_nonzero_fill_value_raises_value_error():
    from trips_py_amd.operators import normalize_boundary
    assert normalize_boundary("constant", 0.0) == "constant"
    with pytest.raises(ValueError):
        normalize_boundary("constant", 1.0)


def test_problem_builders_reject_unknown_modes_before_touching_a_device():
    from trips_py_amd.problems import Deblurring1D, Deblurring2D
    with pytest.raises(ValueError):
        Deblurring1D().forward_Op_1D(3, 64, boundary_condition="periodic")
    with pytest.raises(ValueError):
        Deblurring2D().forward_Op((3, 3), (1, 1), 16, 16, boundary_condition="zero")


def test_mode_codes_match_the_header():
    from trips_py_amd.operators import BOUNDARY_MODES
    txt = open(os.path.join(REPO, "include", "trk.h")).read()
    consts = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define\s+TRK_BOUNDARY_([A-Z]+)\s+(\d+)", txt)}
    assert consts == BOUNDARY_MODES
    assert consts["reflect"] == 0


def test_header_declares_the_boundary_constructor():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "trk.h")).read(), flags=re.S)
    decl = re.search(r"int\s+trk_blur2d_create_bc\s*\(([^)]*)\)\s*;", txt)
    assert decl, "trk_blur2d_create_bc is not declared"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == 7 and params[5].startswith("int ") and params[6].startswith("trk_op**")
    from trips_py_amd import _lib
    assert len(_lib.SIGNATURES["trk_blur2d_create_bc"][1]) == 7


@pytest.mark.parametrize("mode", NEW_MODES)
def test_boundary_goldens_reproduce_scipy(mode):
    g = load_golden("deblur1d_bc_" + mode)
    psf, x = g["psf"], g["x"]
    n = int(g["n"])
    assert psf.shape == (n,) and x.shape == (n,)
    assert relerr(g["Ax"], convolve1d(x, psf, mode=mode)) < 1e-13
    assert relerr(g["ATx"], convolve1d(x, psf[::-1], mode=mode)) < 1e-13
    for k in g:
        assert np.asarray(g[k]).dtype.kind in "fiu", k        # numbers only
    assert int(g["cgls_its"]) == int(g["cgls_max_iter"]) == len(g["cgls_relError"])
