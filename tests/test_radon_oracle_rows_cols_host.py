"""CPU checks behind tests/test_gpu_radon_entrywise.py: the oracle's rows() and cols() of the parallel-beam projector are the rows
and columns of its matrix() to the bit, and the case table of tests/radon_cases.py reaches every forward kernel and every adjoint
route of the dispatch restated there."""
import numpy as np
import pytest

import radon_cases as C

ANGLES = np.concatenate([C.TIES, np.linspace(0.05, np.pi + 0.05, 9, endpoint=False), [-2.2, 4.0, 7.0]])


@pytest.mark.parametrize("N,nd", [(12, 12), (50, 75), (64, 40), (96, 97)])
def test_rows_and_cols_equal_the_matrix_to_the_bit(N, nd):
    from oracle import cpu_ref as O
    Ro = O.Radon2D(N, ANGLES, n_det=nd)
    M = Ro.matrix().copy()
    M.sum_duplicates()                     # the explicit zeros matrix() parks on column 0: x + 0.0 = x
    M.eliminate_zeros()
    assert M.nnz > 0
    R = Ro.rows(np.arange(Ro.shape[0]))
    Cc = Ro.cols(np.arange(N * N))
    assert R.shape == M.shape == Cc.shape and R.dtype == Cc.dtype == np.float64
    assert (R != M).nnz == 0
    assert (Cc.tocsr() != M).nnz == 0
    # subsets, in any order and with repeats, are those rows / columns
    rng = np.random.default_rng(N)
    rays, pix = rng.integers(0, Ro.shape[0], 40), rng.integers(0, N * N, 40)
    assert (Ro.rows(rays) != M[rays]).nnz == 0
    assert (Ro.cols(pix).tocsr() != M[:, pix]).nnz == 0
    mode, w = Ro.geometry(np.arange(Ro.shape[0]))
    ct, st = np.cos(ANGLES), np.sin(ANGLES)
    want_mode = (np.abs(ct) < np.abs(st)).astype(int)
    assert np.array_equal(mode.reshape(len(ANGLES), nd), np.repeat(want_mode[:, None], nd, axis=1))
    with np.errstate(divide="ignore"):
        want_w = np.where(want_mode == 0, 1.0 / np.abs(ct), 1.0 / np.abs(st))
    assert np.array_equal(w.reshape(len(ANGLES), nd)[:, 0], want_w)


def test_case_table_reaches_every_kernel_path():
    got = set()
    for case in C.CASES:
        for batch in (1, 3):
            fwd, (band, nb), adj, nsplit, prep = C.case_paths(case, batch)
            got.add(("fwd", fwd, band if fwd != "k_radon_fwd" and fwd != "k_radon_fwd_lds" else 0, nb > 1))
            got.add(("adj", adj, prep))
            got.add(("nsplit", nsplit))
        if C.case_paths(case)[0] == "k_radon_fwd_quadf+quad":
            got.add(("fwd", C.case_paths(case, 1, ["TRK_RADON_NO_QUADF"])[0]))
    need = [("fwd", "k_radon_fwd", 0, False), ("fwd", "k_radon_fwd", 0, True),
            ("fwd", "k_radon_fwd_lds", 0, False), ("fwd", "k_radon_fwd_lds", 0, True),
            ("fwd", "k_radon_fwd_band", 64, True), ("fwd", "k_radon_fwd_band", 32, True),
            ("fwd", "k_radon_fwd_quadf+quad", 128, True), ("fwd", "k_radon_fwd_quadf+quad", 256, True), ("fwd", "k_radon_fwd_quad"),
            ("nsplit", 4), ("nsplit", 8)]
    need += [("adj", k, True) for k in ("quad", "simple")] + [("adj", "groups", True)]
    need += [("adj", k, p) for k in ("tile32_b8", "tile16_b16", "tile16_b4") for p in (True, False) if (k, p) != ("tile16_b4", True)]
    missing = [n for n in need if n not in got]
    assert not missing, missing
    assert {k for (t, k, *_) in got if t == "adj"} == set(C.ADJ_KINDS)


@pytest.mark.parametrize("name,fwd,bands,adj,nsplit,prep", [
    ("tiny", "k_radon_fwd_lds", (128, 1), "simple", 1, True),
    ("odd50", "k_radon_fwd", (128, 1), "tile16_b16", 1, False),
    ("odd257", "k_radon_fwd", (128, 3), "tile32_b8", 8, True),
    ("odd257few", "k_radon_fwd", (64, 5), "tile16_b16", 1, False),
    ("lds64", "k_radon_fwd_lds", (128, 1), "tile32_b8", 8, True),
    ("lds132", "k_radon_fwd_lds", (64, 3), "tile16_b16", 1, False),
    ("band128", "k_radon_fwd_band", (64, 2), "tile16_b16", 1, False),
    ("band640", "k_radon_fwd_band", (32, 20), "tile32_b8", 4, True),
    ("groups448", "k_radon_fwd_band", (64, 7), "groups", 4, True),
    ("b4_520", "k_radon_fwd_lds", (128, 5), "tile16_b4", 1, False),
    ("tile1000", "k_radon_fwd_lds", (128, 8), "tile32_b8", 1, True),
    ("tile1000few", "k_radon_fwd_lds", (128, 8), "tile32_b8", 1, False),
    ("quad1028", "k_radon_fwd_quadf+quad", (128, 9), "tile32_b8", 1, False),
    ("quad1024", "k_radon_fwd_quadf+quad", (128, 8), "quad", 1, True),
    ("quad2048", "k_radon_fwd_quadf+quad", (256, 8), "quad", 1, True),
    ("dynamic", "k_radon_fwd_band", (64, 4), "tile16_b4", 1, False),
    ("ties96", "k_radon_fwd_lds", (64, 2), "tile16_b16", 1, False),
    ("ties97", "k_radon_fwd_lds", (64, 2), "tile16_b16", 1, False),
])
def test_each_case_reaches_its_path(name, fwd, bands, adj, nsplit, prep):
    case = {c[0]: c for c in C.CASES}[name]
    assert C.case_paths(case) == (fwd, bands, adj, nsplit, prep)


def test_knobs_move_the_cases_to_the_alternative_kernels():
    cases = {c[0]: c for c in C.CASES}
    assert C.case_paths(cases["band128"], 1, ["TRK_RADON_NO_BANDRES"])[:2] == ("k_radon_fwd_lds", (64, 2))
    assert C.case_paths(cases["band640"], 1, ["TRK_RADON_NO_BANDRES"])[:2] == ("k_radon_fwd_lds", (128, 5))
    assert C.case_paths(cases["quad2048"], 1, ["TRK_RADON_NO_ADJQ"])[2:] == ("tile32_b8", 1, False)
    assert C.case_paths(cases["quad1024"], 1, ["TRK_RADON_ADJ_SIMPLE"])[2] == "simple"
    # a batch never takes the split, groups or 32 x 32-below-1024-tiles routes: the 16 x 16 form with records from the pre-pass
    assert C.case_paths(cases["odd257"], 3)[2:] == ("tile16_b16", 1, True)
    assert C.case_paths(cases["groups448"], 3)[2:] == ("tile16_b16", 1, True)
    assert C.br_rows(576) == 64 and C.br_rows(640) == 32
