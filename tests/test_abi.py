"""CPU-side checks of the drop-in boundary: libtrk.so builds for gfx950, loads, and exports every symbol that
include/trk.h declares (no compute calls — there is no GPU here).  Also: the product path fails loudly without a GPU."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    txt = open(os.path.join(REPO, "include", "trk.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(trk_[a-z0-9_]+)\s*\(", txt)))


def test_library_builds_and_exports_every_declared_symbol():
    from trips_py_amd import _lib
    path = _lib.build()
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert len(syms) >= 20
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, f"declared in trk.h but not exported: {missing}"
    # and the ctypes table binds exactly the header's entry points
    assert sorted(_lib.SIGNATURES) == syms


def test_signatures_cover_the_header_with_known_kinds():
    """The ctypes table is parsed from trk.h: it names what header_symbols() finds by another expression, in six kinds only."""
    from trips_py_amd import _lib
    kinds = {ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_float, ctypes.c_void_p, ctypes.c_char_p}
    assert sorted(_lib.SIGNATURES) == header_symbols()
    with open(os.path.join(REPO, "include", "trk.h")) as fh:
        assert _lib.parse_signatures(fh.read()) == _lib.SIGNATURES
    for name, (res, args) in _lib.SIGNATURES.items():
        assert res in (ctypes.c_int, ctypes.c_char_p), name
        assert isinstance(args, list) and set(args) <= kinds - {ctypes.c_char_p}, name


def test_signatures_of_pinned_entries():
    """Entries that together use every C kind of the header, written out as the hand-kept table had them (every pointer flavour —
    POINTER(c_int), POINTER(c_double), POINTER(c_float), POINTER(c_void_p), handles, device pointers, streams — is a c_void_p)."""
    from trips_py_amd import _lib
    i, i64, d, p = ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
    pinned = {
        "trk_last_error": (ctypes.c_char_p, []),
        "trk_op_apply": (i, [p, i, p, i64, p, i64, i, p, p]),
        "trk_axpby": (i, [i64, d, p, p, i, p, d, p, p, i, p, p, p, p]),
        "trk_csr_create": (i, [i64, i64, i64, p, p, p, p, p, p, p]),
        "trk_timer_read": (i, [p, p, i, p]),
        "trk_blockdiag_create": (i, [p, i, p]),
        "trk_cgls_iterate_recompute": (i, [p, i, i, p, p, i64, i, p, p, p, p, i64, p, p, p, p, i, p, p, p, i, p]),
        "trk_pdhg_iterate_iso": (i, [p, p, i, i, i, i, d, d, d, d, d, i, p, p, p, p, p, p, p, p, i64, i, p, p, p, p, i, p]),
    }
    for name, want in pinned.items():
        assert _lib.SIGNATURES[name] == want, name


def test_signature_parser_maps_every_kind_and_refuses_what_it_does_not_know():
    from trips_py_amd import TrkError, _lib
    i, p = ctypes.c_int, ctypes.c_void_p
    got = _lib.parse_signatures("/* int trk_not(int a); */\nint trk_a(void); // int trk_nor(int a);\nconst char* trk_b();\n"
                                "int trk_c(const float* x, trk_op* const* ops,\n          int64_t n, double c, float f, int k, trk_stream s);\n")
    assert got == {"trk_a": (i, []), "trk_b": (ctypes.c_char_p, []),
                   "trk_c": (i, [p, p, ctypes.c_int64, ctypes.c_double, ctypes.c_float, i, p])}
    for bad in ("int trk_x(short n);", "int trk_x(unsigned int n);", "int trk_x(int64_t);", "int trk_x(double v[3]);",
                "int trk_x(int n, ...);", "void trk_x(int n);", "trk_op trk_x(int n);", "int trk_x(int (*cb)(int), int n);",
                "int\ntrk_x(int n);"):
        with pytest.raises(TrkError, match="trk_x"):
            _lib.parse_signatures(bad)


def test_version_and_error_string_callable_without_gpu():
    from trips_py_amd import _lib
    lib = _lib.load()
    assert lib.trk_version() >= 100
    assert isinstance(lib.trk_last_error(), bytes)
    # argument validation happens before any HIP call
    assert lib.trk_op_shape(None, None, None) == -1
    assert b"NULL" in lib.trk_last_error()


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from trips_py_amd import TrkError
    from trips_py_amd.engine import default_engine
    from trips_py_amd.operators import Blur2D
    import numpy as np
    with pytest.raises(TrkError):
        default_engine()
    with pytest.raises(TrkError):
        Blur2D(np.ones((3, 3)) / 9, 8, 8)


def test_product_never_imports_the_oracle():
    bad = []
    for root, _dirs, files in os.walk(os.path.join(REPO, "trips_py_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) or "cpu_ref" in src:
                    bad.append(os.path.join(root, f))
    assert not bad, f"product files referencing the oracle: {bad}"
