"""Build + load libtrk.so (the C-ABI engine, include/trk.h) through ctypes.

There is NO CPU fallback: if the shared library is missing or cannot be loaded, or no GPU is
visible when a kernel is requested, the product path raises.  `build()` cross-compiles for gfx950
with hipcc (no GPU needed) into trips_py_amd/csrc/libtrk.so, in-tree, so the built library
travels with the source snapshot.
"""
import ctypes
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
LIB_PATH = os.path.join(CSRC, "libtrk.so")
SOURCES = ["core.hip", "vecops.hip", "blur2d.hip", "blur_tile.hip", "gemv.hip", "wgram.hip", "tvops.hip", "radon2d.hip", "radon_fwd.hip", "radon_adj.hip", "spmv.hip", "framelet2d.hip", "fanbeam2d.hip", "projected.hip", "host_regparam.hip", "host_worker.hip", "hybrid_host.hip", "cgls_update.hip", "cgls_loop.hip", "mrnsd.hip", "mlem.hip", "subsets.hip", "pdhg.hip", "pdhg_tv.hip", "comm.hip", "cgls_tiled.hip", "cgls_sharded.hip", "ref64.hip", "dense_svd.hip"]
HIPCC_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-I" + INCLUDE, "-I" + CSRC]


class TrkError(RuntimeError):
    pass


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise TrkError("hipcc not found: cannot build libtrk.so (ROCm toolchain required)")
    return exe


STAMP_PATH = LIB_PATH + ".stamp"


def _source_hash():
    """Hash of everything the library is built from.  Staleness is decided by content, not by modification times: a copied
    tree (the GPU box receives a snapshot) must not trigger rebuilds, least of all from eight ranks at once."""
    import hashlib
    h = hashlib.sha256(" ".join(HIPCC_FLAGS[:-2] + SOURCES).encode())
    deps = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    for path in [os.path.join(CSRC, f) for f in deps] + [os.path.join(INCLUDE, "trk.h")]:
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def _stale():
    if not os.path.exists(LIB_PATH) or not os.path.exists(STAMP_PATH):
        return True
    try:
        with open(STAMP_PATH) as fh:
            return fh.read().strip() != _source_hash()
    except OSError:
        return True


def build(force=False, verbose=False):
    """Compile every HIP source for gfx950 and link libtrk.so.  Returns the library path."""
    if not force and not _stale():
        return LIB_PATH
    # one builder at a time (several ranks may import the package together)
    import fcntl
    with open(os.path.join(CSRC, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and not _stale():
                return LIB_PATH
            return _build_locked(force, verbose)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _file_hash(paths, extra=""):
    import hashlib
    h = hashlib.sha256(extra.encode())
    for path in paths:
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def _build_locked(force, verbose):
    hipcc = _hipcc()
    srcs = [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    headers = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join(INCLUDE, "trk.h")]

    def cc(src):
        # an object is reused only if the CONTENT of its source, of every header and the flags are what it was built
        # from (modification times mean nothing in a copied tree)
        obj = os.path.join(CSRC, src.replace(".hip", ".o"))
        key = _file_hash([os.path.join(CSRC, src)] + headers, " ".join(HIPCC_FLAGS[:-2]))
        if not force and os.path.exists(obj) and os.path.exists(obj + ".stamp"):
            with open(obj + ".stamp") as fh:
                if fh.read().strip() == key:
                    return obj
        cmd = [hipcc] + HIPCC_FLAGS + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        if os.path.exists(obj + ".stamp"):
            os.unlink(obj + ".stamp")
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise TrkError(f"hipcc failed on {src}:\n{r.stdout}\n{r.stderr}")
        with open(obj + ".stamp", "w") as fh:
            fh.write(key + "\n")
        return obj

    with ThreadPoolExecutor(max_workers=min(4, len(srcs))) as ex:
        objs = list(ex.map(cc, srcs))
    if os.path.exists(STAMP_PATH):
        os.unlink(STAMP_PATH)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs + ["-ldl"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise TrkError(f"link of libtrk.so failed:\n{r.stdout}\n{r.stderr}")
    with open(STAMP_PATH, "w") as fh:
        fh.write(_source_hash() + "\n")
    return LIB_PATH


# ----------------------------------------------------------------------------- ctypes signatures
# include/trk.h is the only place the ABI is written down: a width, a count or an order that differed between a hand-kept table and
# the header would load cleanly and hand a kernel a garbage length or address.
_BY_VALUE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float": ctypes.c_float,
             "trk_stream": ctypes.c_void_p}           # typedef void* trk_stream (hipStream_t)
_DECL = re.compile(r"^[ \t]*(\w[\w \t*]*?)\b(trk_\w+)\s*\(([^()]*)\)\s*;", re.M)


def parse_signatures(header):
    """name -> (restype, [argtypes]) for every `ret trk_name(args);` in the text of trk.h.  Every pointer — device and host arrays,
    handles, out-parameters — is a c_void_p: device pointers travel as integers (tensor.data_ptr()), and c_void_p also takes
    byref(...), ctypes arrays and pointers, and None.  A type that is not spelled out here raises; nothing is guessed."""
    table = {}
    header = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)
    for ret, name, args in _DECL.findall(header):
        def kind(words):
            if "*" in words:
                return ctypes.c_void_p
            if len(words) != 1 or words[0] not in _BY_VALUE:
                raise TrkError(f"trk.h: no ctypes mapping for '{' '.join(words)}' in: {' '.join((ret + name).split())}(...)")
            return _BY_VALUE[words[0]]

        rtype, *atypes = [[w for w in part.replace("*", " * ").split() if w != "const"] for part in [ret] + args.split(",")]
        if atypes in ([[]], [["void"]]):
            atypes = []
        if not all(w == "*" or w.isidentifier() for words in atypes for w in words):       # arrays, bit widths, defaults
            raise TrkError(f"trk.h: cannot read the arguments of {name}: ({' '.join(args.split())})")
        # an argument is its type, then its name (a pointer may go without): a by-value argument without a name keeps no type and is refused
        atypes = [w if w[-1:] == ["*"] else w[:-1] for w in atypes]
        table[name] = (ctypes.c_char_p if rtype == ["char", "*"] else kind(rtype), [kind(w) for w in atypes])
    skipped = set(re.findall(r"\b(trk_\w+)\s*\(", header)) - set(table)     # a declaration _DECL cannot read must not go unbound
    if skipped:
        raise TrkError(f"trk.h: cannot read the declaration of {sorted(skipped)}")
    return table


with open(os.path.join(INCLUDE, "trk.h")) as _fh:
    SIGNATURES = parse_signatures(_fh.read())

_lib = None


def lib_path():
    return LIB_PATH


def load():
    """dlopen libtrk.so (building it first if hipcc is present and the library is stale/missing)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: its bundled libamdhip64.so (same SONAME as ROCm's) must be the HIP runtime of the
    # process, so that torch's streams / allocations and libtrk's kernels live in one runtime.
    import torch  # noqa: F401
    if _stale():
        # a stale library is never loaded silently: either the rebuild succeeds or the caller hears about it
        # (TRK_ALLOW_STALE=1: load what is there, with a warning - for boxes without hipcc)
        try:
            build()
        except TrkError as exc:
            if not os.path.exists(LIB_PATH) or os.environ.get("TRK_ALLOW_STALE", "0") != "1":
                raise TrkError(f"libtrk.so is out of date with its sources and could not be rebuilt: {exc}") from exc
            print(f"trips_py_amd: WARNING: loading a STALE libtrk.so (TRK_ALLOW_STALE=1): {exc}", file=sys.stderr)
    if not os.path.exists(LIB_PATH):
        raise TrkError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
                       "There is no CPU fallback for the engine.")
    path = LIB_PATH
    exp = os.environ.get("TRK_EXPERIMENT_LIB")
    if exp:
        # A/B measurements on ONE box (a library built from another revision of the sources, e.g. the parent commit): a library of the
        # same ABI under another path.  Announced on stderr; never set by the product.
        if not os.path.exists(exp):
            raise TrkError(f"TRK_EXPERIMENT_LIB={exp}: no such file")
        print(f"trips_py_amd: loading the EXPERIMENT library {exp} instead of {LIB_PATH}", file=sys.stderr)
        path = exp
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError here = header / library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().trk_last_error().decode("utf-8", "replace")
        exc = ValueError if rc == -1 else (NotImplementedError if rc == -4 else TrkError)   # -5 (RCCL): TrkError
        raise exc(f"{what}: trk error {rc}: {msg}")
