"""ctypes binding of libmuon_amd.so (the C-ABI declared in include/muon_amd.h).

The header is the only declaration of the C-ABI: ``SIGNATURES`` (name -> restype, argtypes) is parsed from it at
import (``parse_header``), and a prototype the parser does not recognise is an error at import, not a guess.

The shared object is built in-tree by ``muon_amd/csrc/build.py`` (hipcc, gfx950).  There is
no fallback: if the library is missing, or no MI355X-class device is visible when a kernel
is requested, the product path raises ``MuonAmdError``.

torch is imported *before* the library is loaded on purpose: the PyTorch-ROCm wheel ships its
own ``libamdhip64.so`` (SONAME ``libamdhip64.so.7``); loading ours afterwards makes the dynamic
linker reuse that already-loaded runtime, so device pointers of torch tensors are valid inside
our kernels and there is exactly one HIP runtime in the process.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmuon_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "muon_amd.h")

F32, F64 = 0, 1
TFIDF_LOG_TF, TFIDF_LOG_IDF, TFIDF_LOG_TFIDF = 1, 2, 4


class MuonAmdError(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()

_SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "size_t": C.c_size_t,
            "uint64_t": C.c_uint64, "mu_status": C.c_int}
_PROTOTYPE = re.compile(r"([\w\s\*]+?)\b(mu_\w+)\s*\(([^()]*)\)")


def _ctype(text: str, decl: str):
    """``const char*`` and ``char*`` are c_char_p; every other pointer is c_void_p, which takes an address, None,
    ``byref(...)`` and ctypes arrays - host pointers (``int* count``) as well as device pointers."""
    words = [w for w in text.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        return C.c_char_p if words[0] == "char" else C.c_void_p
    if words and words[0] in _SCALARS:
        return _SCALARS[words[0]]
    raise MuonAmdError(f"include/muon_amd.h: `{text.strip()}` in `{decl}` is no type the ctypes table knows")


def parse_header(src: str) -> dict:
    """name -> (restype, argtypes) of every prototype in the text of include/muon_amd.h.  Whatever is left after the
    comments, the preprocessor lines, the ``mu_status`` enum and the ``extern "C"`` braces must be a prototype of known
    types: anything else raises, with the declaration in the message."""
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", src, flags=re.S)
    src = re.sub(r"^\s*#.*$", " ", src, flags=re.M)
    src = re.sub(r"typedef\s+enum\s*\{[^}]*\}\s*mu_status\s*;", " ", src)
    src = re.sub(r'extern\s+"C"\s*\{|\}', " ", src)
    table = {}
    for decl in (" ".join(d.split()) for d in src.split(";")):
        if not decl:
            continue
        m = _PROTOTYPE.fullmatch(decl)
        if m is None:
            raise MuonAmdError(f"include/muon_amd.h: `{decl}` is no prototype the ctypes table understands")
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        table[name] = (_ctype(ret, decl), [_ctype(p, decl) for p in params])
    return table


# name -> (restype, argtypes): include/muon_amd.h is the one declaration of the C-ABI
with open(HEADER_PATH) as _f:
    SIGNATURES = parse_header(_f.read())


def lib():
    """Load (once) and return the ctypes handle of libmuon_amd.so."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise MuonAmdError(
                f"{LIB_PATH} is missing: build it with `python muon_amd/csrc/build.py` "
                "(or __graft_entry__.build()). muon_amd has no CPU fallback."
            )
        try:
            import torch  # noqa: F401  (loads the HIP runtime we must share; see module docstring)
        except Exception:  # pragma: no cover - torch is part of the image
            pass
        handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().mu_last_error()
        raise MuonAmdError(f"libmuon_amd error {rc}: {msg.decode() if msg else '?'}")


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().mu_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def require_gpu() -> None:
    """Fail loudly when the HIP path cannot run (no silent CPU fallback)."""
    import torch

    if not torch.cuda.is_available() or device_count() <= 0:
        raise MuonAmdError(
            "muon_amd needs an AMD Instinct (gfx950) GPU: no HIP device is visible and there "
            "is deliberately no CPU fallback. Use the reference (scverse/muon) on CPU instead."
        )
