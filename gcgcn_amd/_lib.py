"""ctypes binding of libgcgcn_hip.so (the C ABI declared in include/gcgcn.h).

The header is the single source of the binding: SIGNATURES is parsed from it at import, so a new entry point is bound by declaring it
there (the extension headers -- gcgcn_optim.h, gcgcn_bert_embed.h, gcgcn_producer_rec.h, gcgcn_bert_frontend.h -- are parsed the same
way into tables of their own).  There is no CPU or eager-PyTorch fallback: if the shared library is missing this module raises, and every op raises when
handed a non-GPU tensor.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# GCGCN_LIB=<path> loads another build of the same ABI (A/B timing of kernel variants)
LIB_PATH = os.environ.get("GCGCN_LIB") or os.path.join(_HERE, "lib", "libgcgcn_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gcgcn.h")
OPTIM_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gcgcn_optim.h")    # the optimiser extension, symbols gcopt_*
BERT_EMBED_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gcgcn_bert_embed.h")    # the embeddings stage, symbols gcbe_*
PRODUCER_REC_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gcgcn_producer_rec.h")    # the producer's record route, symbols gcpr_*
BERT_FRONTEND_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gcgcn_bert_frontend.h")    # the BERT model's glue, symbols gcbf_*

ABI_VERSION = 7

SALT_GAT = 0x47415431
SALT_MHA = 0x4D484131
SALT_GCN = 0x47434E31
SALT_GLUE = 0x474C5531
SALT_BERT_ATTN = 0x42415431
SALT_BERT_AO = 0x42414F31
SALT_BERT_OUT = 0x424F5531
SALT_BERT_EMB = 0x42454D31

P, I, F, L = c_void_p, c_int, c_float, c_int64  # short names for tests and tools; every device pointer crosses the ABI as void*


class MhaHook(ctypes.Structure):
    """gcgcn_mha_hook: MultiHeadAttention's work riding inside the MultiGraphConvolution calls of the same hop (include/gcgcn.h)."""
    _fields_ = [("flat_q", c_void_p), ("Q", c_void_p), ("P", c_void_p), ("A", c_void_p), ("dQ", c_void_p), ("rng_snap", c_void_p),
                ("p", ctypes.c_float)]


class EdgeRide(ctypes.Structure):
    """gcgcn_edge_ride: an edge-tensor pass riding along with a gcn_fwd / gcn_bwd call (include/gcgcn.h)."""
    _fields_ = [("B", ctypes.c_int32), ("N", ctypes.c_int32), ("D", ctypes.c_int32),
                ("inp", c_void_p), ("n_valid", c_void_p), ("out", c_void_p)]


# ---- the header's declarations as ctypes ---------------------------------------------------------------------------------------
_SCALARS = {"int": c_int, "int32_t": c_int, "int64_t": c_int64, "uint64_t": c_uint64, "float": c_float, "double": c_double}
_DECL = re.compile(r"([\w\s*]+?)\b(gcgcn_\w+)\s*\(([^()]*)\)")                     # <ret> gcgcn_<name>(<args>)
_DECL_OPTIM = re.compile(r"([\w\s*]+?)\b(gcopt_\w+)\s*\(([^()]*)\)")               # the same in gcgcn_optim.h
_DECL_BERT_EMBED = re.compile(r"([\w\s*]+?)\b(gcbe_\w+)\s*\(([^()]*)\)")          # and in gcgcn_bert_embed.h
_DECL_PRODUCER_REC = re.compile(r"([\w\s*]+?)\b(gcpr_\w+)\s*\(([^()]*)\)")        # and in gcgcn_producer_rec.h
_DECL_BERT_FRONTEND = re.compile(r"([\w\s*]+?)\b(gcbf_\w+)\s*\(([^()]*)\)")       # and in gcgcn_bert_frontend.h
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;")


def _ctype(text: str, symbol: str, named: bool = True, header: str = "include/gcgcn.h"):
    """One parameter or field ("const float* x", "int B"), or with named=False one return type ("int64_t", "void"), as ctypes.
    const char* is c_char_p, every other pointer c_void_p, a scalar what _SCALARS says; anything else raises."""
    toks = text.replace("*", " * ").split()
    if "*" in toks:
        return c_char_p if toks[:3] == ["const", "char", "*"] and toks.count("*") == 1 else c_void_p
    toks = [t for t in toks if t != "const"]
    if toks == ["void"] and not named:
        return None
    if toks and toks[0] in _SCALARS and len(toks) <= 1 + named:
        return _SCALARS[toks[0]]
    bad = toks[0] if toks and toks[0] not in _SCALARS else " ".join(toks[1:]) or "an empty declaration"
    raise RuntimeError(f"gcgcn_amd: cannot bind {symbol}: no ctypes type for {bad!r} in {text.strip()!r} ({header})")


def _parse_header(text: str, pattern=_DECL, header: str = "include/gcgcn.h"):
    """The text of gcgcn.h -> (name -> (restype, argtypes), struct -> [(field, type)]), both in the header's order.  Comments,
    preprocessor lines and the extern "C" braces are dropped; every statement left must be a typedef struct or a gcgcn_* declaration
    (`pattern`: what a declaration looks like, and `header`: the file's name in error messages; gcgcn_optim.h's symbols are
    gcopt_*)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    structs = {}
    for name, body in _STRUCT.findall(text):
        structs[name] = []
        for decl in filter(str.strip, body.split(";")):
            first, *more = decl.split(",")                                          # "int32_t B, N, D": one type, several names
            ctype = _ctype(first, name, header=header)
            if more and "*" in first:
                raise RuntimeError(f"gcgcn_amd: cannot bind {name}: several names behind a pointer in {decl.strip()!r} ({header})")
            structs[name] += [(n.replace("*", " ").split()[-1], ctype) for n in (first, *more)]
    sigs = {}
    for stmt in filter(str.strip, re.sub(r'extern\s+"C"\s*\{|\}', " ", _STRUCT.sub(" ", text)).split(";")):
        m = pattern.fullmatch(stmt.strip())
        if not m or m.group(2) in sigs:
            raise RuntimeError(f"gcgcn_amd: cannot bind {m.group(2) if m else header}: "
                               f"{'declared twice' if m else 'not a declaration'}: {' '.join(stmt.split())[:100]!r}")
        ret, name, args = m.groups()
        sigs[name] = (_ctype(ret, name, named=False, header=header),
                      [] if args.strip() == "void" else [_ctype(a, name, header=header) for a in args.split(",")])
    return sigs, structs


def _load_header():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"gcgcn_amd: {HEADER_PATH} not found. The binding is derived from the C header of the source tree; "
                           "there is no recorded copy to fall back to.")
    with open(HEADER_PATH) as f:
        sigs, structs = _parse_header(f.read())
    for cls, name in ((MhaHook, "gcgcn_mha_hook"), (EdgeRide, "gcgcn_edge_ride")):
        declared = [("inp" if n == "in" else n, t) for n, t in structs.get(name, [])]  # `in` is a Python keyword
        if cls._fields_ != declared:
            raise RuntimeError(f"gcgcn_amd: {cls.__name__}._fields_ {cls._fields_} differ from {name} in include/gcgcn.h: {declared}")
    return sigs


def _load_optim_header():
    if not os.path.exists(OPTIM_HEADER_PATH):
        raise RuntimeError(f"gcgcn_amd: {OPTIM_HEADER_PATH} not found. The binding is derived from the C headers of the source tree.")
    with open(OPTIM_HEADER_PATH) as f:
        sigs, structs = _parse_header(f.read(), _DECL_OPTIM, "include/gcgcn_optim.h")
    if structs:
        raise RuntimeError(f"gcgcn_amd: include/gcgcn_optim.h declares structs {list(structs)}; its tables travel as const void*")
    return sigs


def _load_bert_embed_header():
    if not os.path.exists(BERT_EMBED_HEADER_PATH):
        raise RuntimeError(f"gcgcn_amd: {BERT_EMBED_HEADER_PATH} not found. The binding is derived from the C headers of the source tree.")
    with open(BERT_EMBED_HEADER_PATH) as f:
        sigs, structs = _parse_header(f.read(), _DECL_BERT_EMBED, "include/gcgcn_bert_embed.h")
    if structs:
        raise RuntimeError(f"gcgcn_amd: include/gcgcn_bert_embed.h declares structs {list(structs)}; it takes plain arguments only")
    return sigs


def _load_producer_rec_header():
    if not os.path.exists(PRODUCER_REC_HEADER_PATH):
        raise RuntimeError(f"gcgcn_amd: {PRODUCER_REC_HEADER_PATH} not found. The binding is derived from the C headers of the source tree.")
    with open(PRODUCER_REC_HEADER_PATH) as f:
        sigs, structs = _parse_header(f.read(), _DECL_PRODUCER_REC, "include/gcgcn_producer_rec.h")
    if structs:
        raise RuntimeError(f"gcgcn_amd: include/gcgcn_producer_rec.h declares structs {list(structs)}; it takes plain arguments only")
    return sigs


def _load_bert_frontend_header():
    if not os.path.exists(BERT_FRONTEND_HEADER_PATH):
        raise RuntimeError(f"gcgcn_amd: {BERT_FRONTEND_HEADER_PATH} not found. The binding is derived from the C headers of the source tree.")
    with open(BERT_FRONTEND_HEADER_PATH) as f:
        sigs, structs = _parse_header(f.read(), _DECL_BERT_FRONTEND, "include/gcgcn_bert_frontend.h")
    if structs:
        raise RuntimeError(f"gcgcn_amd: include/gcgcn_bert_frontend.h declares structs {list(structs)}; it takes plain arguments only")
    return sigs


SIGNATURES = _load_header()  # name -> (restype, argtypes), in the order of include/gcgcn.h
OPTIM_SIGNATURES = _load_optim_header()  # the same for include/gcgcn_optim.h; a table of its own, so the core's stays what is recorded
BERT_EMBED_SIGNATURES = _load_bert_embed_header()  # and for include/gcgcn_bert_embed.h
PRODUCER_REC_SIGNATURES = _load_producer_rec_header()  # and for include/gcgcn_producer_rec.h
BERT_FRONTEND_SIGNATURES = _load_bert_frontend_header()  # and for include/gcgcn_bert_frontend.h

_lib = None


def lib() -> ctypes.CDLL:
    """Load the HIP library once.  Raises RuntimeError (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"gcgcn_amd: {LIB_PATH} not found. Build it with `make -C gcgcn_amd/csrc` "
                "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(OPTIM_SIGNATURES.items()) + list(BERT_EMBED_SIGNATURES.items()) + \
                list(PRODUCER_REC_SIGNATURES.items()) + list(BERT_FRONTEND_SIGNATURES.items()):
            fn = getattr(handle, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if handle.gcgcn_version() != ABI_VERSION:
            raise RuntimeError(f"gcgcn_amd: ABI version {handle.gcgcn_version()} != {ABI_VERSION}")
        _lib = handle
    return _lib


def call(name: str, *args):
    """Invoke an int-status entry point; raise RuntimeError with the library's message on failure."""
    h = lib()
    rc = getattr(h, name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {h.gcgcn_last_error().decode()}")


def layout(kind: str, *dims) -> list:
    """Offsets (in floats) of a block's flat parameter buffer, straight from the library."""
    n = {"gat": 9, "mha": 3, "gcn": 7, "producer": 17, "head": 7}[kind]
    out = (c_int64 * n)()
    call(f"gcgcn_{kind}_layout", *dims, ctypes.cast(out, c_void_p))
    return list(out)
