"""The ctypes binding is derived from include/gcgcn.h (gcgcn_amd/_lib.py: _parse_header); no GPU needed.

tests/golden/abi_signatures.json is the hand-written ``_lib.SIGNATURES`` table of the last commit that had one, recorded from that
commit's module (not from the parser): ``{symbol: {"restype": name, "argtypes": [names]}}`` with the ctypes types by name, ``c_int32``
written as ``c_int``.  The parsed table must equal it entry by entry; a symbol added to the header since is added to the fixture by
hand, which is the review of its types.  Beside that: the table against the built library in both directions, the structs, and the
parser on small inline headers.  (What one feature's argument lists have to do with another's -- a _len list is its plain twin's plus
one pointer, and so on -- is asserted in that feature's CPU suite.)"""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest

from conftest import GOLDEN
from gcgcn_amd import _lib

TYPE_NAMES = [(ctypes.c_int, "c_int"), (ctypes.c_int64, "c_int64"), (ctypes.c_uint64, "c_uint64"), (ctypes.c_float, "c_float"),
              (ctypes.c_double, "c_double"), (ctypes.c_char_p, "c_char_p"), (ctypes.c_void_p, "c_void_p"), (None, None)]
I, L, P, F = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float


def _name(t):
    """A ctypes type by name; c_int32 is c_int (one type wherever int has 32 bits, one name here)."""
    return next(n for c, n in TYPE_NAMES if t is c or (t is ctypes.c_int32 and c is ctypes.c_int))


def _header():
    with open(_lib.HEADER_PATH) as f:
        return f.read()


def test_parsed_table_equals_the_recorded_literal_table():
    with open(os.path.join(GOLDEN, "abi_signatures.json")) as f:
        recorded = json.load(f)
    parsed = {name: {"restype": _name(res), "argtypes": [_name(a) for a in args]} for name, (res, args) in _lib.SIGNATURES.items()}
    assert len(recorded) >= 104
    missing, extra = sorted(set(recorded) - set(parsed)), sorted(set(parsed) - set(recorded))
    assert not missing, f"recorded but not declared in include/gcgcn.h: {missing}"
    assert not extra, f"declared in include/gcgcn.h but not recorded in tests/golden/abi_signatures.json: {extra}"
    for name, want in recorded.items():
        got = parsed[name]
        assert got["restype"] == want["restype"], f"{name}: returns {got['restype']}, recorded {want['restype']}"
        assert len(got["argtypes"]) == len(want["argtypes"]), f"{name}: {len(got['argtypes'])} arguments, recorded {len(want['argtypes'])}"
        for i, (g, w) in enumerate(zip(got["argtypes"], want["argtypes"])):
            assert g == w, f"{name}: argument {i} is {g}, recorded {w}"


def test_table_is_in_the_headers_order():
    header = _header()
    at = [re.search(r"^\w[\w *]*\b%s\s*\(" % name, header, re.M).start() for name in _lib.SIGNATURES]
    assert at == sorted(at)


def test_every_declared_symbol_resolves_in_the_library():
    handle = ctypes.CDLL(_lib.LIB_PATH)                      # a handle of its own: nothing that lib() bound is relied on
    for name in _lib.SIGNATURES:
        assert hasattr(handle, name), f"{name} is declared in include/gcgcn.h but missing from {_lib.LIB_PATH}"
    assert _lib.lib().gcgcn_version() == _lib.ABI_VERSION == 7


def test_library_exports_nothing_the_header_does_not_declare():
    if shutil.which("nm") is None:
        pytest.skip("nm (binutils) is not installed: the library's export list cannot be read")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.fullmatch(r"gcgcn_\w+", line.split()[-1])}
    undeclared = sorted(exported - set(_lib.SIGNATURES))
    assert not undeclared, f"exported by the library but not declared in include/gcgcn.h: {undeclared}"
    assert exported == set(_lib.SIGNATURES)


def test_structs_are_the_headers():
    structs = _lib._parse_header(_header())[1]
    assert list(structs) == ["gcgcn_edge_ride", "gcgcn_mha_hook"]
    assert structs["gcgcn_mha_hook"] == _lib.MhaHook._fields_
    # `in` is a Python keyword: the field is EdgeRide.inp
    assert [("inp" if n == "in" else n, t) for n, t in structs["gcgcn_edge_ride"]] == _lib.EdgeRide._fields_
    assert ctypes.sizeof(_lib.EdgeRide) == 40 and ctypes.sizeof(_lib.MhaHook) == 56


def test_import_refuses_an_absent_header_and_a_struct_that_moved(tmp_path, monkeypatch):
    header = _header()
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "gcgcn.h"))
    with pytest.raises(RuntimeError, match="gcgcn.h not found"):
        _lib._load_header()
    moved = header.replace("int32_t B, N, D;", "int64_t B, N, D;")
    assert moved != header
    (tmp_path / "gcgcn.h").write_text(moved)
    with pytest.raises(RuntimeError, match=r"EdgeRide\._fields_ .* differ from gcgcn_edge_ride"):
        _lib._load_header()


# ---- the parser on inline headers ----------------------------------------------------------------------------------------------
def test_parser_void_argument_list():
    assert _lib._parse_header("int gcgcn_x(void);\nvoid* gcgcn_y(void);")[0] == {"gcgcn_x": (I, []), "gcgcn_y": (P, [])}


def test_parser_multi_line_declaration():
    text = "int64_t gcgcn_x(int B, const float* X,\n                const int32_t* n_valid, uint64_t salt,\n\n  double eps, void* stream);"
    assert _lib._parse_header(text)[0] == {"gcgcn_x": (L, [I, P, P, ctypes.c_uint64, ctypes.c_double, P])}


def test_parser_ignores_a_mention_in_a_comment():
    text = ("/* == gcgcn_y(B, N, D); or gcgcn_z(a,\n * b) */\nint gcgcn_x(int n); /* as gcgcn_w(n); */\n// int gcgcn_v(int n);\n"
            "#define GCGCN_K 12\nvoid gcgcn_u(void* queue);")
    assert _lib._parse_header(text)[0] == {"gcgcn_x": (I, [I]), "gcgcn_u": (None, [P])}


def test_parser_pointer_returns():
    sigs = _lib._parse_header("const void* gcgcn_x(int n);\nconst char* gcgcn_y(void);\nint gcgcn_z(const char* name, float p);")[0]
    assert sigs == {"gcgcn_x": (P, [I]), "gcgcn_y": (ctypes.c_char_p, []), "gcgcn_z": (I, [ctypes.c_char_p, F])}


def test_parser_struct_pointer_argument_and_struct_block():
    text = ("typedef struct gcgcn_s {\n  int32_t B, N;\n  const float* in; /* may be NULL */\n  float p;\n} gcgcn_s;\n"
            "int gcgcn_x(const gcgcn_s* s, const float* const* params, int32_t n);")
    sigs, structs = _lib._parse_header(text)
    assert sigs == {"gcgcn_x": (I, [P, P, I])}
    assert structs == {"gcgcn_s": [("B", I), ("N", I), ("in", P), ("p", F)]}


@pytest.mark.parametrize("text,symbol,token", [
    ("int gcgcn_x(int a, size_t n);", "gcgcn_x", "size_t"),                    # an unknown scalar
    ("int gcgcn_x(int a, uint8_t flag);", "gcgcn_x", "uint8_t"),               # known to C, not to the mapping
    ("unsigned gcgcn_x(int a);", "gcgcn_x", "unsigned"),                      # as a return type
    ("int gcgcn_x(unsigned int a);", "gcgcn_x", "unsigned"),
    ("int gcgcn_x(long long a);", "gcgcn_x", "long"),
    ("void gcgcn_x(void a);", "gcgcn_x", "void"),                             # void is a return type only
    ("int gcgcn_x();", "gcgcn_x", "empty"),                                   # (void) is how the header says "no arguments"
    ("int gcgcn_x(int a); int gcgcn_x(int b);", "gcgcn_x", "twice"),
    ("int other(int a);", "gcgcn.h", "not a declaration"),
    ("typedef struct gcgcn_s { long n; } gcgcn_s;", "gcgcn_s", "long"),
])
def test_parser_raises_on_what_it_cannot_map(text, symbol, token):
    with pytest.raises(RuntimeError) as e:
        _lib._parse_header(text)
    assert symbol in str(e.value) and token in str(e.value), str(e.value)
