"""The ctypes table in ops/native.py must equal the C ABI declared in
ops/csrc/abom_api.h (which the compiler holds the definitions to).

Pure text + ctypes: needs neither the built library nor a GPU.
"""

from __future__ import annotations

import ctypes
import re
from pathlib import Path

from agentbom_amd.ops import native

HEADER = Path(native.__file__).resolve().parent / "csrc" / "abom_api.h"

C_TO_CTYPES = {
    "void*": ctypes.c_void_p,
    "const void*": ctypes.c_void_p,
    "long long": ctypes.c_longlong,
    "unsigned int": ctypes.c_uint,
    "int": ctypes.c_int,
    "double": ctypes.c_double,
    "const float*": ctypes.POINTER(ctypes.c_float),
    "const char*": ctypes.c_char_p,
}

PROTOTYPE = re.compile(r"(const char\*|int)\s+(abom_\w+)\s*\(([^)]*)\)\s*;")


def _header_signatures() -> dict:
    text = re.sub(r"//[^\n]*", "", HEADER.read_text())
    sigs = {}
    for restype, name, params in PROTOTYPE.findall(text):
        assert name not in sigs, f"{name} declared twice"
        argtypes = []
        for param in filter(None, (p.strip() for p in params.split(","))):
            ctype, pname = re.fullmatch(r"(.+?)\s*(\w+)", param).groups()
            assert ctype in C_TO_CTYPES, f"{name}: parameter {pname!r} has type {ctype!r}"
            argtypes.append(C_TO_CTYPES[ctype])
        sigs[name] = (argtypes, C_TO_CTYPES[restype])
    return sigs


def test_header_declares_every_bound_function():
    assert set(_header_signatures()) == set(native._SIGNATURES)


def test_signatures_match_header():
    header = _header_signatures()
    assert len(header) >= 15
    for name, (argtypes, restype) in native._SIGNATURES.items():
        assert (list(argtypes), restype) == header[name], name
