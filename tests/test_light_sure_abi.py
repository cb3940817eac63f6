"""swim_debug_light_sure at the C-ABI boundary (include/swimhip_debug.h): no GPU needed.

The header, the ctypes mirror and the built library must agree, the index constants must match the Python names, and
the symbol stays out of include/swimhip.h (the oracle exports every symbol of that header and has no such path)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from swimhip import LIB_PATH, _abi

INCLUDE = Path(__file__).resolve().parent.parent / "include"
HEADER = INCLUDE / "swimhip_debug.h"
# SWIM_LS_* in index order, as _abi.LIGHT_SURE_NAMES names them
DEFINES = ["SKIPPED", "FIRST_DEAD", "MIN_DEAD"]


def test_header_declares_and_ctypes_mirrors_it():
    text = HEADER.read_text()
    assert re.search(r"\bint swim_debug_light_sure\(swim_handle\* h, uint64_t\* out, size_t n\);", text)
    assert _abi.DEBUG_SIGNATURES["swim_debug_light_sure"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t])
    assert len(_abi.LIGHT_SURE_NAMES) == len(DEFINES)
    for i, (define, name) in enumerate(zip(DEFINES, _abi.LIGHT_SURE_NAMES)):
        assert re.search(rf"#define SWIM_LS_{define}\s+{i}u", text), define
        assert name == define.lower(), (define, name)


def test_main_header_does_not_declare_it(oracle):
    assert "swim_debug_light_sure" not in (INCLUDE / "swimhip.h").read_text()
    assert "swim_debug_light_sure" not in _abi.SIGNATURES
    assert not hasattr(oracle, "swim_debug_light_sure")


def test_engine_library_exports_it():
    if not LIB_PATH.exists():
        pytest.skip("libswimhip.so not built (run __graft_entry__.build())")
    lib = _abi.load(LIB_PATH)  # loading initialises no device
    fn = lib.swim_debug_light_sure
    fn.restype, fn.argtypes = _abi.DEBUG_SIGNATURES["swim_debug_light_sure"]
    out = (C.c_uint64 * len(_abi.LIGHT_SURE_NAMES))()
    # refused before any device call: a null handle, a null buffer, more entries than there are
    assert fn(None, out, len(_abi.LIGHT_SURE_NAMES)) == _abi.SWIM_EINVAL
    assert fn(None, None, 0) == _abi.SWIM_EINVAL
    assert fn(None, out, len(_abi.LIGHT_SURE_NAMES) + 1) == _abi.SWIM_EINVAL
