"""The reset preview's two entry points without a GPU: declared in include/cbev.h,
listed and bound in _lib, exported by the library (ABI 7, additive), and a null
context or a null `out` refused with a message before anything touches a device.
"""
from __future__ import annotations

import ctypes
import re

from carlabev_env_amd import _lib
from carlabev_env_amd import layout as LY


def _declared(name):
    text = open(LY.HEADER.replace("cbev_layout.h", "cbev.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"include/cbev.h does not declare {name}"
    return [" ".join(a.split()) for a in m.group(1).split(",")], text


def test_header_declares_both_entry_points():
    args, text = _declared("cbev_set_reset_preview")
    assert args == ["cbev_ctx* ctx", "int on"]
    args, _ = _declared("cbev_reset_preview_counts")
    assert args == ["cbev_ctx* ctx", "uint64_t out[2]"]
    assert re.search(r"#define\s+CBEV_ABI_VERSION\s+7\b", text)  # additive


def test_symbols_exported_and_listed():
    L = _lib.lib()
    P, I = ctypes.c_void_p, ctypes.c_int
    for name, argtypes in (("cbev_set_reset_preview", [P, I]), ("cbev_reset_preview_counts", [P, P])):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(L, name)
        assert list(getattr(L, name).argtypes) == argtypes and getattr(L, name).restype is I
    assert L.cbev_abi_version() == 7


def test_null_context_and_null_out_are_refused_with_a_message():
    L = _lib.lib()
    out = (ctypes.c_uint64 * 2)()
    assert L.cbev_set_reset_preview(None, 1) == -1 and len(L.cbev_last_error()) > 0
    assert L.cbev_reset_preview_counts(None, out) == -1 and len(L.cbev_last_error()) > 0
    # the arguments are checked before the context is looked at: any non-null pointer stands in for one
    stand_in = (ctypes.c_uint8 * 64)()
    assert L.cbev_reset_preview_counts(ctypes.cast(stand_in, ctypes.c_void_p), None) == -1
    assert b"null" in L.cbev_last_error()
