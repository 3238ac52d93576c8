"""The four step entries' argument checks that need no GPU."""
from __future__ import annotations

import ctypes

import pytest

from carlabev_env_amd import _lib


def _calls(L, p):
    return {
        "cbev_step": lambda: L.cbev_step(None, p, 1, p, p, p, p, p, p, None, None),
        "cbev_step_repeat": lambda: L.cbev_step_repeat(None, p, 1, p, 2, p, p, p, p, p, None, None),
        "cbev_step_masked": lambda: L.cbev_step_masked(None, p, 1, p, p, 2, p, p, p, p, p, p, None, None),
        "cbev_step_heads": lambda: L.cbev_step_heads(None, p, 1, p, p, 2, p, 3, p, p, p, p, p, None, None),
    }


@pytest.mark.parametrize("entry", ["cbev_step", "cbev_step_repeat", "cbev_step_masked", "cbev_step_heads"])
def test_null_context_is_refused_with_a_message(entry):
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert _calls(L, p)[entry]() == -1
    assert len(L.cbev_last_error()) > 0
