"""Action repeat (cbev_step_repeat, action_repeat=k): the C-ABI surface and the
argument validation, none of which needs a GPU."""
from __future__ import annotations

import ctypes
import re

import pytest

from carlabev_env_amd import _lib
from carlabev_env_amd import layout as LY


def _header():
    return open(LY.HEADER.replace("cbev_layout.h", "cbev.h")).read()


def test_header_declares_step_repeat():
    text = _header()
    assert re.search(r"\bint\s+cbev_step_repeat\s*\(", text)
    m = re.search(r"#define\s+CBEV_REPEAT_MAX\s+(\d+)", text)
    assert m and int(m.group(1)) == 64 == _lib.REPEAT_MAX
    assert re.search(r"#define\s+CBEV_ABI_VERSION\s+7\b", text)  # additive


def test_symbol_exported_and_listed():
    assert "cbev_step_repeat" in _lib.EXPORTED_SYMBOLS
    L = _lib.lib()
    assert hasattr(L, "cbev_step_repeat")
    assert L.cbev_abi_version() == 7


def test_null_context_is_refused_with_a_message():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.cbev_step_repeat(None, p, 1, p, 2, p, p, p, p, p, None, None) == -1
    assert len(L.cbev_last_error()) > 0


@pytest.mark.parametrize("k", [0, 65, 2.5, -1, "4", True, None])
def test_action_repeat_is_validated_before_the_gpu(k):
    from carlabev_env_amd import EnvConfig, make_env
    cfg = EnvConfig(size=128, obs_size=(128, 128), render_mode="rgb_array", obs_mode="bev_semantic")
    with pytest.raises(ValueError, match="action_repeat"):
        make_env({"env": cfg, "num_envs": 2}, action_repeat=k)
