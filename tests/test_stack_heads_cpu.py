"""Per-env frame-stack heads (cbev_step_heads, cbev_expand_obs_heads,
make_env(cfg, stack_heads="per_env")): the C-ABI surface and the argument
validation, none of which needs a GPU."""
from __future__ import annotations

import ctypes
import re

import pytest

from carlabev_env_amd import _lib
from carlabev_env_amd import layout as LY

STEP_ARGS = ["cbev_ctx* ctx", "void* records", "int n", "const void* actions", "const uint8_t* active", "int repeat",
             "uint8_t* ring", "int n_frames", "uint8_t* heads", "double* reward", "uint8_t* term", "uint8_t* trunc",
             "int32_t* cause", "float* info", "void* stream"]
EXPAND_ARGS = ["cbev_ctx* ctx", "const uint8_t* ring", "int n", "int n_frames", "const uint8_t* heads", "int kind",
               "int n_channels", "const uint32_t* channel_lut_host", "int out_dtype", "void* out", "void* stream"]


def _declared(name):
    text = open(LY.HEADER.replace("cbev_layout.h", "cbev.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"include/cbev.h does not declare {name}"
    assert re.search(r"#define\s+CBEV_ABI_VERSION\s+7\b", text)  # additive
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_both_entry_points():
    assert _declared("cbev_step_heads") == STEP_ARGS and len(STEP_ARGS) == 15
    assert _declared("cbev_expand_obs_heads") == EXPAND_ARGS and len(EXPAND_ARGS) == 11


def test_symbols_exported_and_listed():
    L = _lib.lib()
    P, I = ctypes.c_void_p, ctypes.c_int
    want = {"cbev_step_heads": [P, P, I, P, P, I, P, I, P, P, P, P, P, P, P],
            "cbev_expand_obs_heads": [P, P, I, I, P, I, I, P, I, P, P]}
    for name, argtypes in want.items():
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(L, name)
        assert list(getattr(L, name).argtypes) == argtypes, name
        assert getattr(L, name).restype is I
    # pointer arguments of the declaration are the void pointers of the binding
    for decl, argtypes in ((STEP_ARGS, want["cbev_step_heads"]), (EXPAND_ARGS, want["cbev_expand_obs_heads"])):
        assert [P if "*" in d else I for d in decl] == argtypes
    assert L.cbev_abi_version() == 7


def test_null_context_is_refused_with_a_message():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.cbev_step_heads(None, p, 1, p, p, 1, p, 3, p, p, p, p, p, None, None) == -1
    assert len(L.cbev_last_error()) > 0
    assert L.cbev_expand_obs_heads(None, p, 1, 3, p, 0, 6, p, 0, p, None) == -1
    assert len(L.cbev_last_error()) > 0


def _cfg(**kw):
    from carlabev_env_amd import EnvConfig
    base = dict(size=128, obs_size=(128, 128), render_mode="rgb_array", obs_mode="bev_semantic")
    base.update(kw)
    return EnvConfig(**base)


@pytest.mark.parametrize("sh", ["per-env", "PER_ENV", "", None, True, 1])
def test_stack_heads_is_validated_before_the_gpu(sh):
    from carlabev_env_amd import CarlaBEVVectorEnv, make_env
    for make in (make_env, CarlaBEVVectorEnv):
        with pytest.raises(ValueError, match="stack_heads"):
            make({"env": _cfg(), "num_envs": 2}, stack_heads=sh)


def test_per_env_refuses_a_resize_before_the_gpu():
    from carlabev_env_amd import CarlaBEVVectorEnv, make_env
    for make in (make_env, CarlaBEVVectorEnv):
        with pytest.raises(ValueError, match="stack_heads.*resize"):
            make({"env": _cfg(obs_size=(96, 96)), "num_envs": 2}, stack_heads="per_env")


def test_per_env_refuses_wrappers_false_before_the_gpu():
    from carlabev_env_amd import CarlaBEVVectorEnv, make_env
    for make in (make_env, CarlaBEVVectorEnv):
        with pytest.raises(ValueError, match="stack_heads.*wrappers"):
            make({"env": _cfg(), "num_envs": 2}, stack_heads="per_env", wrappers=False)


def test_stack_heads_is_not_a_config_field():
    from carlabev_env_amd import EnvConfig
    from carlabev_env_amd.config import RunConfig
    assert "stack_heads" not in EnvConfig.model_fields and "stack_heads" not in RunConfig.model_fields
