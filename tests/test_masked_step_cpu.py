"""The masked step (cbev_step_masked, step(active=...), freeze_done=True): the
C-ABI surface and the argument validation, none of which needs a GPU."""
from __future__ import annotations

import ctypes
import re

import numpy as np
import pytest

from carlabev_env_amd import _lib
from carlabev_env_amd import layout as LY


def _header():
    return open(LY.HEADER.replace("cbev_layout.h", "cbev.h")).read()


def test_header_declares_step_masked():
    text = _header()
    m = re.search(r"\bint\s+cbev_step_masked\s*\(([^;]*)\)\s*;", text)
    assert m, "include/cbev.h does not declare cbev_step_masked"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["cbev_ctx* ctx", "void* records", "int n", "const void* actions", "const uint8_t* active",
                    "int repeat", "const uint8_t* prev_frames", "uint8_t* frames", "double* reward", "uint8_t* term",
                    "uint8_t* trunc", "int32_t* cause", "float* info", "void* stream"]
    assert re.search(r"#define\s+CBEV_ABI_VERSION\s+7\b", text)  # additive


def test_symbol_exported_and_listed():
    assert "cbev_step_masked" in _lib.EXPORTED_SYMBOLS
    L = _lib.lib()
    assert hasattr(L, "cbev_step_masked")
    assert len(L.cbev_step_masked.argtypes) == 14
    assert L.cbev_abi_version() == 7


def test_null_context_is_refused_with_a_message():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.cbev_step_masked(None, p, 1, p, p, 1, p, p, p, p, p, p, None, None) == -1
    assert len(L.cbev_last_error()) > 0


@pytest.mark.parametrize("fd", [0, 1, "yes", None, 2.0])
def test_freeze_done_is_validated_before_the_gpu(fd):
    from carlabev_env_amd import EnvConfig, make_env
    cfg = EnvConfig(size=128, obs_size=(128, 128), render_mode="rgb_array", obs_mode="bev_semantic")
    with pytest.raises(ValueError, match="freeze_done"):
        make_env({"env": cfg, "num_envs": 2}, freeze_done=fd)


def test_freeze_done_is_not_a_config_field():
    from carlabev_env_amd import EnvConfig
    from carlabev_env_amd.config import RunConfig
    assert "freeze_done" not in EnvConfig.model_fields and "freeze_done" not in RunConfig.model_fields


def test_active_mask_validation():
    torch = pytest.importorskip("torch")
    from carlabev_env_amd.vector_env import validate_active
    n, dev = 6, torch.device("cpu")
    for ok in (torch.ones(n, dtype=torch.bool), torch.zeros(n, dtype=torch.uint8), np.ones(n, np.bool_),
               np.zeros(n, np.uint8)):
        assert validate_active(ok, n, dev) is ok
    with pytest.raises(ValueError, match="shape"):
        validate_active(torch.ones(n + 1, dtype=torch.bool), n, dev)
    with pytest.raises(ValueError, match="shape"):
        validate_active(np.ones((n, 1), np.uint8), n, dev)
    with pytest.raises(ValueError, match="dtype"):
        validate_active(torch.ones(n, dtype=torch.float32), n, dev)
    with pytest.raises(ValueError, match="dtype"):
        validate_active(np.ones(n, np.int64), n, dev)
    with pytest.raises(ValueError, match="env on cuda:0"):
        validate_active(torch.ones(n, dtype=torch.bool), n, torch.device("cuda", 0))
    with pytest.raises(ValueError, match="torch tensor or a numpy array"):
        validate_active([1] * n, n, dev)
