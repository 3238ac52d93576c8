"""Same-step autoreset (cbev_final_frames, make_env(cfg, autoreset="same_step")):
the C-ABI surface, the argument validation and the place of the new kernels in
the built library's code object, none of which needs a GPU."""
from __future__ import annotations

import ctypes
import re
import struct

import pytest

from carlabev_env_amd import _lib
from carlabev_env_amd import layout as LY

ARGS = ["cbev_ctx* ctx", "const uint8_t* ring", "int n", "int n_frames", "int head", "const uint8_t* heads",
        "const uint8_t* mask", "uint8_t* out", "int32_t* out_env", "int32_t* out_count", "void* stream"]


def _header():
    return open(LY.HEADER.replace("cbev_layout.h", "cbev.h")).read()


def test_header_declares_the_entry_point():
    m = re.search(r"\bint\s+cbev_final_frames\s*\(([^;]*)\)\s*;", _header())
    assert m, "include/cbev.h does not declare cbev_final_frames"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ARGS and len(ARGS) == 11


def test_symbol_exported_listed_and_bound_as_declared():
    L = _lib.lib()
    P, I = ctypes.c_void_p, ctypes.c_int
    assert "cbev_final_frames" in _lib.EXPORTED_SYMBOLS
    assert hasattr(L, "cbev_final_frames")
    assert list(L.cbev_final_frames.argtypes) == [P if "*" in d else I for d in ARGS]
    assert L.cbev_final_frames.restype is I


def test_abi_version_is_still_7():
    assert re.search(r"#define\s+CBEV_ABI_VERSION\s+7\b", _header())  # additive
    assert _lib.lib().cbev_abi_version() == 7


def test_null_context_is_refused_with_a_message():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.cbev_final_frames(None, p, 1, 3, 0, None, p, p, p, p, None) == -1
    assert len(L.cbev_last_error()) > 0


def _cfg(**kw):
    from carlabev_env_amd import EnvConfig
    base = dict(size=128, obs_size=(128, 128), render_mode="rgb_array", obs_mode="bev_semantic")
    base.update(kw)
    return EnvConfig(**base)


@pytest.mark.parametrize("ar", ["same-step", "SAME_STEP", "", None, True, 1])
def test_autoreset_is_validated_before_the_gpu(ar):
    from carlabev_env_amd import CarlaBEVVectorEnv, make_env
    for make in (make_env, CarlaBEVVectorEnv):
        with pytest.raises(ValueError, match="autoreset"):
            make({"env": _cfg(), "num_envs": 2}, autoreset=ar)


def test_same_step_refuses_freeze_done_before_the_gpu():
    from carlabev_env_amd import CarlaBEVVectorEnv, make_env
    for make in (make_env, CarlaBEVVectorEnv):
        with pytest.raises(ValueError, match="autoreset.*freeze_done"):
            make({"env": _cfg(), "num_envs": 2}, autoreset="same_step", freeze_done=True)


def test_autoreset_is_not_a_config_field():
    from carlabev_env_amd import EnvConfig
    from carlabev_env_amd.config import RunConfig
    assert "autoreset" not in EnvConfig.model_fields and "autoreset" not in RunConfig.model_fields


def _elf_sections(b):
    """{name: (offset, size, entsize, link)} of a little-endian ELF64 image."""
    assert b[:4] == b"\x7fELF" and b[4] == 2 and b[5] == 1
    shoff, = struct.unpack_from("<Q", b, 0x28)
    entsize, num, strndx = struct.unpack_from("<HHH", b, 0x3A)
    sh = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * entsize) for i in range(num)]
    names = sh[strndx][4]
    return {b[names + s[0]:b.index(b"\0", names + s[0])].decode(): (s[4], s[5], s[9], s[6]) for s in sh}, sh


def _kernels_by_address(lib_path):
    """The gfx950 kernels of the library's code object (the functions with a
    kernel descriptor NAME.kd), in the order of their addresses."""
    b = open(lib_path, "rb").read()
    off, size, _, _ = _elf_sections(b)[0][".hip_fatbin"]
    fat = b[off:off + size]
    assert fat[:24] == b"__CLANG_OFFLOAD_BUNDLE__", "the code objects are not an uncompressed offload bundle"
    n, = struct.unpack_from("<Q", fat, 24)
    pos, dev = 32, None
    for _ in range(n):
        o, sz, tl = struct.unpack_from("<QQQ", fat, pos)
        triple = fat[pos + 24:pos + 24 + tl].decode()
        pos += 24 + tl
        if "gfx950" in triple:
            dev = fat[o:o + sz]
    assert dev is not None, "no gfx950 code object"
    secs, sh = _elf_sections(dev)
    soff, ssize, sent, link = secs[".symtab"]
    stroff = sh[link][4]
    syms = {}
    for i in range(ssize // sent):
        nm, info, _, _, value, _ = struct.unpack_from("<IBBHQQ", dev, soff + i * sent)
        syms[dev[stroff + nm:dev.index(b"\0", stroff + nm)].decode()] = (info & 15, value)
    kernels = [(v, k) for k, (typ, v) in syms.items() if typ == 2 and k + ".kd" in syms]
    return [k for _, k in sorted(kernels)]


def test_final_frames_kernels_are_emitted_after_every_other_kernel():
    """emitted among the other kernels, k_final_frames moved them
    in the code object and config 3's step by 0.6 us. It is a template first used
    at the end of cbev.hip so that it comes last; this holds that in place."""
    order = _kernels_by_address(_lib.LIB_PATH)
    assert len(order) > 90
    new = [k for k in order if "k_final_frames" in k]
    assert len(new) == 2 and order[-2:] == new, order[-4:]
