"""The compact wire types of the semantic observation, host side: the pure
functions of carlabev_env_amd.obs_pipeline (wire_obs_spec, pack_bits_ref,
unpack_bits_ref) that state shapes, dtypes, refusals and the bit layout."""
from __future__ import annotations

import numpy as np
import pytest

from carlabev_env_amd import obs_pipeline as OP
from carlabev_env_amd.semantics import semantic_mask_channels

MODES = ("binary", "2-class", "4-class", "5-class", "6-class", "7-class")
FUSIONS = ("stack", "vehicle_temporal", "vehicle_weighted")
NP_DTYPE = {"float32": np.float32, "float16": np.float16, "uint8": np.uint8, "bits": np.uint8}


def test_obs_dtypes_are_the_abi_codes_in_order():
    assert OP.OBS_DTYPES == ("float32", "float16", "uint8", "bits")
    assert [OP.obs_dtype_code(d) for d in OP.OBS_DTYPES] == [0, 1, 2, 3]


@pytest.mark.parametrize("hw", [(5, 7), (128, 128)])
@pytest.mark.parametrize("mode", MODES)
def test_wire_obs_spec_shapes_and_dtypes(mode, hw):
    F = 4
    h, w = hw
    chans = semantic_mask_channels(mode)
    C = len(chans)
    for fusion in FUSIONS:
        if fusion != "stack" and "vehicle" not in chans:
            with pytest.raises(ValueError):
                OP.wire_obs_spec(mode, fusion, F, hw, "float16")
            continue
        Cw = {"stack": F * C, "vehicle_temporal": C + 2, "vehicle_weighted": C}[fusion]
        assert Cw == OP.fused_channels(mode, fusion, F)
        for dt in OP.OBS_DTYPES:
            if fusion == "vehicle_weighted" and dt in ("uint8", "bits"):
                with pytest.raises(ValueError, match="vehicle_weighted"):
                    OP.wire_obs_spec(mode, fusion, F, hw, dt)
                continue
            shape, dtype, low, high = OP.wire_obs_spec(mode, fusion, F, hw, dt)
            assert dtype == np.dtype(NP_DTYPE[dt])
            if dt == "bits":
                assert shape == (Cw, -(-h * w // 8)) and (low, high) == (0, 255)
            else:
                assert shape == (Cw, h, w) and (low, high) == (0, 1)


def test_wire_obs_spec_small_frame_last_dimension():
    shape, dtype, low, high = OP.wire_obs_spec("6-class", "stack", 4, (5, 7), "bits")
    assert shape == (24, 5) and dtype == np.uint8 and (low, high) == (0, 255)
    assert OP.wire_obs_spec("6-class", "stack", 4, (128, 128), "bits")[0] == (24, 2048)
    assert OP.wire_obs_spec("6-class", "vehicle_temporal", 4, (128, 128), "float16")[:2] == ((8, 128, 128), np.float16)
    # the default is the float32 contract
    assert OP.wire_obs_spec("6-class", "stack", 4, (128, 128)) == ((24, 128, 128), np.dtype(np.float32), 0, 1)


def test_wire_obs_spec_refusals():
    with pytest.raises(ValueError, match="obs_dtype"):
        OP.wire_obs_spec("6-class", "stack", 4, (128, 128), "bfloat16")
    with pytest.raises(ValueError, match="obs_dtype"):
        OP.obs_dtype_code("float64")
    for dt in ("uint8", "bits"):
        with pytest.raises(ValueError, match="vehicle_weighted"):
            OP.wire_obs_spec("6-class", "vehicle_weighted", 4, (128, 128), dt)
    OP.wire_obs_spec("6-class", "vehicle_weighted", 4, (128, 128), "float16")
    with pytest.raises(ValueError):  # the fusions' own checks still hold
        OP.wire_obs_spec("6-class", "vehicle_temporal", 2, (128, 128), "bits")


@pytest.mark.parametrize("P", [1, 7, 8, 9, 35, 64, 4096])
def test_pack_bits_round_trip_and_layout(P):
    rng = np.random.default_rng(P)
    x = (rng.random((3, 2, P)) < 0.5).astype(np.float32)
    packed = OP.pack_bits_ref(x)
    assert packed.dtype == np.uint8 and packed.shape == (3, 2, (P + 7) // 8)
    # the layout is numpy's little-endian packbits, plane by plane
    assert np.array_equal(packed, np.packbits(x.astype(np.uint8), axis=-1, bitorder="little"))
    for p in range(min(P, 70)):
        assert ((packed[..., p >> 3] >> (p & 7)) & 1 == x[..., p]).all()
    for dtype in (np.float32, np.float16, np.uint8):
        back = OP.unpack_bits_ref(packed, P, dtype)
        assert back.dtype == dtype and np.array_equal(back, x.astype(dtype))
    # pad bits: the unused high bits of the last byte are zero, even for all-ones planes
    ones = OP.pack_bits_ref(np.ones((P,), np.uint8))
    if P % 8:
        assert ones[-1] == (1 << (P % 8)) - 1
        assert (packed[..., -1] >> (P % 8) == 0).all()
    assert (ones[: P // 8] == 255).all()


def test_unpack_bits_ref_checks_the_byte_count():
    with pytest.raises(ValueError):
        OP.unpack_bits_ref(np.zeros((2, 4), np.uint8), 35)
