"""GPU parity of the wire types of the semantic observation
(cbev_expand_obs_typed: float32, float16, uint8, bit-packed; cbev_unpack_obs) against the
wrapper oracle (oracle/wrappers.py), through the C-ABI, and of the vector env's
obs_dtype end to end.

Bar: bit-exact. Every value of a semantic observation is 0 or 1 (the weighted
vehicle history: a multiple of 0.25), exactly representable in float16 and, for
the 0 / 1 kinds, in uint8 and in one bit; there is no tolerance to choose.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import wrappers as W
from carlabev_env_amd import obs_pipeline as OP
from carlabev_env_amd._lib import OBS_BITS, OBS_F16, OBS_F32, OBS_U8, check, lib
from carlabev_env_amd.semantics import gray_lut, rgb_lut, semantic_lut, semantic_mask_channels
from gpu_harness import P_, ptr
from gpu_scenes import CODES, GUARD, cout, dtypes_of, obs_world, out_bytes

pytestmark = pytest.mark.gpu

MODES = ("binary", "2-class", "4-class", "5-class", "6-class", "7-class")
VMODES = ("4-class", "5-class", "6-class", "7-class")
FUSION = {0: "stack", 3: "vehicle_temporal", 4: "vehicle_weighted"}
# 35, 36, 72, 96, 7056, 16384 pixels: no multiple of 4; of 4, not 8 (float32 wide, float16 narrow); of 8, not 16;
# of 32; of 16, not 32; the benchmark's
SIZES = [(5, 7), (6, 6), (9, 8), (8, 12), (84, 84), (128, 128)]
N_MAX = 9


def kinds_of(mode):
    return (0, 3, 4) if mode in VMODES else (0,)


def convert(ref: np.ndarray, dt: str) -> np.ndarray:
    """float32[..., C, h, w] (or [..., C, P]) expectation -> the wire type's bytes."""
    if dt == "float32":
        return ref.astype(np.float32)
    if dt == "float16":
        return ref.astype(np.float16)
    if dt == "uint8":
        return ref.astype(np.uint8)
    planes = ref.reshape(*ref.shape[:-2], -1) if ref.ndim >= 3 else ref
    return np.packbits(planes.astype(np.uint8), axis=-1, bitorder="little")


def typed_expand(c, ring_d, n, F, head, kind, C, lut, dt, Cout, P, offset=0, stream=None, buf=None):
    """One typed expansion into an 0xA5-filled buffer with GUARD bytes after the
    output (and `offset` bytes before it); returns (output bytes, untouched?)."""
    nb = out_bytes(dt, n, Cout, P)
    if buf is None:
        buf = torch.full((offset + nb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[offset:offset + nb]
    check(lib().cbev_expand_obs_typed(c.ctx, ptr(ring_d), n, F, head, kind, C, lut.ctypes.data_as(P_), CODES[dt],
                                      ptr(out), stream), "expand_typed")
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    intact = bool((b[:offset] == 0xA5).all() and (b[offset + nb:] == 0xA5).all())
    return b[offset:offset + nb], intact


def as_wire(raw: np.ndarray, dt, n, Cout, hw):
    if dt in ("float32", "float16"):
        return raw.view(dt).reshape(n, Cout, *hw)
    if dt == "uint8":
        return raw.reshape(n, Cout, *hw)
    return raw.reshape(n, Cout, -1)


def seeded_ring(hw, F, seed, off_palette=False):
    """uint8[F][N_MAX][h][w] of palette ids 0-9 with a dense vehicle block in every env."""
    h, w = hw
    rng = np.random.default_rng(seed)
    ring = rng.integers(0, 10, (F, N_MAX, h, w)).astype(np.uint8)
    bh, bw = h // 2 + 1, w // 2 + 1
    ring[:, :, :bh, :bw] = np.where(rng.random((F, N_MAX, bh, bw)) < 0.5, 3, ring[:, :, :bh, :bw])
    if off_palette:
        ring[rng.random(ring.shape) < 0.1] = OP.OFF_PALETTE
    return ring


@functools.lru_cache(maxsize=16)  # one case's modes x kinds
def oracle_obs(hw, F, head, mode, kind):
    """float32[N_MAX][Cout][h][w]: wrap_obs_stack on the host ring, computed once
    per case and shared by the wire types (read-only)."""
    ring = seeded_ring(hw, F, 1000 * hw[0] + 10 * F + head)
    order = [(head + 1 + f) % F for f in range(F)]  # oldest first
    ref = np.stack([W.wrap_obs_stack(ring[order, e], "bev_semantic", mode, fusion=FUSION[kind])
                    for e in range(N_MAX)])
    ref.setflags(write=False)
    return ref


# ------------------------------------------------------------ 1. typed expansion == oracle
@pytest.mark.parametrize("F,head", [(4, 1), (3, 0), (5, 4)])
@pytest.mark.parametrize("hw", SIZES)
def test_typed_expansion_matches_oracle(hw, F, head):
    c = obs_world(hw)
    P = hw[0] * hw[1]
    ring_h = seeded_ring(hw, F, 1000 * hw[0] + 10 * F + head)
    for n in (1, N_MAX):
        ring_d = torch.from_numpy(np.ascontiguousarray(ring_h[:, :n])).cuda()
        for mode in MODES:
            C = len(semantic_mask_channels(mode))
            lut = semantic_lut(mode)
            for kind in kinds_of(mode):
                Cout = cout(kind, F, C)
                ref = oracle_obs(hw, F, head, mode, kind)[:n]
                assert ref.shape == (n, Cout, *hw)
                for dt in dtypes_of(kind):
                    raw, intact = typed_expand(c, ring_d, n, F, head, kind, C, lut, dt, Cout, P)
                    want = convert(ref, dt)
                    got = as_wire(raw, dt, n, Cout, hw)
                    # every output byte is written (0xA5A5A5A5 / 0xA5A5 / 0xA5 is no float32 / float16 /
                    # uint8 value of an observation; for bits every byte is compared) and nothing past it
                    assert got.shape == want.shape and np.array_equal(got, want), (hw, n, mode, kind, dt)
                    assert intact, (hw, n, mode, kind, dt)
                    if dt == "bits" and P % 8:
                        assert (got[..., -1] >> (P % 8) == 0).all()


@pytest.mark.parametrize("hw", [(8, 12), (128, 128)])
def test_typed_expansion_into_unaligned_output(hw):
    """An output or a ring that is not 16-byte aligned takes the byte-granular kernels."""
    c = obs_world(hw)
    F, head, mode, P = 4, 1, "6-class", hw[0] * hw[1]
    n = N_MAX if P < 1000 else 2
    ring_d = torch.from_numpy(np.ascontiguousarray(seeded_ring(hw, F, 1000 * hw[0] + 10 * F + head)[:, :n])).cuda()
    lut = semantic_lut(mode)
    for kind in (0, 3, 4):
        ref = oracle_obs(hw, F, head, mode, kind)[:n]
        for dt in dtypes_of(kind):
            raw, intact = typed_expand(c, ring_d, n, F, head, kind, 6, lut, dt, cout(kind, F, 6), P,
                                       offset={"float32": 4, "float16": 2}.get(dt, 1))
            assert np.array_equal(as_wire(raw.copy(), dt, n, cout(kind, F, 6), hw), convert(ref, dt)), (kind, dt)
            assert intact, (kind, dt)
    if hw != (8, 12):
        return
    # the ring as a view that starts 1 byte into a device buffer, the output aligned
    odd = torch.empty((ring_d.numel() + 1,), dtype=torch.uint8, device="cuda")[1:]
    odd.copy_(ring_d.reshape(-1))
    assert odd.data_ptr() % 2 == 1
    for kind in (0, 3):
        ref = oracle_obs(hw, F, head, mode, kind)[:n]
        for dt in dtypes_of(kind):
            raw, intact = typed_expand(c, odd, n, F, head, kind, 6, lut, dt, cout(kind, F, 6), P)
            assert np.array_equal(as_wire(raw, dt, n, cout(kind, F, 6), hw), convert(ref, dt)), ("ring + 1", kind, dt)
            assert intact, ("ring + 1", kind, dt)


# ------------------------------------------------------------ 2. off-palette, consistency with float32
def expected_f32(ring_h, head, kind, C, lut):
    """float32[n][Cout][h][w] from the channel masks alone: bit c of lut[id] per
    pixel and frame, laid out in the kind's stack order (cbev.h, cbev_expand_obs)."""
    F = ring_h.shape[0]
    masks = lut[ring_h[[(head + 1 + f) % F for f in range(F)]]]  # [F][n][h][w], oldest first
    bits = np.stack([(masks >> c) & 1 for c in range(C)], axis=2).astype(np.float32)  # [F][n][C][h][w]
    if kind == 0:
        return bits.transpose(1, 0, 2, 3, 4).reshape(bits.shape[1], F * C, *bits.shape[3:])
    v = int(lut[3]).bit_length() - 1  # the channel the vehicle id (3) sets
    static = np.delete(bits[-1], v, axis=1)
    v0, v1, v2 = bits[-1][:, v], bits[-2][:, v], bits[-3][:, v]
    if kind == 3:
        return np.concatenate([static, np.stack([v0, v1, v2], axis=1)], axis=1)
    return np.concatenate([static, np.clip(v0 + 0.5 * v1 + 0.25 * v2, 0, 1)[:, None]], axis=1)


@pytest.mark.parametrize("hw", [(9, 8), (128, 128)])
def test_typed_equals_float32_expansion_with_off_palette_ids(hw):
    c = obs_world(hw)
    F, head, n, P = 4, 2, 3, hw[0] * hw[1]
    ring_h = np.ascontiguousarray(seeded_ring(hw, F, 77, off_palette=True)[:, :n])
    assert (ring_h == OP.OFF_PALETTE).any()
    ring_d = torch.from_numpy(ring_h).cuda()
    cases = [(mode, semantic_lut(mode), len(semantic_mask_channels(mode)), kinds_of(mode)) for mode in MODES]
    # any 16 channel masks are a valid LUT (n_channels <= 16): all 16 channels, stack only
    cases.append(("16 random masks", np.random.default_rng(5).integers(0, 1 << 16, 16).astype(np.uint32), 16, (0,)))
    for mode, lut, C, kinds in cases:
        for kind in kinds:
            Cout = cout(kind, F, C)
            f32 = torch.full((n, Cout, *hw), -7.0, dtype=torch.float32, device="cuda")
            check(lib().cbev_expand_obs(c.ctx, ptr(ring_d), n, F, head, kind, C, lut.ctypes.data_as(P_), ptr(f32),
                                        None), "expand")
            via = torch.full_like(f32, -7.0)
            check(lib().cbev_expand_obs_typed(c.ctx, ptr(ring_d), n, F, head, kind, C, lut.ctypes.data_as(P_),
                                              OBS_F32, ptr(via), None), "expand_typed f32")
            torch.cuda.synchronize()
            ref = f32.cpu().numpy()
            assert np.array_equal(via.cpu().numpy(), ref)
            assert np.array_equal(ref, expected_f32(ring_h, head, kind, C, lut)), (mode, kind)
            if mode in MODES and kind != 0:  # id 15 sets no channel: nothing of the newest frame where it is
                assert lut[OP.OFF_PALETTE] == 0
                assert not ref[:, :C - 1].transpose(1, 0, 2, 3)[:, ring_h[head] == OP.OFF_PALETTE].any()
            for dt in dtypes_of(kind):
                raw, intact = typed_expand(c, ring_d, n, F, head, kind, C, lut, dt, Cout, P)
                assert np.array_equal(as_wire(raw, dt, n, Cout, hw), convert(ref, dt)), (mode, kind, dt)
                assert intact


# ------------------------------------------------------------ 3. unpack
@pytest.mark.parametrize("pixels", [35, 96, 16384])
@pytest.mark.parametrize("rows", [1, 7, 216])
def test_unpack_obs_matches_reference(rows, pixels):
    c = obs_world()
    rng = np.random.default_rng(rows * 31 + pixels)
    nb = (pixels + 7) // 8
    packed_h = rng.integers(0, 256, (rows, nb), dtype=np.uint8)
    if pixels % 8:  # the pad bits are zero on the wire
        packed_h[:, -1] &= (1 << (pixels % 8)) - 1
    packed = torch.from_numpy(packed_h).cuda()
    idx_h = rng.integers(0, rows, 5)
    gathered = packed[torch.from_numpy(idx_h).cuda()]  # a minibatch gathered from a rollout buffer
    for code, tdt, ndt in ((OBS_F32, torch.float32, np.float32), (OBS_F16, torch.float16, np.float16),
                           (OBS_U8, torch.uint8, np.uint8)):
        for src, src_h in ((packed, packed_h), (gathered, packed_h[idx_h])):
            r = src.shape[0]
            esz = torch.empty((), dtype=tdt).element_size()
            buf = torch.full((r * pixels * esz + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            out = buf[:r * pixels * esz].view(tdt).reshape(r, pixels)
            check(lib().cbev_unpack_obs(c.ctx, ptr(src), r, pixels, code, ptr(out), None), "unpack")
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), OP.unpack_bits_ref(src_h, pixels, ndt)), (code, r)
            assert (buf[r * pixels * esz:].cpu().numpy() == 0xA5).all()
    out = torch.zeros((rows, pixels), dtype=torch.float32, device="cuda")
    assert lib().cbev_unpack_obs(c.ctx, ptr(packed), rows, pixels, OBS_BITS, ptr(out), None) != 0
    assert b"dtype" in lib().cbev_last_error()


# ------------------------------------------------------------ 4. refusals
def test_typed_expansion_refusals_leave_the_output_untouched():
    c = obs_world()
    n, F = 2, 4
    ring = torch.zeros((F, n, 128, 128), dtype=torch.uint8, device="cuda")
    out = torch.full((n * 24 * 128 * 128 * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    sem, gray, rgb = semantic_lut("6-class"), gray_lut(), rgb_lut()
    cases = [(4, 6, sem, OBS_U8), (4, 6, sem, OBS_BITS), (0, 6, sem, 4), (0, 6, sem, -1), (3, 6, sem, 17)]
    for kind, C, lut in ((1, 1, gray), (5, 1, gray), (2, 3, rgb)):
        cases += [(kind, C, lut, dt) for dt in (OBS_F32, OBS_F16, OBS_BITS)]
    for kind, C, lut, dt in cases:
        marker = f"refusal {kind}/{dt}".encode()
        assert lib().cbev_unpack_obs(None, None, 0, 0, 0, None, None) != 0  # a different message is pending
        rc = lib().cbev_expand_obs_typed(c.ctx, ptr(ring), n, F, 0, kind, C, lut.ctypes.data_as(P_), dt, ptr(out), None)
        assert rc != 0, marker
        msg = lib().cbev_last_error()
        assert msg and b"dtype" in msg, (marker, msg)
    # cbev_expand_obs's own checks hold for the typed call
    for dt in (OBS_F16, OBS_U8, OBS_BITS):
        assert lib().cbev_expand_obs_typed(c.ctx, ptr(ring), n, F, F, 0, 6, sem.ctypes.data_as(P_), dt, ptr(out), None) != 0
        assert lib().cbev_expand_obs_typed(c.ctx, ptr(ring), n, F, 0, 0, 17, sem.ctypes.data_as(P_), dt, ptr(out), None) != 0
        assert lib().cbev_expand_obs_typed(c.ctx, ptr(ring), n, F, 0, 0, 6, None, dt, ptr(out), None) != 0
        assert lib().cbev_expand_obs_typed(c.ctx, ptr(ring), n, 2, 0, 3, 6, sem.ctypes.data_as(P_), dt, ptr(out), None) != 0
        assert lib().cbev_expand_obs_typed(c.ctx, ptr(ring), n, F, 0, 3, 2, semantic_lut("2-class").ctypes.data_as(P_),
                                           dt, ptr(out), None) != 0
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    # the kinds that are uint8 already forward with CBEV_OBS_U8
    g = torch.zeros((n, F, 128, 128), dtype=torch.uint8, device="cuda")
    g2 = torch.ones_like(g)
    ring.copy_(torch.randint(0, 10, ring.shape, dtype=torch.uint8, device="cuda"))
    check(lib().cbev_expand_obs(c.ctx, ptr(ring), n, F, 1, 1, 1, gray.ctypes.data_as(P_), ptr(g), None), "gray")
    check(lib().cbev_expand_obs_typed(c.ctx, ptr(ring), n, F, 1, 1, 1, gray.ctypes.data_as(P_), OBS_U8, ptr(g2), None),
          "gray typed")
    assert torch.equal(g, g2)


# ------------------------------------------------------------ 5. env level
def _env_obs_expect(f32: "torch.Tensor", dt: str) -> np.ndarray:
    return convert(f32.cpu().numpy(), dt)


@pytest.mark.parametrize("obs_size,fusion,caps,difficulty", [
    ((96, 96), "stack", None, "rt_medium_v1"),  # resized frames
    ((128, 128), "vehicle_temporal", dict(actor_cap=0, actor_route_cap=2), "rt_no_traffic_v1"),  # folded reset
])
def test_vector_env_obs_dtype_matches_float32_env(obs_size, fusion, caps, difficulty):
    from carlabev_env_amd import EnvConfig, RandomNavigationReset, build_random_navigation_options, make_env
    from carlabev_env_amd import layout as LY
    n = 5
    cfg = EnvConfig(size=128, obs_size=obs_size, render_mode="rgb_array", obs_mode="bev_semantic",
                    semantic_mask_ch="6-class", temporal_fusion_mode=fusion, max_vehicles=6)
    opts = build_random_navigation_options(RandomNavigationReset(difficulty_id=difficulty))
    h, w = obs_size
    for copy_obs in (True, False):
        envs = {dt: make_env({"env": cfg, "num_envs": n}, caps=caps, copy_obs=copy_obs, obs_dtype=dt)
                for dt in OP.OBS_DTYPES}
        for dt, env in envs.items():
            shape, ndt, low, high = OP.wire_obs_spec("6-class", fusion, cfg.frame_stack, obs_size, dt)
            sp = env.single_observation_space
            assert tuple(sp.shape) == shape and sp.dtype == ndt and sp.low.min() == low and sp.high.max() == high
            assert tuple(env.observation_space.shape) == (n, *shape) and env.observation_space.dtype == ndt
            assert tuple(env.obs_buf.shape) == (n, *shape) and env.obs_dtype == dt

        def compare(obs, what):
            ref = obs["float32"]
            assert ref.dtype == torch.float32
            for dt in ("float16", "uint8", "bits"):
                o = obs[dt]
                assert tuple(o.shape[1:]) == envs[dt].single_observation_space.shape, (what, dt)
                assert np.array_equal(o.cpu().numpy(), _env_obs_expect(ref, dt)), (what, dt, copy_obs)
            for tdt in (torch.float32, torch.float16, torch.uint8):
                assert torch.equal(envs["bits"].unpack_obs(obs["bits"], dtype=tdt), ref.to(tdt)), (what, tdt)

        compare({dt: env.reset(seed=11, options=opts)[0] for dt, env in envs.items()}, "reset")
        for env in envs.values():
            env.attach_bank(env.build_bank([900 + k for k in range(4)], opts))
        rng = np.random.default_rng(3)
        terminated = 0
        for t in range(6):
            a = rng.integers(0, 9, n)
            compare({dt: env.step(a)[0] for dt, env in envs.items()}, f"step {t}")
            if t == 2:  # push two envs off the road, so that the next step terminates them
                for env in envs.values():
                    hrec = env.records_host()
                    for e in (1, 3):
                        LY.RecordView(hrec[e], env.layout).hd[LY.HD["X"]] += 60.0
                    env.records.copy_(torch.from_numpy(hrec))
            if t == 3:
                terminated = int(envs["float32"].term.sum())
                compare({dt: env.reset_terminated() for dt, env in envs.items()}, "reset_terminated")
        assert terminated > 0
        # a rollout of packed observations, a gathered minibatch of it, and `out`
        bits = envs["bits"]
        roll = torch.stack([bits._obs() for _ in range(3)])
        out = torch.empty((2, n, *envs["float16"].single_observation_space.shape), dtype=torch.float16, device="cuda")
        assert bits.unpack_obs(roll[[2, 0]], dtype=torch.float16, out=out) is out
        assert torch.equal(out[0], envs["float16"]._obs())
        for env in envs.values():
            env.close()


def test_obs_dtype_refused_outside_the_semantic_wrapper_stack():
    from carlabev_env_amd import EnvConfig, make_env
    from carlabev_env_amd.vector_env import CarlaBEVVectorEnv
    gray = EnvConfig(size=128, obs_size=(84, 84), render_mode="rgb_array", obs_mode="bev_rgb")
    sem = EnvConfig(size=128, obs_size=(128, 128), render_mode="rgb_array", obs_mode="bev_semantic",
                    temporal_fusion_mode="vehicle_weighted")
    with pytest.raises(ValueError, match="obs_dtype"):
        make_env({"env": gray, "num_envs": 2}, obs_dtype="bits")
    with pytest.raises(ValueError, match="obs_dtype"):
        CarlaBEVVectorEnv({"env": sem, "num_envs": 2}, wrappers=False, obs_dtype="float16")
    with pytest.raises(ValueError, match="obs_dtype"):
        make_env({"env": sem, "num_envs": 2}, obs_dtype="int8")
    for dt in ("uint8", "bits"):
        with pytest.raises(ValueError, match="vehicle_weighted"):
            make_env({"env": sem, "num_envs": 2}, obs_dtype=dt)
    env = make_env({"env": sem, "num_envs": 2}, obs_dtype="float16")  # the fractional channel fits float16
    assert env.single_observation_space.dtype == np.float16 and env.obs_buf.dtype == torch.float16
    env.close()


# ------------------------------------------------------------ 6. graph capture
@pytest.mark.parametrize("dt,kind", [("bits", 0), ("uint8", 3), ("float16", 4)])
def test_typed_expansion_under_graph_capture(dt, kind):
    """cbev_expand_obs_typed allocates nothing: captured once, each replay expands
    the ring as it is at replay time."""
    hw, F, head, n, mode = (128, 128), 4, 1, 3, "6-class"
    c = obs_world(hw)
    P, Cout, lut = hw[0] * hw[1], cout(kind, F, 6), semantic_lut(mode)
    order = [(head + 1 + f) % F for f in range(F)]
    rings = [np.ascontiguousarray(seeded_ring(hw, F, s)[:, :n]) for s in (21, 22)]
    ring_d = torch.from_numpy(rings[0]).cuda()
    nb = out_bytes(dt, n, Cout, P)
    buf = torch.full((nb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            check(lib().cbev_expand_obs_typed(c.ctx, ptr(ring_d), n, F, head, kind, 6, lut.ctypes.data_as(P_),
                                              CODES[dt], ptr(buf), P_(torch.cuda.current_stream().cuda_stream)),
                  "expand_typed (capture)")
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())  # the capture ran nothing
    for ring_h in rings:
        ring_d.copy_(torch.from_numpy(ring_h))
        g.replay()
        torch.cuda.synchronize()
        ref = np.stack([W.wrap_obs_stack(ring_h[order, e], "bev_semantic", mode, fusion=FUSION[kind])
                        for e in range(n)])
        b = buf.cpu().numpy()
        assert np.array_equal(as_wire(b[:nb], dt, n, Cout, hw), convert(ref, dt))
        assert (b[nb:] == 0xA5).all()
