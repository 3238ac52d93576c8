"""Directed GPU parity over the authored edge cases (tests/edge_cases.py): the
device step against the C oracle on states the scene generator never produces.
The oracle's frames and rebuilt routes for these cases are themselves checked
against independent restatements, and the cases' branch coverage is counted, in
test_edge_cases_cpu.py.

Same bar as test_gpu_parity.py (run_parity): reset and step frames, whole
records, flags, rewards and info after every step, and no error flag at the end
(no CBEV_ERR_RASTER_WINDOW).

The actor target search matrix (EC.actor_search_batch) is held to the float64
NumPy statement as well: every actor's AI_TIDX is an integer run_parity
compares exactly, and the oracle's equals max(tid0, argmin hypot) on the CPU.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import edge_cases as EC
from carlabev_env_amd import layout as LY
from carlabev_env_amd._lib import lib
from carlabev_env_amd._lib import check
from gpu_harness import assert_same_state, error_flags, make_lanes, reset_counts, step_all, step_repeat
from gpu_scenes import cached_bank_frames_match_render, run_parity

pytestmark = pytest.mark.gpu


def _run(P, padded, caps, recs, acts, **kw):
    return run_parity(None, len(recs), len(acts), caps=caps, recs=recs, world_=(P, padded), acts=acts, **kw)


@pytest.mark.parametrize("geo", EC.GEOMETRIES, ids=[f"{s}-{a}" for s, a in EC.GEOMETRIES])
def test_raster_matrix(geo):
    """Headings x positions x painted content of one geometry: reset, a step with
    nothing pressed (the pose stays), a step with gas."""
    P, padded, caps, recs, layout, acts = EC.raster_batch(*geo)
    _run(P, padded, caps, recs, acts)


REDUCED_IDS = [EC.reduced_id(g) for g in EC.REDUCED_GEOMETRIES]


def _reduced_batch(geo):
    P, padded, _ = EC.reduced_world(*geo)
    return EC.raster_batch(*geo[:2], world=(P, padded))


@pytest.mark.parametrize("geo", EC.REDUCED_GEOMETRIES, ids=REDUCED_IDS)
def test_raster_matrix_reduced_crop(geo):
    """The same matrix under a crop smaller than the reference's (any crop in
    [size, 400] is accepted): the rotated surface misses part of the output and
    samples leave the crop, so most envs take tile_out_check (black outside the
    surface, crop_background's painted corner, windows clipped by the crop, r90
    on the checked path), through k_ego's RS_FAST word in the steps and through
    raster_job<RESET> in the reset. Sizes 128 and 256 run the split step."""
    P, padded, caps, recs, layout, acts = _reduced_batch(geo)
    _run(P, padded, caps, recs, acts)


def test_reduced_crop_fov_masked():
    """overlay16's corner mask after tile_out_check (every env at this geometry)."""
    P, padded, caps, recs, layout, acts = _reduced_batch((128, 0.2, 150, 241))
    _run(P, padded, caps, recs, acts, fov=True)


@pytest.mark.parametrize("geo", [(64, 0.2, 70, 119), (128, 0.2, 150, 241)], ids=["64-crop70", "128-crop150"])
def test_reduced_crop_bank_frames_match_render(geo):
    """k_bank_frames, cbev_reset_frames and cbev_reset into a 4-slot ring (nout = 4
    in tile_out_check) where every reset frame takes the checked path, against
    each other and against the oracle's reset frames."""
    P, padded, caps, recs, layout, _ = _reduced_batch(geo)
    cached_bank_frames_match_render(P, padded, caps, np.ascontiguousarray(recs[0::7][:48]),
                                     np.ascontiguousarray(recs[3::40][:9]), 4)


def test_reduced_crop_split_equals_unsplit_bitwise():
    """tile_out_check shares k_raster's launch with the tail workgroups of the
    split step: the matrix's two steps at (128, 0.5, crop 128) in two contexts,
    unsplit and split, frames, records and outputs equal bit for bit."""
    P, padded, caps, recs, layout, acts = _reduced_batch((128, 0.5, 128, 128))
    lanes = make_lanes(P, padded, caps, recs, None, 1, [dict(split=0), dict(split=1)], stats=False)
    A, B = lanes
    torch.cuda.synchronize()
    assert torch.equal(A.ring, B.ring), "reset frames"
    for t in range(len(acts)):
        step_all(lanes, acts[t], t)
        assert torch.equal(A.ring, B.ring), (t, "frames")
        assert torch.equal(A.recs, B.recs), (t, "records")
        for k in A.out:
            assert torch.equal(A.out[k], B.out[k]), (t, k)
    assert error_flags(A.dw.ctx) == 0 and error_flags(B.dw.ctx) == 0


def _create(P):
    L = lib()
    ctx = ctypes.c_void_p()
    rc = L.cbev_create(ctypes.byref(P), ctypes.byref(EC.CAPS_RASTER.c()), 0, ctypes.byref(ctx))
    return rc, ctx, L.cbev_last_error()


@pytest.mark.parametrize("size", [64, 128, 256])
def test_crop_range_at_create(size):
    """crop = size - 1 is refused with a message naming it; the ends of the
    accepted range, size and 400, create and destroy (nothing is launched)."""
    P0, _, _ = EC.authored_world(size, 0.5)
    P = type(P0).from_buffer_copy(P0)
    P.crop = size - 1
    rc, ctx, msg = _create(P)
    assert rc != 0 and f"crop {size - 1}".encode() in msg and not ctx.value
    for crop in (size, 400):
        P.crop = crop
        rc, ctx, msg = _create(P)
        assert rc == 0 and ctx.value, (crop, msg)
        lib().cbev_destroy(ctx)


def test_render_surface_below_crop_is_refused():
    """A render surface narrower or lower than the crop (d_crop_origin would
    clamp its maximum to 0 and the staging read a crop-wide window from a
    smaller map): refused at cbev_create, each axis alone."""
    P0, _, _ = EC.authored_world(128, 0.5)
    for mw, mh in ((100, 1280), (1024, 100)):
        P = type(P0).from_buffer_copy(P0)
        P.pad, P.crop = 10, 128
        P.map_w, P.map_h = mw, mh
        P.render_w, P.render_h = mw + 2 * P.pad, mh + 2 * P.pad
        P.map_pitch = (P.render_w + 63) // 64 * 64
        rc, ctx, msg = _create(P)
        assert rc != 0 and b"smaller than crop 128" in msg and not ctx.value, msg
    P.map_w = P.map_h = 108  # render 128 x 128 = the crop: accepted
    P.render_w = P.render_h = P.map_pitch = 128
    rc, ctx, msg = _create(P)
    assert rc == 0 and ctx.value, msg
    lib().cbev_destroy(ctx)


def test_crop_above_400_is_refused():
    """256 with anchor_y 0.2 or 0.8 gives crop 482: cbev_create refuses it."""
    for ay in (0.2, 0.8):
        P, _, _ = EC.authored_world(256, ay)
        assert P.crop == 482
        L = lib()
        ctx = ctypes.c_void_p()
        rc = L.cbev_create(ctypes.byref(P), ctypes.byref(EC.CAPS_RASTER.c()), 0, ctypes.byref(ctx))
        assert rc != 0 and b"crop 482" in L.cbev_last_error()


def test_more_than_64_actors_painted():
    """70 vehicles and 10 pedestrians in one crop: paint_tile's actor loops past thread 63."""
    P, padded, caps, recs, layout, acts = EC.many_actor_batch()
    _run(P, padded, caps, recs, acts)


@pytest.mark.parametrize("caps", [EC.CAPS_EGO8, EC.CAPS_EGO16], ids=["ego8", "ego16"])
def test_long_ego_routes(caps):
    """Ego routes of 33 to 128 points: vis / vis_draw words 1-3, the target paint
    past thread 63, k_ego's S2 and S5 past their prefetch (16 envs per workgroup
    at the small capacities), consumption and TIDX across word boundaries."""
    P, padded, caps, recs, layout, acts, _ = EC.long_route_batch(caps)
    _run(P, padded, caps, recs, acts)


def test_long_ego_routes_64_envs_per_workgroup(monkeypatch):
    monkeypatch.setenv("CBEV_EGO_NE", "64")
    P, padded, caps, recs, layout, acts, _ = EC.long_route_batch(EC.CAPS_EGO16)
    _run(P, padded, caps, recs, acts)


@pytest.mark.parametrize("caps", EC.CAPS_RETREAT, ids=["slots32", "slots48", "slots96"])
def test_retreats_at_pinned_route_lengths(caps):
    """wave_start_retreat at NROUTE 2 to 13, 32, 63 and 64, the +1e-3 fallback, a
    dropped duplicate first point, and sixteen retreats in one wave on one step;
    then the walk along the rebuilt routes. 32, 48 and 96 actor slots:
    k_actors_g4, k_actors<false>, k_actors<true>."""
    P, padded, caps, recs, layout, acts, cases = EC.retreat_batch(caps)
    seen = {}

    def on_step(t, views, causes):
        if t == 0:
            seen["nroute"] = sorted(int(v.ai[LY.AI["NROUTE"], s]) for v, cs in zip(views, cases) for s, _, _ in cs)
            seen["state"] = {int(v.ai[LY.AI["BSTATE"], s]) for v, cs in zip(views, cases) for s, _, _ in cs}

    _run(P, padded, caps, recs, acts, on_step=on_step)
    assert seen["state"] == {LY.BSTATE["retreating"]}
    assert set(seen["nroute"]) == set(range(2, 14)) | {32, 63, 64}


@pytest.mark.parametrize("caps", EC.CAPS_SEARCH, ids=[f"slots{c.actor_cap}" for c in EC.CAPS_SEARCH])
def test_actor_target_search_matrix(caps):
    """calc_target_index at its edges: exact ties, near-ties float32 cannot
    separate, the hypot collapse, route lengths around every block and batch
    boundary, the window's clamp, minima far behind and far ahead of the window,
    1 to 80 actors with frozen ones in between. 32, 64 and 96 actor slots:
    k_actors_g4 at every group width, k_actors<false, 1> (2 lanes and the
    unwindowed actor_search<1>), k_actors<true> (the serial path). Two steps: the
    second searches from the index the first chose. Every actor's TIDX after
    each step is the float64 NumPy arg-min's."""
    P, padded, caps, recs, layout, acts, cases = EC.actor_search_batch(caps)
    AD, AI = LY.AD, LY.AI
    want = []
    for e, row in enumerate(cases):
        v = LY.RecordView(recs[e], layout)
        want.append({slot: EC.expected_tidx(v.acx[slot, :c.n], v.acy[slot, :c.n], v.ad[AD["X"], slot], v.ad[AD["Y"], slot],
                                            v.ad[AD["YAW"], slot], c.tid0) for slot, c, _, _ in row})
    seen = []

    def on_step(t, views, causes):  # the oracle's records, which the device's equal (actor ints exactly)
        for e, (v, row) in enumerate(zip(views, cases)):
            for slot, c, aw, _ in row:
                assert v.ai[AI["TIDX"], slot] == want[e][slot], (t, e, slot, c.name, aw, int(v.ai[AI["TIDX"], slot]))
        seen.append(t)

    assert _run(P, padded, caps, recs, acts, on_step=on_step) == 0
    assert seen == list(range(EC.SEARCH_STEPS))


def test_actor_target_search_under_repeat():
    """The 32-slot matrix through cbev_step_repeat(k = 2) (k_actors_g4_rep: the
    gated body sees the same ties) against two plain steps: records, frame,
    outputs (rewards summed), statistics and reset counts equal bit for bit."""
    P, padded, caps, recs, layout, acts, cases = EC.actor_search_batch(EC.CAPS_SEARCH[0])
    n, L = len(recs), lib()
    A, B = make_lanes(P, padded, caps, recs, None, 1, [{}, {}])
    a = torch.from_numpy(np.ascontiguousarray(acts[0])).cuda()
    check(step_repeat(L, A.dw, A.recs, n, a, 2, A.ring[0], A.out), "step_repeat")
    rsum = torch.zeros(n, dtype=torch.float64, device="cuda")
    for t in range(2):
        step_all([B], acts[t], 0)
        assert not B.out["term"].any()
        rsum = rsum + B.out["rew"]
    B.out["rew"].copy_(rsum)
    torch.cuda.synchronize()
    assert_same_state(A, B, 0, n, counts_a=reset_counts(L, A.dw, n), counts_b=reset_counts(L, B.dw, n))
    assert error_flags(A.dw.ctx) == 0 and error_flags(B.dw.ctx) == 0
    got = A.recs.cpu().numpy()
    for e, row in enumerate(cases):
        v = LY.RecordView(got[e], layout)
        for slot, c, _, _ in row:
            assert v.ai[LY.AI["TIDX"], slot] == EC.expected_tidx(c.px, c.py, c.fx - EC.SEARCH_WHEELBASE, c.fy, 0.0, c.tid0)
