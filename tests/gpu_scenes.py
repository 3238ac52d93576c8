"""What more than one GPU test module builds or runs: the oracle parity run and
its record comparison, authored scenes (long routes, walls, size 64), the lane
pairs of the bitwise tests (built on gpu_harness.make_lanes), the evaluation
envs and the wire-type tables of the expansion tests. Not collected; nothing
here touches the GPU or the library at import.
"""
from __future__ import annotations

import dataclasses
from functools import lru_cache

import numpy as np
import torch

import edge_cases as EC
import oracle as O
from carlabev_env_amd import layout as LY
from carlabev_env_amd._lib import OBS_BITS, OBS_F16, OBS_F32, OBS_U8, check, lib
from gpu_harness import (P_, DevWorld, EpisodeStatsOn, assert_same, error_flags, make_lanes, out_bufs,
                         preview_counts, ptr, reset_counts, reset_terminated_all, set_term, step_all, term_of)
from helpers import CAPS_FULL, action_stream, bench_caps, build_records, world
import episode_fixture as EF


# ---------------------------------------------------------------------- the device against the oracle
def angles_close(a, b, tol=1e-9):
    """Headings equal modulo 2 pi. A retreat's rebuilt route is np.unwrap'ed: where a
    segment heading sits on the +-pi cut, ulp-level differences in the smoothed
    route (device Savitzky-Golay tables vs the oracle's long-double fit, device vs
    glibc sin/cos in the actor's position) can flip atan2's sign there and offset
    every later heading by exactly 2 pi, which angle_mod and cos/sin absorb."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.remainder(a - b + np.pi, 2 * np.pi) - np.pi
    return bool(np.all(np.abs(d) <= tol * (1 + np.abs(b))))


def compare_records(a: np.ndarray, b: np.ndarray, layout, tag=""):
    va, vb = LY.RecordView(a, layout), LY.RecordView(b, layout)
    ints = ("TIDX", "NROUTE", "NACT", "TILE", "COLLIDED", "ACTOR_ID", "CAUSE", "TERM", "TRUNC", "EP_LEN",
            "HAS_PREV_COMFORT", "S_PREV_VALID", "KSTEPS", "OFFROAD", "NACTSTATE")
    for k in ints:
        assert va.i(k) == vb.i(k), (tag, k, va.i(k), vb.i(k))
    assert np.array_equal(va.vis, vb.vis), (tag, "vis")
    assert np.array_equal(va.vis_draw, vb.vis_draw), (tag, "vis_draw")
    assert np.allclose(va.hd, vb.hd, rtol=1e-9, atol=1e-9, equal_nan=True), (
        tag, [(n, va.hd[i], vb.hd[i]) for n, i in LY.HD.items()
              if not np.isclose(va.hd[i], vb.hd[i], rtol=1e-9, atol=1e-9, equal_nan=True)])
    n = va.i("NACT")
    assert np.array_equal(va.ai[:, :n], vb.ai[:, :n]), (tag, "actor ints")
    yaw = LY.AD["YAW"]
    rows = [i for i in range(va.ad.shape[0]) if i != yaw]
    assert np.allclose(va.ad[rows, :n], vb.ad[rows, :n], rtol=1e-9, atol=1e-9), (tag, "actor doubles")
    assert angles_close(va.ad[yaw, :n], vb.ad[yaw, :n]), (tag, "actor yaw")
    for a in range(n):  # actor routes (rebuilt on a jaywalk retreat): smoothed up to NROUTE, raw up to NRX
        m, k = va.ai[LY.AI["NROUTE"], a], va.ai[LY.AI["NRX"], a]
        for arr in ("acx", "acy", "arx", "ary"):
            mk = k if arr in ("arx", "ary") else m
            assert np.allclose(getattr(va, arr)[a, :mk], getattr(vb, arr)[a, :mk], rtol=1e-9, atol=1e-9), (tag, arr, a)
        assert angles_close(va.acyaw[a, :m], vb.acyaw[a, :m]), (tag, "acyaw", a)
        # a: the device record; its float32 route copy (the target search's first
        # pass) follows every rebuild of the smoothed route
        assert np.array_equal(va.acf[a, :m, 0], va.acx[a, :m].astype(np.float32)), (tag, "acf x", a)
        assert np.array_equal(va.acf[a, :m, 1], va.acy[a, :m].astype(np.float32)), (tag, "acf y", a)
        # and its pruning circles (acb) hold every block's float32 points
        assert acb_holds(va.acb[a], va.acf[a, :m]), (tag, "acb", a)


def acb_holds(acb, pts) -> bool:
    """Every float32 route point lies inside its block's circle (cbev_layout.h acb)."""
    P = LY.ACB_PTS
    for b in range((len(pts) + P - 1) // P):
        w0, w1 = int(acb[b, 0]), int(acb[b, 1])
        c = np.array([(w0 & 0xFFFF) - 32768, (w0 >> 16) - 32768], np.float64) / 8.0
        q = pts[P * b: P * (b + 1)].astype(np.float64)
        if np.hypot(q[:, 0] - c[0], q[:, 1] - c[1]).max() > w1 / 8.0:
            return False
    return True


def info_of(v, cause):
    """The per-step export cbev_step writes to `info` (include/cbev.h), from an oracle record."""
    o = np.zeros(16, np.float32)
    o[0:7] = v.hd[LY.HD["C_SPEED"]:LY.HD["C_SPEED"] + 7]
    o[7:11] = v.hd[LY.HD["U_GAS"]:LY.HD["U_GAS"] + 4]
    o[11] = v.h("REWARD")
    o[12] = v.h("DIST2WP")
    o[13] = v.i("TILE")
    o[14] = v.i("COLLIDED")
    o[15] = v.i("NACTSTATE")
    return o


def run_parity(kinds, n_envs, steps, size=128, profile="discrete9_v1", reward="carl_base_v1", seed0=0, anchor_y=0.5,
               act_seed=1234, edit=None, fov=False, caps=CAPS_FULL, options=None, acts=None, on_step=None,
               stats=False, recs=None, world_=None):
    """Every env of a small batch stepped on the device and by the oracle, compared
    whole after each step. recs (with world_ = (P, padded map) and caps): authored
    records (tests/edge_cases.py) instead of the scene builder's; acts: an
    explicit (steps, n[, 3]) action array instead of the seeded stream; on_step(t, views, causes): sees the oracle's records after
    each step (branch-coverage probes); stats: with the device episode statistics
    on (EpisodeStatsOn), the headline's k_ego variant."""
    if recs is not None:  # authored records: no scene generator (size 64 has none that works)
        P, padded = world_
        layout = LY.Layout.make(caps)
        recs = recs.copy()
        assert recs.shape == (n_envs, layout.record_bytes) and edit is None
    else:
        cfg, P, padded, layout, builder = world(size, profile, reward, anchor_y, caps=caps)
        if options is None:
            recs, _ = build_records(builder, n_envs, kinds, seed0=seed0)
        else:  # explicit scene options (e.g. more vehicles than the difficulty presets)
            recs, _ = builder.build_many([seed0 + i for i in range(n_envs)],
                                         lambda k, s: dict(options[k % len(options)], scene_seed=s))
    if edit is not None:  # hand-made states on top of the seeded scenes
        edit(recs, layout, P)
    dw = DevWorld(P, padded, caps)
    L = lib()
    S = P.size
    omask = None
    if fov:  # device: the product's mask; oracle: its own restatement, blacked out after the render
        import wrappers as W
        from carlabev_env_amd.fov_mask import fov_corner_mask
        dmask = fov_corner_mask(S)
        check(L.cbev_set_fov_mask(dw.ctx, dmask.ctypes.data_as(P_)), "fov")
        omask = W.fov_mask(S)
    d_recs = torch.from_numpy(recs.copy()).cuda()
    d_frames = torch.zeros((n_envs, S, S), dtype=torch.uint8, device="cuda")
    check(L.cbev_reset(dw.ctx, ptr(d_recs), n_envs, None, 0, None, None, 0, ptr(d_frames), 1, None), "reset")
    orc = O.Oracle(P, padded, caps.c(), layout.record_bytes)
    h_frames = np.zeros((n_envs, S, S), np.uint8)
    for e in range(n_envs):
        orc.reset_obs(recs[e], h_frames[e])
        if omask is not None:
            h_frames[e][omask] = 8  # CBEV_PX_BLACK
    torch.cuda.synchronize()
    assert np.array_equal(d_frames.cpu().numpy(), h_frames), "reset frames differ"
    if acts is None:
        acts = action_stream(P, n_envs, steps, seed=act_seed)
    st = EpisodeStatsOn(dw.ctx, n_envs) if stats else None
    rew, term, trunc, cause, info = out_bufs(n_envs).values()
    n_term = 0
    for t in range(steps):
        a = torch.from_numpy(np.ascontiguousarray(acts[t])).cuda()
        check(L.cbev_step(dw.ctx, ptr(d_recs), n_envs, ptr(a), ptr(d_frames), ptr(rew), ptr(term), ptr(trunc),
                          ptr(cause), ptr(info), None), "step")
        h_cause = np.zeros(n_envs, np.int32)
        for e in range(n_envs):
            h_cause[e] = orc.step_one(recs[e], np.ascontiguousarray(acts[t, e]), h_frames[e])
            if omask is not None:
                h_frames[e][omask] = 8  # CBEV_PX_BLACK
        torch.cuda.synchronize()
        df = d_frames.cpu().numpy()
        bad = np.argwhere(df != h_frames)
        assert bad.size == 0, (t, bad[:8], df[tuple(bad[0])], h_frames[tuple(bad[0])])
        dr = d_recs.cpu().numpy()
        for e in range(n_envs):
            compare_records(dr[e], recs[e], layout, tag=(t, e))
        views = [LY.RecordView(recs[e], layout) for e in range(n_envs)]
        assert np.array_equal(term.cpu().numpy(), np.array([v.i("TERM") for v in views], np.uint8))
        assert np.array_equal(trunc.cpu().numpy(), np.array([v.i("TRUNC") for v in views], np.uint8))
        assert np.allclose(rew.cpu().numpy(), [v.h("REWARD") for v in views], rtol=1e-9, atol=1e-12)
        # this step's cause (not the record's sticky last non-None cause) and the per-step export
        assert np.array_equal(cause.cpu().numpy(), h_cause), (t, cause.cpu().numpy(), h_cause)
        want = np.stack([info_of(v, h_cause[e]) for e, v in enumerate(views)])
        got = info.cpu().numpy()
        assert np.array_equal(got[:, 13:], want[:, 13:]), (t, "info ints")
        assert np.allclose(got, want, rtol=1e-6, atol=1e-6), (t, "info")
        if st is not None:
            st.check(t, term.cpu().numpy(), np.arange(n_envs), views, h_cause)
        if on_step is not None:
            on_step(t, views, h_cause)
        n_term += int(term.sum())
    # no raster tile exceeded its LDS window bound (CBEV_ERR_RASTER_WINDOW), no bad action index
    assert error_flags(dw.ctx) == 0
    return n_term


def edge_states(recs, layout, P):
    """One env per branch the seeded rollouts rarely reach."""
    V = [LY.RecordView(recs[e], layout) for e in range(recs.shape[0])]
    X, Y, YAW, VEL = (LY.HD[k] for k in ("X", "Y", "YAW", "V"))
    V[1].hd[X] += 40.0  # off the road: NON_DRIVABLE tile (collision) or sidewalk
    V[2].hd[X], V[2].hd[Y] = V[2].hd[LY.HD["GOAL_X"]], V[2].hd[LY.HD["GOAL_Y"]]  # on the goal: success
    V[3].hd[X] += 120.0  # far from the route: out of bounds or off-road
    V[4].hd[VEL] = 60.0  # over the CaRL speed limit, brake/clip paths
    if V[5].i("NACT") > 0:  # on an actor: vehicle / pedestrian collision
        V[5].hd[X], V[5].hd[Y] = V[5].ad[LY.AD["X"], 0], V[5].ad[LY.AD["Y"], 0]
    V[6].hd[YAW], V[6].hd[VEL] = -np.pi / 2, 0.0  # exact multiple of 90 degrees: rotate90 in the step raster
    V[7].hd[YAW] = np.pi  # yaw at the angle_mod wrap
    V[8].hd[VEL] = -3.0  # reversing
    V[9].hd[X] = 3.0  # at the map's left edge: crop clamped against the padding


def cached_bank_frames_match_render(P, padded, caps, recs, bank, F):
    n, B = len(recs), len(bank)
    dw = DevWorld(P, padded, caps)
    L = lib()
    S = P.size
    d_bank = torch.from_numpy(bank.copy()).cuda()
    mask = (torch.arange(n) % 4 != 1).to(torch.uint8).cuda()
    bidx = ((torch.arange(n) * 7) % B).to(torch.int32).cuda()
    outs = []
    for cached in (False, True):
        d_recs = torch.from_numpy(recs.copy()).cuda()
        ring = torch.full((F, n, S, S), 13, dtype=torch.uint8, device="cuda")
        for idx, off in ((bidx, 0), (None, 5)):
            if cached:
                bf = torch.zeros((B, S, S), dtype=torch.uint8, device="cuda")
                check(L.cbev_bank_frames(dw.ctx, ptr(d_bank), B, ptr(bf), None), "bank_frames")
                check(L.cbev_reset_frames(dw.ctx, ptr(d_recs), n, ptr(d_bank), B, ptr(mask), ptr(idx), off, ptr(bf),
                                          ptr(ring), F, None), "reset_frames")
            else:
                check(L.cbev_reset(dw.ctx, ptr(d_recs), n, ptr(d_bank), B, ptr(mask), ptr(idx), off, ptr(ring), F,
                                   None), "reset")
        torch.cuda.synchronize()
        outs.append((d_recs.cpu().numpy(), ring.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])
    # and the ring of a reset env is the oracle's reset frame of its bank row (second call: b = (e + 5) % B)
    orc = O.Oracle(P, padded, caps.c(), LY.Layout.make(caps).record_bytes)
    f = np.zeros((S, S), np.uint8)
    for e in range(0, n, 5):
        if e % 4 != 1:
            orc.reset_obs(bank[(e + 5) % B].copy(), f)
            for s in range(F):
                assert np.array_equal(outs[1][1][s, e], f), (S, e, s)


# ---------------------------------------------------------------------- pairs on the scene generator's records
def deferred_pair(n, B, F, caps, seed0, bank_seed0, stats=True):
    """Two lanes on the same scenes and bank: reset_terminated launched at once
    (A) and deferred into the next step (B, cbev_set_deferred_reset); with the
    device episode statistics on in both (stats: the headline's k_ego variant)."""
    cfg, P, padded, layout, builder = world(caps=caps)
    recs, _ = build_records(builder, n, ["rt_no_traffic_v1"], seed0=seed0)
    bank, _ = build_records(builder, B, ["rt_no_traffic_v1"], seed0=bank_seed0)
    return P, layout, make_lanes(P, padded, caps, recs, bank, F, (dict(deferred=0), dict(deferred=1)), stats=stats)


def split_pair(n, caps, size, kinds, seed0, bank_seed0, n_bank=53, F=3, distinct=48, bank_distinct=17):
    """Two lanes on the same records and bank, the unsplit step (0) and the
    split step (1), the reset deferred into the next step and the episode
    statistics on in both. The bank is test_stats_folded_reset_small's: every
    third row starts off the road, so an env reset from it terminates in the step
    that takes the reset; every second env starts off the road too, so the first
    step already terminates some."""
    cfg, P, padded, layout, builder = world(size, caps=caps)
    base, _ = build_records(builder, min(n, distinct), list(kinds), seed0=seed0)
    recs = base[np.arange(n) % len(base)].copy()
    for e in range(0, n, 2):
        LY.RecordView(recs[e], layout).hd[LY.HD["X"]] += 60.0
    bdist, _ = build_records(builder, bank_distinct, list(kinds), seed0=bank_seed0)
    bank = bdist[np.arange(n_bank) % bank_distinct].copy()
    for b in range(0, n_bank, 3):
        LY.RecordView(bank[b], layout).hd[LY.HD["X"]] += 60.0
    return P, make_lanes(P, padded, caps, recs, bank, F, (dict(split=0, deferred=1), dict(split=1, deferred=1)))


def twins(n, caps, size, kinds, seed0, bank_seed0, n_bank=53, F=3):
    """split_pair's two lanes with the split step and the deferred reset off
    in both: cbev_step_repeat then runs the kernels the masked step gates."""
    P, lanes = split_pair(n, caps, size, kinds, seed0, bank_seed0, n_bank=n_bank, F=F)
    L = lib()
    for lane in lanes:
        check(L.cbev_set_split_step(lane.dw.ctx, 0), "split off")
        check(L.cbev_set_deferred_reset(lane.dw.ctx, 0), "deferred off")
    return P, lanes


def mask_stream(n, steps, seed):
    """The active masks of a run, bool[steps][n]. Envs are active with
    probability 0.65; with more than 32 envs, envs 0-15 (a whole ego workgroup
    at 16 envs per workgroup) are all inactive on every fourth step, 16-31 stay
    mixed and the rest is the ragged tail; every third env is inactive on the
    first step after the reset."""
    rng = np.random.default_rng(seed)
    m = rng.random((steps, n)) < 0.65
    if n > 32:
        m[1::4, :16] = False
    m[0, ::3] = False
    m[0, 1] = True
    return m


def relaid(ring: torch.Tensor, heads: torch.Tensor) -> torch.Tensor:
    """ring2[f][e] = ring[(heads[e] + 1 + f) % F][e]: the ring whose global head F - 1 shows
    every env's frames in its own head order (oldest first)."""
    F, n = ring.shape[:2]
    f = torch.arange(F, device=ring.device)[:, None]
    slot = (heads.long()[None, :] + 1 + f) % F
    return ring[slot, torch.arange(n, device=ring.device)[None, :]].contiguous()


# ---------------------------------------------------------------------- authored records
def ego_only_64(n):
    """n ego-only scenes at size 64 (the scene generator builds none at this
    size): routes of 24 to 64 points along the map's longest straight road at
    bench config 2's capacities; every third env starts beside the road, every
    fourth at a heading across it."""
    from carlabev_env_amd.scene_pack import SceneSpec
    caps = bench_caps(2)
    P, padded, _ = EC.authored_world(64)
    y, x0, x1 = EC._road_run(64)
    specs = []
    for e in range(n):
        m = 24 + 5 * e
        sp = max(1, min(3, (x1 - x0 - 8) // (m - 1)))
        rx = [x0 + 4 + sp * i for i in range(m)]
        ry = [y + ((i // 8) % 2) for i in range(m)]
        specs.append(SceneSpec(agent_rx=rx, agent_ry=ry, initial_speed_mps=0.0, hero_jitter_seed=e,
                               actor_jitter_seed=e, vehicles=[], pedestrians=[]))
    recs, layout, views = EC.pack_records(specs, 64, caps)
    for e, v in enumerate(views):
        i = (3 * e) % (v.i("NROUTE") - 1)
        EC.set_pose(v, v.cx[i] + (9.0 if e % 3 == 2 else 0.0), v.cy[i], v.cyaw[i] + (1.3 if e % 4 == 3 else 0.0),
                    4.0 * (e % 3))
        v.hi[LY.HI["TIDX"]] = i
    return P, padded, caps, recs, layout


N_BANK, F = 53, 3  # the small bank and the 3-slot ring of the split-step pairs on authored records
# the bench's capacities of configs 2 (ego only: the reset folds into the step)
# and 3 (25 actor slots: 8 envs per tail group) with room for 128-point routes
CAPS_LONG2 = LY.Caps(128, 0, 2, 0)
CAPS_LONG3 = LY.Caps(128, 25, 288, 0)


def off_road_dy(x, y):
    """A row offset that takes (x, y) off the drivable texels of the 128 map."""
    _, _, classes = EC.authored_world(128)
    for d in range(8, 200):
        for dy in (d, -d):
            if 0 <= int(y) + dy < classes.shape[0] and classes[int(y) + dy, int(x)] != 1:
                return float(dy)
    raise AssertionError("no off-road texel above or below the road")


def long_records(n, caps, seed0, off_every):
    """n records with ego routes of 65, 127, 128, 64 and 33 points (long_route_spec),
    each placed on a route point and driving at 30 px/s; every off_every-th one
    starts off the road, so it terminates in its first step."""
    lengths = (65, 127, 128, 64, 33)
    specs = []
    for e in range(n):
        s = EC.long_route_spec(lengths[e % len(lengths)], 128, seed=seed0 + e)
        if caps.actor_cap == 0:
            s = dataclasses.replace(s, vehicles=[], pedestrians=[])
        specs.append(s)
    recs, layout, views = EC.pack_records(specs, 128, caps)
    for e, v in enumerate(views):
        nr = v.i("NROUTE")
        i = (7 * e + 3) % (nr - 1)
        EC.set_pose(v, v.cx[i], v.cy[i], v.cyaw[i], 30.0)
        if e % 2 == 0:
            v.hi[LY.HI["TIDX"]] = i
        if e % off_every == 0:
            v.hd[LY.HD["Y"]] += off_road_dy(v.cx[i], v.cy[i])
    return recs, layout


UNSPLIT_AND_PREVIEW = ((0, 1), (1, 1))


def split_lanes(P, padded, caps, recs, bank, modes=((0, None), (1, None))):
    """One lane per (split, preview) of `modes` on the same records and bank (by
    default the unsplit and the split step, the preview as the library sets it):
    the reset deferred into the next step, a 3-slot ring, the statistics on."""
    return make_lanes(P, padded, caps, recs, bank, F, [dict(split=s, preview=p, deferred=1) for s, p in modes])


def _wall_dy(classes, x, y):
    """A row offset that puts (x, y) inside class 0 (a hero tile of class 0 is a
    collision, the first thing the reward checks), with a margin for the env's
    first steps along the road."""
    for d in range(20, 200):
        for dy in (-d, d):
            yy, xx = int(y) + dy, int(x)
            if yy - 3 >= 0 and xx - 12 >= 0 and not classes[yy - 3:yy + 4, xx - 12:xx + 13].any() \
                    and classes[yy - 3:yy + 4, xx - 12:xx + 13].shape == (7, 25):
                return float(dy)
    raise AssertionError("no class-0 block above or below the road")


def _road_records(n, seed0):
    """long_records without actors, every record on one of the first points of its
    route (33 to 128 points, 3 px apart) at 30 px/s."""
    lengths = (65, 127, 128, 64, 33)
    specs = [dataclasses.replace(EC.long_route_spec(lengths[e % len(lengths)], 128, seed=seed0 + e), vehicles=[],
                                 pedestrians=[]) for e in range(n)]
    recs, layout, views = EC.pack_records(specs, 128, CAPS_LONG2)
    for e, v in enumerate(views):
        i = 2 + e % 5
        EC.set_pose(v, v.cx[i], v.cy[i], v.cyaw[i], 30.0)
        if e % 2 == 0:
            v.hi[LY.HI["TIDX"]] = i
    return recs, layout


def wall_world(n, wall_rows, n_bank=N_BANK):
    """n records on the road and a bank whose rows `wall_rows` start inside class 0:
    an env reset to one terminates in that very step, and in every later one until
    it is reset. Every other row, and every record, starts near the head of its
    route and terminates in none of the few steps of these tests."""
    P, padded, classes = EC.authored_world(128)
    recs, layout = _road_records(n, 100)
    bank, _ = _road_records(n_bank, 500)
    for b in wall_rows:
        v = LY.RecordView(bank[b], layout)
        v.hd[LY.HD["Y"]] += _wall_dy(classes, v.h("X"), v.h("Y"))
    return P, padded, recs, bank, layout


def prime(lanes, n, envs, acts):
    """Steps 0 and 1 with the envs `envs` reset by hand in between (two passes: step
    0 folded nothing), to bank rows that start inside a wall: they terminate in
    step 1, whose tail writes their previews. Returns the counts after step 1 and
    step 1's terminations (the envs whose previews exist)."""
    step_all(lanes, acts, 0)
    assert_same(lanes, 0)
    mask = np.zeros(n, np.uint8)
    mask[list(envs)] = 1
    set_term(lanes, mask)
    reset_terminated_all(lanes)
    step_all(lanes, acts, 1)
    assert_same(lanes, 1)
    term1 = term_of(lanes[1])
    assert not reset_counts(lib(), lanes[1].dw, n)[~term1].any(), "nothing terminated but the envs reset into a wall"
    assert term1[list(envs)].all(), "the envs reset into a wall terminate in step 1"
    assert preview_counts(lanes[1]) == (0, len(envs))
    return preview_counts(lanes[1]), term1


N4, T4 = 19, (1, 4, 17)


def primed_case(extra_off=()):
    """The unsplit and the split lane on wall_world's N4 envs after prime(): the envs
    T4 have terminated in step 1, so their previews exist."""
    P, padded, recs, bank, layout = wall_world(N4, tuple(T4) + tuple(extra_off))
    lanes = split_lanes(P, padded, CAPS_LONG2, recs, bank, UNSPLIT_AND_PREVIEW)
    acts = np.ones(N4, np.int32)
    base, term1 = prime(lanes, N4, T4, acts)
    return P, bank, layout, lanes, acts, base, term1


def preview_delta(lanes, base):
    hcount, fcount = preview_counts(lanes[1])
    return hcount - base[0], fcount - base[1]


# ---------------------------------------------------------------------- a bank of episodes that end at once
STATS_CAUSES = ("collision", "success", "out_of_bounds", "max_actions", "off_road")
# (cause, steps the episode lasts) of the rows one pass of stats_bank adds
STATS_ROW_KINDS = (("collision", 1), ("success", 1), ("success", 2), ("success", 3), ("out_of_bounds", 1),
                   ("max_actions", 1), ("max_actions", 2), ("max_actions", 3), ("off_road", 1))
STATS_ACTION = 1  # gas, every env on every step


def _class_dy(classes, x, y, cls):
    """The nearest row offset at which the hero's next few steps along the road (a
    5 x 14 block of texels ahead of x) lie in class cls."""
    xx = int(round(x))
    for d in range(1, 60):
        for dy in (-d, d):
            yy = int(round(y)) + dy
            if yy >= 2 and (classes[yy - 2:yy + 3, xx - 2:xx + 12] == cls).all():
                return float(dy)
    raise AssertionError(f"no block of class {cls} within 60 texels of the road")


@lru_cache(maxsize=None)
def stats_bank(max_life=3, presets=False, passes=2):
    """Ego-only records (CAPS_LONG2: the canonical reset folds into the step) under
    the shaping reward, the one profile that reaches all five terminal causes,
    each ending after 1 to max_life steps of STATS_ACTION: the hero on a class-0
    texel (collision), 1 to 3 steps short of the goal (success), 70 texels beside
    its route (out_of_bounds), KSTEPS 1 to 3 short of max_actions (max_actions,
    the truncation, which no rate counts), and on the sidewalk with OFFROAD one
    short of offroad_terminate_after (off_road). presets: every third row starts
    with EP_RETURN at about +-1e9 instead of 0, which a bank row is free to do,
    so an episode of one step can bring a large return into the window.
    CTX_ID is 100 + b and NUM_VEH b % 5, so a row's scene columns tell the rows apart.
    Returns (P, padded, bank, layout, table); table[b] = (steps to the end, cause,
    return) of row b, as the CPU oracle runs it."""
    P, padded, classes = EC.authored_world(128, reward_profile="shaping_base_v1")
    kinds = [k for _ in range(passes) for k in STATS_ROW_KINDS if k[1] <= max_life]
    lengths = (65, 127, 128, 64, 33)
    specs = [dataclasses.replace(EC.long_route_spec(lengths[b % len(lengths)], 128, seed=700 + b), vehicles=[],
                                 pedestrians=[]) for b in range(len(kinds))]
    bank, layout, views = EC.pack_records(specs, 128, CAPS_LONG2)
    rng = np.random.default_rng(77)
    for b, (v, (kind, life)) in enumerate(zip(views, kinds)):
        nr = v.i("NROUTE")
        i = nr - 2 - life if kind == "success" else 11 + b % 5
        EC.set_pose(v, v.cx[i], v.cy[i], v.cyaw[i], 30.0)
        v.hi[LY.HI["TIDX"]] = i
        if kind == "collision":
            v.hd[LY.HD["Y"]] += _class_dy(classes, v.cx[i], v.cy[i], 0)
        elif kind == "out_of_bounds":
            v.hd[LY.HD["Y"]] += 70.0
        elif kind == "max_actions":
            v.hi[LY.HI["KSTEPS"]] = P.max_actions - life
        elif kind == "off_road":
            v.hd[LY.HD["Y"]] += _class_dy(classes, v.cx[i], v.cy[i], 2)
            v.hi[LY.HI["OFFROAD"]] = P.offroad_terminate_after - 1
        v.hi[LY.HI["CTX_ID"]], v.hd[LY.HD["NUM_VEH"]] = 100 + b, float(b % 5)  # what a summary row reports of its scene
        if presets and b % 3 == 1:
            v.hd[LY.HD["EP_RETURN"]] = (-1.0) ** (b // 3) * 1e9 * rng.uniform(0.5, 1.0)
    orc = O.Oracle(P, padded, CAPS_LONG2.c(), layout.record_bytes)
    table = []
    for b, (kind, life) in enumerate(kinds):
        r, act = bank[b].copy(), np.array(STATS_ACTION, np.int32)
        for t in range(1, life + 1):
            orc.step_one(r, act, None)
            v = LY.RecordView(r, layout)
            assert bool(v.i("TERM")) == (t == life), (b, kind, life, t, v.i("CAUSE"))
        assert v.i("CAUSE") == LY.CAUSE[kind], (b, kind, LY.CAUSE_NAME[v.i("CAUSE")])
        table.append((life, LY.CAUSE[kind], float(v.h("EP_RETURN"))))
    bank.setflags(write=False)
    return P, padded, bank, layout, tuple(table)


# ---------------------------------------------------------------------- the evaluation envs
def eval_cfg(monkeypatch, max_actions, obs=128):
    """The episode limit is the reward profile's (params.build_params), so a
    small one comes from a shaping profile registered for the test."""
    from carlabev_env_amd import EnvConfig
    from carlabev_env_amd import config as CF
    monkeypatch.setitem(CF.REWARD_PROFILES, "shaping_short_eval", {"family": "shaping",
                                                                   "parameters": {"max_actions": max_actions}})
    return EnvConfig(size=128, obs_size=(obs, obs), render_mode="rgb_array", obs_mode="bev_semantic", frame_stack=4,
                     reward_mode="shaping", reward_profile_id="shaping_short_eval")


EGO_ONLY = dict(route_cap=64, actor_cap=0, actor_route_cap=2, tl_cap=0)


def eval_pair(monkeypatch, N, max_actions, **kw):
    from carlabev_env_amd import RandomNavigationReset, build_random_navigation_options, make_env
    cfg = eval_cfg(monkeypatch, max_actions)
    envs = [make_env({"env": cfg, "num_envs": N}, num_envs=N, caps=EGO_ONLY, freeze_done=fd, **kw)
            for fd in (True, False)]
    opts = build_random_navigation_options(RandomNavigationReset(difficulty_id="rt_no_traffic_v1"))
    o0, _ = envs[0].reset(seed=11, options=opts)
    o1, _ = envs[1].reset(seed=11, options=opts)
    assert torch.equal(o0, o1)
    # env e is truncated after 2 + 5 e % 37 substeps (KSTEPS counts towards max_actions;
    # the episode length counts from 0), so the envs end on different steps
    ends = 2 + (5 * np.arange(N)) % 37
    assert ends.max() < max_actions and len(set(ends.tolist())) > N // 2
    o = envs[0].layout.off["hi"] + 4 * LY.HI["KSTEPS"]
    k = torch.from_numpy((max_actions - ends).astype(np.int32)).cuda().view(torch.uint8).reshape(N, 4)
    for env in envs:
        env.records[:, o:o + 4] = k
    return envs, opts


def eval_actions(N, t):
    return np.random.default_rng(500 + t).choice(9, size=N, p=np.array([1, 8, 1, 1, 1, 1, 1, 1, 1]) / 16.0)


# ---------------------------------------------------------------------- the typed expansion's tables
CODES = {"float32": OBS_F32, "float16": OBS_F16, "uint8": OBS_U8, "bits": OBS_BITS}
GUARD = 64


def obs_world(hw=(128, 128)):
    """A size-128 context at the test capacities whose observations are hw."""
    cfg, P, padded, layout, builder = world(size=128)
    return DevWorld(P, padded, CAPS_FULL, obs_hw=None if hw == (128, 128) else hw)


def dtypes_of(kind):
    return ("float32", "float16") if kind == 4 else ("float32", "float16", "uint8", "bits")


def cout(kind, F, C):
    return {0: F * C, 3: C + 2, 4: C}[kind]


def out_bytes(dt, n, Cout, P):
    return n * Cout * {"float32": 4 * P, "float16": 2 * P, "uint8": P, "bits": (P + 7) // 8}[dt]


# ---------------------------------------------------------------------- the device against a recorded fixture
LIBM = 1e-9            # device libm against glibc / NumPy (test_gpu_parity.py's bar)
F32_ULP = 2.0 ** -23


def summary_of_row(row):
    """The fields of an episode summary row (CBEV_EP_FIELDS) under the fixture's names."""
    E = LY.EP
    return {"return": row[E["RETURN"]], "length": row[E["LENGTH"]], "mean_speed": row[E["MEAN_SPEED"]],
            "mean_abs_accel_long": row[E["MEAN_ABS_AL"]], "mean_abs_accel_lat": row[E["MEAN_ABS_ALAT"]],
            "mean_abs_jerk_long": row[E["MEAN_ABS_JL"]], "mean_abs_jerk_lat": row[E["MEAN_ABS_JLAT"]],
            "mean_abs_yaw_rate": row[E["MEAN_ABS_YR"]], "mean_abs_yaw_acc": row[E["MEAN_ABS_YACC"]],
            "comfort_violation_rate": row[E["VIOL_RATE"]], "harsh_brake_rate": row[E["HARSH_RATE"]],
            "num_vehicles": row[E["NUM_VEH"]], "len_ego_route": row[E["LEN_ROUTE_M"]]}


def fixture_info(ep, t):
    """cbev_step's per-step float32 export (include/cbev.h) from a fixture episode."""
    M = ep._fx.meta
    o = np.zeros(16, np.float64)
    o[0:7], o[7:11] = ep.comfort[t], ep.control[t]
    o[11], o[12] = ep.reward[t], ep.dist2wp[t]
    o[13], o[14], o[15] = ep.tile[t], LY.COLL[M["coll_names"][int(ep.collided[t])]], ep.n_actors_state[t]
    return o.astype(np.float32)


def replay_on_device(eps, split, ends=True):
    """The fixture episodes `eps` (one configuration) as one batch in one context
    through cbev_reset and cbev_step with the device episode statistics on,
    compared with the fixture directly after the reset and after every step: the
    records (episode_fixture.compare_step), reward / term / trunc / cause / info
    and, with ends (whole episodes, which end on their last step), the summary
    row at an env's terminal step. An env is compared up to its last recorded
    step and ignored afterwards. split: cbev_set_split_step's argument, or None
    for the context's default. Returns (env-steps compared, Deviation)."""
    n = len(eps)
    P, padded = EF.world_of(eps[0].config)
    caps = CAPS_FULL
    layout = LY.Layout.make(caps)
    recs = np.zeros((n, layout.record_bytes), np.uint8)
    for e, ep in enumerate(eps):
        need = ep.scene_spec().caps_needed()
        assert all(a <= b for a, b in zip(need, (caps.route_cap, caps.actor_cap, caps.actor_route_cap, caps.tl_cap))), need
        recs[e], _, _ = EF.pack_episode(ep, caps)
    L = lib()
    dw = DevWorld(P, padded, caps)
    if split is not None:
        check(L.cbev_set_split_step(dw.ctx, split), "split_step")
    S = P.size
    d_recs = torch.from_numpy(recs).cuda()
    frames = torch.zeros((n, S, S), dtype=torch.uint8, device="cuda")
    check(L.cbev_reset(dw.ctx, ptr(d_recs), n, None, 0, None, None, 0, ptr(frames), 1, None), "reset")
    stats = EpisodeStatsOn(dw.ctx, n)
    torch.cuda.synchronize()
    dev = EF.Deviation(libm=LIBM, actor_yaw_mod=True)
    h = d_recs.cpu().numpy()
    for e, ep in enumerate(eps):
        EF.compare_reset(ep, LY.RecordView(h[e], layout), dev, None)
    rew, term, trunc, cause, info = out_bufs(n).values()
    cont = P.action_kind == 1
    compared = rows_seen = 0
    for t in range(max(ep.n_steps for ep in eps)):
        live = [e for e, ep in enumerate(eps) if t < ep.n_steps]
        acts = np.zeros((n, 3), np.float32) if cont else np.zeros(n, np.int32)  # finished envs: nothing pressed
        for e in live:
            acts[e] = eps[e].action(t)
        a = torch.from_numpy(acts).cuda()
        check(L.cbev_step(dw.ctx, ptr(d_recs), n, ptr(a), ptr(frames), ptr(rew), ptr(term), ptr(trunc), ptr(cause),
                          ptr(info), None), "step")
        torch.cuda.synchronize()
        h = d_recs.cpu().numpy()
        h_rew, h_term, h_trunc = rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy()
        h_cause, h_info = cause.cpu().numpy(), info.cpu().numpy()
        slot = t % stats.RING
        rows = stats.rows[slot, :int(stats.counts[slot].item())].cpu().numpy()
        by_env = {int(r[LY.EP["ENV"]]): r for r in rows}
        for e in live:
            ep, tag = eps[e], (eps[e].name, t)
            EF.compare_step(ep, t, LY.RecordView(h[e], layout), int(h_cause[e]), dev)
            dev.check("reward", [h_rew[e]], [ep.reward[t]], tag + ("reward output",))
            assert h_term[e] == ep.terminated[t] and h_trunc[e] == ep.truncated[t], tag + ("term, trunc outputs",)
            want = fixture_info(ep, t)
            assert np.array_equal(h_info[e, 13:], want[13:]), tag + ("info ints", h_info[e, 13:], want[13:])
            assert np.all(np.abs(h_info[e, :13].astype(np.float64) - want[:13]) <=
                          EF.BOUND["reward"][0] + LIBM + F32_ULP * np.abs(want[:13])), tag + ("info", h_info[e], want)
            if ep.terminated[t]:
                assert e in by_env, tag + ("no summary row at the terminal step",)
                row = by_env[e]
                assert row[LY.EP["EPISODE"]] == 0, tag
                if ends:
                    EF.compare_summary(ep, summary_of_row(row), int(row[LY.EP["CAUSE"]]), dev)
                rows_seen += 1
            else:
                assert e not in by_env, tag + ("a summary row before the terminal step",)
            compared += 1
    assert compared == sum(ep.n_steps for ep in eps)
    assert rows_seen == (n if ends else sum(int(ep.terminated[-1]) for ep in eps))
    assert error_flags(dw.ctx) == 0
    return compared, dev
