"""The split step's thin head: k_ego_head computes only what k_raster reads (S1,
the physics, the render set-up, vis_draw, a folded reset's record on registers,
no record staging) and the tail in k_raster's launch runs the target search
(S2), the index update and comfort after it. Against the unsplit k_ego
(bitwise) and the oracle where the move can go wrong: ego routes past the
tail's S2 prefetch, every reset composition of a head workgroup, ties in the
target search, an action index out of range in a reset and in a kept env.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import edge_cases as EC
from carlabev_env_amd import layout as LY
from carlabev_env_amd._lib import lib
from gpu_harness import (assert_same, error_flags, flush_all, reset_counts, reset_rows, reset_terminated_all, step_all,
                         term_of)
from gpu_scenes import CAPS_LONG2, CAPS_LONG3, N_BANK, long_records, run_parity, split_lanes
from helpers import bench_caps

pytestmark = pytest.mark.gpu

CB_DT = 0.1
WHEELBASE = 2.9


@pytest.mark.parametrize("caps", [CAPS_LONG2, CAPS_LONG3], ids=["ego-only", "config3-actors"])
def test_split_equals_unsplit_bitwise_long_routes(caps):
    """40 steps of step + reset_terminated at n = 19 with ego routes of up to 128
    points (past the 64 the tail's S2 prefetch covers at 16 envs per group):
    everything equal after every step; the target index moved past point 64 in
    some env, and some env was reset and terminated in consecutive steps."""
    n, steps = 19, 40
    P, padded, _ = EC.authored_world(128)
    recs, layout = long_records(n, caps, 100, off_every=2)
    bank, _ = long_records(N_BANK, caps, 500, off_every=3)
    assert max(LY.RecordView(r, layout).i("NROUTE") for r in recs) > 64
    lanes = split_lanes(P, padded, caps, recs, bank)
    rng = np.random.default_rng(19)
    p = np.ones(P.n_discrete)
    p[1] += 4.0
    acts = rng.choice(P.n_discrete, size=(steps, n), p=p / p.sum()).astype(np.int32)
    was_reset = np.zeros(n, bool)
    reset_then_term, tidx_max = 0, 0
    for t in range(steps):
        step_all(lanes, acts[t], t)
        assert_same(lanes, t)
        tn = term_of(lanes[1])
        reset_then_term += int(np.sum(was_reset & tn))
        was_reset = tn
        hr = lanes[1].recs.cpu().numpy()
        tidx_max = max(tidx_max, max(LY.RecordView(hr[e], layout).i("TIDX") for e in range(n)))
        reset_terminated_all(lanes)
    flush_all(lanes)
    assert torch.equal(lanes[0].recs, lanes[1].recs) and torch.equal(lanes[0].ring, lanes[1].ring)
    assert reset_then_term > 0 and tidx_max > 64


@pytest.mark.parametrize("edit_after", [False, True], ids=["mask-before-reset", "mask-edited-after-reset"])
@pytest.mark.parametrize("head_ne", [16, 64])
def test_reset_composition_of_a_head_group(head_ne, edit_after, monkeypatch):
    """n = 3 head groups + 3: the term bytes set by hand so that one group has every
    env reset, one none, one a mix and the partial last group one; then the step.
    Everything equals the unsplit step's; a reset env's X1 / Y1 / YAW1 are its bank
    row's pose and its jerks follow the row's HAS_PREV_COMFORT. The mask is read
    when the step runs: edited after cbev_reset_terminated it counts the same."""
    monkeypatch.setenv("CBEV_HEAD_NE", str(head_ne))
    caps = bench_caps(2)
    n = 3 * head_ne + 3
    P, padded, _ = EC.authored_world(128)
    lengths = (33, 64)
    specs = [dataclasses.replace(EC.long_route_spec(lengths[e % 2], 128, seed=e), vehicles=[], pedestrians=[])
             for e in range(max(n, N_BANK))]
    recs, layout, views = EC.pack_records(specs, 128, caps)
    for e, v in enumerate(views):
        i = (5 * e + 2) % (v.i("NROUTE") - 1)
        EC.set_pose(v, v.cx[i], v.cy[i], v.cyaw[i], 20.0 + e % 7)
    bank = recs[:N_BANK].copy()
    recs = recs[:n].copy()
    for b in range(N_BANK):
        v = LY.RecordView(bank[b], layout)
        EC.set_pose(v, v.h("X") + 1.5, v.h("Y"), v.h("YAW") + 0.01 * (b % 5), 12.0 + b % 9)
        if b % 2 == 0:  # a row saved mid-episode: comfort history present
            v.hi[LY.HI["HAS_PREV_COMFORT"]] = 1
            v.hd[LY.HD["PREV_AL"]], v.hd[LY.HD["PREV_ALAT"]], v.hd[LY.HD["PREV_YR"]] = 0.75, -0.25, 2.0
    lanes = split_lanes(P, padded, caps, recs, bank)
    acts = np.ones((2, n), np.int32)
    step_all(lanes, acts[0], 0)
    assert_same(lanes, 0)
    mask = np.zeros(n, np.uint8)
    mask[0:head_ne] = 1                                    # every env of group 0
    mask[2 * head_ne:3 * head_ne:3] = 1                    # a mix in group 2 (group 1: none)
    mask[2 * head_ne + 1] = 1
    mask[3 * head_ne + 1] = 1                              # one of the partial last group
    L = lib()
    tcount = reset_counts(L, lanes[1].dw, n)
    m = torch.from_numpy(mask).cuda()
    if not edit_after:
        for c in lanes:
            c.out["term"].copy_(m)
    reset_terminated_all(lanes)
    if edit_after:
        for c in lanes:
            c.out["term"].copy_(m)
    torch.cuda.synchronize()
    step_all(lanes, acts[1], 1)
    assert_same(lanes, 1)
    ids, rows = reset_rows(mask, tcount, N_BANK)
    h = head_ne
    assert mask[:h].all() and not mask[h:2 * h].any() and 0 < mask[2 * h:3 * h].sum() < h and mask[3 * h:].sum() == 1
    assert len(ids) == int(mask.sum())
    hr = lanes[1].recs.cpu().numpy()
    seen_prev = set()
    for e, row in zip(ids, rows):
        v, bv = LY.RecordView(hr[e], layout), LY.RecordView(bank[row], layout)
        for k in ("X", "Y", "YAW"):
            assert v.h(k + "1") == bv.h(k), (e, k)
        assert v.i("SCENE_ID") == bv.i("SCENE_ID") and v.i("HAS_PREV_COMFORT") == 1
        has_prev = bv.i("HAS_PREV_COMFORT")
        seen_prev.add(has_prev)
        for out, cur, prev in (("C_JL", "C_AL", "PREV_AL"), ("C_JLAT", "C_ALAT", "PREV_ALAT"), ("C_YACC", "C_YR", "PREV_YR")):
            want = (v.h(cur) - bv.h(prev)) / CB_DT if has_prev else 0.0
            assert v.h(out) == want, (e, out, v.h(out), want)
    assert seen_prev == {0, 1}
    kept = np.flatnonzero(mask == 0)
    h0 = lanes[0].recs.cpu().numpy()
    assert all(LY.RecordView(h0[e], layout).i("SCENE_ID") == e for e in kept)


def _tie_records(caps):
    """Out-and-back ego routes of 100 points on the straight road: point 99 - i
    lies exactly on point i, so the front axle is equally far from both. The ego
    stands on point i heading out, so the nearest points are i + 1 and 98 - i:
    env 0 ties inside the first 64 points (41 | 58), env 1 across them (31 | 68:
    the second in the tail's loop past its prefetch at 16 envs per group), env 2
    the same with its target index already at 80 (it must not move back), env 3
    far apart (11 | 88)."""
    spec = EC.long_route_spec(100, 128, seed=0)
    if caps.actor_cap == 0:
        spec = dataclasses.replace(spec, vehicles=[], pedestrians=[])
    recs, layout, views = EC.pack_records([spec] * 4, 128, caps)
    starts = (40, 30, 30, 10)
    for v, i in zip(views, starts):
        assert v.i("NROUTE") == 100
        y0 = float(v.cy[0])
        x = np.array(v.cx[:50], np.float64)
        v.cx[:100] = np.concatenate([x, x[::-1]])
        v.cy[:100] = y0
        EC.set_pose(v, float(v.cx[i]), y0, 0.0, 0.0)
        v.hi[LY.HI["TIDX"]] = 0
    views[2].hi[LY.HI["TIDX"]] = 80
    return recs, layout, starts


@pytest.mark.parametrize("caps", [CAPS_LONG2, CAPS_LONG3], ids=["ego-only", "config3-actors"])
def test_target_search_ties_take_the_first_argmin(caps):
    """Two route points at the same distance from the front axle: TIDX is the first
    arg-min (np.argmin of the hypots), never moves back, equals the unsplit step's
    bitwise and the oracle's."""
    P, padded, _ = EC.authored_world(128)
    recs, layout, starts = _tie_records(caps)
    n, steps = len(recs), 4
    want = []
    for e in range(n):
        v = LY.RecordView(recs[e], layout)
        fx, fy = v.h("X") + WHEELBASE * np.cos(v.h("YAW")), v.h("Y") + WHEELBASE * np.sin(v.h("YAW"))
        d = np.hypot(fx - np.asarray(v.cx[:100]), fy - np.asarray(v.cy[:100]))
        bi = int(np.argmin(d))
        assert np.count_nonzero(d == d[bi]) == 2 and bi < 50  # a tie, and its first index
        want.append(max(v.i("TIDX"), bi))
    acts = np.ones((steps, n), np.int32)
    lanes = split_lanes(P, padded, caps, recs, recs[np.arange(N_BANK) % n].copy())
    prev = np.array([LY.RecordView(recs[e], layout).i("TIDX") for e in range(n)])
    for t in range(steps):
        step_all(lanes, acts[t], t)
        assert_same(lanes, t)
        hr = lanes[1].recs.cpu().numpy()
        tidx = np.array([LY.RecordView(hr[e], layout).i("TIDX") for e in range(n)])
        if t == 0:
            assert tidx.tolist() == want, (tidx, want)
        assert np.all(tidx >= prev) and tidx[2] == 80
        prev = tidx
    del lanes
    run_parity(None, n, steps, caps=caps, recs=recs, world_=(P, padded), acts=acts, stats=True)


def test_oracle_parity_thin_head():
    """The split step against the oracle (whole records, frames, outputs and the
    episode statistics every step), 30 steps at n = 19: ego only, with actors,
    and size 256 (4 tiles per env, traffic lights)."""
    run_parity(["rt_no_traffic_v1"], 19, 30, seed0=10_600, caps=bench_caps(2), stats=True)
    run_parity(["rt_hard_v1"], 19, 30, seed0=20_600, act_seed=7, caps=bench_caps(3), stats=True)
    run_parity(["mix3"], 19, 30, size=256, seed0=30_600, caps=bench_caps(5), stats=True)


def test_action_index_out_of_range_in_reset_and_kept_envs():
    """An out-of-range discrete action in an env the folded reset takes and in one
    it keeps: the error flag is raised in both contexts, and records and outputs
    equal the unsplit step's (the index steps as action 0)."""
    caps = CAPS_LONG2
    n = 19
    P, padded, _ = EC.authored_world(128)
    recs, layout = long_records(n, caps, 900, off_every=1000)
    bank, _ = long_records(N_BANK, caps, 950, off_every=1000)
    lanes = split_lanes(P, padded, caps, recs, bank)
    acts = np.ones((2, n), np.int32)
    step_all(lanes, acts[0], 0)
    assert_same(lanes, 0)
    assert error_flags(lanes[0].dw.ctx) == 0 and error_flags(lanes[1].dw.ctx) == 0
    mask = np.zeros(n, np.uint8)
    mask[[2, 17]] = 1
    for c in lanes:
        c.out["term"].copy_(torch.from_numpy(mask).cuda())
    reset_terminated_all(lanes)
    acts[1, 2] = P.n_discrete + 5   # in a reset env
    acts[1, 7] = -P.n_discrete - 1  # in a kept env
    step_all(lanes, acts[1], 1)
    assert_same(lanes, 1)
    fa, fb = error_flags(lanes[0].dw.ctx), error_flags(lanes[1].dw.ctx)
    assert fa == fb and fa != 0
    # stepped as action 0 in both envs
    ref = acts[1].copy()
    ref[[2, 7]] = 0
    lanes2 = split_lanes(P, padded, caps, recs, bank)
    step_all(lanes2, acts[0], 0)
    for c in lanes2:
        c.out["term"].copy_(torch.from_numpy(mask).cuda())
    reset_terminated_all(lanes2)
    step_all(lanes2, ref, 1)
    assert torch.equal(lanes2[1].recs, lanes[1].recs) and torch.equal(lanes2[1].out["rew"], lanes[1].out["rew"])
    assert error_flags(lanes2[1].dw.ctx) == 0
