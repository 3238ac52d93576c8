"""The folded reset without the head's record copy: k_ego_head stores only the
words it computes for a reset env, k_raster's raster role reads such an env's
scene from its bank row, and the tail role stages the row and puts it into the
record's place beside the raster. Scheduling only: everything here is bitwise
against the unsplit step on the same inputs after every step (whole records,
every ring slot, reward, term, trunc, cause, info, episode rows and counts,
termination counts), with the preview counters asserted.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import edge_cases as EC
from carlabev_env_amd import layout as LY
from carlabev_env_amd._lib import check, lib
from gpu_harness import (P_, assert_same, assert_same_outputs, error_flags, preview_counts, ptr, reset_counts,
                         reset_rows, reset_terminated_all, set_term, step_all, term_of)
from gpu_scenes import (CAPS_LONG2, N_BANK, UNSPLIT_AND_PREVIEW, long_records, preview_delta, prime, primed_case,
                        split_lanes, wall_world)

pytestmark = pytest.mark.gpu


def _same(lanes, t, want=None):
    """assert_same and the preview counters: the unsplit step has no head, the split
    one's are `want` (when given)."""
    assert_same(lanes, t)
    assert preview_counts(lanes[0]) == (0, 0), t
    if want is not None:
        assert preview_counts(lanes[1]) == want, (t, preview_counts(lanes[1]), want)


def _off_road_dy(classes, x, y):
    """A row offset that puts (x, y) inside a block of class 0 (a hero tile of class
    0 is a collision, the first thing the reward checks) wide enough for the first
    steps' motion along the road at either map scale."""
    s = max(1, classes.shape[1] // 1024)
    my, mx = 4 * s, 14 * s
    for d in range(8, 600):
        for dy in (d, -d):
            yy, xx = int(y) + dy, int(x)
            if yy - my < 0 or xx - mx < 0 or yy + my >= classes.shape[0] or xx + mx >= classes.shape[1]:
                continue
            if not classes[yy - my:yy + my + 1, xx - mx:xx + mx + 1].any():
                return float(dy)
    raise AssertionError("no class-0 block above or below the road")


def _records(n, size, seed0, off_every, lengths=(65, 127, 128, 64, 33)):
    """gpu_scenes.long_records without actors at any size: every
    off_every-th record starts inside a wall and terminates in its first step."""
    _, _, classes = EC.authored_world(size)
    specs = [dataclasses.replace(EC.long_route_spec(lengths[e % len(lengths)], size, seed=seed0 + e), vehicles=[],
                                 pedestrians=[]) for e in range(n)]
    recs, layout, views = EC.pack_records(specs, size, CAPS_LONG2)
    for e, v in enumerate(views):
        i = (7 * e + 3) % (v.i("NROUTE") - 1)
        EC.set_pose(v, v.cx[i], v.cy[i], v.cyaw[i], 30.0)
        if e % 2 == 0:
            v.hi[LY.HI["TIDX"]] = i
        if off_every and e % off_every == 0:
            v.hd[LY.HD["Y"]] += _off_road_dy(classes, v.cx[i], v.cy[i])
    return recs, layout


def _loop(lanes, acts, steps):
    """The canonical loop; returns the resets folded per step and how often an env
    terminated in the very step that took its reset."""
    n = acts.shape[1]
    was_reset = np.zeros(n, bool)
    reset_then_term, folded = 0, []
    for t in range(steps):
        step_all(lanes, acts[t], t)
        _same(lanes, t)
        tn = term_of(lanes[0])
        reset_then_term += int(np.sum(was_reset & tn))
        was_reset = tn
        if t < steps - 1:
            folded.append(int(tn.sum()))
            reset_terminated_all(lanes)
    return folded, reset_then_term


def _acts(P, steps, n, seed):
    p = np.ones(P.n_discrete)
    p[1] += 4.0
    return np.random.default_rng(seed).choice(P.n_discrete, size=(steps, n), p=p / p.sum()).astype(np.int32)


def _rest_equals_row(rec, row, layout):
    """Every byte of a reset env's record the step does not compute is its bank
    row's: all but HD, HI and the vis group, up to record_bytes; of HI, the scene's
    counts and id."""
    o = layout.off
    v1 = o["vis"] + 8 * layout.vis_words
    assert np.array_equal(rec[o["cx"]:o["vis"]], row[o["cx"]:o["vis"]])
    assert np.array_equal(rec[v1:layout.record_bytes], row[v1:layout.record_bytes])
    a, b = LY.RecordView(rec, layout), LY.RecordView(row, layout)
    for k in ("NROUTE", "NACT", "NVEH", "NTL", "NRAW", "SCENE_ID"):
        assert a.i(k) == b.i(k), k


# ---------------------------------------------------------------------- 1. the canonical loop
@pytest.mark.parametrize("n,head_ne", [(19, 16), (3 * 64 + 3, 64)])
def test_canonical_loop_equals_unsplit(n, head_ne, monkeypatch):
    """40 steps of step + reset_terminated with a 3-slot ring: equal to the unsplit
    step after every step; a third of the bank rows lie off the road, so some env
    terminates in the very step that takes its reset."""
    monkeypatch.setenv("CBEV_HEAD_NE", str(head_ne))
    steps = 40
    P, padded, _ = EC.authored_world(128)
    recs, _ = long_records(n, CAPS_LONG2, 100, off_every=2)
    bank, _ = long_records(N_BANK, CAPS_LONG2, 500, off_every=3)
    lanes = split_lanes(P, padded, CAPS_LONG2, recs, bank, UNSPLIT_AND_PREVIEW)
    folded, reset_then_term = _loop(lanes, _acts(P, steps, n, 19), steps)
    assert sum(folded[1:]) >= 10 and reset_then_term > 0
    assert preview_counts(lanes[1]) == (sum(folded[1:]), folded[0])
    assert error_flags(lanes[0].dw.ctx) == 0 and error_flags(lanes[1].dw.ctx) == 0


# ---------------------------------------------------------------------- 2. compositions of a group
@pytest.mark.parametrize("preview", [1, 0], ids=["preview-on", "preview-off"])
def test_group_compositions(preview):
    """Head and tail groups of 16: group 0 every env reset (from its preview when it
    is on), group 1 none, group 2 previews, two-pass resets and kept envs, group 3
    one reset env, the partial last group one two-pass reset. After the step a reset
    env's record is its row in every byte the step does not compute."""
    h = 16
    n = 4 * h + 3
    fast = list(range(h)) + [2 * h, 2 * h + 3, 2 * h + 6, 3 * h + 5]
    slow = [2 * h + 1, 2 * h + 4, 4 * h + 1]
    P, padded, recs, bank, layout = wall_world(n, fast, n_bank=71)
    lanes = split_lanes(P, padded, CAPS_LONG2, recs, bank, ((0, 1), (1, preview)))
    acts = np.ones(n, np.int32)
    (h0, f0), term1 = prime(lanes, n, fast, acts)
    assert not term1[slow].any()
    tc = reset_counts(lib(), lanes[1].dw, n)  # (before the reset is recorded: reading the counts applies a pending one)
    reset_terminated_all(lanes)
    mask = np.zeros(n, np.uint8)
    mask[fast] = 1
    mask[slow] = 1
    set_term(lanes, mask)
    step_all(lanes, acts, 2)
    want = (h0 + len(fast), f0 + len(slow)) if preview else (0, f0 + len(fast) + len(slow))
    _same(lanes, 2, want)
    assert mask[:h].all() and not mask[h:2 * h].any() and mask[2 * h:3 * h].sum() == 5 and mask[3 * h:4 * h].sum() == 1
    hr = lanes[1].recs.cpu().numpy()
    ids, rows = reset_rows(mask, tc, 71)
    assert len(ids) == int(mask.sum())
    for e, row in zip(ids, rows):
        _rest_equals_row(hr[e], bank[row], layout)
    for e in np.flatnonzero(mask == 0):
        assert LY.RecordView(hr[e], layout).i("SCENE_ID") == e
    # and the step after it, whose tail and raster read the records this one's tail completed
    reset_terminated_all(lanes)
    step_all(lanes, acts, 3)
    _same(lanes, 3)


# ---------------------------------------------------------------------- 3. a stale record
def _stale_world(world, n):
    """Records and bank rows whose routes differ in length both ways: even envs run
    a 64-point episode with every target visible and 3 px apart around the ego and
    reset to 5-point rows, odd envs the reverse. Every row's pose is turned off the
    road's axis (so, under a crop of the output's size, its item is not `fast` and
    crop_background runs), and the last points of every 64-point route lie on a
    diagonal through the crop's top-left corner at that pose, where only
    crop_background looks."""
    P = world[0]
    lens = lambda first: [first if e % 2 == 0 else 69 - first for e in range(n)]  # noqa: E731

    def build(lengths, seed0, turn):
        specs = [dataclasses.replace(EC.long_route_spec(m, 128, seed=seed0 + e), vehicles=[], pedestrians=[])
                 for e, m in enumerate(lengths)]
        recs, layout, views = EC.pack_records(specs, 128, CAPS_LONG2)
        for e, v in enumerate(views):
            i = 1 + e % 3
            EC.set_pose(v, v.cx[i], v.cy[i], v.cyaw[i] + turn * (1 + e % 4), 25.0)
            if v.i("NROUTE") == 64:
                x, y = v.h("X") - P.crop / 2.0, v.h("Y") - P.crop / 2.0
                for j in range(40, 63):
                    v.cx[j], v.cy[j] = x + 0.5 * (j - 51), y + 0.5 * (j - 51)
        return recs, layout

    recs, layout = build(lens(64), 100, 0.0)
    bank, _ = build(lens(5), 500, 0.21)
    return recs, bank, layout


@pytest.mark.parametrize("geo", [None, (128, 0.5, 128, 128)], ids=["fast-items", "crop128-checked-path"])
def test_stale_record_is_read_by_neither_role(geo):
    """The old episode has 64 route points and the row 5, and the reverse: a raster
    or tail role that read the record's route, counts or vis_draw would paint,
    search or collide differently from the unsplit step, whose k_ego has written
    the whole record before its raster starts."""
    n = 19
    world = EC.authored_world(128) if geo is None else EC.reduced_world(*geo)
    P, padded = world[0], world[1]
    recs, bank, layout = _stale_world(world, n)
    lanes = split_lanes(P, padded, CAPS_LONG2, recs, bank[:n], UNSPLIT_AND_PREVIEW)
    acts = np.ones(n, np.int32)
    step_all(lanes, acts, 0)
    _same(lanes, 0)
    mask = np.ones(n, np.uint8)
    mask[[3, 8]] = 0
    set_term(lanes, mask)
    tc = reset_counts(lib(), lanes[1].dw, n)
    reset_terminated_all(lanes)
    step_all(lanes, acts, 1)
    _same(lanes, 1)
    hr = lanes[1].recs.cpu().numpy()
    ids, rows = reset_rows(mask, tc, n)
    for e, row in zip(ids, rows):
        _rest_equals_row(hr[e], bank[row], layout)
    old_n, new_n = [LY.RecordView(recs[e], layout).i("NROUTE") for e in ids], [LY.RecordView(hr[e], layout).i("NROUTE") for e in ids]
    assert {(a, b) for a, b in zip(old_n, new_n)} >= {(64, 5), (5, 64)}
    if geo is not None:  # the reset envs' items took the checked path
        assert not any(LY.RecordView(hr[e], layout).i("RS_FAST") & 1 for e in ids)
    # the preview path too: every env again, from the previews of the envs that terminated
    reset_terminated_all(lanes)
    step_all(lanes, acts, 2)
    _same(lanes, 2)


# ---------------------------------------------------------------------- 4. an edited mask
def test_mask_byte_cleared_after_reset_terminated_keeps_the_old_episode_whole():
    """A byte cleared after cbev_reset_terminated: the head decides from the mask as
    it stands at the launch, and the tail and the raster follow the head's word,
    not the byte: the record stays the old episode's in every byte the step does
    not compute. A byte set for an env that never terminated is a reset."""
    P, bank, layout, lanes, acts, base, term1 = primed_case()
    before = lanes[1].recs.cpu().numpy().copy()
    tc = reset_counts(lib(), lanes[1].dw, len(acts))  # (before the reset is recorded: reading the counts applies a pending one)
    reset_terminated_all(lanes)
    mask = term_of(lanes[1]).astype(np.uint8)
    assert mask[4] and not mask[[0, 9]].any()
    mask[4] = 0
    mask[[0, 9]] = 1
    set_term(lanes, mask)
    step_all(lanes, acts, 2)
    _same(lanes, 2)
    assert preview_delta(lanes, base) == (int(term1.sum()) - 1, 2)
    hr = lanes[1].recs.cpu().numpy()
    _rest_equals_row(hr[4], before[4], layout)
    ids, rows = reset_rows(mask, tc, N_BANK)
    assert {0, 9} <= set(ids.tolist()) and 4 not in ids
    for e, row in zip(ids, rows):
        _rest_equals_row(hr[e], bank[row], layout)


# ---------------------------------------------------------------------- 5. S = 256: four tiles read the row
def test_size_256_four_tiles_read_the_row():
    n, steps = 19, 12
    P, padded, _ = EC.authored_world(256)
    recs, _ = _records(n, 256, 100, off_every=2)
    bank, _ = _records(N_BANK, 256, 500, off_every=3)
    lanes = split_lanes(P, padded, CAPS_LONG2, recs, bank, UNSPLIT_AND_PREVIEW)
    folded, reset_then_term = _loop(lanes, _acts(P, steps, n, 5), steps)
    assert sum(folded[1:]) >= 5 and reset_then_term > 0
    assert preview_counts(lanes[1]) == (sum(folded[1:]), folded[0])


# ---------------------------------------------------------------------- 6. graph capture
def test_captured_step_replayed_twice():
    """A step captured while a reset is pending, replayed twice against the eager
    unsplit run: the tail and the raster of each replay take the rows the head of
    that replay chose."""
    P, bank, layout, lanes, acts, base, term1 = primed_case(extra_off=[(e + lib().cbev_bank_stride(N_BANK)) % N_BANK for e in (1, 4, 17)])
    L = lib()
    A, B = lanes
    n = len(acts)
    a = torch.from_numpy(acts).cuda()

    def step(c, stream):
        dw, d_bank, bf, d_recs, ring, b = c
        check(L.cbev_step(dw.ctx, ptr(d_recs), n, ptr(a), ptr(ring[2]), ptr(b["rew"]), ptr(b["term"]),
                          ptr(b["trunc"]), ptr(b["cause"]), ptr(b["info"]), stream), "step")

    reset_terminated_all([B])
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            step(B, P_(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    resets = []
    for rep in range(2):
        resets.append(int(term_of(A).sum()))
        reset_terminated_all([A])
        step(A, None)
        g.replay()
        torch.cuda.synchronize()
        assert_same_outputs(A, B, rep)
        assert np.array_equal(reset_counts(L, A.dw, n), reset_counts(L, B.dw, n)), (rep, "reset counts")
    assert resets[1] >= 3
    assert preview_delta(lanes, base) == (resets[0], resets[1]) and preview_counts(A) == (0, 0)
