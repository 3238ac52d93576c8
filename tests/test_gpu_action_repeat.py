"""Action repeat (cbev_step_repeat): k simulation substeps per agent step with
one render, against the oracle stepped up to k times per env (stopping after
the first terminal substep), against chained plain steps, and through the
canonical loop, a captured graph and the vector env.

The reference of one agent step is a FrameSkip(k) wrapper directly around each
env: `Oracle.step_one` up to k times into the same frame buffer, rewards summed
in order; an env that terminates in substep j is frozen for the rest.
"""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle as O
from carlabev_env_amd import layout as LY
from carlabev_env_amd._lib import check, lib
from gpu_harness import (P_, DevWorld, EpisodeStatsOn, assert_same, assert_same_outputs, error_flags, flush_all,
                         make_lanes, out_bufs, ptr, reset_counts, reset_terminated_all, step_repeat, term_of)
from gpu_scenes import compare_records, deferred_pair, edge_states, info_of, split_pair
from helpers import CAPS_FULL, action_stream, bench_caps, build_records, world

pytestmark = pytest.mark.gpu

CBEV_EINVAL = -1


def oracle_agent_step(orc, recs, layout, acts_t, frames, k):
    """One agent step of every env on the oracle. Returns the summed rewards, the
    last executed substep's causes, and that substep's number (1..k) per env."""
    n = len(recs)
    rsum, cause, last = np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(n, np.int64)
    for e in range(n):
        v = LY.RecordView(recs[e], layout)
        a = np.ascontiguousarray(acts_t[e])
        for j in range(1, k + 1):
            cause[e] = orc.step_one(recs[e], a, frames[e])
            rsum[e] += v.h("REWARD")
            last[e] = j
            if v.i("TERM"):
                break
    return rsum, cause, last


def run_repeat_parity(kinds, n, agent_steps, k, size=128, reward="carl_base_v1", seed0=0, act_seed=1234, caps=None,
                      edit=None, recs=None, world_=None, acts=None, on_step=None):
    """cbev_step_repeat against the oracle with the episode statistics on: whole
    records, frames bit-exact, the summed reward, term / trunc / cause / info and
    the statistics' rows after every agent step; no resets. Returns the counts of
    (env, agent step) pairs [no termination, ended at substep 1, ..., at substep k]."""
    if recs is not None:
        P, padded = world_
        layout = LY.Layout.make(caps)
        recs = recs.copy()
    else:
        cfg, P, padded, layout, builder = world(size, "discrete9_v1", reward, caps=caps)
        recs, _ = build_records(builder, n, kinds, seed0=seed0)
    if edit is not None:
        edit(recs, layout, P)
    dw = DevWorld(P, padded, caps)
    L = lib()
    S = P.size
    d_recs = torch.from_numpy(recs.copy()).cuda()
    d_frames = torch.zeros((n, S, S), dtype=torch.uint8, device="cuda")
    check(L.cbev_reset(dw.ctx, ptr(d_recs), n, None, 0, None, None, 0, ptr(d_frames), 1, None), "reset")
    orc = O.Oracle(P, padded, caps.c(), layout.record_bytes)
    h_frames = np.zeros((n, S, S), np.uint8)
    for e in range(n):
        orc.reset_obs(recs[e], h_frames[e])
    if acts is None:
        acts = action_stream(P, n, agent_steps, seed=act_seed)
    st = EpisodeStatsOn(dw.ctx, n)
    b = out_bufs(n)
    hist = np.zeros(k + 1, np.int64)
    views = [LY.RecordView(recs[e], layout) for e in range(n)]
    for t in range(agent_steps):
        a = torch.from_numpy(np.ascontiguousarray(acts[t])).cuda()
        check(step_repeat(L, dw, d_recs, n, a, k, d_frames, b), "step_repeat")
        rsum, h_cause, last = oracle_agent_step(orc, recs, layout, acts[t], h_frames, k)
        h_term = np.array([v.i("TERM") for v in views], np.uint8)
        for e in range(n):
            hist[last[e] if h_term[e] else 0] += 1
        torch.cuda.synchronize()
        df = d_frames.cpu().numpy()
        bad = np.argwhere(df != h_frames)
        assert bad.size == 0, (t, bad[:8])
        dr = d_recs.cpu().numpy()
        for e in range(n):
            compare_records(dr[e], recs[e], layout, tag=(t, e))
        assert np.array_equal(b["term"].cpu().numpy(), h_term), t
        assert np.array_equal(b["trunc"].cpu().numpy(), np.array([v.i("TRUNC") for v in views], np.uint8)), t
        assert np.allclose(b["rew"].cpu().numpy(), rsum, rtol=1e-9, atol=1e-12), (t, b["rew"].cpu().numpy(), rsum)
        assert np.array_equal(b["cause"].cpu().numpy(), h_cause), (t, b["cause"].cpu().numpy(), h_cause)
        want = np.stack([info_of(v, h_cause[e]) for e, v in enumerate(views)])
        got = b["info"].cpu().numpy()
        assert np.array_equal(got[:, 13:], want[:, 13:]), (t, "info ints")
        assert np.allclose(got, want, rtol=1e-6, atol=1e-6), (t, "info")
        st.check(t, h_term, np.arange(n), views, h_cause)
        if on_step is not None:
            on_step(t, views, h_cause, last)
    assert error_flags(dw.ctx) == 0
    return hist


def _covers_every_substep(hist):
    """Asserted from the oracle's side: every substep position ends some (env, agent
    step) pair, and some pair runs all k substeps without terminating."""
    assert all(int(c) > 0 for c in hist), hist


REPEAT_CASES = [
    # the counts the oracle alone gives for these inputs
    pytest.param(2, ["rt_no_traffic_v1"], 19, 128, 10_000, 1234, 4, 40, [481, 260, 11, 5, 3], id="config2-k4"),
    pytest.param(2, ["rt_no_traffic_v1"], 19, 128, 10_000, 1234, 2, 40, [705, 51, 4], id="config2-k2"),
    pytest.param(3, ["rt_hard_v1"], 8, 128, 20_000, 7, 3, 30, [199, 33, 6, 2], id="config3-k3"),
    pytest.param(5, ["mix3"], 5, 256, 30_000, 1234, 2, 30, [69, 78, 3], id="config5-k2"),
]


@pytest.mark.parametrize("config,kinds,n,size,seed0,act_seed,k,steps,counts", REPEAT_CASES)
def test_repeat_matches_the_oracle(config, kinds, n, size, seed0, act_seed, k, steps, counts):
    hist = run_repeat_parity(kinds, n, steps, k, size=size, seed0=seed0, act_seed=act_seed, caps=bench_caps(config))
    _covers_every_substep(hist)
    assert hist.tolist() == counts


@pytest.mark.parametrize("ne", ["2", "64"])
def test_repeat_ego_workgroup_shapes(ne, monkeypatch):
    """k_ego_rep with 4 envs per workgroup (CBEV_EGO_NE=2 is raised to the floor)
    and with the most the LDS admits (read at cbev_create: the gated kernel needs
    the same dynamic LDS limit as k_ego); odd env counts leave a partial last
    workgroup, whose frozen mask covers fewer than ne envs."""
    monkeypatch.setenv("CBEV_EGO_NE", ne)
    hist = run_repeat_parity(["rt_no_traffic_v1"], 47, 30, 3, seed0=10_000, caps=bench_caps(2))
    _covers_every_substep(hist)  # the oracle alone: [1226, 164, 11, 9]
    run_repeat_parity(["rt_hard_v1"], 13, 8, 2, seed0=20_000, act_seed=7, caps=bench_caps(3))


def test_truncation_inside_a_repeat():
    """max_actions counts substeps: env 0 is truncated at substep 2 of the first
    agent step (EP_LEN advanced by 2, frozen after it), env 1 at substep 4."""
    k = 4
    seen = {}

    def edit(recs, layout, P):
        x1 = LY.RecordView(recs[1], layout).hd[LY.HD["X"]]
        edge_states(recs, layout, P)
        # _edge_states moves env 1 off the road, where it collides in substep 1 and
        # would never reach its truncation: env 1 keeps its own pose here
        LY.RecordView(recs[1], layout).hd[LY.HD["X"]] = x1
        LY.RecordView(recs[0], layout).hi[LY.HI["KSTEPS"]] = P.max_actions - 2
        LY.RecordView(recs[1], layout).hi[LY.HI["KSTEPS"]] = P.max_actions - 4
        seen["len0"] = [LY.RecordView(recs[e], layout).i("EP_LEN") for e in (0, 1)]

    def on_step(t, views, causes, last):
        if t == 0:
            seen["first"] = [(int(last[e]), views[e].i("TERM"), views[e].i("TRUNC"), views[e].i("EP_LEN"),
                              int(causes[e])) for e in (0, 1)]

    run_repeat_parity(["rt_easy_v1"], 10, 2, k, reward="shaping_base_v1", seed0=4242, caps=CAPS_FULL, edit=edit,
                      on_step=on_step)
    (j0, term0, trunc0, len0, c0), (j1, term1, trunc1, len1, c1) = seen["first"]
    assert (j0, term0, trunc0, len0 - seen["len0"][0], c0) == (2, 1, 1, 2, LY.CAUSE["max_actions"])
    assert (j1, term1, trunc1, len1 - seen["len0"][1], c1) == (4, 1, 1, 4, LY.CAUSE["max_actions"])


def test_repeat_at_size_64():
    """k_raster<1> after the gated substeps, on authored records."""
    import edge_cases as EC
    P, padded, caps, recs, layout, acts = EC.raster_batch(64, 0.5)
    idx = np.arange(0, len(recs), 15)[:7]  # every 15th case of the raster matrix, as _authored64 takes them
    assert len(idx) >= 5
    run_repeat_parity(None, len(idx), len(acts), 2, caps=caps, recs=np.ascontiguousarray(recs[idx]),
                      world_=(P, padded), acts=np.ascontiguousarray(acts[:, idx]))


def test_repeat_1_is_the_plain_step_bitwise():
    """cbev_step_repeat(repeat=1) forwards to cbev_step: the folded reset included."""
    n, n_bank, F, steps = 19, 53, 3, 20
    P, lanes = split_pair(n, bench_caps(2), 128, ("rt_no_traffic_v1",), 10_319, 14_319, n_bank=n_bank, F=F)
    L = lib()
    for lane in lanes:
        check(L.cbev_set_split_step(lane.dw.ctx, 0), "split off")
    acts = action_stream(P, n, steps, seed=5)
    A, B = lanes
    folded = 0
    for t in range(steps):
        a = torch.from_numpy(np.ascontiguousarray(acts[t])).cuda()
        folded += L.cbev_reset_pending(B.dw.ctx)
        dw, _, _, d_recs, ring, b = A
        check(L.cbev_step(dw.ctx, ptr(d_recs), n, ptr(a), ptr(ring[t % F]), ptr(b["rew"]), ptr(b["term"]),
                          ptr(b["trunc"]), ptr(b["cause"]), ptr(b["info"]), None), "step")
        dw, _, _, d_recs, ring, b = B
        check(step_repeat(L, dw, d_recs, n, a, 1, ring[t % F], b), "step_repeat")
        assert L.cbev_reset_pending(dw.ctx) == 0  # taken by the step, as cbev_step takes it
        torch.cuda.synchronize()
        assert_same(lanes, t)
        reset_terminated_all(lanes)
    flush_all(lanes)
    assert torch.equal(A.recs, B.recs) and torch.equal(A.ring, B.ring)
    assert folded >= steps - 1 and int(reset_counts(L, A.dw, n).sum()) > 0


def test_repeat_equals_chained_plain_steps_bitwise():
    """Over envs that did not terminate within the agent step, k gated substeps
    and one render leave the records, the frame and the reward that k plain
    cbev_step calls leave (rewards summed on the host in order). Both contexts
    start every agent step from the repeat context's records."""
    n, k, steps = 19, 4, 40
    caps = bench_caps(2)
    cfg, P, padded, layout, builder = world(128, caps=caps)
    recs, _ = build_records(builder, n, ["rt_no_traffic_v1"], seed0=10_000)
    acts = action_stream(P, n, steps, seed=1234)
    L = lib()
    (dA, _, _, rA, gA, bA), (dB, _, _, rB, gB, bB) = make_lanes(P, padded, caps, recs, None, 1, [{}, {}], stats=False)
    fA, fB = gA[0], gB[0]
    same = 0
    for t in range(steps):
        a = torch.from_numpy(np.ascontiguousarray(acts[t])).cuda()
        rB.copy_(rA)
        check(step_repeat(L, dA, rA, n, a, k, fA, bA), "step_repeat")
        rsum = torch.zeros(n, dtype=torch.float64, device="cuda")
        any_term = torch.zeros(n, dtype=torch.bool, device="cuda")
        for _ in range(k):
            check(L.cbev_step(dB.ctx, ptr(rB), n, ptr(a), ptr(fB), ptr(bB["rew"]), ptr(bB["term"]), ptr(bB["trunc"]),
                              ptr(bB["cause"]), ptr(bB["info"]), None), "step")
            rsum = rsum + bB["rew"]
            any_term |= bB["term"].bool()
        torch.cuda.synchronize()
        live = ~any_term
        assert torch.equal(live, ~bA["term"].bool()), t  # frozen exactly where the chain terminated
        assert torch.equal(rA[live], rB[live]), (t, "records")
        assert torch.equal(fA[live], fB[live]), (t, "frames")
        assert torch.equal(bA["rew"][live], rsum[live]), (t, "reward")
        for key in ("trunc", "cause", "info"):
            assert torch.equal(bA[key][live], bB[key][live]), (t, key)
        same += int(live.sum())
    assert same >= n * steps // 2, same


def test_canonical_loop_deferred_equals_immediate():
    """cbev_step_repeat(k = 3) + cbev_reset_terminated with the deferred reset on
    (the repeat step launches the recorded reset before substep 1) against the
    same with it off: everything equal after every agent step."""
    n, B, F, k, steps = 45, 13, 3, 3, 25
    P, layout, lanes = deferred_pair(n, B, F, bench_caps(2), 7000, 17000)
    L = lib()
    for dw, d_bank, bf, d_recs, ring, b in lanes:  # every third bank row starts off the road
        check(L.cbev_flush(dw.ctx), "flush")
        h = d_bank.cpu().numpy()
        for r in range(0, B, 3):
            LY.RecordView(h[r], layout).hd[LY.HD["X"]] += 60.0
        d_bank.copy_(torch.from_numpy(h))
        check(L.cbev_bank_frames(dw.ctx, ptr(d_bank), B, ptr(bf), None), "bank_frames")
        h = d_recs.cpu().numpy()
        for e in range(0, n, 2):
            LY.RecordView(h[e], layout).hd[LY.HD["X"]] += 60.0
        d_recs.copy_(torch.from_numpy(h))
    acts = action_stream(P, n, steps, seed=21)
    A, Bc = lanes
    was_reset = np.zeros(n, bool)
    reset_then_term = pending = 0
    for t in range(steps):
        a = torch.from_numpy(np.ascontiguousarray(acts[t])).cuda()
        pending += L.cbev_reset_pending(Bc.dw.ctx)
        for dw, d_bank, bf, d_recs, ring, b in lanes:
            check(step_repeat(L, dw, d_recs, n, a, k, ring[t % F], b), "step_repeat")
            assert L.cbev_reset_pending(dw.ctx) == 0
        torch.cuda.synchronize()
        assert_same(lanes, t)
        tn = term_of(Bc)
        reset_then_term += int(np.sum(was_reset & tn))
        was_reset = tn
        reset_terminated_all(lanes)
    flush_all(lanes)
    assert torch.equal(A.recs, Bc.recs) and torch.equal(A.ring, Bc.ring)
    assert pending >= steps - 1 and reset_then_term > 0


def _repeat_world(n, F, seed0, push_every):
    caps = bench_caps(2)
    cfg, P, padded, layout, builder = world(128, caps=caps)
    recs, _ = build_records(builder, n, ["rt_no_traffic_v1"], seed0=seed0)
    for e in range(0, n, push_every):
        LY.RecordView(recs[e], layout).hd[LY.HD["X"]] += 60.0
    return P, layout, make_lanes(P, padded, caps, recs, None, F, [{}, {}])


def test_repeat_under_graph_capture():
    """One repeat step (k = 3) captured into a graph (a linear chain, nothing
    allocated) and replayed twice equals two eager calls from the same start."""
    n, F, k = 19, 2, 3
    P, layout, lanes = _repeat_world(n, F, 10_500, 4)
    L = lib()
    acts = torch.ones(n, dtype=torch.int32, device="cuda")

    def step(dw, d_recs, ring, b):
        check(step_repeat(L, dw, d_recs, n, acts, k, ring[0], b, P_(torch.cuda.current_stream().cuda_stream)),
              "step_repeat")

    (dA, _, _, rA, gA, bA), (dB, _, _, rB, gB, bB) = lanes
    step(dA, rA, gA, bA)  # one eager call each: the kernels are loaded before the capture
    step(dB, rB, gB, bB)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            step(dB, rB, gB, bB)
    torch.cuda.synchronize()
    assert torch.equal(rA, rB)  # the capture ran nothing
    for rep in range(2):
        step(dA, rA, gA, bA)
        g.replay()
        torch.cuda.synchronize()
        assert_same_outputs(*lanes, rep)
    assert int(bA["term"].sum()) > 0


def test_refusals_leave_a_live_context_untouched():
    n, F = 19, 2
    P, layout, lanes = _repeat_world(n, F, 10_600, 4)
    L = lib()
    dw, _, _, d_recs, ring, b = lanes[0]
    acts = torch.ones(n, dtype=torch.int32, device="cuda")
    check(step_repeat(L, dw, d_recs, n, acts, 2, ring[0], b), "step_repeat")
    torch.cuda.synchronize()
    before = [d_recs.clone(), ring.clone()] + [b[key].clone() for key in ("rew", "term", "trunc", "cause", "info")]
    for bad in (0, 65, -3):
        assert step_repeat(L, dw, d_recs, n, acts, bad, ring[0], b) == CBEV_EINVAL
        assert b"repeat" in L.cbev_last_error()
    assert L.cbev_step_repeat(dw.ctx, None, n, ptr(acts), 2, ptr(ring[0]), ptr(b["rew"]), ptr(b["term"]),
                              ptr(b["trunc"]), ptr(b["cause"]), None, None) == CBEV_EINVAL
    torch.cuda.synchronize()
    after = [d_recs, ring] + [b[key] for key in ("rew", "term", "trunc", "cause", "info")]
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    check(step_repeat(L, dw, d_recs, n, acts, 64, ring[1], b), "step_repeat")  # the largest repeat runs
    torch.cuda.synchronize()
    assert error_flags(dw.ctx) == 0


def test_vector_env_action_repeat():
    """make_env(action_repeat=4) against action_repeat=1 stepped 4 times with the
    same actions from the same seed, over envs that have not terminated: the
    same newest frame and wire observation of it, the reward the host sum, and
    infos["episode"]["l"] counting substeps where an env terminates."""
    from carlabev_env_amd import EnvConfig, RandomNavigationReset, build_random_navigation_options, make_env
    k, N = 4, 6
    cfg = EnvConfig(size=128, obs_size=(128, 128), render_mode="rgb_array", obs_mode="bev_semantic")
    envs = [make_env({"env": cfg, "num_envs": N}, num_envs=N, action_repeat=r) for r in (k, 1)]
    assert [e.action_repeat for e in envs] == [k, 1]
    opts = build_random_navigation_options(RandomNavigationReset(difficulty_id="rt_medium_v1"))
    o4, _ = envs[0].reset(seed=3, options=opts)
    o1, _ = envs[1].reset(seed=3, options=opts)
    assert torch.equal(o4, o1)
    C = o4.shape[1] // envs[0].F  # channels of one frame of the stack
    alive = np.ones(N, bool)
    lengths = {}
    compared = 0
    for t in range(60):
        if not alive.any():
            break
        a = np.random.default_rng(100 + t).choice(9, size=N, p=np.array([1, 8, 1, 1, 1, 1, 1, 1, 1]) / 16.0)
        obs4, r4, term4, trunc4, info4 = envs[0].step(a)
        rsum = torch.zeros(N, dtype=torch.float64, device=r4.device)
        term1 = np.zeros(N, bool)
        len1 = {}
        for j in range(k):
            obs1, r1, tm, _, info1 = envs[1].step(a)
            rsum = rsum + r1
            tm = tm.cpu().numpy()
            for e in np.flatnonzero(tm & alive & ~term1):
                len1[int(e)] = int(info1["episode"]["l"][e])
            term1 |= tm
        t4 = term4.cpu().numpy()
        assert np.array_equal(t4[alive], term1[alive]), t
        live = alive & ~term1
        idx = torch.from_numpy(np.flatnonzero(live)).to(r4.device)
        assert torch.equal(envs[0].frames()[idx], envs[1].frames()[idx]), t
        assert torch.equal(obs4[idx][:, -C:], obs1[idx][:, -C:]), t
        assert torch.equal(r4[idx], rsum[idx]), t
        compared += int(live.sum())
        for e in np.flatnonzero(alive & t4):
            assert info4["_episode"][e]
            lengths[int(e)] = (int(info4["episode"]["l"][e]), len1[int(e)])
        alive &= ~term1
    assert compared > 0 and lengths, (compared, lengths)
    for e, (l4, l1) in lengths.items():
        assert l4 == l1 > 0, (e, l4, l1)  # substeps, as the plain env counted its steps
    for env in envs:
        env.close()
