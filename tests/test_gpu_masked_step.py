"""The masked step (cbev_step_masked) and the freeze-on-done evaluation mode
(make_env(cfg, freeze_done=True)): against the oracle stepping only the active
envs, against cbev_step_repeat (all active), with every env inactive, the error
flags, the ego workgroup shapes, a captured graph, a pending deferred reset, the
refusals and the vector env.

The reference of one masked agent step: an active env is stepped by the oracle
up to `repeat` times into its frame buffer (stopping after a terminal substep,
rewards summed in order); an inactive env is not touched at all, so its record,
its frame and its last term / trunc / cause / info stay, and its reward is 0.
"""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle as O
from carlabev_env_amd import layout as LY
from carlabev_env_amd._lib import ERR_ACTION_INDEX, check, lib
from gpu_harness import (KEYS, P_, DevWorld, EpisodeStatsOn, assert_same, assert_same_outputs, error_flags, flush_all,
                         out_bufs, ptr, reset_counts, reset_terminated_all, step_masked, step_repeat, termination_count)
from gpu_scenes import (EGO_ONLY, compare_records, deferred_pair, ego_only_64, eval_actions, eval_cfg, eval_pair,
                        info_of, mask_stream, twins)
from helpers import action_stream, bench_caps, build_records, world

pytestmark = pytest.mark.gpu

CBEV_EINVAL = -1


def run_masked_parity(kinds, n, steps, k, size=128, seed0=0, act_seed=1234, caps=None, mask_seed=0, F=2, recs=None,
                      world_=None, fov=False, reward="carl_base_v1", device=True):
    """cbev_step_masked against the oracle with the episode statistics on, after
    every step: whole records (an inactive env's bytes also against the step
    before), the new ring slot, reward, term / trunc / cause / info, the
    statistics' rows, counts and accumulators, cbev_reset_counts and the
    termination count; no resets. F = 2 alternates two ring slots (prev_frames
    is the other one), F = 1 passes prev_frames == frames. device=False runs
    the oracle's side alone (how the seeds below were chosen). Returns what the
    inputs covered, from the oracle's side."""
    if recs is not None:
        P, padded = world_
        layout = LY.Layout.make(caps)
        recs = recs.copy()
    else:
        cfg, P, padded, layout, builder = world(size, "discrete9_v1", reward, caps=caps)
        recs, _ = build_records(builder, n, kinds, seed0=seed0)
        for e in range(2, n, 5):  # every fifth env starts off the road: it ends in its first active substep
            LY.RecordView(recs[e], layout).hd[LY.HD["X"]] += 60.0
    S = P.size
    masks = mask_stream(n, steps, mask_seed)
    acts = action_stream(P, n, steps, seed=act_seed)
    omask = None
    if fov:
        import wrappers as W
        omask = W.fov_mask(S)
    orc = O.Oracle(P, padded, caps.c(), layout.record_bytes)
    h_frames = np.zeros((n, S, S), np.uint8)
    for e in range(n):
        orc.reset_obs(recs[e], h_frames[e])
        if omask is not None:
            h_frames[e][omask] = 8  # CBEV_PX_BLACK
    views = [LY.RecordView(recs[e], layout) for e in range(n)]
    h_term, h_trunc = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    h_cause, h_info = np.zeros(n, np.int32), np.zeros((n, 16), np.float32)
    tcount = np.zeros(n, np.int64)
    if device:
        L = lib()
        dw = DevWorld(P, padded, caps)
        if fov:
            from carlabev_env_amd.fov_mask import fov_corner_mask
            dmask = fov_corner_mask(S)
            check(L.cbev_set_fov_mask(dw.ctx, dmask.ctypes.data_as(P_)), "fov")
        d_recs = torch.from_numpy(recs.copy()).cuda()
        ring = torch.zeros((F, n, S, S), dtype=torch.uint8, device="cuda")
        check(L.cbev_reset(dw.ctx, ptr(d_recs), n, None, 0, None, None, 0, ptr(ring), F, None), "reset")
        st = EpisodeStatsOn(dw.ctx, n)
        b = out_bufs(n)
    hist = np.zeros(k + 1, np.int64)
    seen_active, seen_inactive, ended = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    cov = dict(term_then_inactive=0, inactive_live=0, inactive_first=0)
    for t in range(steps):
        act = masks[t]
        new = (t + 1) % F
        if device:
            a = torch.from_numpy(np.ascontiguousarray(acts[t])).cuda()
            d_act = torch.from_numpy(act.astype(np.uint8)).cuda()
            recs_before, stats_before = d_recs.clone(), st.stats.clone()
            b["rew"].fill_(-7.0)
            check(step_masked(L, dw, d_recs, n, a, d_act, k, ring[t % F], ring[new], b), "step_masked")
        rsum, wrote = np.zeros(n, np.float64), np.zeros(n, np.uint8)
        cov["inactive_live"] += int(np.sum(~act & (h_term == 0)))
        cov["term_then_inactive"] += int(np.sum(~act & ended))
        if t == 0:
            cov["inactive_first"] = int(np.sum(~act))
        for e in np.flatnonzero(act):
            v, ae = views[e], np.ascontiguousarray(acts[t, e])
            last = 0
            for j in range(1, k + 1):
                h_cause[e] = orc.step_one(recs[e], ae, h_frames[e])
                rsum[e] += v.h("REWARD")
                last = j
                if v.i("TERM"):
                    break
            if omask is not None:
                h_frames[e][omask] = 8
            h_term[e], h_trunc[e] = v.i("TERM"), v.i("TRUNC")
            h_info[e] = info_of(v, h_cause[e])
            hist[last if h_term[e] else 0] += 1
            if h_term[e]:
                wrote[e] = 1
                tcount[e] += 1
                ended[e] = True
        seen_active |= act
        seen_inactive |= ~act
        if not device:
            continue
        torch.cuda.synchronize()
        df = ring[new].cpu().numpy()
        bad = np.argwhere(df != h_frames)
        assert bad.size == 0, (t, bad[:8], act[bad[0][0]])
        dr = d_recs.cpu().numpy()
        for e in range(n):
            compare_records(dr[e], recs[e], layout, tag=(t, e))
        off = torch.from_numpy(np.flatnonzero(~act)).cuda()
        assert torch.equal(d_recs[off], recs_before[off]), (t, "an inactive env's record changed")
        assert torch.equal(st.stats[off], stats_before[off]), (t, "an inactive env's Stats changed")
        assert np.array_equal(b["term"].cpu().numpy(), h_term), t
        assert np.array_equal(b["trunc"].cpu().numpy(), h_trunc), t
        rew = b["rew"].cpu().numpy()
        assert np.all(rew[~act] == 0.0), (t, rew, act)
        assert np.allclose(rew, rsum, rtol=1e-9, atol=1e-12), (t, rew, rsum)
        assert np.array_equal(b["cause"].cpu().numpy(), h_cause), (t, b["cause"].cpu().numpy(), h_cause)
        got = b["info"].cpu().numpy()
        assert np.array_equal(got[:, 13:], h_info[:, 13:]), (t, "info ints")
        assert np.allclose(got, h_info, rtol=1e-6, atol=1e-6), (t, "info")
        on = np.flatnonzero(act)
        st.check(t, wrote, on, [views[e] for e in on], h_cause[on])
        assert np.array_equal(reset_counts(L, dw, n).astype(np.int64), tcount), (t, "reset counts")
        assert termination_count(L, dw) == int(tcount.sum()), (t, "termination count")
    if device:
        assert error_flags(dw.ctx) == 0
    cov.update(hist=hist.tolist(), both=bool(np.all(seen_active & seen_inactive)))
    return cov


def _covers_every_case(cov, every_substep):
    """Conditions on the inputs, from the oracle's side: every env is active on
    some steps and inactive on others; some env terminated while active and was
    inactive later (term == 1 retained); some env was inactive with term == 0;
    some env was inactive on the first step after the reset; every_substep:
    every substep position ended some active env and some active env ran them all."""
    assert cov["both"], cov
    assert cov["term_then_inactive"] > 0 and cov["inactive_live"] > 0 and cov["inactive_first"] > 0, cov
    if every_substep:
        assert all(c > 0 for c in cov["hist"]), cov
    else:
        assert cov["hist"][0] > 0 and sum(cov["hist"][1:]) > 0, cov


MASKED_CASES = [
    # config, kinds, n, size, seed0, act_seed, k, steps, F
    pytest.param(2, ["rt_no_traffic_v1"], 37, 128, 10_000, 21, 1, 40, 2, id="config2-k1"),
    pytest.param(2, ["rt_no_traffic_v1"], 37, 128, 10_000, 21, 3, 40, 2, id="config2-k3"),
    pytest.param(3, ["rt_hard_v1"], 8, 128, 20_000, 7, 2, 30, 2, id="config3-k2"),
    pytest.param(5, ["mix3"], 5, 256, 30_000, 1234, 1, 30, 1, id="config5-k1"),
]


@pytest.mark.parametrize("config,kinds,n,size,seed0,act_seed,k,steps,F", MASKED_CASES)
def test_masked_step_matches_the_oracle(config, kinds, n, size, seed0, act_seed, k, steps, F):
    cov = run_masked_parity(kinds, n, steps, k, size=size, seed0=seed0, act_seed=act_seed, caps=bench_caps(config),
                            mask_seed=100 + n, F=F)
    _covers_every_case(cov, every_substep=(k == 3))


def test_masked_step_at_size_64_ego_only():
    """k_raster_mask<1> and prev_frames == frames, on authored ego-only records."""
    n = 9
    P, padded, caps, recs, layout = ego_only_64(n)
    cov = run_masked_parity(None, n, 30, 1, caps=caps, recs=recs, world_=(P, padded), mask_seed=109, F=1)
    _covers_every_case(cov, every_substep=False)


@pytest.mark.parametrize("config,kinds,k", [(2, ("rt_no_traffic_v1",), 1), (2, ("rt_no_traffic_v1",), 4),
                                            (3, ("rt_hard_v1", "rt_medium_v1"), 4)])
def test_all_active_equals_step_repeat_bitwise(config, kinds, k):
    """Every env active: the masked step and cbev_step_repeat leave the same
    bytes everywhere, through cbev_reset_terminated after each step (which reads
    the context's last term buffer and env count, set by either call)."""
    n, n_bank, F, steps = 19, 53, 3, 20
    P, lanes = twins(n, bench_caps(config), 128, kinds, 10_419, 14_419, n_bank=n_bank, F=F)
    L = lib()
    acts = action_stream(P, n, steps, seed=5)
    ones = torch.ones(n, dtype=torch.uint8, device="cuda")
    A, B = lanes
    for t in range(steps):
        a = torch.from_numpy(np.ascontiguousarray(acts[t])).cuda()
        dw, _, _, d_recs, ring, b = A
        check(step_repeat(L, dw, d_recs, n, a, k, ring[(t + 1) % F], b), "step_repeat")
        dw, _, _, d_recs, ring, b = B
        check(step_masked(L, dw, d_recs, n, a, ones, k, ring[t % F], ring[(t + 1) % F], b), "step_masked")
        torch.cuda.synchronize()
        assert_same(lanes, t)
        reset_terminated_all(lanes)
    torch.cuda.synchronize()
    assert torch.equal(A.recs, B.recs) and torch.equal(A.ring, B.ring)
    assert int(reset_counts(L, A.dw, n).sum()) > 0
    for dw, *_ in lanes:
        assert error_flags(dw.ctx) == 0


@pytest.mark.parametrize("same_slot", [False, True])
def test_all_inactive_touches_nothing_but_reward_and_frames(same_slot):
    n, F, k = 21, 2, 2
    P, lanes = twins(n, bench_caps(3), 128, ("rt_hard_v1",), 10_519, 14_519, F=F)
    L = lib()
    dw, d_bank, bf, d_recs, ring, b = lanes[0]
    a = torch.ones(n, dtype=torch.int32, device="cuda")
    ones, zeros = torch.ones(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    check(step_masked(L, dw, d_recs, n, a, ones, k, ring[1], ring[0], b), "step_masked")  # step 0: some terminate
    torch.cuda.synchronize()
    assert int(b["term"].sum()) > 0 and int((b["term"] == 0).sum()) > 0
    st = b["stats"]
    before = [d_recs.clone(), st.stats.clone(), st.rows.clone()] + [b[key].clone() for key in KEYS[1:]]
    ring0, counts0, nterm0 = ring.clone(), reset_counts(L, dw, n), termination_count(L, dw)
    b["rew"].fill_(3.5)
    dst = ring[0] if same_slot else ring[1]
    assert not torch.equal(ring[0], ring[1])
    check(step_masked(L, dw, d_recs, n, a, zeros, k, ring[0], dst, b), "step_masked")  # step 1: nobody moves
    torch.cuda.synchronize()
    after = [d_recs, st.stats, st.rows] + [b[key] for key in KEYS[1:]]
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert torch.equal(b["rew"], torch.zeros_like(b["rew"]))
    assert torch.equal(ring[0], ring0[0])
    assert torch.equal(ring[1], ring0[1] if same_slot else ring0[0])
    assert int(st.counts[1 % st.RING].item()) == 0  # step 1 wrote no episode row
    assert np.array_equal(reset_counts(L, dw, n), counts0) and termination_count(L, dw) == nterm0
    assert error_flags(dw.ctx) == 0


def test_an_inactive_env_raises_no_action_error():
    n = 21
    P, lanes = twins(n, bench_caps(2), 128, ("rt_no_traffic_v1",), 10_619, 14_619, F=2)
    L = lib()
    dw, d_bank, bf, d_recs, ring, b = lanes[0]
    a = torch.ones(n, dtype=torch.int32, device="cuda")
    a[5], a[18] = 100, -100  # out of range for discrete9_v1
    act = torch.ones(n, dtype=torch.uint8, device="cuda")
    act[5] = act[18] = 0
    for k in (1, 3):
        check(step_masked(L, dw, d_recs, n, a, act, k, ring[0], ring[1], b), "step_masked")
        torch.cuda.synchronize()
        assert error_flags(dw.ctx) == 0
    act[18] = 1
    check(step_masked(L, dw, d_recs, n, a, act, 1, ring[1], ring[0], b), "step_masked")
    torch.cuda.synchronize()
    assert error_flags(dw.ctx) == ERR_ACTION_INDEX


@pytest.mark.parametrize("ne", ["2", "64"])
def test_masked_ego_workgroup_shapes(ne, monkeypatch):
    """k_ego_mask with 4 envs per workgroup (CBEV_EGO_NE=2 is raised to the
    floor) and with the most the LDS admits (read at cbev_create: the masked
    kernels need k_ego's dynamic LDS limit): whole workgroups inactive, mixed
    ones, and a partial last one."""
    monkeypatch.setenv("CBEV_EGO_NE", ne)
    cov = run_masked_parity(["rt_no_traffic_v1"], 37, 24, 3, seed0=10_000, caps=bench_caps(2), mask_seed=137)
    assert cov["both"] and sum(cov["hist"][1:]) > 0, cov
    run_masked_parity(["rt_hard_v1"], 13, 8, 2, seed0=20_000, act_seed=7, caps=bench_caps(3), mask_seed=113)


def test_masked_step_fov_masked():
    """The FOV corner mask in k_raster_mask's render path and in the kept frames."""
    from helpers import CAPS_FULL
    cov = run_masked_parity(["rt_medium_v1"], 16, 16, 2, seed0=77, caps=CAPS_FULL, mask_seed=116, fov=True)
    assert cov["both"], cov


def test_masked_step_under_graph_capture():
    """One masked step (k = 2) captured into a graph and replayed twice with the
    mask tensor edited between the replays equals two eager calls with those
    masks from the same start: the mask is read when the launches run."""
    n, F, k = 19, 2, 2
    P, lanes = twins(n, bench_caps(2), 128, ("rt_no_traffic_v1",), 10_719, 14_719, F=F)
    L = lib()
    acts = torch.ones(n, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(3)
    masks = [torch.from_numpy((rng.random(n) < 0.5).astype(np.uint8)).cuda() for _ in range(3)]
    assert not torch.equal(masks[1], masks[2])
    m_graph = masks[0].clone()

    def step(c, m):
        dw, _, _, d_recs, ring, b = c
        check(step_masked(L, dw, d_recs, n, acts, m, k, ring[0], ring[1], b,
                          P_(torch.cuda.current_stream().cuda_stream)), "step_masked")

    A, B = lanes
    step(A, masks[0])  # one eager call each: the kernels are loaded before the capture
    step(B, m_graph)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            step(B, m_graph)
    torch.cuda.synchronize()
    assert torch.equal(A.recs, B.recs)  # the capture ran nothing
    for rep in (1, 2):
        step(A, masks[rep])
        m_graph.copy_(masks[rep])
        g.replay()
        torch.cuda.synchronize()
        assert_same_outputs(A, B, rep)
        assert torch.equal(B.out["rew"][m_graph == 0], torch.zeros_like(B.out["rew"])[m_graph == 0]), rep
    assert int(A.out["term"].sum()) > 0


def test_pending_deferred_reset_is_applied_before_the_masked_step():
    """cbev_step_masked + cbev_reset_terminated with the deferred reset on (the
    masked step launches the recorded reset before substep 1) against the same
    with it off: everything equal after every step."""
    n, B, F, k, steps = 45, 13, 3, 2, 20
    P, layout, lanes = deferred_pair(n, B, F, bench_caps(2), 7100, 17100)
    L = lib()
    for dw, d_bank, bf, d_recs, ring, b in lanes:  # every second env starts off the road
        check(L.cbev_flush(dw.ctx), "flush")
        h = d_recs.cpu().numpy()
        for e in range(0, n, 2):
            LY.RecordView(h[e], layout).hd[LY.HD["X"]] += 60.0
        d_recs.copy_(torch.from_numpy(h))
    acts = action_stream(P, n, steps, seed=21)
    masks = mask_stream(n, steps, 145)
    A, Bc = lanes
    pending = 0
    for t in range(steps):
        a = torch.from_numpy(np.ascontiguousarray(acts[t])).cuda()
        m = torch.from_numpy(masks[t].astype(np.uint8)).cuda()
        pending += L.cbev_reset_pending(Bc.dw.ctx)
        for dw, d_bank, bf, d_recs, ring, b in lanes:
            check(step_masked(L, dw, d_recs, n, a, m, k, ring[t % F], ring[(t + 1) % F], b), "step_masked")
            assert L.cbev_reset_pending(dw.ctx) == 0
        torch.cuda.synchronize()
        assert_same(lanes, t)
        reset_terminated_all(lanes)
    flush_all(lanes)
    assert torch.equal(A.recs, Bc.recs) and torch.equal(A.ring, Bc.ring)
    assert pending >= steps - 1 and int(reset_counts(L, A.dw, n).sum()) > 0


def test_refusals_leave_a_live_context_untouched():
    n, F = 19, 2
    P, lanes = twins(n, bench_caps(2), 128, ("rt_no_traffic_v1",), 10_819, 14_819, F=F)
    L = lib()
    dw, d_bank, bf, d_recs, ring, b = lanes[0]
    acts = torch.full((n,), 100, dtype=torch.int32, device="cuda")  # would raise the action flag if anything ran
    ones = torch.ones(n, dtype=torch.uint8, device="cuda")
    good = torch.ones(n, dtype=torch.int32, device="cuda")
    check(step_masked(L, dw, d_recs, n, good, ones, 2, ring[0], ring[1], b), "step_masked")
    torch.cuda.synchronize()
    st = b["stats"]
    before = [d_recs.clone(), ring.clone(), st.stats.clone(), st.rows.clone(), st.counts.clone()] + [
        b[key].clone() for key in KEYS]
    counts0, nterm0 = reset_counts(L, dw, n), termination_count(L, dw)

    def call(act=ones, prev=ring[1], k=2, n_=n):
        return L.cbev_step_masked(dw.ctx, ptr(d_recs), n_, ptr(acts), ptr(act), k, ptr(prev), ptr(ring[0]),
                                  ptr(b["rew"]), ptr(b["term"]), ptr(b["trunc"]), ptr(b["cause"]), ptr(b["info"]), None)

    assert call(act=None) == CBEV_EINVAL and b"active" in L.cbev_last_error()
    assert call(prev=None) == CBEV_EINVAL and b"prev_frames" in L.cbev_last_error()
    for bad in (0, 65, -3):
        assert call(k=bad) == CBEV_EINVAL and b"repeat" in L.cbev_last_error()
    assert call(n_=n + 1) == CBEV_EINVAL and b"episode stats" in L.cbev_last_error()  # above the statistics' ep_n
    torch.cuda.synchronize()
    after = [d_recs, ring, st.stats, st.rows, st.counts] + [b[key] for key in KEYS]
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(reset_counts(L, dw, n), counts0) and termination_count(L, dw) == nterm0
    assert error_flags(dw.ctx) == 0
    check(step_masked(L, dw, d_recs, n, good, ones, 64, ring[1], ring[0], b), "step_masked")  # the largest repeat runs
    torch.cuda.synchronize()
    assert error_flags(dw.ctx) == 0


# ---------------------------------------------------------------------- the vector env
def _run_eval(envs, N, limit):
    """Step the freeze_done env and its plain twin with the same actions until
    all_done(). Returns {env: (r, l)} of the frozen env's infos (asserting one
    episode per env) and of the twin's first episode per env."""
    frozen, plain = envs
    got, first = {}, {}
    done_before = np.zeros(N, bool)
    steps = 0
    while not frozen.all_done():
        assert steps < limit, "the evaluation did not end"
        a = eval_actions(N, steps)
        rec0 = frozen.records.clone()
        _, r, term, _, infos = frozen.step(a)
        _, _, term1, _, infos1 = plain.step(a)
        assert torch.equal(frozen.records[torch.from_numpy(done_before).to(rec0.device)],
                           rec0[torch.from_numpy(done_before).to(rec0.device)]), (steps, "a done env's record moved")
        assert torch.equal(r[torch.from_numpy(done_before).to(r.device)],
                           torch.zeros(int(done_before.sum()), dtype=r.dtype, device=r.device))
        if "_episode" in infos:
            for e in np.flatnonzero(infos["_episode"]):
                assert int(e) not in got, (steps, e, "a second episode row")
                got[int(e)] = (float(infos["episode"]["r"][e]), int(infos["episode"]["l"][e]))
        if "_episode" in infos1:
            for e in np.flatnonzero(infos1["_episode"]):
                first.setdefault(int(e), (float(infos1["episode"]["r"][e]), int(infos1["episode"]["l"][e])))
        done_before = frozen.done_mask().cpu().numpy()
        assert np.array_equal(done_before, term.cpu().numpy())  # the latch is what step() returns
        steps += 1
    return got, first, steps


def test_freeze_done_runs_one_episode_per_env(monkeypatch):
    N, max_actions = 24, 40
    envs, opts = eval_pair(monkeypatch, N, max_actions)
    frozen, plain = envs
    assert frozen.params.max_actions == max_actions
    assert frozen.freeze_done and not plain.freeze_done
    assert not frozen.all_done()
    got, first, steps = _run_eval(envs, N, max_actions + 2)
    assert sorted(got) == list(range(N))  # every env exactly once
    for e in range(N):
        assert got[e][1] == first[e][1] and got[e][0] == first[e][0], (e, got[e], first[e])
    assert [got[e][1] for e in range(N)] == (2 + (5 * np.arange(N)) % 37).tolist()  # ended where eval_pair set it
    assert steps == max(got[e][1] for e in range(N))  # the others stood still until the slowest was done
    assert frozen.termination_count() == N
    assert plain.termination_count() > N  # the plain env went on terminating
    assert frozen.errors() == 0
    # a reset of some envs clears their latch only
    m = np.zeros(N, bool)
    m[:5] = True
    frozen.reset(seed=11, options=dict(opts, reset_mask=m))
    assert np.array_equal(frozen.done_mask().cpu().numpy(), ~m)
    rec0 = frozen.records.clone()
    frozen.step(eval_actions(N, 0))
    moved = (frozen.records != rec0).any(dim=1).cpu().numpy()
    assert np.array_equal(moved, m)
    # reset_terminated() clears the latch and the envs run again
    bank = frozen.build_bank(list(range(900, 916)), opts)
    frozen.attach_bank(bank)
    while not frozen.all_done():
        frozen.step(eval_actions(N, 1))
    frozen.reset_terminated()
    assert not frozen.done_mask().any()
    rec0 = frozen.records.clone()
    _, r, term, _, _ = frozen.step(eval_actions(N, 2))
    assert (frozen.records != rec0).any(dim=1).all()
    for env in envs:
        env.close()


def test_freeze_done_with_bits_and_action_repeat(monkeypatch):
    N, max_actions = 24, 40
    envs, _ = eval_pair(monkeypatch, N, max_actions, obs_dtype="bits", action_repeat=2)
    got, first, steps = _run_eval(envs, N, max_actions // 2 + 2)
    assert sorted(got) == list(range(N))
    for e in range(N):
        assert got[e] == first[e], (e, got[e], first[e])
    assert envs[0].termination_count() == N and envs[0].errors() == 0
    for env in envs:
        env.close()


def test_step_with_an_active_mask_on_a_resize_config(monkeypatch):
    """step(a, active=m) on obs 96 at size 128 against the C-ABI call on a copy
    of the env's own records and render-size frames (frames == prev_frames: an
    inactive env's frame stays and is resized again)."""
    from carlabev_env_amd import RandomNavigationReset, build_random_navigation_options, make_env
    N = 10
    env = make_env({"env": eval_cfg(monkeypatch, 200, obs=96), "num_envs": N}, num_envs=N, caps=EGO_ONLY,
                   info_mode="none")
    opts = build_random_navigation_options(RandomNavigationReset(difficulty_id="rt_no_traffic_v1"))
    env.reset(seed=5, options=opts)
    assert env.resize and env.full is not None
    L = lib()
    dw = DevWorld(env.params, env.map_host, env.caps)
    b = out_bufs(N)
    rng = np.random.default_rng(9)
    for t in range(6):
        a = eval_actions(N, t).astype(np.int32)
        m = rng.random(N) < 0.5
        d_recs, fr = env.records.clone(), env.full.clone()
        ring0, head0 = env.ring.clone(), env.head
        d_a, d_m = torch.from_numpy(a).cuda(), torch.from_numpy(m.astype(np.uint8)).cuda()
        check(step_masked(L, dw, d_recs, N, d_a, d_m, 1, fr, fr, b), "step_masked")
        active = m if t % 2 else torch.from_numpy(m).cuda()  # a numpy mask is uploaded
        _, r, term, trunc, _ = env.step(d_a, active=active)
        torch.cuda.synchronize()
        assert torch.equal(env.records, d_recs) and torch.equal(env.full, fr), t
        assert torch.equal(r, b["rew"]) and bool((r[~torch.from_numpy(m).cuda()] == 0).all()), t
        off = torch.from_numpy(np.flatnonzero(~m)).cuda()
        assert env.head == (head0 + 1) % env.F
        assert torch.equal(env.ring[env.head][off], ring0[head0][off]), (t, "an inactive env's frame is kept")
    with pytest.raises(ValueError, match="shape"):
        env.step(d_a, active=torch.ones(N + 1, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="dtype"):
        env.step(d_a, active=torch.ones(N, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="cpu"):
        env.step(d_a, active=torch.ones(N, dtype=torch.bool))
    env.close()
