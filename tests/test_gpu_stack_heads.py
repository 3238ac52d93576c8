"""Per-env frame-stack heads: cbev_expand_obs_heads against the global-head
expansion on the re-laid ring, cbev_step_heads against cbev_step_masked on a
one-slot frame buffer with a host deque per env, the time-warp invariance of
make_env(cfg, stack_heads="per_env"), freeze_done in that mode, resets, a
captured step + expansion, and the refusals. Everything is bitwise: both sides
run the same arithmetic, there is no tolerance to choose.
"""
from __future__ import annotations

from collections import deque

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from carlabev_env_amd import layout as LY
from carlabev_env_amd._lib import check, lib
from carlabev_env_amd.semantics import gray_lut, semantic_lut, semantic_mask_channels
from gpu_harness import (KEYS, P_, DevWorld, EpisodeStatsOn, assert_same_outputs, error_flags, out_bufs, ptr,
                         reset_counts, same_stats, step_masked, termination_count)
from gpu_scenes import (CODES, EGO_ONLY, GUARD, cout, dtypes_of, ego_only_64, eval_actions, eval_cfg, eval_pair,
                        mask_stream, obs_world, out_bytes, relaid, twins)
from helpers import CAPS_FULL, action_stream, bench_caps, build_records, world

pytestmark = pytest.mark.gpu

CBEV_EINVAL = -1
MODE = "7-class"  # a semantic mode with a vehicle channel: the three fusions apply


def step_heads(L, dw, d_recs, n, a, act, k, ring, F, heads, b, stream=None):
    return L.cbev_step_heads(dw.ctx, ptr(d_recs), n, ptr(a), ptr(act), k, ptr(ring), F, ptr(heads), ptr(b["rew"]),
                             ptr(b["term"]), ptr(b["trunc"]), ptr(b["cause"]), ptr(b["info"]), stream)


# ---------------------------------------------------------------------- 1. the expansion
def _expand(c, heads_call, ring_d, n, F, head, kind, C, lut, dt, Cout, P, offset):
    nb = out_bytes(dt, n, Cout, P)
    buf = torch.full((offset + nb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[offset:offset + nb]
    lp = lut.ctypes.data_as(P_) if lut is not None else None
    if heads_call:
        rc = lib().cbev_expand_obs_heads(c.ctx, ptr(ring_d), n, F, ptr(head), kind, C, lp, CODES[dt], ptr(out), None)
    else:
        rc = lib().cbev_expand_obs_typed(c.ctx, ptr(ring_d), n, F, head, kind, C, lp, CODES[dt], ptr(out), None)
    check(rc, "expand")
    return buf


def _kinds(F):
    """(kind, wire type, lut, channels) of a case: FUSE 0 / 1 / 2 in their wire types
    (the fusions keep 3 frames) and the two gray stacks."""
    C = len(semantic_mask_channels(MODE))
    out = []
    for kind in (0, 3, 4) if F >= 3 else (0,):
        out += [(kind, dt, semantic_lut(MODE), C) for dt in dtypes_of(kind)]
    return out + [(1, "uint8", gray_lut(), 1), (5, "uint8", None, 1)]


EXPAND_CASES = [
    # hw, n, F, offset in elements
    pytest.param((64, 64), 37, 4, 0, id="64x64-F4"),    # every wide path
    pytest.param((64, 64), 37, 3, 0, id="64x64-F3"),
    pytest.param((84, 84), 11, 4, 0, id="84x84-F4"),    # bits V = 8, the others wide
    pytest.param((5, 7), 37, 3, 0, id="5x7-F3"),        # V = 1 everywhere
    pytest.param((64, 64), 37, 4, 1, id="64x64-misaligned"),  # V = 1 through a misaligned out
    pytest.param((64, 64), 37, 1, 0, id="64x64-F1"),
]


@pytest.mark.parametrize("hw,n,F,off_elems", EXPAND_CASES)
def test_expansion_equals_the_global_head_kernels_on_the_relaid_ring(hw, n, F, off_elems):
    c = obs_world(hw)
    P = hw[0] * hw[1]
    rng = np.random.default_rng(1000 * hw[0] + 10 * F + off_elems)
    ring = torch.from_numpy(rng.integers(0, 10, (F, n, *hw)).astype(np.uint8)).cuda()
    h = np.arange(n) % F
    rng.shuffle(h)
    assert set(h.tolist()) == set(range(F))  # every head value occurs
    heads = torch.from_numpy(h.astype(np.uint8)).cuda()
    ring2 = relaid(ring, heads)
    for kind, dt, lut, C in _kinds(F):
        if off_elems and kind in (1, 5):
            continue  # the gray stacks pick their width from the pixel count alone
        Cout = cout(kind, F, C) if kind in (0, 3, 4) else F
        off = off_elems * {"float32": 4, "float16": 2, "uint8": 1, "bits": 1}[dt]
        want = _expand(c, False, ring2, n, F, F - 1, kind, C, lut, dt, Cout, P, off)
        got = _expand(c, True, ring, n, F, heads, kind, C, lut, dt, Cout, P, off)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (kind, dt)  # the output and the 0xA5 bytes around it
        assert bool((want[off:off + 64] != 0xA5).any())


def test_a_head_byte_out_of_range_stays_inside_the_ring():
    hw, n, F = (64, 64), 13, 4
    c = obs_world(hw)
    rng = np.random.default_rng(5)
    ring = torch.from_numpy(rng.integers(0, 10, (F, n, *hw)).astype(np.uint8)).cuda()
    h = (np.arange(n) % F).astype(np.uint8)
    bad = [3, 8]
    good = torch.from_numpy(np.setdiff1d(np.arange(n), bad)).cuda()
    heads_ok = torch.from_numpy(h).cuda()
    h[3], h[8] = 255, F  # caller errors: unspecified frame order for these envs, no fault
    heads = torch.from_numpy(h).cuda()
    ring2 = relaid(ring, heads_ok)
    P = hw[0] * hw[1]
    for kind, dt, lut, C in _kinds(F):
        Cout = cout(kind, F, C) if kind in (0, 3, 4) else F
        want = _expand(c, False, ring2, n, F, F - 1, kind, C, lut, dt, Cout, P, 0)
        got = _expand(c, True, ring, n, F, heads, kind, C, lut, dt, Cout, P, 0)  # check(): it returned 0
        torch.cuda.synchronize()  # raises on a fault
        nb = out_bytes(dt, n, Cout, P)
        assert torch.equal(got[:nb].reshape(n, -1)[good], want[:nb].reshape(n, -1)[good]), (kind, dt)
        assert torch.equal(got[nb:], want[nb:])


def test_expansion_refusals():
    c = obs_world((64, 64))
    L = lib()
    buf = torch.zeros(4 * 64 * 64 * 64, dtype=torch.uint8, device="cuda")
    ring, heads = buf[:3 * 64 * 64], buf[:1]
    lut = semantic_lut(MODE).ctypes.data_as(P_)

    def call(ring_=ring, heads_=heads, kind=0, dt="float32", F=3):
        return L.cbev_expand_obs_heads(c.ctx, ptr(ring_), 1, F, ptr(heads_), kind, 7, lut, CODES[dt], ptr(buf), None)

    assert call(heads_=None) == CBEV_EINVAL
    assert call(ring_=None) == CBEV_EINVAL
    assert call(kind=2, dt="uint8") == CBEV_EINVAL and b"kind 2" in L.cbev_last_error()
    assert call(kind=4, dt="uint8") == CBEV_EINVAL and call(kind=4, dt="bits") == CBEV_EINVAL
    assert call(kind=1, dt="float32") == CBEV_EINVAL and call(kind=5, dt="bits") == CBEV_EINVAL
    assert call(kind=3, F=2) == CBEV_EINVAL and call(F=0) == CBEV_EINVAL and call(F=256) == CBEV_EINVAL
    assert call(kind=9) == CBEV_EINVAL
    assert L.cbev_expand_obs_heads(c.ctx, ptr(ring), 1, 3, ptr(heads), 0, 7, lut, 7, ptr(buf), None) == CBEV_EINVAL
    torch.cuda.synchronize()
    assert not bool(buf.any())  # nothing was launched


# ---------------------------------------------------------------------- 2. the step
def _step_world(case):
    """(P, padded, caps, recs) of a case: run_masked_parity's records (every fifth
    env starts off the road, so it ends in its first active substep)."""
    if case["recs"] == "ego64":
        P, padded, caps, recs, layout = ego_only_64(case["n"])
        for e in (2, 5):  # far beside the road: they end within their first active steps
            LY.RecordView(recs[e], layout).hd[LY.HD["Y"]] += 25.0
        return P, padded, caps, recs
    caps = case["caps"]
    cfg, P, padded, layout, builder = world(case["size"], caps=caps)
    recs, _ = build_records(builder, case["n"], case["kinds"], seed0=case["seed0"])
    for e in range(2, case["n"], 5):
        LY.RecordView(recs[e], layout).hd[LY.HD["X"]] += 60.0
    return P, padded, caps, recs


def _case(**kw):
    base = dict(recs="built", size=128, fov=False, steps=14, act_seed=21)
    base.update(kw)
    return base


STEP_CASES = [
    pytest.param(_case(caps=bench_caps(2), kinds=["rt_no_traffic_v1"], n=37, seed0=10_000, k=1, mask_seed=137),
                 id="config2-k1"),
    pytest.param(_case(caps=bench_caps(2), kinds=["rt_no_traffic_v1"], n=37, seed0=10_000, k=3, mask_seed=137),
                 id="config2-k3"),
    pytest.param(_case(caps=bench_caps(3), kinds=["rt_hard_v1"], n=19, seed0=20_000, k=2, mask_seed=119, act_seed=7),
                 id="config3-k2"),
    pytest.param(_case(recs="ego64", n=9, k=1, mask_seed=109, act_seed=1234, steps=16), id="size64"),
    pytest.param(_case(caps=bench_caps(5), kinds=["mix3"], n=5, size=256, seed0=30_000, k=1, mask_seed=105,
                       act_seed=1234, steps=16), id="size256"),
    pytest.param(_case(caps=CAPS_FULL, kinds=["rt_medium_v1"], n=16, seed0=77, k=2, mask_seed=116, act_seed=1234,
                       fov=True, steps=12), id="fov"),
]


@pytest.mark.parametrize("case", STEP_CASES)
def test_step_heads_equals_step_masked_on_one_slot(case):
    """Twin A: cbev_step_masked on a one-slot frame buffer (prev_frames ==
    frames) and a host deque of F frames per env, pushed on the env's active
    steps only. Twin B: cbev_step_heads on an F-slot ring. The heads start at
    arbitrary slots: a reset fills every slot, so any head is right after it."""
    n, k, F, steps = case["n"], case["k"], 3, case["steps"]
    P, padded, caps, recs = _step_world(case)
    S = P.size
    L = lib()
    masks = mask_stream(n, steps, case["mask_seed"])
    acts = action_stream(P, n, steps, seed=case["act_seed"])
    twins = []
    for nf in (1, F):
        dw = DevWorld(P, padded, caps)
        if case["fov"]:
            from carlabev_env_amd.fov_mask import fov_corner_mask
            check(L.cbev_set_fov_mask(dw.ctx, fov_corner_mask(S).ctypes.data_as(P_)), "fov")
        d_recs = torch.from_numpy(recs.copy()).cuda()
        ring = torch.zeros((nf, n, S, S), dtype=torch.uint8, device="cuda")
        check(L.cbev_reset(dw.ctx, ptr(d_recs), n, None, 0, None, None, 0, ptr(ring), nf, None), "reset")
        b = out_bufs(n)
        b["stats"] = EpisodeStatsOn(dw.ctx, n)
        twins.append((dw, d_recs, ring, b))
    (dA, rA, fA, bA), (dB, rB, gB, bB) = twins
    torch.cuda.synchronize()
    h = ((7 * np.arange(n) + 1) % F).astype(np.uint8)
    heads = torch.from_numpy(h.copy()).cuda()
    dq = [deque([fA[0, e].cpu().numpy()] * F, maxlen=F) for e in range(n)]
    ar = torch.arange(n, device="cuda")
    ended = np.zeros(n, bool)
    end_beside_inactive = ended_then_inactive = 0
    for t in range(steps):
        act = masks[t]
        a = torch.from_numpy(np.ascontiguousarray(acts[t])).cuda()
        d_act = torch.from_numpy(act.astype(np.uint8)).cuda()
        ring0, heads0 = gB.clone(), heads.clone()
        for b in (bA, bB):
            b["rew"].fill_(-7.0)
        check(step_masked(L, dA, rA, n, a, d_act, k, fA[0], fA[0], bA), "step_masked")
        check(step_heads(L, dB, rB, n, a, d_act, k, gB, F, heads, bB), "step_heads")
        torch.cuda.synchronize()
        assert torch.equal(rA, rB), (t, "records")
        for key in KEYS:
            assert torch.equal(bA[key], bB[key]), (t, key)
        assert same_stats(bA["stats"], bB["stats"], t, n), (t, "episode stats")
        assert torch.equal(bA["stats"].counts, bB["stats"].counts), (t, "row counts")
        assert np.array_equal(reset_counts(L, dA, n), reset_counts(L, dB, n)), (t, "reset counts")
        assert termination_count(L, dA) == termination_count(L, dB), (t, "termination count")
        h[act] = (h[act] + 1) % F  # once per call, whatever k is
        assert np.array_equal(heads.cpu().numpy(), h), (t, "heads")
        assert torch.equal(gB[heads.long(), ar], fA[0]), (t, "the newest frame")
        fa = fA[0].cpu().numpy()
        gb = relaid(gB, heads).cpu().numpy()  # [f][e], oldest first
        for e in range(n):
            if act[e]:
                dq[e].append(fa[e])
            assert all(np.array_equal(gb[f, e], dq[e][f]) for f in range(F)), (t, e, "head order against the deque")
        off = torch.from_numpy(np.flatnonzero(~act)).cuda()
        assert torch.equal(heads[off], heads0[off]) and torch.equal(gB[:, off], ring0[:, off]), (t, "an inactive env")
        # what the inputs covered, from twin A's outputs
        term = bA["term"].cpu().numpy().astype(bool)
        end_beside_inactive += int((term & act & ~ended).any() and (~act).any())
        ended_then_inactive += int((ended & ~act).sum())
        ended |= term & act
    assert end_beside_inactive > 0 and ended_then_inactive > 0, (end_beside_inactive, ended_then_inactive)
    assert error_flags(dA.ctx) == 0 and error_flags(dB.ctx) == 0


# ---------------------------------------------------------------------- 3-5. the vector env
def _pair(monkeypatch, N, max_actions=200, obs_mode="bev_semantic", **kw):
    """A default env and a stack_heads="per_env" one on the same seeded reset."""
    from carlabev_env_amd import RandomNavigationReset, build_random_navigation_options, make_env
    cfg = eval_cfg(monkeypatch, max_actions).model_copy(update={"obs_mode": obs_mode})
    envs = [make_env({"env": cfg, "num_envs": N}, num_envs=N, caps=EGO_ONLY, stack_heads=sh, **kw)
            for sh in ("global", "per_env")]
    opts = build_random_navigation_options(RandomNavigationReset(difficulty_id="rt_no_traffic_v1"))
    o0, _ = envs[0].reset(seed=11, options=opts)
    o1, _ = envs[1].reset(seed=11, options=opts)
    assert torch.equal(o0, o1)
    return envs, opts


@pytest.mark.parametrize("obs_mode,obs_dtype", [("bev_semantic", "float32"), ("bev_semantic", "bits"),
                                                ("bev_rgb", "float32")])
def test_time_warp_invariance(monkeypatch, obs_mode, obs_dtype):
    """Env e's observation after its k-th active step of a masked run equals the
    observation after step k of a plain run with the same actions, until its
    first termination; after an inactive step it equals its previous one."""
    N, T = 24, 10
    (plain, warped), _ = _pair(monkeypatch, N, obs_mode=obs_mode, obs_dtype=obs_dtype)
    assert warped.stack_heads == "per_env" and warped.F == 4 and warped.heads.dtype == torch.uint8
    assert plain.stack_heads == "global" and plain.heads is None
    a = np.stack([eval_actions(N, t) for t in range(T)]).astype(np.int32)
    obs_A, term_A = [], []
    for t in range(T):
        o, _, term, _, _ = plain.step(a[t])
        obs_A.append(o)
        term_A.append(term.cpu().numpy())
    alive = np.logical_not(np.logical_or.accumulate(np.stack(term_A), axis=0))  # [k][e]: no termination up to step k
    rng = np.random.default_rng(3)
    kc = np.zeros(N, np.int64)
    prev = warped._obs()
    compared = kept = 0
    for t in range(T):
        m = rng.random(N) < 0.5
        m[t % N] = False
        act = a[np.minimum(kc, T - 1), np.arange(N)]
        o, r, _, _, _ = warped.step(act, active=torch.from_numpy(m).cuda())
        for e in range(N):
            if m[e]:
                k = kc[e]
                if k == 0 or alive[k - 1, e]:  # the env had not terminated before this step
                    assert torch.equal(o[e], obs_A[k][e]), (t, e, k)
                    compared += 1
            else:
                assert torch.equal(o[e], prev[e]), (t, e, "an inactive env's observation changed")
                kept += 1
        kc += m
        prev = o
    assert compared > N and kept > N
    assert torch.equal(warped.frames(), warped.ring[warped.heads.long(), torch.arange(N, device="cuda")])
    assert len(warped.render()) == N and warped.render_device().shape == (N, 128, 128, 3)
    assert warped.errors() == 0
    for env in (plain, warped):
        env.close()


def test_plain_steps_in_per_env_mode_equal_the_default_env(monkeypatch):
    """No mask: cbev_step_heads with the cached all-ones mask. Observation, reward
    and flags equal the default env's step, with action_repeat."""
    N = 24
    (plain, heads), _ = _pair(monkeypatch, N, action_repeat=2)
    for t in range(6):
        a = eval_actions(N, t)
        x, y = plain.step(a), heads.step(a)
        assert all(torch.equal(p, q) for p, q in zip(x[:4], y[:4])), t
    assert torch.equal(heads.heads, torch.full((N,), 6 % 4, dtype=torch.uint8, device="cuda"))
    for env in (plain, heads):
        env.close()


def test_freeze_done_with_per_env_heads(monkeypatch):
    """One episode per env, and a finished env's observation stays bit-identical
    from its terminal step until all_done()."""
    N, max_actions = 24, 40
    envs, _ = eval_pair(monkeypatch, N, max_actions, stack_heads="per_env")
    frozen, plain = envs
    assert frozen.freeze_done and frozen.stack_heads == "per_env" and plain.stack_heads == "per_env"
    got, first = {}, {}
    done = np.zeros(N, bool)
    kept, steps, prev = 0, 0, None
    while not frozen.all_done():
        assert steps < max_actions + 2, "the evaluation did not end"
        a = eval_actions(N, steps)
        o, r, term, _, infos = frozen.step(a)
        _, _, _, _, infos1 = plain.step(a)
        for e in np.flatnonzero(done):
            assert torch.equal(o[e], prev[e]), (steps, e, "a finished env's observation changed")
            kept += 1
        for src, dst in ((infos, got), (infos1, first)):
            if "_episode" in src:
                for e in np.flatnonzero(src["_episode"]):
                    assert dst is first or int(e) not in dst, (steps, e, "a second episode row")
                    dst.setdefault(int(e), (float(src["episode"]["r"][e]), int(src["episode"]["l"][e])))
        done = term.cpu().numpy()
        prev = o
        steps += 1
    assert sorted(got) == list(range(N)) and kept > N
    assert all(got[e] == first[e] for e in range(N))
    assert [got[e][1] for e in range(N)] == (2 + (5 * np.arange(N)) % 37).tolist()
    assert frozen.termination_count() == N and frozen.errors() == 0
    for env in envs:
        env.close()


def test_resets_in_per_env_mode_equal_the_default_env(monkeypatch):
    """reset_from_bank(mask) and reset(reset_mask=...) after masked steps that left
    the heads apart: a reset env's observation equals the same reset's in a
    default env, whatever its head was."""
    N = 24
    (plain, heads), opts = _pair(monkeypatch, N)
    rng = np.random.default_rng(8)
    for t in range(5):
        a = eval_actions(N, t)
        plain.step(a)
        heads.step(a, active=torch.from_numpy(rng.random(N) < 0.5).cuda())
    assert len(set(heads.heads.cpu().numpy().tolist())) > 1
    for env in (plain, heads):
        env.attach_bank(env.build_bank(list(range(900, 916)), opts))
    m = np.zeros(N, bool)
    m[::3] = True
    idx = torch.from_numpy(np.flatnonzero(m)).cuda()
    dm = torch.from_numpy(m).cuda()
    o0, o1 = plain.reset_from_bank(dm), heads.reset_from_bank(dm)
    assert torch.equal(o0[idx], o1[idx])
    m2 = np.roll(m, 1)
    idx2 = torch.from_numpy(np.flatnonzero(m2)).cuda()
    (o0, _), (o1, _) = (env.reset(seed=77, options=dict(opts, reset_mask=m2)) for env in (plain, heads))
    assert torch.equal(o0[idx2], o1[idx2])
    assert torch.equal(plain.frames()[idx2], heads.frames()[idx2])
    for env in (plain, heads):
        env.close()


# ---------------------------------------------------------------------- 6. graph capture
def test_step_and_expansion_under_graph_capture():
    """cbev_step_heads + cbev_expand_obs_heads captured once and replayed twice
    with the mask edited in place in between equal two eager pairs on a twin: the
    heads are advanced on the device, so a replay continues where the last stopped."""
    n, F, k = 19, 3, 2
    P, lanes = twins(n, bench_caps(2), 128, ("rt_no_traffic_v1",), 10_719, 14_719, F=F)
    L = lib()
    S = P.size
    C = len(semantic_mask_channels(MODE))
    lut = semantic_lut(MODE)
    acts = torch.ones(n, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(3)
    masks = [torch.from_numpy((rng.random(n) < 0.5).astype(np.uint8)).cuda() for _ in range(3)]
    assert not torch.equal(masks[1], masks[2])
    m_graph = masks[0].clone()
    state = [dict(heads=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                  obs=torch.zeros((n, F * C, S, S), dtype=torch.float32, device="cuda")) for _ in lanes]

    def step(c, st, m):
        dw, _, _, d_recs, ring, b = c
        s = P_(torch.cuda.current_stream().cuda_stream)
        check(step_heads(L, dw, d_recs, n, acts, m, k, ring, F, st["heads"], b, s), "step_heads")
        check(L.cbev_expand_obs_heads(dw.ctx, ptr(ring), n, F, ptr(st["heads"]), 0, C, lut.ctypes.data_as(P_),
                                      CODES["float32"], ptr(st["obs"]), s), "expand_heads")

    A, B = lanes
    step(A, state[0], masks[0])  # one eager pair each: the kernels are loaded before the capture
    step(B, state[1], m_graph)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            step(B, state[1], m_graph)
    torch.cuda.synchronize()
    assert torch.equal(A.recs, B.recs) and torch.equal(state[0]["heads"], state[1]["heads"])  # the capture ran nothing
    for rep in (1, 2):
        step(A, state[0], masks[rep])
        m_graph.copy_(masks[rep])
        g.replay()
        torch.cuda.synchronize()
        assert_same_outputs(A, B, rep)
        assert torch.equal(state[0]["heads"], state[1]["heads"]), (rep, "heads")
        assert torch.equal(state[0]["obs"], state[1]["obs"]), (rep, "observation")
    want = sum(m.long() for m in masks) % F
    assert torch.equal(state[1]["heads"].long(), want)
    assert int(A.out["term"].sum()) > 0


# ---------------------------------------------------------------------- 7. refusals
def test_refusals_leave_a_live_context_untouched():
    n, F = 19, 3
    P, lanes = twins(n, bench_caps(2), 128, ("rt_no_traffic_v1",), 10_819, 14_819, F=F)
    L = lib()
    dw, d_bank, bf, d_recs, _, b = lanes[0]
    S = P.size
    store = torch.zeros(F * n * S * S + 16, dtype=torch.uint8, device="cuda")
    ring = store[:F * n * S * S].view(F, n, S, S)
    check(L.cbev_reset(dw.ctx, ptr(d_recs), n, None, 0, None, None, 0, ptr(ring), F, None), "reset")
    acts = torch.full((n,), 100, dtype=torch.int32, device="cuda")  # would raise the action flag if anything ran
    ones = torch.ones(n, dtype=torch.uint8, device="cuda")
    good = torch.ones(n, dtype=torch.int32, device="cuda")
    heads = torch.zeros(n, dtype=torch.uint8, device="cuda")
    check(step_heads(L, dw, d_recs, n, good, ones, 2, ring, F, heads, b), "step_heads")
    torch.cuda.synchronize()
    st = b["stats"]
    before = [d_recs.clone(), store.clone(), heads.clone(), st.stats.clone(), st.rows.clone(), st.counts.clone()] + [
        b[key].clone() for key in KEYS]
    counts0, nterm0 = reset_counts(L, dw, n), termination_count(L, dw)

    def call(act=ones, ring_=ring, heads_=heads, k=2, n_=n, nf=F):
        return L.cbev_step_heads(dw.ctx, ptr(d_recs), n_, ptr(acts), ptr(act), k, ptr(ring_), nf, ptr(heads_),
                                 ptr(b["rew"]), ptr(b["term"]), ptr(b["trunc"]), ptr(b["cause"]), ptr(b["info"]), None)

    assert call(act=None) == CBEV_EINVAL and b"active" in L.cbev_last_error()
    assert call(ring_=None) == CBEV_EINVAL and b"ring" in L.cbev_last_error()
    assert call(heads_=None) == CBEV_EINVAL and b"heads" in L.cbev_last_error()
    for bad in (0, 65, -3):
        assert call(k=bad) == CBEV_EINVAL and b"repeat" in L.cbev_last_error()
    for bad in (0, 256, -1):
        assert call(nf=bad) == CBEV_EINVAL and b"n_frames" in L.cbev_last_error()
    assert call(ring_=store[8:]) == CBEV_EINVAL and b"aligned" in L.cbev_last_error()
    assert call(n_=n + 1) == CBEV_EINVAL and b"episode stats" in L.cbev_last_error()  # above the statistics' ep_n
    torch.cuda.synchronize()
    after = [d_recs, store, heads, st.stats, st.rows, st.counts] + [b[key] for key in KEYS]
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(reset_counts(L, dw, n), counts0) and termination_count(L, dw) == nterm0
    assert error_flags(dw.ctx) == 0
    check(step_heads(L, dw, d_recs, n, good, ones, 64, ring, F, heads, b), "step_heads")  # the largest repeat runs
    torch.cuda.synchronize()
    assert error_flags(dw.ctx) == 0 and torch.equal(heads, torch.full_like(heads, 2))
