"""The split step (cbev_set_split_step): the ego update's front as k_ego_head, its
collision / reward / termination tail as the leading workgroups of k_raster's
launch, against the unsplit k_ego (bitwise) and against the oracle, at the
shapes where the split can go wrong: one env, a partial tail group with surplus
tail workgroups (the multiple-of-8 padding), a batch across the n & ~511
XCD-mapping boundary, actor capacities (8-env groups, actor scratch) and size
256 (4 tiles per env); the size-64 fallback; a captured step.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import edge_cases as EC
from carlabev_env_amd import layout as LY
from carlabev_env_amd._lib import check, lib
from helpers import bench_caps, build_records, world
from test_gpu_parity import DevWorld, EpisodeStatsOn, P_, _counts, _same_stats, ptr, run_parity

pytestmark = pytest.mark.gpu

CBEV_EINVAL = -1


def _bufs(n):
    return dict(rew=torch.zeros(n, dtype=torch.float64, device="cuda"),
                term=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                trunc=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                cause=torch.zeros(n, dtype=torch.int32, device="cuda"),
                info=torch.zeros((n, 16), dtype=torch.float32, device="cuda"))


def _split_pair(n, caps, size, kinds, seed0, bank_seed0, n_bank=53, F=3, distinct=48, bank_distinct=17):
    """Two contexts on the same records and bank, the unsplit step (0) and the
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
    L = lib()
    S = P.size
    out = []
    for split in (0, 1):
        dw = DevWorld(P, padded, caps)
        check(L.cbev_set_split_step(dw.ctx, split), "split_step")
        check(L.cbev_set_deferred_reset(dw.ctx, 1), "deferred")
        d_bank = torch.from_numpy(bank.copy()).cuda()
        bf = torch.zeros((n_bank, S, S), dtype=torch.uint8, device="cuda")
        check(L.cbev_bank_frames(dw.ctx, ptr(d_bank), n_bank, ptr(bf), None), "bank_frames")
        d_recs = torch.from_numpy(recs.copy()).cuda()
        ring = torch.zeros((F, n, S, S), dtype=torch.uint8, device="cuda")
        check(L.cbev_reset(dw.ctx, ptr(d_recs), n, None, 0, None, None, 0, ptr(ring), F, None), "reset")
        b = _bufs(n)
        b["stats"] = EpisodeStatsOn(dw.ctx, n)
        out.append((dw, d_bank, bf, d_recs, ring, b))
    return P, out


CASES = [
    pytest.param(1, 2, 128, ("rt_no_traffic_v1",), id="n1"),
    pytest.param(19, 2, 128, ("rt_no_traffic_v1",), id="n19"),
    pytest.param(531, 2, 128, ("rt_no_traffic_v1",), id="n531"),
    pytest.param(19, 3, 128, ("rt_hard_v1", "rt_medium_v1"), id="n19-actors"),
    pytest.param(19, 5, 256, ("mix3",), id="n19-size256"),
]


@pytest.mark.parametrize("n,config,size,kinds", CASES)
def test_split_equals_unsplit_bitwise(n, config, size, kinds):
    """40 steps of step + reset_terminated (folded into the next step where the
    context can fold) in both contexts: records, the 3-slot ring, reward, term,
    trunc, cause, info, the episode statistics (rows and counts) and the per-env
    reset counts are equal after every step, and some env of the split context
    was reset and terminated in consecutive steps."""
    n_bank, F, steps = 53, 3, 40
    P, ctxs = _split_pair(n, bench_caps(config), size, kinds, 10_300 + n, 14_300 + n, n_bank=n_bank, F=F)
    L = lib()
    rng = np.random.default_rng(n)
    p = np.ones(P.n_discrete)
    p[1] += 4.0
    acts = rng.choice(P.n_discrete, size=(steps, n), p=p / p.sum()).astype(np.int32)
    (dA, _, _, rA, gA, bA), (dB, _, _, rB, gB, bB) = ctxs
    was_reset = np.zeros(n, bool)
    reset_then_term = 0
    for t in range(steps):
        a = torch.from_numpy(np.ascontiguousarray(acts[t])).cuda()
        for dw, d_bank, bf, d_recs, ring, b in ctxs:
            check(L.cbev_step(dw.ctx, ptr(d_recs), n, ptr(a), ptr(ring[t % F]), ptr(b["rew"]), ptr(b["term"]),
                              ptr(b["trunc"]), ptr(b["cause"]), ptr(b["info"]), None), "step")
        torch.cuda.synchronize()
        for k in ("rew", "term", "trunc", "cause", "info"):
            assert torch.equal(bA[k], bB[k]), (t, k)
        assert torch.equal(rA, rB), (t, "records")
        assert torch.equal(gA, gB), (t, "ring")
        assert _same_stats(bA["stats"], bB["stats"], t, n), (t, "episode stats")
        assert np.array_equal(_counts(L, dA, n), _counts(L, dB, n)), (t, "reset counts")
        tn = bB["term"].cpu().numpy().astype(bool)
        reset_then_term += int(np.sum(was_reset & tn))
        was_reset = tn
        for dw, d_bank, bf, d_recs, ring, b in ctxs:
            check(L.cbev_reset_terminated(dw.ctx, ptr(d_recs), n, ptr(d_bank), n_bank, ptr(bf), ptr(ring), F, None),
                  "reset_terminated")
    for dw, *_ in ctxs:
        check(L.cbev_flush(dw.ctx), "flush")
    torch.cuda.synchronize()
    assert torch.equal(rA, rB) and torch.equal(gA, gB)
    assert np.array_equal(_counts(L, dA, n), _counts(L, dB, n))
    assert reset_then_term > 0


def _split_supported(size, caps):
    cfg, P, padded, layout, builder = world(size, caps=caps)
    dw = DevWorld(P, padded, caps)
    return lib().cbev_set_split_step(dw.ctx, 1) == 0


def test_oracle_parity_on_the_split_path():
    """The split step (the default at these shapes) against the oracle, whole
    records, frames and outputs every step: a partial tail group, ego-only and
    with actors, the statistics on."""
    assert _split_supported(128, bench_caps(2)) and _split_supported(128, bench_caps(3))
    run_parity(["rt_no_traffic_v1"], 19, 30, seed0=10_400, caps=bench_caps(2), stats=True)
    run_parity(["rt_hard_v1"], 19, 30, seed0=20_400, act_seed=7, caps=bench_caps(3), stats=True)


def test_size_64_keeps_the_unsplit_step():
    """Size 64 reports the split unsupported (k_raster<1> runs 8 waves per SIMD:
    the tail does not fit its registers) and still steps with parity."""
    P, padded, caps, recs, layout, acts = EC.raster_batch(64, 0.5, step_deg=15.0)
    dw = DevWorld(P, padded, caps)
    L = lib()
    assert L.cbev_set_split_step(dw.ctx, 1) == CBEV_EINVAL
    assert len(L.cbev_last_error()) > 0
    assert L.cbev_set_split_step(dw.ctx, 0) == 0
    del dw
    run_parity(None, len(recs), len(acts), caps=caps, recs=recs, world_=(P, padded), acts=acts)


def test_split_step_under_graph_capture():
    """A split step captured into a graph (two kernel nodes, nothing allocated)
    and replayed twice equals the eager split step; no reset is pending after."""
    n, F = 19, 2
    caps = bench_caps(2)
    cfg, P, padded, layout, builder = world(128, caps=caps)
    recs, _ = build_records(builder, n, ["rt_no_traffic_v1"], seed0=10_500)
    for e in range(0, n, 4):
        LY.RecordView(recs[e], layout).hd[LY.HD["X"]] += 60.0
    L = lib()
    S = P.size
    ctxs = []
    for _ in range(2):
        dw = DevWorld(P, padded, caps)
        check(L.cbev_set_split_step(dw.ctx, 1), "split_step")
        d_recs = torch.from_numpy(recs.copy()).cuda()
        ring = torch.zeros((F, n, S, S), dtype=torch.uint8, device="cuda")
        check(L.cbev_reset(dw.ctx, ptr(d_recs), n, None, 0, None, None, 0, ptr(ring), F, None), "reset")
        b = _bufs(n)
        b["stats"] = EpisodeStatsOn(dw.ctx, n)
        ctxs.append((dw, d_recs, ring, b))
    acts = torch.ones(n, dtype=torch.int32, device="cuda")

    def step(dw, d_recs, ring, b):
        check(L.cbev_step(dw.ctx, ptr(d_recs), n, ptr(acts), ptr(ring[0]), ptr(b["rew"]), ptr(b["term"]),
                          ptr(b["trunc"]), ptr(b["cause"]), ptr(b["info"]),
                          P_(torch.cuda.current_stream().cuda_stream)), "step")

    for c in ctxs:  # one eager step each: the kernels are loaded before the capture
        step(*c)
    torch.cuda.synchronize()
    (dA, rA, gA, bA), (dB, rB, gB, bB) = ctxs
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
        for k in ("rew", "term", "trunc", "cause", "info"):
            assert torch.equal(bA[k], bB[k]), (rep, k)
        assert torch.equal(rA, rB), (rep, "records")
        assert torch.equal(gA, gB), (rep, "ring")
    assert int(bA["term"].sum()) > 0  # the envs pushed off the road terminate in every step
    assert L.cbev_reset_pending(dB.ctx) == 0
