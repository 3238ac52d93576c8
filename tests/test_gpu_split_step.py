"""The split step (cbev_set_split_step): the ego update's front as k_ego_head, its
collision / reward / termination tail as the leading workgroups of k_raster's
launch, against the unsplit k_ego (bitwise) and against the oracle, at the
shapes where the split can go wrong: one env, a partial tail group with surplus
tail workgroups (the multiple-of-8 padding), a batch across the n & ~511
XCD-mapping boundary, actor capacities (8-env groups, actor scratch) and size
256 (4 tiles per env); the size-64 fallback; a captured step.
"""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import edge_cases as EC
from carlabev_env_amd import layout as LY
from carlabev_env_amd._lib import check, lib
from gpu_harness import (P_, DevWorld, assert_same, assert_same_outputs, flush_all, make_lanes, ptr, reset_counts,
                         reset_terminated_all, step_all, term_of)
from gpu_scenes import run_parity, split_pair
from helpers import bench_caps, build_records, world

pytestmark = pytest.mark.gpu

CBEV_EINVAL = -1

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
    P, lanes = split_pair(n, bench_caps(config), size, kinds, 10_300 + n, 14_300 + n, n_bank=n_bank, F=F)
    L = lib()
    rng = np.random.default_rng(n)
    p = np.ones(P.n_discrete)
    p[1] += 4.0
    acts = rng.choice(P.n_discrete, size=(steps, n), p=p / p.sum()).astype(np.int32)
    A, B = lanes
    was_reset = np.zeros(n, bool)
    reset_then_term = 0
    for t in range(steps):
        step_all(lanes, acts[t], t)
        assert_same(lanes, t)
        tn = term_of(B)
        reset_then_term += int(np.sum(was_reset & tn))
        was_reset = tn
        reset_terminated_all(lanes)
    flush_all(lanes)
    assert torch.equal(A.recs, B.recs) and torch.equal(A.ring, B.ring)
    assert np.array_equal(reset_counts(L, A.dw, n), reset_counts(L, B.dw, n))
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
    lanes = make_lanes(P, padded, caps, recs, None, F, [dict(split=1)] * 2)
    acts = torch.ones(n, dtype=torch.int32, device="cuda")

    def step(dw, d_recs, ring, b):
        check(L.cbev_step(dw.ctx, ptr(d_recs), n, ptr(acts), ptr(ring[0]), ptr(b["rew"]), ptr(b["term"]),
                          ptr(b["trunc"]), ptr(b["cause"]), ptr(b["info"]),
                          P_(torch.cuda.current_stream().cuda_stream)), "step")

    (dA, _, _, rA, gA, bA), (dB, _, _, rB, gB, bB) = lanes
    step(dA, rA, gA, bA)  # one eager step each: the kernels are loaded before the capture
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
    assert int(bA["term"].sum()) > 0  # the envs pushed off the road terminate in every step
    assert L.cbev_reset_pending(dB.ctx) == 0
