"""The reset preview: when the tail of a step that folded a reset terminates an
env, it fetches the inputs of the bank row the env's next reset takes, and the
next step's k_ego_head computes that reset in the same pass as the kept envs.
Scheduling only: everything here is bitwise against the unsplit step on the
same inputs after every step, with cbev_reset_preview_counts proving which
path each reset env took (one pass from a preview / two passes from the row).
"""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import edge_cases as EC
from carlabev_env_amd import layout as LY
from carlabev_env_amd._lib import check, lib
from gpu_harness import (P_, assert_same, assert_same_outputs, error_flags, preview_counts, ptr, reset_counts,
                         reset_rows, reset_terminated_all, set_term, step_all, term_of)
from gpu_scenes import (CAPS_LONG2, F, N4, N_BANK, T4, UNSPLIT_AND_PREVIEW, long_records, preview_delta, prime,
                        primed_case, run_parity, split_lanes, wall_world)
from helpers import bench_caps

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------- 1. the canonical loop
@pytest.mark.parametrize("n,head_ne", [(19, 16), (3 * 64 + 3, 64)])
def test_canonical_loop_equals_unsplit(n, head_ne, monkeypatch):
    """40 steps of step + reset_terminated: equal to the unsplit step after every
    step; every reset after step 1's is computed from its preview (the envs that
    terminated in step 0 in two passes: step 0 folded nothing, so nothing was
    fetched), and some env is reset and terminates in consecutive steps."""
    monkeypatch.setenv("CBEV_HEAD_NE", str(head_ne))
    steps = 40
    P, padded, _ = EC.authored_world(128)
    recs, _ = long_records(n, CAPS_LONG2, 100, off_every=2)
    bank, _ = long_records(N_BANK, CAPS_LONG2, 500, off_every=3)
    lanes = split_lanes(P, padded, CAPS_LONG2, recs, bank, UNSPLIT_AND_PREVIEW)
    rng = np.random.default_rng(19)
    p = np.ones(P.n_discrete)
    p[1] += 4.0
    acts = rng.choice(P.n_discrete, size=(steps, n), p=p / p.sum()).astype(np.int32)
    was_reset = np.zeros(n, bool)
    reset_then_term, folded = 0, []
    for t in range(steps):
        step_all(lanes, acts[t], t)
        assert_same(lanes, t)
        tn = term_of(lanes[0])  # the unsplit run's
        reset_then_term += int(np.sum(was_reset & tn))
        was_reset = tn
        if t < steps - 1:
            folded.append(int(tn.sum()))
            reset_terminated_all(lanes)
    assert sum(folded[1:]) >= 10 and reset_then_term > 0
    hits, fallbacks = preview_counts(lanes[1])
    assert hits >= 1 and hits + fallbacks == sum(folded)
    assert (hits, fallbacks) == (sum(folded[1:]), folded[0])
    assert preview_counts(lanes[0]) == (0, 0)  # the unsplit step has no head


# ---------------------------------------------------------------------- 2. on against off, and the oracle
def test_preview_on_equals_preview_off():
    """The same split step with the preview on and off, bitwise after every step;
    off computes every reset in two passes."""
    n, steps = 19, 24
    P, padded, _ = EC.authored_world(128)
    recs, _ = long_records(n, CAPS_LONG2, 100, off_every=2)
    bank, _ = long_records(N_BANK, CAPS_LONG2, 500, off_every=3)
    lanes = split_lanes(P, padded, CAPS_LONG2, recs, bank, ((1, 0), (1, 1)))
    acts = np.random.default_rng(3).integers(0, P.n_discrete, size=(steps, n)).astype(np.int32)
    total = 0
    for t in range(steps):
        step_all(lanes, acts[t], t)
        assert_same(lanes, t)
        if t < steps - 1:
            total += int(term_of(lanes[0]).sum())
            reset_terminated_all(lanes)
    off, on = preview_counts(lanes[0]), preview_counts(lanes[1])
    assert off == (0, total) and on[0] >= 1 and sum(on) == total


def test_oracle_parity_with_the_preview():
    """The split step with the preview (the default) against the oracle, the bench's
    config-2 capacities, the statistics on."""
    run_parity(["rt_no_traffic_v1"], 19, 30, seed0=10_600, caps=bench_caps(2), stats=True)


# ---------------------------------------------------------------------- 3. compositions of a head group
def test_group_compositions_at_a_step_with_previews():
    """Three head groups of 16 and a partial one at a step whose previews exist: group
    0 every env from its preview, group 1 no reset, group 2 previews, two-pass
    resets (envs that never terminated, their bytes set by hand) and kept envs."""
    n, h = 3 * 16 + 3, 16
    fast = list(range(h)) + [2 * h, 2 * h + 3, 2 * h + 6]
    slow = [2 * h + 1, 2 * h + 4, 3 * h + 1]
    P, padded, recs, bank, layout = wall_world(n, fast)  # no termination yet: env e takes row e (n <= N_BANK)
    lanes = split_lanes(P, padded, CAPS_LONG2, recs, bank, UNSPLIT_AND_PREVIEW)
    acts = np.ones(n, np.int32)
    tc0 = reset_counts(lib(), lanes[1].dw, n)
    ids, rows = reset_rows(np.isin(np.arange(n), fast), tc0, N_BANK)
    assert sorted(rows.tolist()) == sorted(fast)
    (h0, f0), term1 = prime(lanes, n, fast, acts)
    assert not term1[slow].any()
    reset_terminated_all(lanes)
    mask = np.zeros(n, np.uint8)
    mask[fast] = 1
    mask[slow] = 1
    set_term(lanes, mask)
    step_all(lanes, acts, 2)
    assert_same(lanes, 2)
    assert mask[:h].all() and not mask[h:2 * h].any() and mask[2 * h:3 * h].sum() == 5
    h1, f1 = preview_counts(lanes[1])
    assert (h1 - h0, f1 - f0) == (len(fast), len(slow))
    # each reset env holds the row its count gives
    tc = reset_counts(lib(), lanes[1].dw, n)
    hr = lanes[1].recs.cpu().numpy()
    tnow = term_of(lanes[1])
    ids, rows = reset_rows(mask, tc - tnow, N_BANK)  # the counts the head saw: before this step's terminations
    for e, row in zip(ids, rows):
        assert LY.RecordView(hr[e], layout).i("SCENE_ID") == LY.RecordView(bank[row], layout).i("SCENE_ID"), e


# ---------------------------------------------------------------------- 4. invalidation
def test_cleared_byte_keeps_running_and_a_later_termination_rewrites_the_entry():
    P, bank, layout, lanes, acts, base, term1 = primed_case()
    reset_terminated_all(lanes)
    mask = term_of(lanes[1]).astype(np.uint8)
    mask[4] = 0
    set_term(lanes, mask)
    step_all(lanes, acts, 2)
    assert_same(lanes, 2)
    n1 = int(term1.sum())
    assert preview_delta(lanes, base) == (n1 - 1, 0)
    t2 = term_of(lanes[1])
    assert t2[4], "env 4 is still inside the wall: it terminates again"
    tc = reset_counts(lib(), lanes[1].dw, N4)
    assert tc[4] == 2
    reset_terminated_all(lanes)
    step_all(lanes, acts, 3)
    assert_same(lanes, 3)
    assert preview_delta(lanes, base) == (n1 - 1 + int(t2.sum()), 0)
    _, rows = reset_rows(np.arange(N4) == 4, tc, N_BANK)
    hr = lanes[1].recs.cpu().numpy()
    assert LY.RecordView(hr[4], layout).i("SCENE_ID") == LY.RecordView(bank[rows[0]], layout).i("SCENE_ID")


def test_byte_set_for_an_env_that_never_terminated_takes_two_passes():
    P, bank, layout, lanes, acts, base, term1 = primed_case()
    reset_terminated_all(lanes)
    mask = term_of(lanes[1]).astype(np.uint8)
    assert not term1[[0, 9]].any()
    mask[[0, 9]] = 1
    set_term(lanes, mask)
    step_all(lanes, acts, 2)
    assert_same(lanes, 2)
    assert preview_delta(lanes, base) == (int(term1.sum()), 2)


def test_bank_row_edited_and_rendered_again_takes_two_passes_with_the_new_bytes():
    P, bank, layout, lanes, acts, base, term1 = primed_case()
    tc = reset_counts(lib(), lanes[1].dw, N4)
    ids, rows = reset_rows(term_of(lanes[1]), tc, N_BANK)
    new_x = {}
    for c in lanes:
        hb = c.bank.cpu().numpy()
        for row in rows:
            v = LY.RecordView(hb[row], layout)
            v.hd[LY.HD["X"]] += 2.5
            v.hd[LY.HD["V"]] += 1.0
            new_x[int(row)] = v.h("X")
        c.bank.copy_(torch.from_numpy(hb))
        check(lib().cbev_bank_frames(c.dw.ctx, ptr(c.bank), N_BANK, ptr(c.bank_frames), None), "bank_frames")
    reset_terminated_all(lanes)
    step_all(lanes, acts, 2)
    assert_same(lanes, 2)
    assert preview_delta(lanes, base) == (0, int(term1.sum()))
    hr = lanes[1].recs.cpu().numpy()
    for e, row in zip(ids, rows):
        assert LY.RecordView(hr[e], layout).h("X1") == new_x[int(row)], e
    # the step after it folds from an unchanged bank again
    t2 = int(term_of(lanes[1]).sum())
    reset_terminated_all(lanes)
    step_all(lanes, acts, 3)
    assert_same(lanes, 3)
    assert preview_delta(lanes, base) == (t2, int(term1.sum()))


def test_another_bank_pointer_takes_two_passes():
    P, bank, layout, lanes, acts, base, term1 = primed_case()
    L = lib()
    clones = [c.bank.clone() for c in lanes]
    for c, d_bank in zip(lanes, clones):
        assert d_bank.data_ptr() != c.bank.data_ptr()
        check(L.cbev_reset_terminated(c.dw.ctx, ptr(c.recs), N4, ptr(d_bank), N_BANK, ptr(c.bank_frames), ptr(c.ring), F,
                                      None),
              "reset_terminated")
    step_all(lanes, acts, 2)
    assert_same(lanes, 2)
    assert preview_delta(lanes, base) == (0, int(term1.sum()))


def test_step_repeat_in_between_takes_two_passes():
    P, bank, layout, lanes, acts, base, term1 = primed_case()
    L = lib()
    a = torch.from_numpy(acts).cuda()
    for dw, d_bank, bf, d_recs, ring, b in lanes:
        check(L.cbev_step_repeat(dw.ctx, ptr(d_recs), N4, ptr(a), 2, ptr(ring[2]), ptr(b["rew"]), ptr(b["term"]),
                                 ptr(b["trunc"]), ptr(b["cause"]), ptr(b["info"]), None), "step_repeat")
    torch.cuda.synchronize()
    assert_same(lanes, 2)
    mask = term_of(lanes[1]).astype(np.uint8)
    mask[list(T4)] = 1
    set_term(lanes, mask)
    reset_terminated_all(lanes)
    step_all(lanes, acts, 3)
    assert_same(lanes, 3)
    assert preview_delta(lanes, base) == (0, int(mask.sum()))


def test_terminated_twice_before_its_reset_takes_the_row_of_the_count_as_it_stands():
    P, bank, layout, lanes, acts, base, term1 = primed_case()
    step_all(lanes, acts, 2)  # no reset: the envs are still inside the wall and terminate again
    assert_same(lanes, 2)
    t2 = term_of(lanes[1])
    assert t2[list(T4)].all()
    tc = reset_counts(lib(), lanes[1].dw, N4)
    assert (tc[list(T4)] == 2).all()
    reset_terminated_all(lanes)
    step_all(lanes, acts, 3)
    assert_same(lanes, 3)
    assert preview_delta(lanes, base) == (0, int(t2.sum()))  # step 2 folded nothing: no previews
    ids, rows = reset_rows(t2, tc, N_BANK)
    hr = lanes[1].recs.cpu().numpy()
    for e, row in zip(ids, rows):
        assert LY.RecordView(hr[e], layout).i("SCENE_ID") == LY.RecordView(bank[row], layout).i("SCENE_ID"), e


def test_reset_masked_at_once_then_an_edited_mask_takes_two_passes():
    P, bank, layout, lanes, acts, base, term1 = primed_case()
    L = lib()
    for dw, d_bank, bf, d_recs, ring, b in lanes:
        check(L.cbev_reset_masked(dw.ctx, ptr(d_recs), N4, ptr(b["term"]), ptr(d_bank), N_BANK, ptr(bf), ptr(ring), F,
                                  None), "reset_masked")
    torch.cuda.synchronize()
    step_all(lanes, acts, 2)
    assert_same(lanes, 2)
    assert preview_delta(lanes, base) == (0, 0)
    mask = np.zeros(N4, np.uint8)
    mask[4] = 1  # reset again with no new termination: the same row
    reset_terminated_all(lanes)
    set_term(lanes, mask)
    step_all(lanes, acts, 3)
    assert_same(lanes, 3)
    assert preview_delta(lanes, base) == (0, 1)


# ---------------------------------------------------------------------- 5. graph capture
def test_captured_step_with_resets_pending_replayed_twice():
    """A step captured while a reset is pending and previews exist, replayed twice:
    equal to the eager unsplit run; the first replay takes the previews, the second
    computes its resets in two passes (the tags are the capture's). Nothing is
    allocated under the capture: torch captures in the global error mode, in which a
    hipMalloc, hipFree or synchronising call of the capturing thread fails and
    invalidates the capture, so check() would raise inside the `with` block and
    the graph would not instantiate."""
    P, bank, layout, lanes, acts, base, term1 = primed_case(extra_off=[(e + lib().cbev_bank_stride(N_BANK)) % N_BANK for e in T4])
    L = lib()
    A, B = lanes
    a = torch.from_numpy(acts).cuda()

    def step(c, stream):
        dw, d_bank, bf, d_recs, ring, b = c
        check(L.cbev_step(dw.ctx, ptr(d_recs), N4, ptr(a), ptr(ring[2]), ptr(b["rew"]), ptr(b["term"]),
                          ptr(b["trunc"]), ptr(b["cause"]), ptr(b["info"]), stream), "step")

    reset_terminated_all([B])  # recorded before the capture
    assert L.cbev_reset_pending(B.dw.ctx) == 1
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    before = B.recs.clone()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            step(B, P_(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(before, B.recs)  # the capture ran nothing
    for rep in range(2):
        reset_terminated_all([A])
        step(A, None)
        g.replay()
        torch.cuda.synchronize()
        # a replay writes its episode rows into the ring slot of the capture, so past the
        # first replay the rows are not where the eager run's are: the rest is compared
        if rep == 0:
            assert_same(lanes, 2)
        assert_same_outputs(A, B, rep)
        assert np.array_equal(reset_counts(L, A.dw, N4), reset_counts(L, B.dw, N4)), (rep, "reset counts")
        if rep == 0:
            assert preview_delta(lanes, base) == (int(term1.sum()), 0)
            t2 = int(term_of(A).sum())
            assert t2 >= len(T4), "the second rows start inside a wall too: the second replay has resets"
        else:
            assert preview_delta(lanes, base) == (int(term1.sum()), t2)


def test_bank_edited_between_capture_and_replay_takes_two_passes_with_the_new_bytes():
    """The host cannot tell a captured step that the bank changed after the capture:
    cbev_bank_frames clears the previews' tags on the device, so the replay computes
    its resets in two passes from the new bytes, as the eager unsplit run does."""
    P, bank, layout, lanes, acts, base, term1 = primed_case()
    L = lib()
    A, B = lanes
    a = torch.from_numpy(acts).cuda()

    def step(c, stream):
        dw, d_bank, bf, d_recs, ring, b = c
        check(L.cbev_step(dw.ctx, ptr(d_recs), N4, ptr(a), ptr(ring[2]), ptr(b["rew"]), ptr(b["term"]),
                          ptr(b["trunc"]), ptr(b["cause"]), ptr(b["info"]), stream), "step")

    tc = reset_counts(L, B.dw, N4)
    ids, rows = reset_rows(term1, tc, N_BANK)
    reset_terminated_all([B])
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            step(B, P_(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    new_x = {}
    for c in lanes:
        hb = c.bank.cpu().numpy()
        for row in rows:
            v = LY.RecordView(hb[row], layout)
            v.hd[LY.HD["X"]] += 2.5
            v.hd[LY.HD["V"]] += 1.0
            new_x[int(row)] = v.h("X")
        c.bank.copy_(torch.from_numpy(hb))
        check(L.cbev_bank_frames(c.dw.ctx, ptr(c.bank), N_BANK, ptr(c.bank_frames), None), "bank_frames")
    torch.cuda.synchronize()
    reset_terminated_all([A])
    step(A, None)
    g.replay()
    torch.cuda.synchronize()
    assert_same(lanes, 2)
    assert preview_delta(lanes, base) == (0, int(term1.sum()))
    hr = B.recs.cpu().numpy()
    for e, row in zip(ids, rows):
        assert LY.RecordView(hr[e], layout).h("X1") == new_x[int(row)], e


# ---------------------------------------------------------------------- 6. action index out of range
def test_action_index_out_of_range_in_a_preview_reset_and_a_kept_env():
    P, bank, layout, lanes, acts, base, term1 = primed_case()
    assert error_flags(lanes[0].dw.ctx) == 0 and error_flags(lanes[1].dw.ctx) == 0
    reset_terminated_all(lanes)
    bad = acts.copy()
    bad[4] = P.n_discrete + 5    # an env reset from its preview
    bad[7] = -P.n_discrete - 1   # a kept env
    step_all(lanes, bad, 2)
    assert_same(lanes, 2)
    assert not term1[7] and preview_delta(lanes, base) == (int(term1.sum()), 0)
    fa, fb = error_flags(lanes[0].dw.ctx), error_flags(lanes[1].dw.ctx)
    assert fa == fb and fa != 0
