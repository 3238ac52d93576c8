"""The reset preview: when the tail of a step that folded a reset terminates an
env, it fetches the inputs of the bank row the env's next reset takes, and the
next step's k_ego_head computes that reset in the same pass as the kept envs.
Scheduling only: everything here is bitwise against the unsplit step on the
same inputs after every step, with cbev_reset_preview_counts proving which
path each reset env took (one pass from a preview / two passes from the row).
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import edge_cases as EC
from carlabev_env_amd import layout as LY
from carlabev_env_amd._lib import check, lib
from helpers import bench_caps
from test_gpu_parity import DevWorld, EpisodeStatsOn, P_, _counts, error_flags, ptr, reset_rows, run_parity
from test_gpu_split_step import _bufs
from test_gpu_thin_head import CAPS_LONG2, _assert_same, _long_records, _reset_terminated, _step

pytestmark = pytest.mark.gpu

N_BANK, F = 53, 3  # the small bank and the 3-slot ring of test_gpu_thin_head


def _make(P, padded, caps, recs, bank, modes):
    """One context per (split, preview) of `modes` on the same records and bank: the
    reset deferred into the next step, a 3-slot ring, the statistics on (the tuples
    test_gpu_thin_head's _step / _reset_terminated / _assert_same take)."""
    L = lib()
    S, n = P.size, len(recs)
    out = []
    for split, preview in modes:
        dw = DevWorld(P, padded, caps)
        check(L.cbev_set_split_step(dw.ctx, split), "split_step")
        check(L.cbev_set_reset_preview(dw.ctx, preview), "reset_preview")
        check(L.cbev_set_deferred_reset(dw.ctx, 1), "deferred")
        d_bank = torch.from_numpy(bank.copy()).cuda()
        bf = torch.zeros((len(bank), S, S), dtype=torch.uint8, device="cuda")
        check(L.cbev_bank_frames(dw.ctx, ptr(d_bank), len(bank), ptr(bf), None), "bank_frames")
        d_recs = torch.from_numpy(recs.copy()).cuda()
        ring = torch.zeros((F, n, S, S), dtype=torch.uint8, device="cuda")
        check(L.cbev_reset(dw.ctx, ptr(d_recs), n, None, 0, None, None, 0, ptr(ring), F, None), "reset")
        b = _bufs(n)
        b["stats"] = EpisodeStatsOn(dw.ctx, n)
        out.append((dw, d_bank, bf, d_recs, ring, b))
    return out


UNSPLIT_AND_PREVIEW = ((0, 1), (1, 1))


def _pv(c):
    """(one-pass resets, two-pass resets) of a context since its creation."""
    out = (ctypes.c_uint64 * 2)()
    check(lib().cbev_reset_preview_counts(c[0].ctx, out), "reset_preview_counts")
    return int(out[0]), int(out[1])


def _term(c):
    return c[5]["term"].cpu().numpy().astype(bool)


def _set_term(ctxs, mask):
    m = torch.from_numpy(np.asarray(mask, np.uint8)).cuda()
    for c in ctxs:
        c[5]["term"].copy_(m)
    torch.cuda.synchronize()


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
    """test_gpu_thin_head's _long_records without actors, every record on one of the
    first points of its route (33 to 128 points, 3 px apart) at 30 px/s."""
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


def _world(n, wall_rows, n_bank=N_BANK):
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


def _prime(ctxs, n, envs, acts):
    """Steps 0 and 1 with the envs `envs` reset by hand in between (two passes: step
    0 folded nothing), to bank rows that start inside a wall: they terminate in
    step 1, whose tail writes their previews. Returns the counts after step 1 and
    step 1's terminations (the envs whose previews exist)."""
    _step(ctxs, acts, 0)
    _assert_same(ctxs, 0)
    mask = np.zeros(n, np.uint8)
    mask[list(envs)] = 1
    _set_term(ctxs, mask)
    _reset_terminated(ctxs)
    _step(ctxs, acts, 1)
    _assert_same(ctxs, 1)
    term1 = _term(ctxs[1])
    assert not _counts(lib(), ctxs[1][0], n)[~term1].any(), "nothing terminated but the envs reset into a wall"
    assert term1[list(envs)].all(), "the envs reset into a wall terminate in step 1"
    assert _pv(ctxs[1]) == (0, len(envs))
    return _pv(ctxs[1]), term1


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
    recs, _ = _long_records(n, CAPS_LONG2, 100, off_every=2)
    bank, _ = _long_records(N_BANK, CAPS_LONG2, 500, off_every=3)
    ctxs = _make(P, padded, CAPS_LONG2, recs, bank, UNSPLIT_AND_PREVIEW)
    rng = np.random.default_rng(19)
    p = np.ones(P.n_discrete)
    p[1] += 4.0
    acts = rng.choice(P.n_discrete, size=(steps, n), p=p / p.sum()).astype(np.int32)
    was_reset = np.zeros(n, bool)
    reset_then_term, folded = 0, []
    for t in range(steps):
        _step(ctxs, acts[t], t)
        _assert_same(ctxs, t)
        tn = _term(ctxs[0])  # the unsplit run's
        reset_then_term += int(np.sum(was_reset & tn))
        was_reset = tn
        if t < steps - 1:
            folded.append(int(tn.sum()))
            _reset_terminated(ctxs)
    assert sum(folded[1:]) >= 10 and reset_then_term > 0
    hits, fallbacks = _pv(ctxs[1])
    assert hits >= 1 and hits + fallbacks == sum(folded)
    assert (hits, fallbacks) == (sum(folded[1:]), folded[0])
    assert _pv(ctxs[0]) == (0, 0)  # the unsplit step has no head


# ---------------------------------------------------------------------- 2. on against off, and the oracle
def test_preview_on_equals_preview_off():
    """The same split step with the preview on and off, bitwise after every step;
    off computes every reset in two passes."""
    n, steps = 19, 24
    P, padded, _ = EC.authored_world(128)
    recs, _ = _long_records(n, CAPS_LONG2, 100, off_every=2)
    bank, _ = _long_records(N_BANK, CAPS_LONG2, 500, off_every=3)
    ctxs = _make(P, padded, CAPS_LONG2, recs, bank, ((1, 0), (1, 1)))
    acts = np.random.default_rng(3).integers(0, P.n_discrete, size=(steps, n)).astype(np.int32)
    total = 0
    for t in range(steps):
        _step(ctxs, acts[t], t)
        _assert_same(ctxs, t)
        if t < steps - 1:
            total += int(_term(ctxs[0]).sum())
            _reset_terminated(ctxs)
    off, on = _pv(ctxs[0]), _pv(ctxs[1])
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
    P, padded, recs, bank, layout = _world(n, fast)  # no termination yet: env e takes row e (n <= N_BANK)
    ctxs = _make(P, padded, CAPS_LONG2, recs, bank, UNSPLIT_AND_PREVIEW)
    acts = np.ones(n, np.int32)
    tc0 = _counts(lib(), ctxs[1][0], n)
    ids, rows = reset_rows(np.isin(np.arange(n), fast), tc0, N_BANK)
    assert sorted(rows.tolist()) == sorted(fast)
    (h0, f0), term1 = _prime(ctxs, n, fast, acts)
    assert not term1[slow].any()
    _reset_terminated(ctxs)
    mask = np.zeros(n, np.uint8)
    mask[fast] = 1
    mask[slow] = 1
    _set_term(ctxs, mask)
    _step(ctxs, acts, 2)
    _assert_same(ctxs, 2)
    assert mask[:h].all() and not mask[h:2 * h].any() and mask[2 * h:3 * h].sum() == 5
    h1, f1 = _pv(ctxs[1])
    assert (h1 - h0, f1 - f0) == (len(fast), len(slow))
    # each reset env holds the row its count gives
    tc = _counts(lib(), ctxs[1][0], n)
    hr = ctxs[1][3].cpu().numpy()
    tnow = _term(ctxs[1])
    ids, rows = reset_rows(mask, tc - tnow, N_BANK)  # the counts the head saw: before this step's terminations
    for e, row in zip(ids, rows):
        assert LY.RecordView(hr[e], layout).i("SCENE_ID") == LY.RecordView(bank[row], layout).i("SCENE_ID"), e


# ---------------------------------------------------------------------- 4. invalidation
N4, T4 = 19, (1, 4, 17)


def _case(extra_off=()):
    P, padded, recs, bank, layout = _world(N4, tuple(T4) + tuple(extra_off))
    ctxs = _make(P, padded, CAPS_LONG2, recs, bank, UNSPLIT_AND_PREVIEW)
    acts = np.ones(N4, np.int32)
    base, term1 = _prime(ctxs, N4, T4, acts)
    return P, bank, layout, ctxs, acts, base, term1


def _delta(ctxs, base):
    hcount, fcount = _pv(ctxs[1])
    return hcount - base[0], fcount - base[1]


def test_cleared_byte_keeps_running_and_a_later_termination_rewrites_the_entry():
    P, bank, layout, ctxs, acts, base, term1 = _case()
    _reset_terminated(ctxs)
    mask = _term(ctxs[1]).astype(np.uint8)
    mask[4] = 0
    _set_term(ctxs, mask)
    _step(ctxs, acts, 2)
    _assert_same(ctxs, 2)
    n1 = int(term1.sum())
    assert _delta(ctxs, base) == (n1 - 1, 0)
    t2 = _term(ctxs[1])
    assert t2[4], "env 4 is still inside the wall: it terminates again"
    tc = _counts(lib(), ctxs[1][0], N4)
    assert tc[4] == 2
    _reset_terminated(ctxs)
    _step(ctxs, acts, 3)
    _assert_same(ctxs, 3)
    assert _delta(ctxs, base) == (n1 - 1 + int(t2.sum()), 0)
    _, rows = reset_rows(np.arange(N4) == 4, tc, N_BANK)
    hr = ctxs[1][3].cpu().numpy()
    assert LY.RecordView(hr[4], layout).i("SCENE_ID") == LY.RecordView(bank[rows[0]], layout).i("SCENE_ID")


def test_byte_set_for_an_env_that_never_terminated_takes_two_passes():
    P, bank, layout, ctxs, acts, base, term1 = _case()
    _reset_terminated(ctxs)
    mask = _term(ctxs[1]).astype(np.uint8)
    assert not term1[[0, 9]].any()
    mask[[0, 9]] = 1
    _set_term(ctxs, mask)
    _step(ctxs, acts, 2)
    _assert_same(ctxs, 2)
    assert _delta(ctxs, base) == (int(term1.sum()), 2)


def test_bank_row_edited_and_rendered_again_takes_two_passes_with_the_new_bytes():
    P, bank, layout, ctxs, acts, base, term1 = _case()
    tc = _counts(lib(), ctxs[1][0], N4)
    ids, rows = reset_rows(_term(ctxs[1]), tc, N_BANK)
    new_x = {}
    for c in ctxs:
        hb = c[1].cpu().numpy()
        for row in rows:
            v = LY.RecordView(hb[row], layout)
            v.hd[LY.HD["X"]] += 2.5
            v.hd[LY.HD["V"]] += 1.0
            new_x[int(row)] = v.h("X")
        c[1].copy_(torch.from_numpy(hb))
        check(lib().cbev_bank_frames(c[0].ctx, ptr(c[1]), N_BANK, ptr(c[2]), None), "bank_frames")
    _reset_terminated(ctxs)
    _step(ctxs, acts, 2)
    _assert_same(ctxs, 2)
    assert _delta(ctxs, base) == (0, int(term1.sum()))
    hr = ctxs[1][3].cpu().numpy()
    for e, row in zip(ids, rows):
        assert LY.RecordView(hr[e], layout).h("X1") == new_x[int(row)], e
    # the step after it folds from an unchanged bank again
    t2 = int(_term(ctxs[1]).sum())
    _reset_terminated(ctxs)
    _step(ctxs, acts, 3)
    _assert_same(ctxs, 3)
    assert _delta(ctxs, base) == (t2, int(term1.sum()))


def test_another_bank_pointer_takes_two_passes():
    P, bank, layout, ctxs, acts, base, term1 = _case()
    L = lib()
    clones = [c[1].clone() for c in ctxs]
    for c, d_bank in zip(ctxs, clones):
        assert d_bank.data_ptr() != c[1].data_ptr()
        check(L.cbev_reset_terminated(c[0].ctx, ptr(c[3]), N4, ptr(d_bank), N_BANK, ptr(c[2]), ptr(c[4]), F, None),
              "reset_terminated")
    _step(ctxs, acts, 2)
    _assert_same(ctxs, 2)
    assert _delta(ctxs, base) == (0, int(term1.sum()))


def test_step_repeat_in_between_takes_two_passes():
    P, bank, layout, ctxs, acts, base, term1 = _case()
    L = lib()
    a = torch.from_numpy(acts).cuda()
    for dw, d_bank, bf, d_recs, ring, b in ctxs:
        check(L.cbev_step_repeat(dw.ctx, ptr(d_recs), N4, ptr(a), 2, ptr(ring[2]), ptr(b["rew"]), ptr(b["term"]),
                                 ptr(b["trunc"]), ptr(b["cause"]), ptr(b["info"]), None), "step_repeat")
    torch.cuda.synchronize()
    _assert_same(ctxs, 2)
    mask = _term(ctxs[1]).astype(np.uint8)
    mask[list(T4)] = 1
    _set_term(ctxs, mask)
    _reset_terminated(ctxs)
    _step(ctxs, acts, 3)
    _assert_same(ctxs, 3)
    assert _delta(ctxs, base) == (0, int(mask.sum()))


def test_terminated_twice_before_its_reset_takes_the_row_of_the_count_as_it_stands():
    P, bank, layout, ctxs, acts, base, term1 = _case()
    _step(ctxs, acts, 2)  # no reset: the envs are still inside the wall and terminate again
    _assert_same(ctxs, 2)
    t2 = _term(ctxs[1])
    assert t2[list(T4)].all()
    tc = _counts(lib(), ctxs[1][0], N4)
    assert (tc[list(T4)] == 2).all()
    _reset_terminated(ctxs)
    _step(ctxs, acts, 3)
    _assert_same(ctxs, 3)
    assert _delta(ctxs, base) == (0, int(t2.sum()))  # step 2 folded nothing: no previews
    ids, rows = reset_rows(t2, tc, N_BANK)
    hr = ctxs[1][3].cpu().numpy()
    for e, row in zip(ids, rows):
        assert LY.RecordView(hr[e], layout).i("SCENE_ID") == LY.RecordView(bank[row], layout).i("SCENE_ID"), e


def test_reset_masked_at_once_then_an_edited_mask_takes_two_passes():
    P, bank, layout, ctxs, acts, base, term1 = _case()
    L = lib()
    for dw, d_bank, bf, d_recs, ring, b in ctxs:
        check(L.cbev_reset_masked(dw.ctx, ptr(d_recs), N4, ptr(b["term"]), ptr(d_bank), N_BANK, ptr(bf), ptr(ring), F,
                                  None), "reset_masked")
    torch.cuda.synchronize()
    _step(ctxs, acts, 2)
    _assert_same(ctxs, 2)
    assert _delta(ctxs, base) == (0, 0)
    mask = np.zeros(N4, np.uint8)
    mask[4] = 1  # reset again with no new termination: the same row
    _reset_terminated(ctxs)
    _set_term(ctxs, mask)
    _step(ctxs, acts, 3)
    _assert_same(ctxs, 3)
    assert _delta(ctxs, base) == (0, 1)


# ---------------------------------------------------------------------- 5. graph capture
def test_captured_step_with_resets_pending_replayed_twice():
    """A step captured while a reset is pending and previews exist, replayed twice:
    equal to the eager unsplit run; the first replay takes the previews, the second
    computes its resets in two passes (the tags are the capture's). Nothing is
    allocated under the capture: torch captures in the global error mode, in which a
    hipMalloc, hipFree or synchronising call of the capturing thread fails and
    invalidates the capture, so check() would raise inside the `with` block and
    the graph would not instantiate."""
    P, bank, layout, ctxs, acts, base, term1 = _case(extra_off=[(e + lib().cbev_bank_stride(N_BANK)) % N_BANK for e in T4])
    L = lib()
    A, B = ctxs
    a = torch.from_numpy(acts).cuda()

    def step(c, stream):
        dw, d_bank, bf, d_recs, ring, b = c
        check(L.cbev_step(dw.ctx, ptr(d_recs), N4, ptr(a), ptr(ring[2]), ptr(b["rew"]), ptr(b["term"]),
                          ptr(b["trunc"]), ptr(b["cause"]), ptr(b["info"]), stream), "step")

    _reset_terminated([B])  # recorded before the capture
    assert L.cbev_reset_pending(B[0].ctx) == 1
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    before = B[3].clone()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            step(B, P_(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(before, B[3])  # the capture ran nothing
    for rep in range(2):
        _reset_terminated([A])
        step(A, None)
        g.replay()
        torch.cuda.synchronize()
        # a replay writes its episode rows into the ring slot of the capture, so past the
        # first replay the rows are not where the eager run's are: the rest is compared
        if rep == 0:
            _assert_same(ctxs, 2)
        for k in ("rew", "term", "trunc", "cause", "info"):
            assert torch.equal(A[5][k], B[5][k]), (rep, k)
        assert torch.equal(A[3], B[3]) and torch.equal(A[4], B[4]), (rep, "records / ring")
        assert np.array_equal(_counts(L, A[0], N4), _counts(L, B[0], N4)), (rep, "reset counts")
        if rep == 0:
            assert _delta(ctxs, base) == (int(term1.sum()), 0)
            t2 = int(_term(A).sum())
            assert t2 >= len(T4), "the second rows start inside a wall too: the second replay has resets"
        else:
            assert _delta(ctxs, base) == (int(term1.sum()), t2)


def test_bank_edited_between_capture_and_replay_takes_two_passes_with_the_new_bytes():
    """The host cannot tell a captured step that the bank changed after the capture:
    cbev_bank_frames clears the previews' tags on the device, so the replay computes
    its resets in two passes from the new bytes, as the eager unsplit run does."""
    P, bank, layout, ctxs, acts, base, term1 = _case()
    L = lib()
    A, B = ctxs
    a = torch.from_numpy(acts).cuda()

    def step(c, stream):
        dw, d_bank, bf, d_recs, ring, b = c
        check(L.cbev_step(dw.ctx, ptr(d_recs), N4, ptr(a), ptr(ring[2]), ptr(b["rew"]), ptr(b["term"]),
                          ptr(b["trunc"]), ptr(b["cause"]), ptr(b["info"]), stream), "step")

    tc = _counts(L, B[0], N4)
    ids, rows = reset_rows(term1, tc, N_BANK)
    _reset_terminated([B])
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            step(B, P_(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    new_x = {}
    for c in ctxs:
        hb = c[1].cpu().numpy()
        for row in rows:
            v = LY.RecordView(hb[row], layout)
            v.hd[LY.HD["X"]] += 2.5
            v.hd[LY.HD["V"]] += 1.0
            new_x[int(row)] = v.h("X")
        c[1].copy_(torch.from_numpy(hb))
        check(L.cbev_bank_frames(c[0].ctx, ptr(c[1]), N_BANK, ptr(c[2]), None), "bank_frames")
    torch.cuda.synchronize()
    _reset_terminated([A])
    step(A, None)
    g.replay()
    torch.cuda.synchronize()
    _assert_same(ctxs, 2)
    assert _delta(ctxs, base) == (0, int(term1.sum()))
    hr = B[3].cpu().numpy()
    for e, row in zip(ids, rows):
        assert LY.RecordView(hr[e], layout).h("X1") == new_x[int(row)], e


# ---------------------------------------------------------------------- 6. action index out of range
def test_action_index_out_of_range_in_a_preview_reset_and_a_kept_env():
    P, bank, layout, ctxs, acts, base, term1 = _case()
    assert error_flags(ctxs[0][0].ctx) == 0 and error_flags(ctxs[1][0].ctx) == 0
    _reset_terminated(ctxs)
    bad = acts.copy()
    bad[4] = P.n_discrete + 5    # an env reset from its preview
    bad[7] = -P.n_discrete - 1   # a kept env
    _step(ctxs, bad, 2)
    _assert_same(ctxs, 2)
    assert not term1[7] and _delta(ctxs, base) == (int(term1.sum()), 0)
    fa, fb = error_flags(ctxs[0][0].ctx), error_flags(ctxs[1][0].ctx)
    assert fa == fb and fa != 0
