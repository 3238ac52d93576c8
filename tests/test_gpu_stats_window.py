"""GPU: the device episode statistics (cbev.hip, d_episode_summary) past the
200-episode window, through the C-ABI at size 128.

Every context turns the statistics on before cbev_reset (make_lane's
stats_first) and resets its envs between steps with cbev_reset_terminated from
gpu_scenes.stats_bank: authored ego-only records under the shaping reward that
end after 1 to 3 steps of gas, so an env finishes an episode every step or two
and the reset folds into the next step. Incoming causes, all five terminal
ones (asserted per test): collision (the hero on a class-0 texel), success
(1 to 3 steps short of the goal), out_of_bounds (70 texels beside the route),
max_actions (KSTEPS 1 to 3 short of the limit; the truncation, which no rate
counts, like out_of_bounds) and off_road (on the sidewalk, OFFROAD one short
of the limit). None is left out; ckpt is a reward cause, not a terminal one.

The expected window is stats_ref.WindowModel: exact rates, the exact mean
within stats_ref.mean_bound, and the whole struct read back (check_struct).

Measured on an MI355X: the seeded matrix 0.85 s on the split and unsplit lanes
(25 envs each, 6 steps) and 0.12 s under repeat (4 calls), the organic run
4.8 s (19 envs, 685 steps, 410 or 411 episodes an env), each of the six clock
tests 0.26 s (one sleep of 0.25 s). No one-step episode came near the 125 ms
that the restamp check allows.
"""
from __future__ import annotations

import ctypes
import math
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from carlabev_env_amd import layout as LY
from carlabev_env_amd._lib import check, lib
from gpu_harness import (ROW_COLUMNS, assert_same, check_summary_row, error_flags, make_lane, make_lanes, preview_counts,
                         ptr, reset_terminated_all, step_all, step_repeat, window_columns)
from gpu_scenes import CAPS_LONG2, STATS_ACTION, STATS_CAUSES, stats_bank
from stats_ref import (COUNTERS, STATS_HIST, TERMINAL_CAUSES, Stats, WindowModel, episode_summary)

pytestmark = pytest.mark.gpu

F = 3  # frame ring slots


class Dealer:
    """Which bank row each env runs, on the host: env e starts on row e % B (its
    record is a copy of it) and its j-th termination hands it row
    (e + j * cbev_bank_stride(B)) % B (include/cbev.h, cbev_reset_masked)."""

    def __init__(self, n, B):
        self.B, self.stride = B, lib().cbev_bank_stride(B)
        self.env = np.arange(n)
        self.done = np.zeros(n, np.int64)   # terminations so far
        self.row = self.env % B

    def terminated(self, term):
        self.done += term
        self.row = np.where(term, (self.env + self.done * self.stride) % self.B, self.row)


def _ep_return(lane, layout):
    """The eight bytes of EP_RETURN in every device record, a view (n, 8)."""
    o = layout.off["hd"] + 8 * LY.HD["EP_RETURN"]
    return lane.recs[:, o:o + 8]


def _read_returns(lane, layout):
    return _ep_return(lane, layout).contiguous().view(torch.float64).flatten().cpu().numpy()


def _add_to_returns(lane, layout, envs, values):
    """EP_RETURN[e] += value on the device, the caller's edit of its own records
    (envs that no pending reset selects)."""
    cur = _ep_return(lane, layout).contiguous().view(torch.float64).flatten()
    idx = torch.from_numpy(np.asarray(envs, np.int64)).cuda()
    cur[idx] += torch.from_numpy(np.asarray(values, np.float64)).cuda()
    _ep_return(lane, layout).copy_(cur.view(torch.uint8).reshape(-1, 8))
    torch.cuda.synchronize()


def _out(lane, key):
    return lane.out[key].cpu().numpy()


# ---------------------------------------------------------------------- B1. seeded windows
MATRIX = ((0, 0), (1, 1), (198, 198), (199, 199), (200, 0), (200, 1), (200, 100), (200, 199))
CONTENTS = ("uniform", "pairs", "equal")
ROUNDS = 4


def _seeded_models():
    """One WindowModel per case of MATRIX x CONTENTS, and an empty one (the
    all-zero struct): returns uniform in [-3, 3]; the same with pairs of about
    +-1e9, the first pair in the two oldest slots and half of a second pair in
    the third, so the next three evictions remove one of a pair, its partner,
    and one whose partner stays; all returns equal. Causes drawn from the five
    terminal ones."""
    rng = np.random.default_rng(4242)
    models, names = [], []
    for n, head in MATRIX:
        for kind in CONTENTS:
            rets = rng.uniform(-3, 3, n)
            if kind == "equal":
                rets[:] = 0.7
            big = lambda s: s * 1e9 * rng.uniform(0.5, 1.0)  # noqa: E731
            if kind == "pairs":
                for i, v in ((0, big(1.0)), (1, big(-1.0)), (2, big(1.0)), (n // 2 + 3, big(-1.0))):
                    if i < n:
                        rets[i] = v
            causes = rng.choice(TERMINAL_CAUSES, n)
            m = WindowModel(zip(rets, causes), episode=n + 300 * (n == STATS_HIST))
            m.head = head
            models.append(m)
            names.append((n, head, kind))
    models.append(WindowModel())
    names.append((0, 0, "zero"))
    return models, names


def _seed_structs(lane, models):
    st = lane.out["stats"]
    host = st.structs().copy()
    for e, m in enumerate(models):
        if len(m) or m.episode:  # the last env keeps its all-zero struct
            t0 = host[e]["t0"]
            host[e] = m.to_struct(t0=t0)
    st.stats.copy_(torch.from_numpy(host.view(np.uint8).reshape(len(models), -1)).cuda())
    torch.cuda.synchronize()


def _run_matrix(modes, repeat):
    P, padded, bank, layout, table = stats_bank(max_life=2, presets=True)
    B = len(bank)
    names = _seeded_models()[1]
    n = len(names)
    recs = bank[np.arange(n) % B]
    lanes = make_lanes(P, padded, CAPS_LONG2, recs, bank, F, modes, stats_first=True)
    per_lane = []
    for lane in lanes:
        models = _seeded_models()[0]
        _seed_structs(lane, models)
        for e, m in enumerate(models):
            m.check_struct(lane.out["stats"].structs()[e], ("seeded", names[e]))
        per_lane.append((models, Dealer(n, B)))
    acts = np.full(n, STATS_ACTION, np.int32)
    a = torch.from_numpy(acts).cuda()
    rng = np.random.default_rng(99)
    bank_ret = np.array([LY.RecordView(bank[b].copy(), layout).h("EP_RETURN") for b in range(B)])
    fresh = np.ones(n, bool)     # the env runs a row it has not stepped yet (its reset is pending, or step 0)
    incoming = {c: 0 for c in TERMINAL_CAUSES}
    big_in = 0
    t = 0
    while min(d.done.min() for _, d in per_lane) < ROUNDS:
        assert t < 3 * ROUNDS, "every row ends within two steps"
        # the caller's edit before the step: a value added to EP_RETURN of the envs no pending reset selects
        live = np.flatnonzero(~fresh)
        inject = np.where(rng.random(len(live)) < 0.25, rng.choice([-1.0, 1.0], len(live)) * 1e9 * rng.uniform(0.5, 1, len(live)),
                          rng.uniform(-3, 3, len(live)))
        base = []
        for lane, (models, deal) in zip(lanes, per_lane):
            if repeat == 1 and len(live):
                _add_to_returns(lane, layout, live, inject)
            b = _read_returns(lane, layout)
            base.append(np.where(fresh, bank_ret[deal.row], b))
        if repeat == 1:
            step_all(lanes, acts, t)
        else:
            for lane in lanes:
                check(step_repeat(lib(), lane.dw, lane.recs, n, a, repeat, lane.ring[t % F], lane.out), "step_repeat")
            torch.cuda.synchronize()
        if len(lanes) == 2:
            assert_same(lanes, t)
        for k, (lane, (models, deal)) in enumerate(zip(lanes, per_lane)):
            st = lane.out["stats"]
            term, rew, cause = _out(lane, "term").astype(bool), _out(lane, "rew"), _out(lane, "cause")
            by_env, cnt = st.step_rows(t)
            assert cnt == int(term.sum()) and set(by_env) == set(np.flatnonzero(term).tolist()), (t, k)
            after = _read_returns(lane, layout)
            life = np.array([table[r][0] for r in deal.row])
            if repeat > 1:
                # the whole episode in one call: it ends in substep 1 or 2, one row, one episode. Its reset is
                # always pending before the call, so nothing can be added to its record: large returns come in
                # through the bank's presets alone, all on rows of one step; a row of two steps starts at 0, so
                # its return (0 + r1) + r2 is the call's reward r1 + r2 bit for bit
                assert term.all() and (life <= 2).all() and not base[k][life == 2].any()
            for e in np.flatnonzero(term):
                tag = (t, k, names[e])
                m, row = models[e], by_env[e]
                assert cause[e] == table[deal.row[e]][1] and row[LY.EP["LENGTH"]] == life[e], tag
                # the device's own operation: the return it started the step with, plus the step's reward
                want_ret = base[k][e] + rew[e]
                assert want_ret == after[e], tag
                want = {**window_columns(m), "ENV": e, "CAUSE": cause[e], "RETURN": want_ret}
                check_summary_row(row, want, m.mean_bound(), tag, exact=("RETURN",))
                m.push(row[LY.EP["RETURN"]], int(cause[e]))
                if k == 0:
                    incoming[int(cause[e])] += 1
                    big_in += abs(want_ret) > 1e8
            structs = st.structs()
            for e, m in enumerate(models):
                m.check_struct(structs[e], (t, k, names[e]))
            deal.terminated(term)
            fresh = term.copy()  # the same in every lane (assert_same; a repeat lane runs alone)
        reset_terminated_all(lanes)
        t += 1
    for lane in lanes:
        check(lib().cbev_flush(lane.dw.ctx), "flush")
        assert error_flags(lane.dw.ctx) == 0
    # what the run reached, on the device: the structs equal the models bit for bit (check_struct)
    models, deal = per_lane[0]
    final = lanes[0].out["stats"].structs()
    by_name = dict(zip(names, range(n)))
    assert all(v >= 1 for v in incoming.values()), incoming
    assert big_in >= 4, big_in
    for kind in CONTENTS:
        e = by_name[(199, 199, kind)]   # fills, wraps to head 0, then evicts
        assert final[e]["n"] == STATS_HIST and final[e]["head"] == deal.done[e] - 1 and len(models[e].evicted) >= 2
        e = by_name[(200, 199, kind)]   # wraps while it evicts
        assert final[e]["head"] == deal.done[e] - 1 and len(models[e].evicted) == deal.done[e] >= ROUNDS
    assert len({c for m in models for _, c in m.evicted}) >= 3
    for head in (0, 1, 100, 199):       # a +-1e9 pair left the window, and one whose partner stayed
        ev = [r for r, _ in models[by_name[(200, head, "pairs")]].evicted[:3]]
        assert ev[0] > 4e8 and ev[1] < -4e8 and ev[2] > 4e8, ev
    e = by_name[(0, 0, "zero")]
    assert final[e]["n"] == final[e]["episode"] == final[e]["head"] == deal.done[e]
    return t


def test_seeded_windows_split_and_unsplit():
    """The (n, head) matrix on the split step (the default) and on the unsplit
    one, both with the folded reset, equal to each other after every step
    (assert_same) and each to the model."""
    _run_matrix([dict(deferred=1), dict(split=0, deferred=1)], 1)


def test_seeded_windows_under_repeat():
    """The same matrix through cbev_step_repeat(k = 3) on the unsplit lane: an
    env ends in substep 1 or 2, stays frozen, writes one row and counts one
    episode. No value is added to a record here (every env's reset is pending
    before every call): the large incoming returns are the bank's presets, and
    the expected return is still fl(start + reward_out[e])."""
    assert _run_matrix([dict(split=0, deferred=1)], 3) == ROUNDS


# ---------------------------------------------------------------------- B2. an organic run past two wraps
EPISODES = 2 * STATS_HIST + 10


def _step_infos(h_recs, layout, rew, cause):
    """What EpisodeStats.step reads, per env, after a step (device values)."""
    out = []
    for e in range(len(h_recs)):
        v = LY.RecordView(h_recs[e], layout)
        out.append({"reward": float(rew[e]), "cause": LY.CAUSE_NAME.get(int(cause[e])), "v": v.h("V"),
                    "accel_long": v.h("C_AL"), "accel_lat": v.h("C_ALAT"), "jerk_long": v.h("C_JL"),
                    "jerk_lat": v.h("C_JLAT"), "yaw_rate": v.h("C_YR"), "yaw_acc": v.h("C_YACC")})
    return out


EPISODE_COLUMNS = {"RETURN": "return", "LENGTH": "length", "MEAN_SPEED": "mean_speed", "MEAN_TTC": "mean_ttc",
                   "MEAN_PROGRESS": "mean_progress", "MEAN_ABS_AL": "mean_abs_accel_long",
                   "MEAN_ABS_ALAT": "mean_abs_accel_lat", "MEAN_ABS_JL": "mean_abs_jerk_long",
                   "MEAN_ABS_JLAT": "mean_abs_jerk_lat", "MEAN_ABS_YR": "mean_abs_yaw_rate",
                   "MEAN_ABS_YACC": "mean_abs_yaw_acc", "VIOL_RATE": "comfort_violation_rate",
                   "HARSH_RATE": "harsh_brake_rate"}


def test_organic_run_past_two_wraps():
    """19 envs on the split default, step then reset_terminated, until every env
    has finished 2 * 200 + 10 episodes: every termination's row in every column
    but SECONDS, the per-episode columns from stats_ref's EpisodeStats fed with
    the device's per-step values (1e-9), the window columns from the WindowModel
    fed with the device's returns, the scene columns from the bank row the env
    runs; env 0 also against Stats.terminated() itself; every struct at the end."""
    n = 19
    P, padded, bank, layout, table = stats_bank(max_life=3)
    B = len(bank)
    rows_of = [LY.RecordView(bank[b].copy(), layout) for b in range(B)]
    assert len({v.i("CTX_ID") for v in rows_of}) == B
    lane = make_lane(P, padded, CAPS_LONG2, bank[np.arange(n) % B], bank, F, deferred=1, stats_first=True)
    st = lane.out["stats"]
    acts = np.full(n, STATS_ACTION, np.int32)
    stats, models, deal = [Stats() for _ in range(n)], [WindowModel() for _ in range(n)], Dealer(n, B)
    incoming = {c: 0 for c in TERMINAL_CAUSES}
    three_causes_at_eviction = 0
    t = 0
    while deal.done.min() < EPISODES:
        assert t < 2000, deal.done
        step_all([lane], acts, t)
        term, rew, cause = _out(lane, "term").astype(bool), _out(lane, "rew"), _out(lane, "cause")
        infos = _step_infos(lane.recs.cpu().numpy(), layout, rew, cause)
        by_env, cnt = st.step_rows(t)
        assert cnt == int(term.sum()) and set(by_env) == set(np.flatnonzero(term).tolist()), t
        for e in range(n):
            stats[e].current.step(infos[e])
        for e in np.flatnonzero(term):
            m, row, src = models[e], by_env[e], rows_of[deal.row[e]]
            ep = episode_summary(stats[e].current)
            assert ep["length"] == table[deal.row[e]][0], (t, e)
            want = {col: ep[key] for col, key in EPISODE_COLUMNS.items()}
            want.update(window_columns(m), ENV=e, CAUSE=LY.CAUSE[ep["termination"]], NUM_VEH=src.h("NUM_VEH"),
                        LEN_ROUTE_M=src.h("LEN_ROUTE_M"), CTX_ID=src.i("CTX_ID"))
            assert set(want) == set(ROW_COLUMNS)
            check_summary_row(row, want, m.mean_bound(), (t, int(e)))
            if e == 0:  # the reference's restatement whole, window included, on one env
                ref = stats[e].terminated()
                got = m.summary()
                assert ref["episode"] == m.episode and all(ref[k] == got[k] for k in got if k != "mean_reward"), (t, ref)
                assert abs(ref["mean_reward"] - float(got["mean_reward"])) <= 1e-12 * abs(ref["mean_reward"]), (t, ref)
            else:
                stats[e].reset()
            if len(m) == STATS_HIST and len({c for _, c in m.window}) >= 3:
                three_causes_at_eviction += 1
            m.push(row[LY.EP["RETURN"]], int(cause[e]))
            incoming[int(cause[e])] += 1
        deal.terminated(term)
        reset_terminated_all([lane])
        t += 1
    check(lib().cbev_flush(lane.dw.ctx), "flush")
    assert error_flags(lane.dw.ctx) == 0
    structs = st.structs()
    for e, m in enumerate(models):
        m.check_struct(structs[e], ("end", e))
        assert structs[e]["episode"] == deal.done[e] >= EPISODES and structs[e]["n"] == STATS_HIST
        assert len(m.evicted) == deal.done[e] - STATS_HIST >= STATS_HIST + 10   # the ring went round twice
        evicted = {c for _, c in m.evicted}
        assert evicted >= set(COUNTERS.values()), (e, evicted)  # each rate's counter came down
    assert three_causes_at_eviction >= n and all(v >= n for v in incoming.values()), (three_causes_at_eviction, incoming)
    assert set(LY.CAUSE[c] for c in STATS_CAUSES) == set(incoming)
    hits, fallbacks = preview_counts(lane)
    assert hits >= 1 and hits + fallbacks == deal.done.sum() - int(term.sum())  # every reset but the last was folded


# ---------------------------------------------------------------------- B3. the episode clock
SLEEP = 0.25


def _hz(lane):
    hz = ctypes.c_double()
    check(lib().cbev_wall_clock_hz(lane.dw.ctx, ctypes.byref(hz)), "wall_clock_hz")
    assert math.isfinite(hz.value) and hz.value > 0
    return hz.value


def _seconds(lane, t):
    """(envs, SECONDS, LENGTH) of the rows step t wrote."""
    by_env, _ = lane.out["stats"].step_rows(t)
    envs = sorted(by_env)
    return (np.array(envs), np.array([by_env[e][LY.EP["SECONDS"]] for e in envs]),
            np.array([by_env[e][LY.EP["LENGTH"]] for e in envs]))


def _clock_world(n=19):
    P, padded, bank, layout, table = stats_bank(max_life=2)
    return P, padded, bank, bank[np.arange(n) % len(bank)], n


def _launched_reset(lane, path, n, B, offset):
    L = lib()
    dw, d_bank, bf, d_recs, ring, out = lane
    if path == "reset":
        check(L.cbev_reset(dw.ctx, ptr(d_recs), n, ptr(d_bank), B, None, None, offset, ptr(ring), F, None), path)
    elif path == "reset_frames":
        check(L.cbev_reset_frames(dw.ctx, ptr(d_recs), n, ptr(d_bank), B, None, None, offset, ptr(bf), ptr(ring), F, None),
              path)
    else:
        mask = torch.ones(n, dtype=torch.uint8, device="cuda")
        check(L.cbev_reset_masked(dw.ctx, ptr(d_recs), n, ptr(mask), ptr(d_bank), B, ptr(bf), ptr(ring), F, None), path)
    torch.cuda.synchronize()


@pytest.mark.parametrize("path", ["reset", "reset_frames", "reset_masked"])
def test_clock_is_stamped_by_a_launched_reset(path):
    """k_reset, k_reset_copy and k_reset_mask. (i) reset, synchronise, sleep 0.25 s,
    step: an env that ends in that step reports at least 0.99 of the sleep and at
    most 1.01 of the host's span around reset and step (the device interval lies
    inside the host's and contains the sleep; 1 % for the two clocks' rates).
    (ii) reset again, step at once: under half the sleep; an env whose stamp was
    skipped would report more than the whole sleep."""
    P, padded, bank, recs, n = _clock_world()
    lane = make_lane(P, padded, CAPS_LONG2, recs, bank, F, stats_first=True)
    _hz(lane)
    acts = np.full(n, STATS_ACTION, np.int32)
    t_a = time.perf_counter()
    _launched_reset(lane, path, n, len(bank), 3)
    s0 = time.perf_counter()
    time.sleep(SLEEP)
    slept = time.perf_counter() - s0
    step_all([lane], acts, 0)
    span = time.perf_counter() - t_a
    envs, sec, _ = _seconds(lane, 0)
    assert len(envs) >= n // 2 and slept >= SLEEP
    assert (sec >= 0.99 * slept).all() and (sec <= 1.01 * span).all(), (path, slept, span, sec)
    _launched_reset(lane, path, n, len(bank), 8)
    step_all([lane], acts, 1)
    envs, sec, _ = _seconds(lane, 1)
    assert len(envs) >= 4
    assert (sec >= 0).all() and (sec < 0.5 * slept).all(), (path, slept, sec)


FOLDED = {"unsplit": dict(split=0, deferred=1), "split-preview": dict(deferred=1, preview=1),
          "split-no-preview": dict(deferred=1, preview=0)}


@pytest.mark.parametrize("mode", list(FOLDED))
def test_clock_is_stamped_by_a_folded_reset(mode):
    """cbev_reset_terminated folded into the next step: ego_reset_take (unsplit)
    and the split step's head, with the reset preview on and off. The stamp
    happens inside the step that takes the reset. Four steps first, so that
    previews exist; then step A, a sleep of 0.25 s with the resets of A's
    terminations pending, and step B. (i) An env that took its reset in A and
    ends in B (2 steps long) reports at least 0.99 of the sleep and at most 1.01
    of the host's span around A and B. (ii) An env that takes its reset in B and
    ends in B (1 step long) was last stamped before the sleep: it reports under
    half the sleep, where a skipped stamp would report more than all of it."""
    P, padded, bank, recs, n = _clock_world()
    lane = make_lane(P, padded, CAPS_LONG2, recs, bank, F, stats_first=True, **FOLDED[mode])
    _hz(lane)
    acts = np.full(n, STATS_ACTION, np.int32)
    for t in range(4):
        step_all([lane], acts, t)
        reset_terminated_all([lane])
        assert lib().cbev_reset_pending(lane.dw.ctx) == 1
    t_a = time.perf_counter()
    step_all([lane], acts, 4)   # A
    _, sec_a, len_a = _seconds(lane, 4)
    assert (sec_a[len_a == 1] < 0.5 * SLEEP).all(), (mode, sec_a, len_a)
    reset_terminated_all([lane])
    s0 = time.perf_counter()
    time.sleep(SLEEP)
    slept = time.perf_counter() - s0
    step_all([lane], acts, 5)   # B
    span = time.perf_counter() - t_a
    _, sec, length = _seconds(lane, 5)
    old, new = sec[length == 2], sec[length == 1]
    assert len(old) >= 2 and len(new) >= 4 and slept >= SLEEP, (mode, length)
    assert (old >= 0.99 * slept).all() and (old <= 1.01 * span).all(), (mode, slept, span, old)
    assert (new >= 0).all() and (new < 0.5 * slept).all(), (mode, slept, new)
    hits, fallbacks = preview_counts(lane)
    assert hits + fallbacks > 0 if mode != "unsplit" else (hits, fallbacks) == (0, 0)
    assert (hits > 0) == (mode == "split-preview"), (mode, hits, fallbacks)
