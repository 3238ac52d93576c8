"""What the four step entries (cbev_step, cbev_step_repeat, cbev_step_masked,
cbev_step_heads) share: one episode slot and one profile record per call
whatever the repeat, refusals that leave the context and the records as they
were (a recorded deferred reset included), and one chain behind the three
unsplit entries. Everything is exact: counters, bytes, and both sides of the
chain comparison run the same arithmetic.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from carlabev_env_amd import layout as LY
from carlabev_env_amd._lib import REPEAT_MAX, check, lib
from gpu_harness import KEYS, error_flags, make_lane, ptr
from helpers import action_stream, build_records, world

pytestmark = pytest.mark.gpu

CBEV_EINVAL = -1
N, F, B, SIZE = 8, 3, 5, 128
CAPS = {"ego": (LY.Caps(64, 0, 2, 0), ("rt_no_traffic_v1",)),  # no actors kernel, a reset can be deferred
        "actors": (LY.Caps(64, 4, 288, 4), ("mix3",))}          # the actors launches run
ENTRIES = ("step", "repeat", "masked", "heads")
_HOST = {}


def _host(kind):
    """(P, padded, caps, records, bank) of a capacity set, built once: every second
    env starts off the road, so the first substep already ends some."""
    if kind not in _HOST:
        caps, kinds = CAPS[kind]
        cfg, P, padded, layout, builder = world(SIZE, caps=caps)
        recs, _ = build_records(builder, N, kinds, seed0=50_000)
        for e in range(0, N, 2):
            LY.RecordView(recs[e], layout).hd[LY.HD["X"]] += 60.0
        bank, _ = build_records(builder, B, kinds, seed0=60_000)
        recs.setflags(write=False)
        bank.setflags(write=False)
        _HOST[kind] = (P, padded, caps, recs, bank)
    return _HOST[kind]


class World:
    """A context on the shared records with the episode statistics on (and the
    profile, unless profile=False), an F-slot ring and the per-env heads of
    cbev_step_heads."""

    def __init__(self, kind, deferred=0, profile=True):
        self.P, padded, caps, recs, bank = _host(kind)
        lane = make_lane(self.P, padded, caps, recs, bank, F, split=0, deferred=deferred)
        self.dw, self.bank, self.bank_frames, self.recs, self.ring, self.b = lane
        self.ctx, self.stats = self.dw.ctx, self.b["stats"]
        self.heads = torch.from_numpy((np.arange(N) % F).astype(np.uint8)).cuda()
        self.ones = torch.ones(N, dtype=torch.uint8, device="cuda")
        if profile:
            check(lib().cbev_profile(self.ctx, 1), "profile")
        self.slot = 0  # the ring slot of the newest frame (step, repeat, masked)

    def call(self, entry, a, repeat=1, n=N, rew="rew", frames=None, n_frames=F):
        """One call of `entry` into the next ring slot (cbev_step_heads: into the
        ring); returns its code. rew=None, frames= and n_frames= make the refusals."""
        L, b = lib(), self.b
        out = (ptr(b[rew]) if rew else None, ptr(b["term"]), ptr(b["trunc"]), ptr(b["cause"]), ptr(b["info"]), None)
        new = self.ring[(self.slot + 1) % F]
        dst = ptr(new) if frames is None else frames
        if entry == "step":
            assert repeat == 1
            return L.cbev_step(self.ctx, ptr(self.recs), n, ptr(a), dst, *out)
        if entry == "repeat":
            return L.cbev_step_repeat(self.ctx, ptr(self.recs), n, ptr(a), repeat, dst, *out)
        if entry == "masked":
            return L.cbev_step_masked(self.ctx, ptr(self.recs), n, ptr(a), ptr(self.ones), repeat,
                                      ptr(self.ring[self.slot]), dst, *out)
        ring = ptr(self.ring) if frames is None else frames
        return L.cbev_step_heads(self.ctx, ptr(self.recs), n, ptr(a), ptr(self.ones), repeat, ring, n_frames,
                                 ptr(self.heads), *out)

    def step_count(self):
        c = ctypes.c_int64(-1)
        lib().cbev_episode_slot(self.ctx, ctypes.byref(c))
        return c.value

    def profile(self):
        ms3, steps = (ctypes.c_double * 3)(), ctypes.c_int64(-1)
        check(lib().cbev_profile_read(self.ctx, ms3, ctypes.byref(steps)), "profile_read")
        return list(ms3), steps.value

    def newest(self, entry):
        if entry == "heads":
            return self.ring[self.heads.long(), torch.arange(N, device="cuda")]
        return self.ring[self.slot]


def _actions(P, steps, seed=5):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in action_stream(P, N, steps, seed=seed)]


@pytest.mark.parametrize("kind", list(CAPS))
def test_every_entry_takes_one_episode_slot_and_one_profile_record(kind):
    """Each of the four entries with repeat 1, then the three that take a repeat
    with repeat 3, on one context: after every call the step count of
    cbev_episode_slot and the steps of cbev_profile_read have advanced by exactly
    1, and the three phase sums are finite and not negative."""
    W = World(kind)
    calls = [(e, 1) for e in ENTRIES] + [(e, 3) for e in ENTRIES[1:]]
    acts = _actions(W.P, len(calls))
    assert W.step_count() == 0 and W.profile()[1] == 0
    for t, (entry, k) in enumerate(calls):
        check(W.call(entry, acts[t], repeat=k), f"{entry} k={k}")
        W.slot = (W.slot + 1) % F
        torch.cuda.synchronize()
        ms3, steps = W.profile()
        print(kind, entry, k, "step_count", W.step_count(), "profile steps", steps, "ms", ms3)
        assert W.step_count() == t + 1, (entry, k)
        assert steps == t + 1, (entry, k)
        assert all(math.isfinite(v) and v >= 0.0 for v in ms3), (entry, k, ms3)
    assert error_flags(W.ctx) == 0


# (reason, the entries it applies to, the arguments that make it)
REFUSALS = [
    ("null reward", ENTRIES, dict(rew=None)),
    ("repeat 0", ENTRIES[1:], dict(repeat=0)),
    ("repeat above the maximum", ENTRIES[1:], dict(repeat=REPEAT_MAX + 1)),
    ("misaligned frames", ("masked", "heads"), "misaligned"),
    ("n_frames 0", ("heads",), dict(n_frames=0)),
    ("n above the statistics' envs", ENTRIES, dict(n=N + 1)),
]


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_refused_call_changes_nothing(entry):
    """Every refusal of an entry returns CBEV_EINVAL and leaves the step count,
    the profile's steps, the records, the ring and the outputs as they were; a
    recorded deferred reset stays recorded (in all four entries every check comes
    before the reset is folded or launched). The context then still works: the
    next good call takes the reset and one slot."""
    L = lib()
    W = World("ego", deferred=1)
    acts = _actions(W.P, 2)
    bad = torch.full((N,), 100, dtype=torch.int32, device="cuda")  # would raise the action flag if anything ran
    check(W.call("step", acts[0]), "step")
    W.slot = 1
    check(L.cbev_reset_terminated(W.ctx, ptr(W.recs), N, ptr(W.bank), B, ptr(W.bank_frames), ptr(W.ring), F, None),
          "reset_terminated")
    assert L.cbev_reset_pending(W.ctx) == 1
    torch.cuda.synchronize()
    assert int(W.b["term"].sum()) > 0  # the recorded reset has envs to reset: launched, it would change the records
    keep = [W.recs, W.ring, W.heads, W.stats.stats, W.stats.rows, W.stats.counts] + [W.b[k] for k in KEYS]
    before = [x.clone() for x in keep]
    count0, steps0 = W.step_count(), W.profile()[1]
    assert (count0, steps0) == (1, 1)
    made = 0
    for reason, entries, how in REFUSALS:
        if entry not in entries:
            continue
        if how == "misaligned":
            buf = W.ring if entry == "heads" else W.ring[W.slot + 1]
            how = dict(frames=ctypes.c_void_p(buf.data_ptr() + 4))
        assert W.call(entry, bad, **{"repeat": 1 if entry == "step" else 2, **how}) == CBEV_EINVAL, reason
        assert len(L.cbev_last_error()) > 0, reason
        assert L.cbev_reset_pending(W.ctx) == 1, reason
        assert W.step_count() == count0 and W.profile()[1] == steps0, reason
        made += 1
    assert made == {"step": 2, "repeat": 4, "masked": 5, "heads": 6}[entry]
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, keep))
    assert error_flags(W.ctx) == 0
    check(W.call(entry, acts[1]), entry)
    torch.cuda.synchronize()
    assert L.cbev_reset_pending(W.ctx) == 0
    assert W.step_count() == count0 + 1 and W.profile()[1] == steps0 + 1
    assert not torch.equal(W.recs, before[0])
    assert error_flags(W.ctx) == 0


@pytest.mark.parametrize("kind", list(CAPS))
def test_the_three_unsplit_entries_run_one_chain(kind):
    """From the same records with the same actions, repeat 3: cbev_step_masked
    and cbev_step_heads with every env active leave the records, outputs and
    newest frames of cbev_step_repeat (heads: ring[heads[e]][e])."""
    steps, k = 2, 3
    worlds = {entry: World(kind, profile=False) for entry in ENTRIES[1:]}
    acts = _actions(worlds["repeat"].P, steps, seed=9)
    heads0 = worlds["heads"].heads.clone()
    ended = 0
    for t in range(steps):
        for entry, W in worlds.items():
            check(W.call(entry, acts[t], repeat=k), entry)
            W.slot = (W.slot + 1) % F
        torch.cuda.synchronize()
        ref = worlds["repeat"]
        for entry in ("masked", "heads"):
            W = worlds[entry]
            assert torch.equal(W.recs, ref.recs), (t, entry, "records")
            for key in KEYS:
                assert torch.equal(W.b[key], ref.b[key]), (t, entry, key)
            assert torch.equal(W.newest(entry), ref.newest("repeat")), (t, entry, "the newest frame")
        ended += int(ref.b["term"].sum())
        assert 0 < int(ref.b["term"].sum()) < N, t  # substeps 2.. ran gated for some envs and open for others
    assert torch.equal(worlds["heads"].heads, (heads0 + steps) % F)
    assert ended > 0 and all(error_flags(W.ctx) == 0 for W in worlds.values())
