"""The host model of cbev_episode_stats (stats_ref.STATS_DTYPE, WindowModel,
mean_bound) on the CPU: its layout against the header's, the window against
the reference's recorded summaries past 200 episodes (tests/golden/stats.npz),
the struct round trip at the ring's edges, and the tolerance of MEAN_REWARD
against a restatement of the device's double-double sum on sequences that tell
it apart from a plain running sum.
"""
from __future__ import annotations

import os
from fractions import Fraction

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # gpu_harness imports it

from carlabev_env_amd import layout as LY
from gpu_harness import T0
from stats_ref import (COUNTERS, STATS_DTYPE, STATS_HIST, TERMINAL_CAUSES, WindowModel, dd_add, mean_bound)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stats.npz")


def test_struct_layout_is_the_headers():
    assert STATS_HIST == 200
    assert STATS_DTYPE.itemsize == LY.STATS_BYTES
    assert STATS_DTYPE.fields["t0"][1] == T0.start and T0.stop - T0.start == 8
    assert STATS_DTYPE.names == ("ret", "sum_hi", "sum_lo", "t0", "n", "head", "episode", "n_success", "n_collision",
                                 "n_offroad", "cause", "pad")
    assert STATS_DTYPE.fields["cause"][1] == 8 * STATS_HIST + 24 + 24  # no padding before the cause ring


def test_window_model_matches_the_reference_past_200_episodes():
    """Every termination of the recorded streams: the rates equal, mean_reward
    within 1e-12 relative of the reference's np.mean; streams 0 and 1 run 230
    and 215 episodes, so their windows drop entries."""
    d = np.load(GOLD)
    summ, keys = d["summaries"], [str(k) for k in d["keys"]]
    col = {k: 1 + i for i, k in enumerate(keys)}
    models = {}
    for row in summ:
        m = models.setdefault(int(row[0]), WindowModel())
        got = m.summary()
        assert row[col["episode"]] == m.episode
        for rate in ("success_rate", "collision_rate", "unfinished_rate"):
            assert got[rate] == row[col[rate]], (row[0], m.episode, rate)
        want = row[col["mean_reward"]]
        assert abs(float(got["mean_reward"]) - want) <= 1e-12 * abs(want), (row[0], m.episode)
        m.push(row[col["return"]], int(row[-1]))
    assert [models[k].episode for k in (0, 1)] == [230, 215]
    assert len(models[0].evicted) == 30 and len(models[1].evicted) == 15
    assert {c for m in models.values() for _, c in m.evicted} >= set(COUNTERS.values())


def _window(n, rng):
    return [(rng.uniform(-3, 3), int(rng.choice(TERMINAL_CAUSES))) for _ in range(n)]


@pytest.mark.parametrize("n", [0, 1, 199, 200])
@pytest.mark.parametrize("head", [0, 1, 100, 199])
def test_struct_round_trip(n, head):
    rng = np.random.default_rng(1000 * n + head)
    m = WindowModel(_window(n, rng), episode=n + 7)
    rec = m.to_struct(head)
    assert rec["n"] == n and rec["head"] == head and rec["episode"] == n + 7
    assert np.count_nonzero(rec["cause"]) == n
    if n:
        assert rec["ret"][(head - 1) % STATS_HIST] == m.window[-1][0]  # the newest sits before the next slot
        assert rec["ret"][(head - n) % STATS_HIST] == m.window[0][0]   # a full ring evicts the oldest next
    m.check_struct(rec)
    raw = np.frombuffer(rec.tobytes(), np.uint8)  # as the bytes of a device buffer
    m.check_struct(raw.view(STATS_DTYPE)[0])
    # every field check_struct compares is noticed
    for k in ("n", "head", "episode", *COUNTERS):
        bad = rec.copy()
        bad[k] += 1
        with pytest.raises(AssertionError, match=repr(k)):
            m.check_struct(bad)
    if n:
        for k in ("ret", "cause"):
            bad = rec.copy()
            bad[k][(head - 1) % STATS_HIST] += 1
            with pytest.raises(AssertionError, match=repr(k)):
                m.check_struct(bad)
        bad = rec.copy()
        bad["sum_lo"] += 1e-9
        with pytest.raises(AssertionError, match=repr("sum")):
            m.check_struct(bad)
    # a push moves the model as the device moves the struct
    m.push(1.5, TERMINAL_CAUSES[0])
    assert m.head == (head + 1) % STATS_HIST and len(m) == min(n + 1, STATS_HIST) and len(m.evicted) == (n == 200)


def _adversarial(rng, length=700, big=40):
    """Returns in [-3, 3] with `big` entries of magnitude up to 1e9 at random places."""
    x = rng.uniform(-3, 3, length)
    at = rng.choice(length, big, replace=False)
    x[at] = rng.choice([-1.0, 1.0], big) * 1e9 * rng.uniform(0, 1, big)
    return x.tolist()


def test_double_double_window_sum_stays_within_mean_bound_and_a_plain_sum_does_not():
    """300 sequences of 700 returns sliding through the 200-window: the device's
    arithmetic (dd_add, subtracting the evicted return, then fl(fl(hi + lo) / n))
    against the exact mean stays within mean_bound; a plain float64 running sum
    with subtraction exceeds it, or the inputs are too tame to tell the two apart."""
    rng = np.random.default_rng(2024)
    worst_dd = worst_plain = 0.0
    for _ in range(300):
        x = _adversarial(rng)
        fx = [Fraction(v) for v in x]
        hi = lo = plain = 0.0
        exact = Fraction(0)
        for i, v in enumerate(x):
            if i >= STATS_HIST:
                hi, lo = dd_add(hi, lo, -x[i - STATS_HIST])
                plain -= x[i - STATS_HIST]
                exact -= fx[i - STATS_HIST]
            hi, lo = dd_add(hi, lo, v)
            plain += v
            exact += fx[i]
            assert hi == hi + lo
            if i % 7 and i != len(x) - 1:  # the mean is checked on a seventh of the positions and at the end
                continue
            n = min(i + 1, STATS_HIST)
            mean = exact / n
            bound = mean_bound(mean, n, max(abs(w) for w in x[i + 1 - n:i + 1]))
            worst_dd = max(worst_dd, float(abs(Fraction((hi + lo) / n) - mean) / bound))
            worst_plain = max(worst_plain, float(abs(Fraction(plain / n) - mean) / bound))
    assert worst_dd <= 1.0, worst_dd
    assert worst_plain > 1.0, worst_plain
