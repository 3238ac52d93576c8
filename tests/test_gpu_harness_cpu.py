"""gpu_harness.assert_same_state on CPU tensors: the one bitwise comparison the
split-step, thin-head, preview, tail-copy, repeat and masked-step tests rely on
notices a change in each item it compares, names that item, and ignores only
what same_stats ignores on purpose (the reset clock stamp t0, the elapsed
SECONDS). No GPU, no library: the statistics are a stand-in shaped as
EpisodeStatsOn's.

gpu_harness.check_summary_row, the column comparison of EpisodeStatsOn.check
and of the statistics-window tests: a correct row passes, each single changed
column raises and names the column.
"""
from __future__ import annotations

from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from carlabev_env_amd import layout as LY
from gpu_harness import (EP_MEANS, KEYS, ROW_COLUMNS, T0, Lane, assert_same_state, check_summary_row, episode_columns,
                         window_columns)
from stats_ref import WindowModel

N, F, S, REC, RING, T = 3, 2, 4, 64, 4, 1  # step T writes the statistics' slot T % RING = 1
SLOT, OTHER_SLOT = T % RING, 2


def _state():
    """A lane of CPU tensors after step T and its reset counts: two summary rows
    (envs 2 and 0) in the step's slot, one in another slot."""
    g = torch.Generator().manual_seed(7)
    rnd = lambda shape, dt: torch.randint(0, 200, shape, generator=g).to(dt)  # noqa: E731
    rows = torch.rand((RING, N, len(LY.EP)), generator=g, dtype=torch.float64)
    rows[SLOT, :2, LY.EP["ENV"]] = torch.tensor([2.0, 0.0], dtype=torch.float64)
    stats = SimpleNamespace(stats=rnd((N, LY.STATS_BYTES), torch.uint8), rows=rows,
                            counts=torch.tensor([0, 2, 1, 0], dtype=torch.int32), RING=RING)
    out = dict(rew=torch.rand(N, generator=g, dtype=torch.float64), term=rnd((N,), torch.uint8),
               trunc=rnd((N,), torch.uint8), cause=rnd((N,), torch.int32),
               info=torch.rand((N, 16), generator=g), stats=stats)
    lane = Lane(None, None, None, rnd((N, REC), torch.uint8), rnd((F, N, S, S), torch.uint8), out)
    return lane, np.array([1, 0, 2], np.uint32)


def _bump(t, *idx):
    t[idx] = t[idx] + 1


# (the item the message must name, the change to lane b or its reset counts)
CHANGES = {
    **{k: (k, lambda b, c, k=k: _bump(b.out[k], 1)) for k in KEYS},
    "a record byte": ("records", lambda b, c: _bump(b.recs, 2, 17)),
    "ring slot 0": ("ring", lambda b, c: _bump(b.ring, 0, 1, 2, 3)),
    "ring slot 1": ("ring", lambda b, c: _bump(b.ring, 1, 0, 0, 0)),
    "an accumulator byte outside t0": ("accumulators", lambda b, c: _bump(b.out["stats"].stats, 1, T0.stop)),
    "a row column other than SECONDS": ("rows", lambda b, c: _bump(b.out["stats"].rows, SLOT, 1, LY.EP["RETURN"])),
    "the slot's count": ("row count", lambda b, c: _bump(b.out["stats"].counts, SLOT)),
    "another slot's count": ("counts", lambda b, c: _bump(b.out["stats"].counts, OTHER_SLOT)),
    "a reset count": ("reset counts", lambda b, c: _bump(c, 2)),
}
IGNORED = {
    "the t0 bytes": lambda b: _bump(b.out["stats"].stats, 0, T0.start + 3),
    "the SECONDS column": lambda b: _bump(b.out["stats"].rows, SLOT, 0, LY.EP["SECONDS"]),
}


def _compare(change=None, **kw):
    (a, ca), (b, cb) = _state(), _state()
    if change is not None:
        change(b, cb)
    assert_same_state(a, b, T, N, counts_a=ca, counts_b=cb, **kw)


def test_identical_states_pass():
    _compare()
    _compare(stats_ring=False)


@pytest.mark.parametrize("case", list(CHANGES))
def test_one_changed_element_raises_and_names_the_item(case):
    item, change = CHANGES[case]
    with pytest.raises(AssertionError) as err:
        _compare(change)
    assert repr(item) in str(err.value) and str(T) in str(err.value), err.value


@pytest.mark.parametrize("case", list(IGNORED))
def test_what_same_stats_ignores_still_passes(case):
    _compare(lambda b, c: IGNORED[case](b))


# ---------------------------------------------------------------------- check_summary_row
def _summary_case():
    """A window of three episodes, the record of a fourth at its terminal step (a
    stand-in for a RecordView) and the row a correct device writes for it."""
    m = WindowModel([(1.25, LY.CAUSE["success"]), (-1.0, LY.CAUSE["collision"]), (0.1, LY.CAUSE["off_road"])], episode=9)
    hd = {"EP_RETURN": 2.7, "NUM_VEH": 8.0, "LEN_ROUTE_M": 61.5,
          **{acc: 0.37 * (k + 1) for k, (acc, _) in enumerate(EP_MEANS)}}
    hi = {"EP_LEN": 7, "CAUSE": LY.CAUSE["max_actions"], "CTX_ID": 41}
    view = SimpleNamespace(h=hd.__getitem__, i=hi.__getitem__)
    want = {**episode_columns(2, view), **window_columns(m)}
    row = np.zeros(len(LY.EP))
    for col, w in want.items():
        row[LY.EP[col]] = float(w)
    row[LY.EP["SECONDS"]] = 0.031
    return m, want, row


def test_summary_row_of_a_correct_device_passes():
    m, want, row = _summary_case()
    assert set(want) == set(ROW_COLUMNS) and len(ROW_COLUMNS) == len(LY.EP) - 1
    assert want["MEAN_REWARD"] == Fraction(1.25) / 3 + Fraction(-1.0) / 3 + Fraction(0.1) / 3  # exact, not rounded
    assert (want["SUCCESS_RATE"], want["COLLISION_RATE"], want["UNFINISHED_RATE"], want["EPISODE"]) == (1 / 3,) * 3 + (9,)
    assert want["MEAN_ABS_AL"] == 0.37 * 2 / 7 and want["MEAN_TTC"] == 0.0 and want["MEAN_PROGRESS"] == 0.0
    check_summary_row(row, want, m.mean_bound(), "ok")
    row[LY.EP["SECONDS"]] += 100.0  # the elapsed time is not compared
    check_summary_row(row, want, m.mean_bound(), "ok")
    # a sum in another order (the last bits of a CLOSE column) passes unless the caller asks for equality
    row[LY.EP["RETURN"]] = np.nextafter(row[LY.EP["RETURN"]], 9.0)
    check_summary_row(row, want, m.mean_bound(), "ok")
    with pytest.raises(AssertionError, match="'RETURN'"):
        check_summary_row(row, want, m.mean_bound(), "t", exact=("RETURN",))


@pytest.mark.parametrize("col", ROW_COLUMNS)
def test_one_changed_summary_column_raises_and_names_it(col):
    m, want, row = _summary_case()
    # MEAN_REWARD: three ulps, one more than the two roundings and the binade that mean_bound allows
    row[LY.EP[col]] += 3 * np.spacing(row[LY.EP[col]]) if col == "MEAN_REWARD" else 1e-6 * max(1.0, abs(row[LY.EP[col]]))
    with pytest.raises(AssertionError) as err:
        check_summary_row(row, want, m.mean_bound(), "tagged")
    assert repr(col) in str(err.value) and "tagged" in str(err.value), err.value
    assert sum(repr(c) in str(err.value) for c in ROW_COLUMNS) == 1


@pytest.mark.parametrize("case", list(CHANGES))
def test_stats_ring_off_drops_only_the_other_slots_counts(case):
    item, change = CHANGES[case]
    if case == "another slot's count":
        _compare(change, stats_ring=False)
    else:
        with pytest.raises(AssertionError) as err:
            _compare(change, stats_ring=False)
        assert repr(item) in str(err.value), err.value
