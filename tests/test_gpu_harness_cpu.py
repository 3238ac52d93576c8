"""gpu_harness.assert_same_state on CPU tensors: the one bitwise comparison the
split-step, thin-head, preview, tail-copy, repeat and masked-step tests rely on
notices a change in each item it compares, names that item, and ignores only
what same_stats ignores on purpose (the reset clock stamp t0, the elapsed
SECONDS). No GPU, no library: the statistics are a stand-in shaped as
EpisodeStatsOn's.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from carlabev_env_amd import layout as LY
from gpu_harness import KEYS, T0, Lane, assert_same_state

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


@pytest.mark.parametrize("case", list(CHANGES))
def test_stats_ring_off_drops_only_the_other_slots_counts(case):
    item, change = CHANGES[case]
    if case == "another slot's count":
        _compare(change, stats_ring=False)
    else:
        with pytest.raises(AssertionError) as err:
            _compare(change, stats_ring=False)
        assert repr(item) in str(err.value), err.value
