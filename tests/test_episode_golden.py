"""The whole step against whole-episode traces of the reference.

tests/golden/episodes.npz holds episodes recorded from the reference's own
CarlaBEV.reset / CarlaBEV.step (tests/golden/make_golden_episodes.py): the
realised scene, the reset state, the action stream and, after every step, what
collision_check, the reward function, Stats and _check_termination made of it.
Here scene_pack.pack_scene packs each recorded scene and the C oracle's orc_step
replays the recorded actions; everything recorded is compared after every step,
up to and including the terminal one. The piecewise fixtures
(test_oracle_golden.py) pin the parts; this pins how the step joins them: the
order of _scene_step, which rects collide and which hit wins, the targets'
sizes, ids and consumption, the 35-texel actor list, the tile lookup, and the
way from the info dict to reward, sticky cause, terminated and truncated.

Frames are not part of the fixture: frames, grayscale and resize stay unpinned
at the pygame boundary.

Bounds. Integers, flags, ids, visibility bits and behaviour states are exact,
and no step is excluded (the generator rejects episodes with a near-tie in a
rounding, in the 35-texel compare or in a reward threshold). For float64 values
the bound is 10 x the largest deviation of the oracle from the fixture measured
over all episodes (printed by every run, `pytest -s`), capped by the per-step
bounds of the piecewise tests (hero rtol 1e-11 / atol 1e-9, actors rtol 1e-9 /
atol 1e-7). Measured on the fixture as committed:

  hero state, last_state, dist2wp, dist2goal(_t_1)   abs 1.110e-16   rel 2.203e-16
  actors (x, y, yaw, v; actors_state rows)           abs 1.297e-13   rel 1.538e-13
  rewards, comfort, control, episode summaries       abs 1.041e-15   rel 8.862e-16

(abs over values below 1 in magnitude, rel over the others.)
"""
from __future__ import annotations

import numpy as np

import oracle as O
import episode_fixture as EF
from carlabev_env_amd import layout as LY
from episode_fixture import Deviation, compare_reset, compare_step, compare_summary, pack_episode, world_of


def summary_of(view):
    """Stats.get_episode_info's numeric fields from a record's accumulators (stats.py:127-148)."""
    n = max(view.i("EP_LEN"), 1)
    h = view.h
    return {"return": h("EP_RETURN"), "length": float(view.i("EP_LEN")), "mean_speed": h("EP_SPEED") / n,
            "mean_abs_accel_long": h("EP_ABS_AL") / n, "mean_abs_accel_lat": h("EP_ABS_ALAT") / n,
            "mean_abs_jerk_long": h("EP_ABS_JL") / n, "mean_abs_jerk_lat": h("EP_ABS_JLAT") / n,
            "mean_abs_yaw_rate": h("EP_ABS_YR") / n, "mean_abs_yaw_acc": h("EP_ABS_YACC") / n,
            "comfort_violation_rate": h("EP_VIOL") / n, "harsh_brake_rate": h("EP_HARSH") / n,
            "num_vehicles": h("NUM_VEH")}


def replay(ep, dev):
    """pack_scene + orc_step over one episode, compared with the fixture throughout."""
    P, padded = world_of(ep.config)
    rec, layout, caps = pack_episode(ep)
    view = LY.RecordView(rec, layout)
    orc = O.Oracle(P, padded, caps.c(), layout.record_bytes)
    frame = np.zeros((P.size, P.size), np.uint8)
    orc.reset_obs(rec, frame)  # sets the reset tile, as the reset render does
    compare_reset(ep, view, dev, view.i("TILE"))
    for t in range(ep.n_steps):
        cause = orc.step_one(rec, ep.action(t), None)
        compare_step(ep, t, view, cause, dev)
    assert view.i("TERM") == 1, (ep.name, "the recorded episode ends on its last step")
    compare_summary(ep, summary_of(view), view.i("CAUSE"), dev)


def test_fixture_is_data_only_and_small():
    import os
    fx = EF.load()  # np.load(allow_pickle=False), json
    size = sum(os.path.getsize(os.path.join(EF.GOLDEN, f)) for f in ("episodes.npz", "episodes.json"))
    assert size < 1_000_000, size
    assert all(a.dtype != object for a in fx.arrays.values())
    assert fx.meta["tie"] == 1e-6 and fx.meta["rejected_episodes"] >= 0
    assert 30 <= len(fx.episodes) <= 40


def test_fixture_covers_every_required_case():
    """Counted from the fixture, as the generator counted before it wrote."""
    cov = EF.coverage(EF.load())
    print("\n", cov)
    for k in EF.REQUIRED:
        assert cov[k] >= 1, (k, "is not reached by any recorded episode")
    assert all(ep.terminated[-1] == 1 for ep in EF.load().episodes)


def test_oracle_replays_every_episode():
    """Every episode, every step, nothing skipped: integers exact, floats within BOUND."""
    fx, dev, steps = EF.load(), Deviation(), 0
    for ep in fx.episodes:
        replay(ep, dev)
        steps += ep.n_steps
    print(f"\n{len(fx.episodes)} episodes, {steps} steps, 0 excluded; largest deviations (abs, rel):",
          {k: (f"{a:.3e}", f"{r:.3e}") for k, (a, r) in dev.seen.items()})
    assert steps == int(fx.arrays["step_off"][-1])
