"""The device step on exact thresholds, against cases recorded from the reference.

The same fixture as test_ties_golden.py (tests/golden/ties.npz, recorded from the
reference's own CarlaBEV.reset / CarlaBEV.step by make_golden_ties.py: round() on
half-integers, centre distance exactly 35, rel_speed and delta_progress exactly
0, behaviour timers on the literals 0.1 k), compared with the HIP path directly,
never with the oracle, as test_gpu_episode_golden.py does for whole episodes: all
cases of one configuration run as one batch through cbev_reset and cbev_step,
size 128 with the split step and without, the rounding and distance cases at
sizes 64 and 256 as well. Only tests/golden/ is read.

Bounds: integers, flags, ids, visibility bits and behaviour states exact; float64
values within the CPU test's bound plus the suite's device-libm bar, 1e-9
relative. No case is excluded: every tie value is an exact function of authored
integers and half-integers (entities at rest on yaw 0 or pi / 2, or one step at
5 px/s), and the timers compare sums of the literal 0.1.
"""
from __future__ import annotations

import pytest

torch = pytest.importorskip("torch")

import episode_fixture as EF
from gpu_scenes import replay_on_device

pytestmark = pytest.mark.gpu

EXCLUDED = {}          # case name -> measured device value: none

# (configuration, cbev_set_split_step argument or None for the context's default)
RUNS = [("carl128", 1), ("carl128", 0), ("short128", None), ("carl256", None), ("carl64", None)]


@pytest.mark.parametrize("config,split", RUNS, ids=[f"{c}-{'default' if s is None else 'split' + str(s)}" for c, s in RUNS])
def test_device_replays_the_tie_cases(config, split):
    fx = EF.load("ties")
    eps = [ep for ep in fx.of_config(config) if ep.name not in EXCLUDED]
    n = len(eps)
    assert n >= 3 and len(EXCLUDED) * 10 <= len(fx.episodes)
    compared, dev = replay_on_device(eps, split, ends=False)  # the cases need not end
    print(f"\n{config}: {n} cases, {compared} env-steps, largest deviations (abs, rel):",
          {k: (f"{x:.3e}", f"{r:.3e}") for k, (x, r) in dev.seen.items()})
