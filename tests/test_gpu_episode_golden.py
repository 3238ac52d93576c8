"""The device step against whole-episode traces of the reference.

The same fixture as test_episode_golden.py (tests/golden/episodes.npz, recorded
from the reference's own CarlaBEV.reset / CarlaBEV.step), but the HIP path is
compared with the fixture directly, never with the oracle: an error shared by
the oracle and the kernels cannot hide here. All episodes of one configuration
run as one batch in one context (several envs share a k_ego workgroup), through
cbev_reset and cbev_step with the device episode statistics on. After every step
the device's records, reward / term / trunc / cause / info and, at an env's
terminal step, its episode summary row are compared with what the reference
recorded; an env is compared up to its terminal step and ignored afterwards.
Only tests/golden/ is read.

Bounds: integers, flags, ids, visibility bits and behaviour states exact; float64
values within the CPU test's bound plus the suite's device-libm bar, 1e-9
relative (test_gpu_parity.py). `info` is a float32 export: it is compared with
the fixture's values rounded to float32, within one float32 ulp (2^-23 relative:
two doubles 1e-9 apart round to the same float32 or to neighbours).
"""
from __future__ import annotations

import pytest

torch = pytest.importorskip("torch")

import episode_fixture as EF
from gpu_scenes import replay_on_device

pytestmark = pytest.mark.gpu

# (configuration, cbev_set_split_step argument or None for the context's default)
RUNS = [("carl128", 1), ("carl128", 0), ("shaping128c", None), ("short128", None), ("carl256", None), ("carl64", None)]


@pytest.mark.parametrize("config,split", RUNS, ids=[f"{c}-{'default' if s is None else 'split' + str(s)}" for c, s in RUNS])
def test_device_replays_the_reference_episodes(config, split):
    eps = EF.load().of_config(config)
    n = len(eps)
    assert n >= 1
    compared, dev = replay_on_device(eps, split, ends=True)
    print(f"\n{config}: {n} envs, {compared} env-steps, largest deviations (abs, rel):",
          {k: (f"{x:.3e}", f"{r:.3e}") for k, (x, r) in dev.seen.items()})
