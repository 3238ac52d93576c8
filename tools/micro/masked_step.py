"""The masked step measured: cbev_step_masked at active fractions 1.0, 0.5, 0.1
and 0.0, with a random mask and with one contiguous active block, against the
plain cbev_step (the split step where the context supports it), on the same
build, the same env and the same buffers.

Configs 2 and 3 of bench.py (their envs, caps, scenes and bank), all in one
process. Per config: 20 warm-up steps of every variant, then 5 turns; a turn
times STEPS calls of the plain step and then STEPS calls of each masked
variant, each between device synchronisations on the host clock (no resets: an
env that has terminated keeps being stepped by the plain step and by the
masked step where it is active). Reported: the median turn's us per step of
every variant, every turn's figures, the ratio to the plain step's median, and
cbev_profile's three device intervals (before the actors kernel .. after it ..
after the ego kernel .. after the raster) of one more STEPS calls.

An inactive env's frame is copied from the previous ring slot into the new one
(prev_frames != frames, as the vector env calls it). Two more variants
("sameslot", random mask, fractions 0.5 and 0.0) pass prev_frames == frames, as
a caller with one frame slot or with a resize does: nothing is copied then, which
separates the cost of the copy from the cost of the gate.

Run: python tools/micro/masked_step.py [--out PATH] [--scene-cache DIR]   (GPU)
Writes profiles/masked_step.json; exits non-zero without a GPU.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, REPO)
from carlabev_env_amd._lib import LIB_PATH, check, lib  # noqa: E402

FRACTIONS = (1.0, 0.5, 0.1, 0.0)
KINDS = ("random", "block")
SAME_SLOT_FRACTIONS = (0.5, 0.0)
CONFIGS = (2, 3)
STEPS, WARM, TURNS = 500, 20, 5


def make_mask(n, frac, kind, device):
    k = int(round(frac * n))
    m = np.zeros(n, np.uint8)
    if kind == "block":
        m[:k] = 1
    else:
        m[np.random.default_rng(7).permutation(n)[:k]] = 1
    return torch.from_numpy(m).to(device)


class Runner:
    """The two calls on the env's own records, ring and output buffers."""

    def __init__(self, env):
        self.env, self.L, self.head = env, lib(), 0
        env.flush()

    def step(self, a, mask, same_slot=False):
        env, L = self.env, self.L
        rec, rew, term, trunc, cause, info = env._p_step
        old = self.head
        if not same_slot:
            self.head = (self.head + 1) % env.F
        frames = env._p_ring + self.head * env._slot_bytes
        if mask is None:
            check(L.cbev_step(env._ctx, rec, env.num_envs, a.data_ptr(), frames, rew, term, trunc, cause, info, None),
                  "cbev_step")
        else:
            prev = env._p_ring + old * env._slot_bytes
            check(L.cbev_step_masked(env._ctx, rec, env.num_envs, a.data_ptr(), mask.data_ptr(), 1, prev, frames, rew,
                                     term, trunc, cause, info, None), "cbev_step_masked")

    def loop(self, acts, t, steps, mask, same_slot=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step(acts[t % len(acts)], mask, same_slot)
            t += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e6, t

    def profile(self, acts, t, mask, same_slot=False):
        L = self.L
        check(L.cbev_profile(self.env._ctx, 1), "profile")
        _, t = self.loop(acts, t, STEPS, mask, same_slot)
        buf, cnt = (ctypes.c_double * 3)(), ctypes.c_int64()
        check(L.cbev_profile_read(self.env._ctx, buf, ctypes.byref(cnt)), "profile_read")
        check(L.cbev_profile(self.env._ctx, 0), "profile")
        return [round(buf[i] * 1e3 / max(cnt.value, 1), 2) for i in range(3)], t


def measure(config, scenes):
    import bench
    cfgd = bench.CONFIGS[config]
    n = cfgd["envs"]
    device = torch.device("cuda", 0)
    env, _, _ = bench.build_env(cfgd, n, 0, device, "full", scenes)
    acts_np = bench.make_actions(env.params, n, 64, cfgd["act_seed"], 0)
    acts = [torch.from_numpy(acts_np[i]).to(device) for i in range(len(acts_np))]
    assert not env.resize and env.F > 1
    run = Runner(env)
    # (name, mask kind, active fraction, mask, prev_frames == frames)
    variants = [("plain", None, None, None, False)]
    variants += [(f"masked-{kind}-{frac}", kind, frac, make_mask(n, frac, kind, device), False)
                 for frac in FRACTIONS for kind in KINDS]
    variants += [(f"masked-sameslot-{frac}", "random", frac, make_mask(n, frac, "random", device), True)
                 for frac in SAME_SLOT_FRACTIONS]
    t = 0
    for _, _, _, mask, same in variants:
        _, t = run.loop(acts, t, WARM, mask, same)
    turns = {name: [] for name, *_ in variants}
    for _ in range(TURNS):
        for name, _, _, mask, same in variants:
            us, t = run.loop(acts, t, STEPS, mask, same)
            turns[name].append(round(us, 2))
    plain = statistics.median(turns["plain"])
    rows = []
    for name, kind, frac, mask, same in variants:
        us3, t = run.profile(acts, t, mask, same)
        med = statistics.median(turns[name])
        rows.append({"config": config, "envs": n, "variant": name, "mask": kind, "active_fraction": frac,
                     "prev_is_frames": same, "us_per_step": med, "over_plain": round(med / plain, 4),
                     "turns_us": turns[name], "profile_us_actors_ego_raster": us3})
        print(f"config {config} {name:22s} {med:8.2f} us  x{med / plain:.3f}  profile {us3}", flush=True)
    env.close()
    del env
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "masked_step.json"))
    ap.add_argument("--scene-cache", default=None, help="bench.py's --scene-cache directory")
    args = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        print("masked_step.py needs a GPU", file=sys.stderr)
        return 2
    import bench
    # every config's scenes first: the worker processes start before this process touches the GPU
    scenes = {c: bench.build_scene_sets(bench.CONFIGS[c], bench.CONFIGS[c]["envs"], 0, cache=args.scene_cache)
              for c in CONFIGS}
    if not torch.cuda.is_available():
        print("masked_step.py needs a GPU", file=sys.stderr)
        return 2
    res = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(LIB_PATH),
           "loop": "cbev_step / cbev_step_masked(repeat = 1) on the env's records and ring, no resets "
                   "(bench.py's scenes)",
           "steps_per_turn": STEPS, "warmup_steps": WARM, "turns": TURNS, "rows": []}
    for config in CONFIGS:
        res["rows"] += measure(config, scenes.pop(config))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
