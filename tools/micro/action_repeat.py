"""Action repeat measured: one agent step of k substeps as cbev_step_repeat
(`action_repeat=k`: k gated ego / actor launches, one raster) against the same
agent step as k plain steps, on the same build and the same env.

Configs 2 and 3 of bench.py (their envs, caps, scenes and reset bank), k in
{1, 2, 4, 8}, all in one process. Per (config, k): 20 warm-up agent steps of
each loop, then 5 turns; a turn times AGENT_STEPS agent steps of
    env.step_async_only(a); env.step_infos(); env.reset_terminated()
with action_repeat = k, then AGENT_STEPS times k plain steps of the same loop
with action_repeat = 1 (the reset after every plain step, as a learner that
repeats the action itself runs it), each between device synchronisations on
the host clock. Reported: the median turn's us per agent step, env-substeps/s
(n * k substeps per agent step; a frozen env's skipped substeps are counted,
as the plain loop's reset envs' are), every turn's pair, and cbev_profile's
three intervals of the repeat loop (before substep 1 .. after its k_actors ..
after the last substep's ego kernel .. after k_raster).

Run: python tools/micro/action_repeat.py [--out PATH] [--scene-cache DIR]   (GPU)
Writes profiles/action_repeat.json; exits non-zero without a GPU.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, REPO)
from carlabev_env_amd._lib import LIB_PATH, check, lib  # noqa: E402

KS = (1, 2, 4, 8)
CONFIGS = (2, 3)
AGENT_STEPS, WARM, TURNS = 1000, 20, 5


def loop(env, acts, t, agent_steps, k, repeat):
    """agent_steps agent steps from action row t; returns (seconds, next t)."""
    env.action_repeat = k if repeat else 1
    inner = 1 if repeat else k
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(agent_steps):
        a = acts[t % len(acts)]
        for _ in range(inner):
            env.step_async_only(a)
            env.step_infos()
            env.reset_terminated()
        t += 1
    env.flush()  # the last reset runs inside the timed region, like every other
    torch.cuda.synchronize()
    return time.perf_counter() - t0, t


def profile_repeat(env, acts, t, k):
    L = lib()
    check(L.cbev_profile(env._ctx, 1), "profile")
    _, t = loop(env, acts, t, AGENT_STEPS, k, True)
    buf, cnt = (ctypes.c_double * 3)(), ctypes.c_int64()
    check(L.cbev_profile_read(env._ctx, buf, ctypes.byref(cnt)), "profile_read")
    check(L.cbev_profile(env._ctx, 0), "profile")
    return [round(buf[i] * 1e3 / max(cnt.value, 1), 2) for i in range(3)], t


def measure(config, scenes):
    import bench
    cfgd = bench.CONFIGS[config]
    n = cfgd["envs"]
    device = torch.device("cuda", 0)
    env, _, _ = bench.build_env(cfgd, n, 0, device, "full", scenes)
    acts_np = bench.make_actions(env.params, n, 64, cfgd["act_seed"], 0)
    acts = [torch.from_numpy(acts_np[i]).to(device) for i in range(len(acts_np))]
    rows = []
    t = 0
    for k in KS:
        for repeat in (True, False):
            _, t = loop(env, acts, t, WARM, k, repeat)
        turns = []
        for _ in range(TURNS):
            sr, t = loop(env, acts, t, AGENT_STEPS, k, True)
            sp, t = loop(env, acts, t, AGENT_STEPS, k, False)
            turns.append([round(sr / AGENT_STEPS * 1e6, 2), round(sp / AGENT_STEPS * 1e6, 2)])
        us3, t = profile_repeat(env, acts, t, k)
        rep, plain = statistics.median(x[0] for x in turns), statistics.median(x[1] for x in turns)
        rows.append({"config": config, "envs": n, "k": k, "repeat_us_per_agent_step": rep,
                     "plain_us_per_agent_step": plain, "repeat_over_plain": round(rep / plain, 4),
                     "repeat_env_substeps_per_s": round(n * k / (rep * 1e-6), 0),
                     "plain_env_substeps_per_s": round(n * k / (plain * 1e-6), 0),
                     "turns_us_repeat_plain": turns, "repeat_faster_every_turn": all(a < b for a, b in turns),
                     "profile_us_actors1_egos_raster": us3})
        print(f"config {config} k={k}: repeat {rep:8.2f} us  plain {plain:8.2f} us  x{rep / plain:.3f}  "
              f"profile {us3}", flush=True)
    env.action_repeat = 1
    env.close()
    del env
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "action_repeat.json"))
    ap.add_argument("--scene-cache", default=None, help="bench.py's --scene-cache directory")
    args = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        print("action_repeat.py needs a GPU", file=sys.stderr)
        return 2
    import bench
    # every config's scenes first: the worker processes start before this process touches the GPU
    scenes = {c: bench.build_scene_sets(bench.CONFIGS[c], bench.CONFIGS[c]["envs"], 0, cache=args.scene_cache)
              for c in CONFIGS}
    if not torch.cuda.is_available():
        print("action_repeat.py needs a GPU", file=sys.stderr)
        return 2
    res = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(LIB_PATH),
           "loop": "env.step_async_only(a); env.step_infos(); env.reset_terminated() (bench.py's scenes and bank)",
           "agent_steps_per_turn": AGENT_STEPS, "warmup_agent_steps": WARM, "turns": TURNS, "rows": []}
    for config in CONFIGS:
        res["rows"] += measure(config, scenes.pop(config))
    res["k4_repeat_faster_every_turn"] = all(r["repeat_faster_every_turn"] for r in res["rows"] if r["k"] == 4)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
