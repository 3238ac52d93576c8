"""The reset preview's counters after bench.py's config-2 loop: how many reset
envs k_ego_head computed in one pass from a preview and how many in two passes
from the bank row (cbev_reset_preview_counts), over the canonical loop

    step, step_infos, reset_terminated

on bench.py's env, scenes, bank and action stream, from the seeded start
scenes. Expected: the two-pass resets are the envs that terminated in the first
step (that step folded nothing, so nothing was fetched for them) and nothing
else.

Run: python tools/micro/reset_preview_counts.py [--steps N] [--scene-cache DIR] [--out PATH]   (GPU)
Prints one JSON line; --out also writes it to a file. Exits non-zero without a GPU.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, REPO)
from carlabev_env_amd._lib import check, lib  # noqa: E402

CONFIG = 2


def counts(env):
    out = (ctypes.c_uint64 * 2)()
    check(lib().cbev_reset_preview_counts(env._ctx, out), "cbev_reset_preview_counts")
    return int(out[0]), int(out[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=220)
    ap.add_argument("--scene-cache", default=None, help="bench.py's --scene-cache directory")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        print("no GPU", file=sys.stderr)
        return 2
    import bench
    cfgd = bench.CONFIGS[CONFIG]
    n = cfgd["envs"]
    scenes = bench.build_scene_sets(cfgd, n, 0, cache=args.scene_cache)  # the workers start before the GPU is touched
    if not torch.cuda.is_available():
        print("no GPU", file=sys.stderr)
        return 2
    device = torch.device("cuda", 0)
    env, _, start_recs = bench.build_env(cfgd, n, 0, device, "full", scenes)
    acts = torch.from_numpy(bench.make_actions(env.params, n, args.steps, cfgd["act_seed"], 0)).to(device)
    env.auto_obs = False
    stream = torch.cuda.Stream(device)
    first = None
    with torch.cuda.stream(stream):
        env.load_scenes(start_recs)
        base = counts(env)
        term0 = env.termination_count()
        for t in range(args.steps):
            env.step_async_only(acts[t])
            env.step_infos()
            if t == 0:
                first = env.termination_count() - term0  # synchronises; nothing is pending here
            env.reset_terminated()
        env.flush()  # the last step's reset runs as k_reset_mask: not the head's
        torch.cuda.synchronize()
        one, two = counts(env)
        terms = env.termination_count() - term0
    res = {"config": CONFIG, "envs": n, "steps": args.steps, "one_pass": one - base[0], "two_pass": two - base[1],
           "terminations": int(terms), "terminations_first_step": int(first),
           "resets_per_step": (one - base[0] + two - base[1]) / max(args.steps - 1, 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
