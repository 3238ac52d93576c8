"""Same-step autoreset measured: the loop of make_env(cfg, autoreset="same_step")
against the two forms of `step(); reset_terminated()`, and k_final_frames
beside k_reset_mask.

Loops: bench.py's config 2 env (4096 envs, its caps, start scenes and bank),
obs_dtype "float32" and "bits", copy_obs as it defaults. Per dtype two envs in
one process, a default one and a same-step one, on the same scenes and
actions; 20 warm-up steps of every loop, then 5 turns; a turn times 200 steps
of each loop between device synchronisations on the host clock:
  a   obs, ... = step(a); reset_terminated()   with auto_obs off (one expansion;
      the policy never sees a reset observation)
  b   obs_t, ... = step(a); obs_r = reset_terminated()   with auto_obs on (two
      expansions: today's only way to both observations)
  c   obs, ... = step(a)   under autoreset="same_step"
  c+  the same, and rows, ids = final_obs() every step (one synchronisation)
Reported: the median turn in env-steps/s and us per step, every turn, and the
mean number of envs that ended per step.

Kernels: after those loops, the same-step env's own ring, stash, records and
bank with its last step's term buffer as the mask (copied, so it stays the
same): cbev_final_frames and cbev_reset_masked alternate, each turn is 5
warm-up launches and HIP events around 100 back-to-back launches, median of 5.

Run: python tools/micro/autoreset.py [--out PATH] [--scene-cache DIR]   (GPU)
Writes profiles/autoreset.json; exits non-zero without a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, REPO)
from carlabev_env_amd._lib import LIB_PATH, check, lib  # noqa: E402

STEPS, WARM, TURNS = 200, 20, 5
LAUNCHES, K_WARM = 100, 5
CONFIG = 2


def make(cfgd, scenes, device, obs_dtype, autoreset):
    """bench.build_env's env (its config, caps, bank and start scenes) with a wire type and a mode."""
    import bench
    from carlabev_env_amd.vector_env import CarlaBEVVectorEnv
    host, bank = scenes
    env = CarlaBEVVectorEnv({"env": bench.env_config(cfgd), "num_envs": cfgd["envs"]}, device=device,
                            caps=cfgd["caps"], info_mode="full", obs_dtype=obs_dtype, autoreset=autoreset)
    env.attach_bank(torch.from_numpy(bank).to(device))
    env.load_scenes(torch.from_numpy(host).to(device))
    return env


def loop(env, acts, t, steps, how):
    ended = torch.zeros((), dtype=torch.int64, device=env.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        obs, _, term, _, _ = env.step(acts[t % len(acts)])
        if how in ("a", "b"):
            obs_r = env.reset_terminated()  # None under a  # noqa: F841
        elif how == "c+":
            rows, ids = env.final_obs()  # noqa: F841
        ended += term.sum()
        t += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6, t, int(ended.item()) / steps


def measure_loops(cfgd, scenes, device, obs_dtype):
    import bench
    n = cfgd["envs"]
    acts_np = bench.make_actions(bench_params(cfgd), n, 64, cfgd["act_seed"], 0)
    acts = [torch.from_numpy(acts_np[i]).to(device) for i in range(len(acts_np))]
    D = make(cfgd, scenes, device, obs_dtype, "disabled")
    A = make(cfgd, scenes, device, obs_dtype, "same_step")
    variants = [("a", D, False), ("b", D, True), ("c", A, True), ("c+", A, True)]
    t = {id(D): 0, id(A): 0}
    turns = {name: [] for name, *_ in variants}
    ended = {name: [] for name, *_ in variants}
    for turn in range(-1, TURNS):  # turn -1: the warm-up
        for name, env, auto_obs in variants:
            env.auto_obs = auto_obs
            us, t[id(env)], k = loop(env, acts, t[id(env)], WARM if turn < 0 else STEPS, name)
            if turn >= 0:
                turns[name].append(round(us, 2))
                ended[name].append(round(k, 2))
    obs_bytes = D.obs_buf.numel() * D.obs_buf.element_size()
    rows = []
    for name, *_ in variants:
        med = statistics.median(turns[name])
        rows.append({"obs_dtype": obs_dtype, "loop": name, "us_per_step": med,
                     "env_steps_per_s": round(n / (med * 1e-6), 1), "turns_us": turns[name],
                     "ended_per_step": round(statistics.mean(ended[name]), 2), "obs_bytes": obs_bytes})
        print(f"{obs_dtype:8s} loop {name:2s} {med:9.2f} us/step  {n / med:7.2f} M env-steps/s  "
              f"{rows[-1]['ended_per_step']:.1f} ended/step", flush=True)
    return rows, D, A


def bench_params(cfgd):
    import bench
    from carlabev_env_amd.params import build_params, load_class_map
    cfg = bench.env_config(cfgd)
    return build_params(cfg, load_class_map(cfg.map_name, cfg.size))


def timed(fn, s):
    for _ in range(K_WARM):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(LAUNCHES):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / LAUNCHES  # us per launch


def measure_kernels(A):
    """cbev_final_frames and cbev_reset_masked on the same-step env's buffers with one mask."""
    L = lib()
    s = torch.cuda.current_stream()
    mask = A.term.clone()
    k = int((mask != 0).sum().item())
    n, F, (h, w), B = A.num_envs, A.F, A.obs_hw, A.bank.shape[0]
    stream = A._stream()

    def final():
        check(L.cbev_final_frames(A._ctx, A._p_ring, n, F, A.head, None, mask.data_ptr(), A._final.data_ptr(),
                                  A._final_env.data_ptr(), A._final_count.data_ptr(), stream), "cbev_final_frames")

    def reset():
        check(L.cbev_reset_masked(A._ctx, A._p_step[0], n, mask.data_ptr(), A._p_bank, B, A._p_bank_frames, A._p_ring,
                                  F, stream), "cbev_reset_masked")

    us = {"final": [], "reset": []}
    for _ in range(TURNS):
        us["final"].append(timed(final, s))
        us["reset"].append(timed(reset, s))
    res = {"n": n, "frames": F, "hw": [h, w], "selected": k, "launches_per_turn": LAUNCHES, "turns": TURNS,
           "k_final_frames_us": round(statistics.median(us["final"]), 2),
           "k_final_frames_min_max_us": [round(min(us["final"]), 2), round(max(us["final"]), 2)],
           "k_final_frames_bytes_read_and_written": 2 * k * F * h * w,
           "k_reset_mask_us": round(statistics.median(us["reset"]), 2),
           "k_reset_mask_min_max_us": [round(min(us["reset"]), 2), round(max(us["reset"]), 2)],
           "k_reset_mask_bytes_read_and_written": k * (2 * A.rb + (1 + F) * A.S * A.S)}
    print(f"kernels: {k} of {n} selected  k_final_frames {res['k_final_frames_us']:.2f} us  "
          f"k_reset_mask {res['k_reset_mask_us']:.2f} us", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "autoreset.json"))
    ap.add_argument("--scene-cache", default=None, help="bench.py's --scene-cache directory")
    args = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        print("autoreset.py needs a GPU", file=sys.stderr)
        return 2
    import bench
    cfgd = bench.CONFIGS[CONFIG]
    # the scenes first: the worker processes start before this process touches the GPU
    scenes = bench.build_scene_sets(cfgd, cfgd["envs"], 0, cache=args.scene_cache)
    if not torch.cuda.is_available():
        print("autoreset.py needs a GPU", file=sys.stderr)
        return 2
    device = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(LIB_PATH), "config": CONFIG,
           "envs": cfgd["envs"], "steps_per_turn": STEPS, "warmup_steps": WARM, "turns": TURNS,
           "loops": {"a": "step(); reset_terminated(), auto_obs off", "b": "step(); reset_terminated(), auto_obs on",
                     "c": "step() under autoreset='same_step'", "c+": "c and final_obs() every step"},
           "rows": []}
    for dt in ("float32", "bits"):
        rows, D, A = measure_loops(cfgd, scenes, device, dt)
        res["rows"] += rows
        if dt == "bits":
            res["kernels"] = measure_kernels(A)
        for env in (D, A):
            env.close()
        del D, A
        torch.cuda.empty_cache()
    by = {(r["obs_dtype"], r["loop"]): r["us_per_step"] for r in res["rows"]}
    res["c_below_b"] = {dt: bool(by[dt, "c"] < by[dt, "b"]) for dt in ("float32", "bits")}
    res["c_over_a"] = {dt: round(by[dt, "c"] / by[dt, "a"], 4) for dt in ("float32", "bits")}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
