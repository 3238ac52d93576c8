"""Per-env frame-stack heads measured: cbev_step_heads against cbev_step_masked
and the plain cbev_step, and cbev_expand_obs_heads against
cbev_expand_obs_typed, on the same build, in one process.

Step (the method of tools/micro/masked_step.py): configs 2 and 3 of bench.py
(their envs, caps and scenes). Per config: 20 warm-up steps of every variant,
then 5 turns; a turn times 500 calls of each variant between device
synchronisations on the host clock (no resets). Variants: the plain step (the
split step where the context supports it), cbev_step_masked at active fractions
1.0, 0.5, 0.1 and 0.0 (random mask; an inactive env's frame is copied from the
previous ring slot, as the "global" vector env calls it), and cbev_step_heads at
the same fractions with the same masks. Reported: the median turn's us per
step, every turn, the ratio to the plain step's median, cbev_profile's three
device intervals of 500 more calls, and for every heads row its difference to
the masked row of the same fraction beside that masked row's own max - min.

Expansion (the method of tools/micro/obs_dtype.py): a seeded random ring of
4096 envs x 4 frames (6-class), kind 0 at 128x128 and kind 3 at 96x96, every
wire type; the global-head call (head 1) and the per-env call (random heads)
alternate, each turn is 5 warm-up launches and HIP events around 100
back-to-back launches. A per-env row is allowed the global-head median plus
the global-head row's max - min.

Run: python tools/micro/stack_heads.py [--out PATH] [--scene-cache DIR] [--configs 2,3]   (GPU)
Writes profiles/stack_heads.json; exits non-zero without a GPU.
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
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from carlabev_env_amd import obs_pipeline as OP  # noqa: E402
from carlabev_env_amd._lib import LIB_PATH, check, lib  # noqa: E402
from carlabev_env_amd.semantics import semantic_lut  # noqa: E402
from masked_step import make_mask  # noqa: E402

P_ = ctypes.c_void_p
FRACTIONS = (1.0, 0.5, 0.1, 0.0)
STEPS, WARM, TURNS = 500, 20, 5
N, F, MODE, C = 4096, 4, "6-class", 6
LAUNCHES, EXP_WARM = 100, 5


class Runner:
    """The three calls on the env's own records, ring and output buffers."""

    def __init__(self, env):
        self.env, self.L, self.head = env, lib(), 0
        self.heads = torch.zeros(env.num_envs, dtype=torch.uint8, device=env.device)
        env.flush()

    def step(self, a, how, mask):
        env, L = self.env, self.L
        rec, rew, term, trunc, cause, info = env._p_step
        if how == "heads":
            check(L.cbev_step_heads(env._ctx, rec, env.num_envs, a.data_ptr(), mask.data_ptr(), 1, env._p_ring, env.F,
                                    self.heads.data_ptr(), rew, term, trunc, cause, info, None), "cbev_step_heads")
            return
        old = self.head
        self.head = (self.head + 1) % env.F
        frames = env._p_ring + self.head * env._slot_bytes
        if how == "plain":
            check(L.cbev_step(env._ctx, rec, env.num_envs, a.data_ptr(), frames, rew, term, trunc, cause, info, None),
                  "cbev_step")
        else:
            prev = env._p_ring + old * env._slot_bytes
            check(L.cbev_step_masked(env._ctx, rec, env.num_envs, a.data_ptr(), mask.data_ptr(), 1, prev, frames, rew,
                                     term, trunc, cause, info, None), "cbev_step_masked")

    def loop(self, acts, t, steps, how, mask):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step(acts[t % len(acts)], how, mask)
            t += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e6, t

    def profile(self, acts, t, how, mask):
        L = self.L
        check(L.cbev_profile(self.env._ctx, 1), "profile")
        _, t = self.loop(acts, t, STEPS, how, mask)
        buf, cnt = (ctypes.c_double * 3)(), ctypes.c_int64()
        check(L.cbev_profile_read(self.env._ctx, buf, ctypes.byref(cnt)), "profile_read")
        check(L.cbev_profile(self.env._ctx, 0), "profile")
        return [round(buf[i] * 1e3 / max(cnt.value, 1), 2) for i in range(3)], t


def measure_step(config, scenes):
    import bench
    cfgd = bench.CONFIGS[config]
    n = cfgd["envs"]
    device = torch.device("cuda", 0)
    env, _, _ = bench.build_env(cfgd, n, 0, device, "full", scenes)
    acts_np = bench.make_actions(env.params, n, 64, cfgd["act_seed"], 0)
    acts = [torch.from_numpy(acts_np[i]).to(device) for i in range(len(acts_np))]
    assert not env.resize and env.F > 1
    run = Runner(env)
    masks = {frac: make_mask(n, frac, "random", device) for frac in FRACTIONS}
    variants = [("plain", "plain", None)]
    variants += [(f"masked-{frac}", "masked", frac) for frac in FRACTIONS]
    variants += [(f"heads-{frac}", "heads", frac) for frac in FRACTIONS]
    t = 0
    for _, how, frac in variants:
        _, t = run.loop(acts, t, WARM, how, masks.get(frac))
    turns = {name: [] for name, *_ in variants}
    for _ in range(TURNS):
        for name, how, frac in variants:
            us, t = run.loop(acts, t, STEPS, how, masks.get(frac))
            turns[name].append(round(us, 2))
    plain = statistics.median(turns["plain"])
    rows = []
    for name, how, frac in variants:
        us3, t = run.profile(acts, t, how, masks.get(frac))
        med = statistics.median(turns[name])
        row = {"config": config, "envs": n, "variant": name, "call": how, "active_fraction": frac, "us_per_step": med,
               "over_plain": round(med / plain, 4), "turns_us": turns[name], "profile_us_actors_ego_raster": us3}
        if how == "heads":
            m = turns[f"masked-{frac}"]
            row["minus_masked_us"] = round(med - statistics.median(m), 2)
            row["masked_max_minus_min_us"] = round(max(m) - min(m), 2)
        rows.append(row)
        print(f"config {config} {name:12s} {med:8.2f} us  x{med / plain:.3f}  profile {us3}", flush=True)
    env.close()
    del env
    torch.cuda.empty_cache()
    return rows


def timed(fn, s):
    for _ in range(EXP_WARM):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(LAUNCHES):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / LAUNCHES  # us per launch


def measure_expand():
    from helpers import CAPS_FULL, world
    cfg, P, padded, layout, builder = world(size=128)
    L = lib()
    ctx = P_()
    check(L.cbev_create(ctypes.byref(P), ctypes.byref(CAPS_FULL.c()), 0, ctypes.byref(ctx)), "create")
    check(L.cbev_set_map(ctx, padded.ctypes.data_as(P_), padded.nbytes), "set_map")
    s = torch.cuda.current_stream()
    sp = P_(s.cuda_stream)
    lut = semantic_lut(MODE).ctypes.data_as(P_)
    out = torch.empty(N * F * C * 128 * 128 * 4, dtype=torch.uint8, device="cuda")  # the largest (float32) output
    rows = []
    for (h, w), kind in (((128, 128), 0), ((96, 96), 3)):
        check(L.cbev_set_obs_size(ctx, h, w), "set_obs_size")
        g = torch.Generator(device="cuda").manual_seed(h * 10 + kind)
        ring = torch.randint(0, 10, (F, N, h, w), dtype=torch.uint8, device="cuda", generator=g)
        heads = torch.randint(0, F, (N,), dtype=torch.uint8, device="cuda", generator=g)
        rp, hp, op = P_(ring.data_ptr()), P_(heads.data_ptr()), P_(out.data_ptr())
        us = {(dt, pe): [] for dt in OP.OBS_DTYPES for pe in (False, True)}
        for _ in range(TURNS):
            for code, dt in enumerate(OP.OBS_DTYPES):
                us[dt, False].append(timed(lambda: check(L.cbev_expand_obs_typed(
                    ctx, rp, N, F, 1, kind, C, lut, code, op, sp), "expand_typed"), s))
                us[dt, True].append(timed(lambda: check(L.cbev_expand_obs_heads(
                    ctx, rp, N, F, hp, kind, C, lut, code, op, sp), "expand_heads"), s))
        for dt in OP.OBS_DTYPES:
            g_, p_ = us[dt, False], us[dt, True]
            gm, pm = statistics.median(g_), statistics.median(p_)
            allow = gm + (max(g_) - min(g_))  # the reference row's own spread
            rows.append({"hw": [h, w], "kind": kind, "obs_dtype": dt, "global_us": round(gm, 2),
                         "global_min_max_us": [round(min(g_), 2), round(max(g_), 2)], "per_env_us": round(pm, 2),
                         "per_env_min_max_us": [round(min(p_), 2), round(max(p_), 2)],
                         "allowance_us": round(allow, 2), "within_allowance": bool(pm <= allow)})
            print(f"{h}x{w} kind {kind} {dt:8s} global {gm:9.2f} us  per-env {pm:9.2f} us  allowed {allow:9.2f}",
                  flush=True)
        del ring
    L.cbev_destroy(ctx)
    del out
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stack_heads.json"))
    ap.add_argument("--scene-cache", default=None, help="bench.py's --scene-cache directory")
    ap.add_argument("--configs", default="2,3", help="bench configs of the step rows")
    args = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        print("stack_heads.py needs a GPU", file=sys.stderr)
        return 2
    import bench
    configs = [int(c) for c in args.configs.split(",") if c]
    # every config's scenes first: the worker processes start before this process touches the GPU
    scenes = {c: bench.build_scene_sets(bench.CONFIGS[c], bench.CONFIGS[c]["envs"], 0, cache=args.scene_cache)
              for c in configs}
    if not torch.cuda.is_available():
        print("stack_heads.py needs a GPU", file=sys.stderr)
        return 2
    res = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(LIB_PATH),
           "loop": "cbev_step / cbev_step_masked / cbev_step_heads (repeat = 1) on the env's records and ring, "
                   "no resets (bench.py's scenes)",
           "steps_per_turn": STEPS, "warmup_steps": WARM, "turns": TURNS, "step": [],
           "expand_n": N, "expand_frames": F, "expand_mode": MODE, "launches_per_turn": LAUNCHES}
    for config in configs:
        res["step"] += measure_step(config, scenes.pop(config))
    res["expand"] = measure_expand()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
