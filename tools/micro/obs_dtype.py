"""The wire types of the semantic observation, measured: cbev_expand_obs_typed
per dtype, cbev_unpack_obs, and config 2's step() + observation loop per dtype.

Kernels: a seeded random ring of 4096 envs x 4 frames (6-class), kind 0 at
128x128 and 96x96 and kind 3 at 96x96; the dtypes alternate within the process,
each turn is 5 warm-up launches and HIP events around 100 back-to-back launches,
the median of the turns is reported. Bytes are algorithmic: the n*F*h*w ring
bytes read (kind 3 reads 3 of the frames) plus the output written; the share is
of the 8 TB/s HBM peak, as the README quotes the raster.
Unpack: one 2048 x 24 x 128x128 minibatch of bit planes to float16.
Loop: config 2's env (4096 envs, ego-only, 128x128 6-class stack) per obs_dtype,
`obs, ... = env.step(a); env.reset_terminated()` with a device scene bank,
copy_obs True and False, 20 warm-up steps and at least 2 s timed.

Run: python tools/micro/obs_dtype.py [--kernels-only] [--out PATH]   (GPU)
Writes profiles/obs_dtype_config2.json; exits non-zero without a GPU.
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
sys.path.insert(0, os.path.join(REPO, "tests"))
from carlabev_env_amd import obs_pipeline as OP  # noqa: E402
from carlabev_env_amd._lib import LIB_PATH, OBS_F16, check, lib  # noqa: E402
from carlabev_env_amd.semantics import semantic_lut  # noqa: E402

P_ = ctypes.c_void_p
HBM_PEAK = 8.0e12  # bytes/s
N, F, MODE, C = 4096, 4, "6-class", 6
LAUNCHES, WARM, TURNS = 100, 5, 5


def ptr(t):
    return P_(t.data_ptr())


def timed(fn, s):
    for _ in range(WARM):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(LAUNCHES):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / LAUNCHES  # us per launch


def kernel_shapes(ctx, s):
    L = lib()
    lut = semantic_lut(MODE)
    out = torch.empty(N * F * C * 128 * 128 * 4, dtype=torch.uint8, device="cuda")  # the largest (float32) output
    rows = []
    for (h, w), kind in (((128, 128), 0), ((96, 96), 0), ((96, 96), 3)):
        check(L.cbev_set_obs_size(ctx, h, w), "set_obs_size")
        g = torch.Generator(device="cuda").manual_seed(h * 10 + kind)
        ring = torch.randint(0, 10, (F, N, h, w), dtype=torch.uint8, device="cuda", generator=g)
        fusion = "stack" if kind == 0 else "vehicle_temporal"
        frames_read = F if kind == 0 else OP.HISTORY_FRAMES
        us = {dt: [] for dt in OP.OBS_DTYPES}
        for _ in range(TURNS):
            for code, dt in enumerate(OP.OBS_DTYPES):
                us[dt].append(timed(lambda: check(L.cbev_expand_obs_typed(
                    ctx, ptr(ring), N, F, 1, kind, C, lut.ctypes.data_as(P_), code, ptr(out), P_(s.cuda_stream)),
                    "expand_typed"), s))
        for dt in OP.OBS_DTYPES:
            shape, ndt, _, _ = OP.wire_obs_spec(MODE, fusion, F, (h, w), dt)
            nbytes = N * frames_read * h * w + N * int(np.prod(shape)) * ndt.itemsize
            med = statistics.median(us[dt])
            rows.append({"hw": [h, w], "kind": kind, "fusion": fusion, "obs_dtype": dt, "us_per_launch": round(med, 2),
                         "us_min": round(min(us[dt]), 2), "us_max": round(max(us[dt]), 2),
                         "out_bytes": N * int(np.prod(shape)) * ndt.itemsize, "algorithmic_bytes": nbytes,
                         "bytes_per_s": round(nbytes / (med * 1e-6), 0),
                         "share_of_8TBs": round(nbytes / (med * 1e-6) / HBM_PEAK, 4),
                         "vs_float32": round(med / statistics.median(us["float32"]), 4)})
            print(f"{h}x{w} kind {kind} {dt:8s} {med:9.2f} us  {nbytes / 1e9:6.3f} GB  "
                  f"{nbytes / (med * 1e-6) / 1e12:5.2f} TB/s  x{rows[-1]['vs_float32']:.3f} of float32", flush=True)
        del ring
    check(L.cbev_set_obs_size(ctx, 128, 128), "set_obs_size")
    del out
    return rows


def unpack_minibatch(ctx, s):
    L = lib()
    rows_, P = 2048 * 24, 128 * 128
    g = torch.Generator(device="cuda").manual_seed(7)
    packed = torch.randint(0, 256, (rows_, P // 8), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty((rows_, P), dtype=torch.float16, device="cuda")
    us = statistics.median(timed(lambda: check(L.cbev_unpack_obs(
        ctx, ptr(packed), rows_, P, OBS_F16, ptr(out), P_(s.cuda_stream)), "unpack"), s) for _ in range(TURNS))
    nbytes = packed.numel() + out.numel() * 2
    print(f"unpack 2048x24x128x128 -> float16 {us:9.2f} us  {nbytes / (us * 1e-6) / 1e12:5.2f} TB/s", flush=True)
    return {"minibatch": [2048, 24, 128, 128], "to": "float16", "us_per_launch": round(us, 2),
            "algorithmic_bytes": nbytes, "bytes_per_s": round(nbytes / (us * 1e-6), 0),
            "share_of_8TBs": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)}


def env_loops(seconds=2.0, warmup=20):
    import bench
    from carlabev_env_amd.vector_env import make_env
    cfgd = bench.CONFIGS[2]
    n = cfgd["envs"]
    opts = bench.scene_options(cfgd, 0)
    acts = np.random.default_rng(cfgd["act_seed"]).integers(0, 9, (64, n)).astype(np.int32)
    out = []
    for dt in OP.OBS_DTYPES:
        env = make_env({"env": bench.env_config(cfgd), "num_envs": n}, caps=cfgd["caps"], obs_dtype=dt)
        env.reset(seed=0, options=opts)
        env.attach_bank(env.build_bank([cfgd["seed0"] + k for k in range(32)], opts))
        env.auto_obs = False  # the loop takes the observation from step()
        for copy_obs in (True, False):
            env.copy_obs = copy_obs
            t = 0
            for _ in range(warmup):
                obs, *_ = env.step(acts[t % 64])
                env.reset_terminated()
                t += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps = 0
            while True:
                for _ in range(50):
                    obs, *_ = env.step(acts[t % 64])
                    env.reset_terminated()
                    t += 1
                steps += 50
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
                if el >= seconds:
                    break
            out.append({"obs_dtype": dt, "copy_obs": copy_obs, "env_steps_per_s": round(n * steps / el, 1),
                        "ms_per_step": round(el / steps * 1e3, 4), "steps": steps, "warmup": warmup,
                        "obs_bytes_per_step": obs.numel() * obs.element_size()})
            print(f"loop {dt:8s} copy_obs={copy_obs!s:5s} {out[-1]['env_steps_per_s'] / 1e6:7.2f} M env-steps/s "
                  f"{out[-1]['ms_per_step']:.4f} ms/step", flush=True)
        env.close()
        del env, obs
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true", help="skip the env loops")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "obs_dtype_config2.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("obs_dtype.py needs a GPU", file=sys.stderr)
        return 2
    from helpers import CAPS_FULL, world
    cfg, P, padded, layout, builder = world(size=128)
    L = lib()
    ctx = P_()
    check(L.cbev_create(ctypes.byref(P), ctypes.byref(CAPS_FULL.c()), 0, ctypes.byref(ctx)), "create")
    check(L.cbev_set_map(ctx, padded.ctypes.data_as(P_), padded.nbytes), "set_map")
    s = torch.cuda.current_stream()
    res = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(LIB_PATH),
           "n": N, "frames": F, "mode": MODE, "launches_per_turn": LAUNCHES, "turns": TURNS,
           "expand": kernel_shapes(ctx, s), "unpack": unpack_minibatch(ctx, s)}
    L.cbev_destroy(ctx)
    torch.cuda.empty_cache()
    if not args.kernels_only:
        res["loop"] = {"what": "config 2 env: obs, ... = env.step(a); env.reset_terminated() (device bank of 32 scenes)",
                       "rows": env_loops()}
    slower = [r for r in res["expand"] if r["obs_dtype"] != "float32" and r["vs_float32"] > 1.0]
    res["compact_no_slower_than_float32"] = not slower
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
