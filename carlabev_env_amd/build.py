"""Build libcbev.so in-tree for gfx950 (`python -m carlabev_env_amd.build`)."""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "csrc", "cbev.hip")
OUT = os.path.join(HERE, "libcbev.so")
DEPS = [SRC, os.path.join(HERE, "csrc", "cbev_device.h"), os.path.join(HERE, "csrc", "cbev_expand.inc"),
        os.path.join(REPO, "include", "cbev.h"),
        os.path.join(REPO, "include", "cbev_layout.h")]

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -ffp-contract=off: hipcc contracts a*b+c into FMA by default, which changes
# rounding relative to the reference's (and the oracle's) float64 arithmetic.
# -amdgpu-kernarg-preload-count=16: the leading scalar kernel arguments (up to 16
# dwords; k_ego puts its staging scalars there) arrive in SGPRs at wave start
# instead of through a cold kernarg-segment load (cbev.hip, EgoStage).
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off",
         "-fno-fast-math", "-Wall", "-Wno-unused-function", "-mllvm", "-amdgpu-kernarg-preload-count=16",
         f"-I{os.path.join(REPO, 'include')}"]


# the host-only helpers of scene generation (libcbev_host.so: g++, no HIP, so
# spawned scene-pool workers load it without touching a GPU)
HOST_SRC = os.path.join(HERE, "csrc", "cbev_host.cpp")
HOST_OUT = os.path.join(HERE, "libcbev_host.so")
HOST_DEPS = [HOST_SRC, os.path.join(REPO, "include", "cbev_host.h")]
HOST_FLAGS = ["-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
              f"-I{os.path.join(REPO, 'include')}"]


def _stale(out, deps) -> bool:
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def needs_build() -> bool:
    return _stale(OUT, DEPS)


def build_host(force: bool = False, verbose: bool = False) -> str:
    if force or _stale(HOST_OUT, HOST_DEPS):
        cmd = [os.environ.get("CXX", "g++"), *HOST_FLAGS, "-o", HOST_OUT, HOST_SRC]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    return HOST_OUT


def build(force: bool = False, verbose: bool = False) -> str:
    if force or needs_build():
        cmd = [HIPCC, *FLAGS, "-o", OUT, SRC]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    build_host(force, verbose)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
