"""Reader of the whole-episode fixture (tests/golden/episodes.npz + episodes.json,
written by tests/golden/make_golden_episodes.py from the reference's own
CarlaBEV.reset / CarlaBEV.step). No torch, no GPU, no reference tree: shared by
the generator (which counts coverage with it before it writes), the CPU test and
the GPU test.

Row 0 of an episode's per-row arrays (`act_*`, `visible`) is the reset state;
row 1 + t is the state after step t.
"""
from __future__ import annotations

import json
import os
from functools import lru_cache

import numpy as np

from carlabev_env_amd.params import fov_geometry
from carlabev_env_amd.scene_pack import ActorSpec, SceneSpec, TrafficLightSpec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Episode:
    def __init__(self, fx, e):
        A, M = fx.arrays, fx.meta
        self.index, self.meta = e, M["episodes"][e]
        self.name, self.config_name = self.meta["name"], self.meta["config"]
        self.config = M["configs"][self.config_name]
        s0, s1 = int(A["step_off"][e]), int(A["step_off"][e + 1])
        self.n_steps = s1 - s0
        self.rows = self.n_steps + 1
        self.n_actors, self.n_route = int(A["n_actors"][e]), int(A["n_route"][e])
        for k in ("hero", "hero_last", "comfort", "control", "action_f", "dist2wp", "d2g", "d2g_t1", "reward", "action_i",
                  "tidx", "tile", "collided", "actor_id_kind", "actor_id", "cause", "sticky", "terminated", "truncated",
                  "current_step", "n_actors_state"):
            setattr(self, k, A[k][s0:s1])
        a0 = int(fx.as_off[s0])
        self.as_off = fx.as_off[s0:s1 + 1] - a0
        self.actors_state = A["actors_state"][a0:int(fx.as_off[s1])]
        self.actors_state_type = A["actors_state_type"][a0:int(fx.as_off[s1])]
        r0 = int(fx.act_off[e])
        n = self.rows * self.n_actors
        self.act_state = A["act_state"][r0:r0 + n].reshape(self.rows, self.n_actors, 4)
        self.act_tidx = A["act_tidx"][r0:r0 + n].reshape(self.rows, self.n_actors)
        self.act_bstate = A["act_bstate"][r0:r0 + n].reshape(self.rows, self.n_actors)
        self.act_braking = A["act_braking"][r0:r0 + n].reshape(self.rows, self.n_actors)
        v0 = int(fx.vis_off[e])
        self.visible = fx.vis_bits[v0:v0 + self.rows * self.n_route].reshape(self.rows, self.n_route)
        self.reset_hero, self.reset_tidx = A["reset_hero"][e], int(A["reset_tidx"][e])
        self.reset_tile, self.reset_d2g = int(A["reset_tile"][e]), float(A["reset_d2g"][e])
        g0, g1 = int(A["ego_off"][e]), int(A["ego_off"][e + 1])
        self.ego_rx, self.ego_ry, self.ego_speed = A["ego_rx"][g0:g1], A["ego_ry"][g0:g1], A["ego_speed"][e]
        k0 = int(fx.sa_off[e])
        self.sa = slice(k0, k0 + self.n_actors)
        self.sa_kind, self.sa_size = A["sa_kind"][self.sa], A["sa_size"][self.sa]
        t0, t1 = int(A["tl_off"][e]), int(A["tl_off"][e + 1])
        self.tl = slice(t0, t1)
        self.summary = dict(zip(M["summary_keys"], A["summary"][e]))
        self.termination = int(A["termination"][e])
        self._fx = fx

    def actors_state_rows(self, t):
        return self.actors_state[int(self.as_off[t]):int(self.as_off[t + 1])]

    def action(self, t):
        """The recorded action of step t as orc_step / cbev_step take it."""
        if self.config["action_profile"].startswith("continuous"):
            return np.ascontiguousarray(self.action_f[t], dtype=np.float32)
        return np.asarray(self.action_i[t], dtype=np.int32)

    def scene_spec(self) -> SceneSpec:
        """The realised scene as scene_pack.pack_scene takes it."""
        A, M = self._fx.arrays, self._fx.meta
        actors = {"vehicle": [], "pedestrian": []}
        for k in range(self.sa.start, self.sa.stop):
            r0, r1 = int(A["sa_route_off"][k]), int(A["sa_route_off"][k + 1])
            beh = M["beh_names"][int(A["sa_beh"][k])]
            p0, p1 = (float(v) for v in A["sa_p"][k])
            params = {"timed_brake": {"start_brake_t": p0, "decel_mps2": p1}, "cross": {"start_delay": p0},
                      "stop_mid": {"start_delay": p0}, "yield_return": {"start_delay": p0, "yield_duration": p1},
                      "none": {}}[beh]
            kind = M["kind_names"][int(A["sa_kind"][k])]
            actors[kind].append(ActorSpec(kind=kind, rx=A["sa_rx"][r0:r1].tolist(), ry=A["sa_ry"][r0:r1].tolist(),
                                          speed_mps=float(A["sa_cruise_mps"][k]),
                                          behavior=None if beh == "none" else {"type": beh, "params": params}))
        lights = [TrafficLightSpec(x=float(A["tl_xywl"][k, 0]), y=float(A["tl_xywl"][k, 1]),
                                   orientation=M["tl_orient"][int(A["tl_orient"][k])],
                                   state=M["tl_states"][int(A["tl_state"][k])], width=float(A["tl_xywl"][k, 2]),
                                   length=float(A["tl_xywl"][k, 3])) for k in range(self.tl.start, self.tl.stop)]
        return SceneSpec(agent_rx=self.ego_rx.tolist(), agent_ry=self.ego_ry.tolist(),
                         initial_speed_mps=float(self.ego_speed[0]), target_speed_mps=float(self.ego_speed[1]),
                         vehicles=actors["vehicle"], pedestrians=actors["pedestrian"], traffic_lights=lights,
                         hero_rng_state=self.meta["hero_rng_state"], actor_rng_state=self.meta["actor_rng_state"])


class Fixture:
    def __init__(self, arrays, meta):
        self.arrays, self.meta = arrays, meta
        A = arrays
        rows = np.diff(A["step_off"]) + 1
        self.as_off = np.concatenate(([0], np.cumsum(A["n_actors_state"], dtype=np.int64)))
        self.act_off = np.concatenate(([0], np.cumsum(rows * A["n_actors"], dtype=np.int64)))
        self.vis_off = np.concatenate(([0], np.cumsum(rows * A["n_route"], dtype=np.int64)))
        self.sa_off = np.concatenate(([0], np.cumsum(A["n_actors"], dtype=np.int64)))
        self.vis_bits = np.unpackbits(A["visible"])[:int(self.vis_off[-1])]
        self.episodes = [Episode(self, e) for e in range(len(meta["episodes"]))]

    def of_config(self, config):
        return [ep for ep in self.episodes if ep.config_name == config]


@lru_cache(maxsize=None)
def load() -> Fixture:
    with np.load(os.path.join(GOLDEN, "episodes.npz"), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    with open(os.path.join(GOLDEN, "episodes.json"), encoding="utf-8") as f:
        meta = json.load(f)
    return Fixture(arrays, meta)


# ------------------------------------------------------------------ coverage
def _rect(x, y, size, pad):
    cx, cy = round(pad + x), round(pad + y)
    return cx - size // 2, cy - size // 2, size, size


def _overlap(a, b):
    return a[2] > 0 and b[2] > 0 and a[0] < b[0] + b[2] and a[1] < b[1] + b[3] and a[0] + a[2] > b[0] and a[1] + a[3] > b[1]


def coverage(fx: Fixture) -> dict:
    """What the episodes reach, counted from the recorded data alone. The two
    overlap counters restate the rects (round(pad + x) centres, integer sizes):
    coverage accounting only, no expected value comes from here."""
    M = fx.meta
    cov = dict.fromkeys(("collision_vehicle", "collision_pedestrian", "collision_tile", "success", "off_road",
                         "out_of_bounds", "max_actions_truncated", "vehicle_and_pedestrian", "target_and_actor",
                         "intermediate_target", "final_target", "carl", "shaping", "discrete", "continuous", "red_light",
                         "size128", "size256", "size64", "braking") + tuple(f"beh_{b}" for b in M["beh_names"][1:]) +
                        tuple(f"bstate_{s}" for s in M["bstate_names"]), 0)
    for ep in fx.episodes:
        c = ep.config
        shaping = c["reward_profile"].startswith("shaping")
        cov["shaping" if shaping else "carl"] += 1
        cov["continuous" if c["action_profile"].startswith("continuous") else "discrete"] += 1
        cov[f"size{c['size']}"] += 1
        cov["red_light"] += any(M["tl_states"][int(s)] == "red" for s in fx.arrays["tl_state"][ep.tl])
        for b in fx.arrays["sa_beh"][ep.sa]:
            if b:
                cov[f"beh_{M['beh_names'][int(b)]}"] += 1
        hero_w = int(32 / int(1024 / c["size"]))
        pad = fov_geometry(c["size"], 0.5, c["anchor_y"])[2]
        for t in range(ep.n_steps):
            cause, coll = M["cause_names"][int(ep.cause[t])], M["coll_names"][int(ep.collided[t])]
            if ep.terminated[t]:
                assert t == ep.n_steps - 1, (ep.name, "steps recorded past the terminal one")
                if cause == "collision":
                    cov["collision_tile" if ep.tile[t] == 0 else f"collision_{coll}"] += 1
                elif cause == "max_actions":
                    cov["max_actions_truncated"] += int(ep.truncated[t] == 1 and shaping)
                else:
                    cov[cause] += 1
            taken = np.flatnonzero((ep.visible[t] == 1) & (ep.visible[t + 1] == 0))
            cov["intermediate_target"] += bool(np.any(taken < ep.n_route - 1))
            cov["final_target"] += bool(np.any(taken == ep.n_route - 1))
            hr = _rect(ep.hero[t, 0], ep.hero[t, 1], hero_w, pad)
            hits = {int(ep.sa_kind[a]) for a in range(ep.n_actors)
                    if _overlap(hr, _rect(ep.act_state[t + 1, a, 0], ep.act_state[t + 1, a, 1], int(ep.sa_size[a]), pad))}
            cov["vehicle_and_pedestrian"] += hits == {0, 1}
            cov["target_and_actor"] += bool(len(taken)) and bool(hits)
            for a in range(ep.n_actors):
                cov[f"bstate_{M['bstate_names'][int(ep.act_bstate[t + 1, a])]}"] += 1
                cov["braking"] += int(ep.act_braking[t + 1, a])
    return cov


# every item of the list the episodes must hit (at least once each)
REQUIRED = ("collision_vehicle", "collision_pedestrian", "success", "off_road", "out_of_bounds", "max_actions_truncated",
            "vehicle_and_pedestrian", "target_and_actor", "intermediate_target", "final_target", "carl", "shaping",
            "discrete", "continuous", "red_light", "size128", "size256", "size64", "beh_timed_brake", "beh_cross",
            "beh_stop_mid", "beh_yield_return", "braking", "bstate_idle", "bstate_waiting", "bstate_entering",
            "bstate_yielding", "bstate_stalled", "bstate_crossing", "bstate_cleared", "bstate_retreating",
            "bstate_retreated")
