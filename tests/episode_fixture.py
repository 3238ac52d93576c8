"""Reader of the whole-episode fixture (tests/golden/episodes.npz + episodes.json,
written by tests/golden/make_golden_episodes.py from the reference's own
CarlaBEV.reset / CarlaBEV.step). No torch, no GPU, no reference tree: shared by
the generator (which counts coverage with it before it writes), the CPU test and
the GPU test; and the comparison of a record (the oracle's or the device's)
with a recorded step, which those two tests share.

Row 0 of an episode's per-row arrays (`act_*`, `visible`) is the reset state;
row 1 + t is the state after step t.
"""
from __future__ import annotations

import json
import os
from functools import lru_cache

import numpy as np

from carlabev_env_amd import layout as LY
from carlabev_env_amd.config import EnvConfig
from carlabev_env_amd.params import build_params, fov_geometry, load_class_map, padded_map
from carlabev_env_amd.scene_pack import ActorSpec, SceneSpec, TrafficLightSpec, pack_scene

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
def load(name="episodes") -> Fixture:
    """The fixture `name`: "episodes" (whole episodes) or "ties" (make_golden_ties.py:
    short authored cases on exact thresholds; they need not end)."""
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    with open(os.path.join(GOLDEN, name + ".json"), encoding="utf-8") as f:
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


# ------------------------------------------------------------------ a record against the fixture
# The one table from the fixture's names to the C-ABI constants (include/cbev_layout.h
# CBEV_CAUSE_* / CBEV_COLL_*, mirrored by layout.CAUSE / layout.COLL).
CAUSE_CODE = {None: LY.CAUSE[None], "collision": LY.CAUSE["collision"], "success": LY.CAUSE["success"],
              "ckpt": LY.CAUSE["ckpt"], "out_of_bounds": LY.CAUSE["out_of_bounds"],
              "max_actions": LY.CAUSE["max_actions"], "off_road": LY.CAUSE["off_road"], "unknown": LY.CAUSE["unknown"]}
COLL_CODE = {None: LY.COLL[None], "vehicle": LY.COLL["vehicle"], "pedestrian": LY.COLL["pedestrian"],
             "target": LY.COLL["target"]}
ACTOR_ID_NONE, ACTOR_ID_GOAL = -1, -2  # HI ACTOR_ID: -1 None, -2 "goal", else the reference's int id

# (abs, rel): 10 x the measured deviations (test_episode_golden.py's docstring), capped by the piecewise bounds
MEASURED = {"hero": (1.110e-16, 2.203e-16), "actors": (1.297e-13, 1.538e-13), "reward": (1.041e-15, 8.862e-16)}
CAP = {"hero": (1e-9, 1e-11), "actors": (1e-7, 1e-9), "reward": (1e-9, 1e-11)}
BOUND = {k: (min(10 * MEASURED[k][0], CAP[k][0]), min(10 * MEASURED[k][1], CAP[k][1])) for k in MEASURED}


def world_of(config):
    """(P, padded map) of a fixture configuration."""
    cont = config["action_profile"].startswith("continuous")
    carl = config["reward_profile"].startswith("carl")
    size = config["size"]
    cfg = EnvConfig(size=size, obs_size=(size, size), render_mode="rgb_array", action_mode="continuous" if cont else "discrete",
                    action_profile_id=config["action_profile"], reward_mode="carl" if carl else "shaping",
                    reward_profile_id=config["reward_profile"], ego_anchor_y_frac=config["anchor_y"], obs_mode="bev_semantic")
    classes = load_class_map(cfg.map_name, size)
    P = build_params(cfg, classes)
    P.max_actions = int(config["max_actions"])
    padded, pitch = padded_map(classes, P.pad)
    assert pitch == P.map_pitch
    return P, padded


def pack_episode(ep, caps=None):
    """(record, layout, caps): the episode's scene packed into a zeroed record."""
    spec = ep.scene_spec()
    if caps is None:
        caps = LY.Caps(*spec.caps_needed())
    layout = LY.Layout.make(caps)
    rec = np.zeros(layout.record_bytes, np.uint8)
    view = LY.RecordView(rec, layout)
    pack_scene(view, spec, ep.config["size"], scene_id=ep.index)
    # the scene scalars episode_info reports (carlabev.py:180-181; host_reset sets them after packing)
    view.hd[LY.HD["NUM_VEH"]] = float(len(spec.vehicles))
    view.hd[LY.HD["LEN_ROUTE_M"]] = float(ep.meta["len_ego_route"])
    return rec, layout, caps


class Deviation:
    """Compares float64 values with the fixture and keeps the largest deviations
    seen per class of value: abs where |want| < 1, rel elsewhere. libm: the
    relative bar added for device libm (the GPU test); it applies at the scale of
    the operands, which is at least 1 (positions, angles), so values below 1 in
    magnitude take it as an absolute term, as the parity suite's atol does.
    actor_yaw_mod: actor headings are compared modulo 2 pi (the GPU test; see
    gpu_scenes.angles_close for why a retreat's rebuilt route needs it)."""

    def __init__(self, libm=0.0, actor_yaw_mod=False):
        self.seen = {k: [0.0, 0.0] for k in MEASURED}
        self.libm, self.actor_yaw_mod = libm, actor_yaw_mod

    def check(self, kind, got, want, tag):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        assert got.shape == want.shape, (tag, got.shape, want.shape)
        d = np.abs(got - want)
        small = np.abs(want) < 1.0
        a = float(np.max(d[small], initial=0.0))
        r = float(np.max(d[~small] / np.abs(want[~small]), initial=0.0))
        self.seen[kind][0] = max(self.seen[kind][0], a)
        self.seen[kind][1] = max(self.seen[kind][1], r)
        atol, rtol = BOUND[kind]
        assert a <= atol + self.libm and r <= rtol + self.libm, (tag, kind, "abs", a, "rel", r, got, want)


def vis_bits(view, n):
    return np.array([(int(view.vis[i >> 5]) >> (i & 31)) & 1 for i in range(n)], np.uint8)


def want_actor_id(ep, t):
    kind = ep._fx.meta["actor_id_kinds"][int(ep.actor_id_kind[t])]
    return {"none": ACTOR_ID_NONE, "goal": ACTOR_ID_GOAL}.get(kind, int(ep.actor_id[t]))


def compare_reset(ep, view, dev, tile):
    """tile: the class under the hero at reset, or None where the record does not
    hold it yet (the device writes TILE from the first step on)."""
    dev.check("hero", view.hd[LY.HD["X"]:LY.HD["X"] + 4], ep.reset_hero, (ep.name, "reset hero"))
    assert view.i("TIDX") == ep.reset_tidx and view.i("NROUTE") == ep.n_route, (ep.name, "reset route")
    dev.check("hero", [view.h("D2G"), view.h("D2G_T1")], [ep.reset_d2g] * 2, (ep.name, "reset dist2goal"))
    assert tile is None or tile == ep.reset_tile, (ep.name, "reset tile")
    assert view.i("NACT") == ep.n_actors
    assert np.array_equal(vis_bits(view, ep.n_route), ep.visible[0]) and ep.visible[0].all(), (ep.name, "reset targets")
    compare_actors(ep, view, 0, dev)


def compare_actors(ep, view, row, dev):
    n = ep.n_actors
    if n == 0:
        return
    tag = (ep.name, row - 1, "actors")
    assert np.array_equal(view.ai[LY.AI["KIND"], :n] - 1, ep.sa_kind), tag
    assert np.array_equal(view.ai[LY.AI["SIZE"], :n], ep.sa_size), tag
    got = view.ad[LY.AD["X"]:LY.AD["X"] + 4, :n].T.copy()
    if dev.actor_yaw_mod:  # bring the heading to the recorded one's turn
        got[:, 2] -= 2 * np.pi * np.rint((got[:, 2] - ep.act_state[row, :, 2]) / (2 * np.pi))
    dev.check("actors", got, ep.act_state[row], tag)
    assert np.array_equal(view.ai[LY.AI["TIDX"], :n], ep.act_tidx[row]), tag + ("tidx",)
    names = ep._fx.meta["bstate_names"]
    want = [LY.BSTATE[names[int(b)]] for b in ep.act_bstate[row]]
    assert np.array_equal(view.ai[LY.AI["BSTATE"], :n], want), tag + ("behaviour state",)
    assert np.array_equal(view.ai[LY.AI["BRAKING"], :n], ep.act_braking[row]), tag + ("braking",)


def listed_actors(ep, t, rows):
    """The actors the reference listed in actors_state on step t: each row's position
    is one recorded actor's, and the list keeps the actor order."""
    listed = []
    for r in rows:
        hit = [a for a in range(ep.n_actors) if a not in listed and r[0] == ep.act_state[t + 1, a, 0]
               and r[1] == ep.act_state[t + 1, a, 1]]
        assert hit, (ep.name, t, "an actors_state row that is no recorded actor")
        listed.append(hit[0])
    assert listed == sorted(listed), (ep.name, t, "actors_state out of actor order")
    types = ep.actors_state_type[int(ep.as_off[t]):int(ep.as_off[t + 1])]
    assert np.array_equal(types, ep.sa_kind[listed]), (ep.name, t, "actors_state types")
    return listed


def compare_step(ep, t, view, cause, dev):
    """Everything recorded after step t against a record (the oracle's or the device's)."""
    M = ep._fx.meta
    tag = (ep.name, t)
    hd = view.hd
    dev.check("hero", hd[LY.HD["X"]:LY.HD["X"] + 4], ep.hero[t], tag + ("state",))
    dev.check("hero", hd[LY.HD["X1"]:LY.HD["X1"] + 4], ep.hero_last[t], tag + ("last_state",))
    dev.check("hero", [view.h("DIST2WP"), view.h("D2G"), view.h("D2G_T1")], [ep.dist2wp[t], ep.d2g[t], ep.d2g_t1[t]],
              tag + ("dist2wp, dist2goal, dist2goal_t_1",))
    assert view.i("TIDX") == ep.tidx[t], tag + ("target index",)
    assert view.i("TILE") == ep.tile[t], tag + ("tile",)
    assert view.i("COLLIDED") == COLL_CODE[M["coll_names"][int(ep.collided[t])]], tag + ("collided",)
    assert view.i("ACTOR_ID") == want_actor_id(ep, t), tag + ("actor_id", view.i("ACTOR_ID"))
    assert view.i("NACTSTATE") == ep.n_actors_state[t], tag + ("len(actors_state)",)
    assert np.array_equal(vis_bits(view, ep.n_route), ep.visible[t + 1]), tag + ("target visibility",)
    compare_actors(ep, view, t + 1, dev)
    # the rows of actors_state are (x, y, v cos yaw, v sin yaw) of the listed actors, in actor order: the record keeps
    # their count, the actors above pin their values, and the reward below what the reward functions made of them
    rows = ep.actors_state_rows(t)
    assert len(rows) == ep.n_actors_state[t], tag + ("actors_state rows",)
    if len(rows):
        listed = listed_actors(ep, t, rows)
        x, y, yaw, v = (view.ad[LY.AD[k], listed] for k in ("X", "Y", "YAW", "V"))
        dev.check("actors", np.stack([x, y, v * np.cos(yaw), v * np.sin(yaw)], axis=1), rows, tag + ("actors_state rows",))
    dev.check("reward", [view.h("REWARD")], [ep.reward[t]], tag + ("reward",))
    dev.check("reward", hd[LY.HD["C_SPEED"]:LY.HD["C_SPEED"] + 7], ep.comfort[t], tag + ("comfort",))
    dev.check("reward", hd[LY.HD["U_GAS"]:LY.HD["U_GAS"] + 4], ep.control[t], tag + ("control",))
    assert cause == CAUSE_CODE[M["cause_names"][int(ep.cause[t])]], tag + ("cause", cause)
    assert view.i("CAUSE") == CAUSE_CODE[M["cause_names"][int(ep.sticky[t])]], tag + ("sticky cause",)
    assert view.i("TERM") == ep.terminated[t] and view.i("TRUNC") == ep.truncated[t], tag + ("terminated, truncated",)
    assert view.i("STEP") == ep.current_step[t] == view.i("EP_LEN"), tag + ("_current_step",)


def compare_summary(ep, got, cause, dev):
    M = ep._fx.meta
    keys = [k for k in M["summary_keys"] if k in got]
    dev.check("reward", [got[k] for k in keys], [ep.summary[k] for k in keys], (ep.name, "episode_info", keys))
    assert cause == CAUSE_CODE[M["cause_names"][ep.termination]], (ep.name, "episode_info termination")
