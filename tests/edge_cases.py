"""Authored edge cases shared by the CPU and GPU tests (no torch, no GPU).

Every record here is packed from a hand-written SceneSpec (scene_pack.pack_scene
into a zeroed record), never from the scene generator: the states below are the
ones seeded rollouts do not produce, and size 64 must not depend on a generator
that mostly fails there.

  raster_batch     one env per (heading, position): V = 0 and action 0, so the
                   pose stays where it was put; the scene is painted relative to
                   the env's own crop origin
  reduced_world    the same matrix under a crop smaller than the reference's
                   (REDUCED_GEOMETRIES): the raster's checked output path
  many_actor_batch more than 64 actors in one crop (paint loops past thread 63)
  long_route_batch ego routes of 33-128 points, single-step placements on chosen
                   targets and "drive" envs that cross vis word boundaries
  retreat_batch    yield_return pedestrians one step before their retreat, at
                   chosen route lengths
  raster_classes   the raster's branch predicates restated (coverage accounting
                   only, never expected pixels)
"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

from carlabev_env_amd import layout as LY
from carlabev_env_amd.params import build_params, load_class_map, padded_map
from carlabev_env_amd.config import EnvConfig
from carlabev_env_amd.scene_pack import ActorSpec, SceneSpec, TrafficLightSpec, pack_scene

import raster_ref

# (size, ego_anchor_y_frac): crops 91, 119, 182, 241, 363, 399. 256 with 0.2 or
# 0.8 gives crop 482, which cbev_create refuses (crop above 400).
GEOMETRIES = ((64, 0.5), (64, 0.2), (128, 0.5), (128, 0.2), (256, 0.5), (256, 0.6))

# (size, ego_anchor_y_frac, crop, pad): crops below ceil(2 hypot(mx, my)), which
# cbev_create accepts (any crop in [size, 400]) and the vector env never builds.
# The rotated surface no longer covers the output and samples leave the crop:
# the checked output path (tile_out_check, crop_background, windows clipped by
# the crop). The centred anchors take pad = crop (the render surface rebuilt);
# those at 0.2 keep build_params's pad, so pad != crop, and their surface misses
# part of the output (black). The last one puts the anchor on the output's top
# row: near the axes the lower two of its four tiles lie wholly past the crop
# (a one-row window). With the anchor column centred the surface always spans
# the output's columns, so two more take a fifth entry, the anchor's x fraction:
# the surface ends inside the output on the right and below (0.2, 0.2), on the
# left and above (0.8, 0.8).
REDUCED_GEOMETRIES = ((64, 0.5, 64, 64), (64, 0.2, 70, 119), (128, 0.5, 128, 128), (128, 0.2, 150, 241),
                      (256, 0.5, 256, 256), (256, 0.2, 400, 482), (256, 0.0, 256, 256),
                      (128, 0.2, 150, 241, 0.2), (128, 0.8, 150, 241, 0.8))


def reduced_id(geo):
    return "-".join(str(g) for g in geo[:2]) + f"-crop{geo[2]}-pad{geo[3]}" + (f"-ax{geo[4]}" if len(geo) > 4 else "")

CAPS_RASTER = LY.Caps(128, 8, 16, 4)      # small records: a raster batch has hundreds of envs
CAPS_MANY = LY.Caps(128, 96, 288, 4)      # more than 64 actor slots
CAPS_EGO8 = LY.Caps(128, 32, 288, 4)      # k_ego stages 8 envs per workgroup
CAPS_EGO16 = LY.Caps(128, 4, 64, 4)       # 16 per workgroup: S2 / S5 loop past their prefetch
CAPS_RETREAT = (LY.Caps(128, 32, 64, 4), LY.Caps(128, 48, 64, 4), LY.Caps(128, 96, 64, 4))  # g4, narrow, wide


@lru_cache(maxsize=None)
def authored_world(size, anchor_y=0.5, reward_profile="carl_base_v1"):
    """(P, padded map, class map) of a geometry, without a scene generator."""
    cfg = EnvConfig(size=size, obs_size=(size, size), render_mode="rgb_array", action_mode="discrete",
                    action_profile_id="discrete9_v1", reward_mode="carl" if reward_profile.startswith("carl") else "shaping",
                    reward_profile_id=reward_profile, ego_anchor_y_frac=anchor_y, obs_mode="bev_semantic")
    classes = load_class_map(cfg.map_name, size)
    P = build_params(cfg, classes)
    padded, pitch = padded_map(classes, P.pad)
    assert pitch == P.map_pitch
    return P, padded, classes


@lru_cache(maxsize=None)
def reduced_world(size, anchor_y, crop, pad, anchor_x=None):
    """(P, padded map, class map) of authored_world(size, anchor_y) with a smaller
    crop: pad either stays build_params's (pad != crop, the map as it was) or
    becomes the crop, with the render surface and the padded map rebuilt.
    anchor_x: a fraction that moves the anchor column off the centre as well."""
    P0, padded, classes = authored_world(size, anchor_y)
    P = type(P0).from_buffer_copy(P0)
    assert size <= crop < P0.crop and pad in (crop, P0.pad)
    P.crop = crop
    if anchor_x is not None:
        P.anchor_x = int(round((size - 1) * anchor_x))
    if pad != P0.pad:
        P.pad = pad
        P.render_w, P.render_h = P.map_w + 2 * pad, P.map_h + 2 * pad
        padded, P.map_pitch = padded_map(classes, pad)
    return P, padded, classes


def pack_records(specs, size, caps):
    """One zeroed record per SceneSpec, packed; (recs, layout, views)."""
    layout = LY.Layout.make(caps)
    recs = np.zeros((len(specs), layout.record_bytes), np.uint8)
    views = [LY.RecordView(recs[e], layout) for e in range(len(specs))]
    for e, s in enumerate(specs):
        pack_scene(views[e], s, size, scene_id=e)
    return recs, layout, views


def set_pose(view, x, y, yaw, v=0.0):
    hd = view.hd
    hd[LY.HD["X"]], hd[LY.HD["Y"]], hd[LY.HD["YAW"]], hd[LY.HD["V"]] = x, y, yaw, v


# ------------------------------------------------------------------ raster matrix
def _f32_ulps(a, k):
    a = np.float32(a)
    for _ in range(abs(k)):
        a = np.nextafter(a, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return a


def raster_headings(step_deg=1.5):
    """float32 render angles a (the hero's yaw is radians(a - 90)): the grid, every
    axis and diagonal at 0, +-1 and +-2 float32 ulps, every axis +- small offsets."""
    out = [np.float32(-180.0 + step_deg * i) for i in range(int(round(360.0 / step_deg)) + 1)]
    for a in (-180.0, -90.0, 0.0, 90.0, 180.0, -135.0, -45.0, 45.0, 135.0):
        out += [_f32_ulps(a, k) for k in (0, 1, -1, 2, -2)]
    for a in (-180.0, -90.0, 0.0, 90.0, 180.0):
        for d in (1e-5, 1e-3, 0.01, 0.1, 0.5):
            out += [np.float32(a + d), np.float32(a - d)]
    return out


def raster_positions(P, mirrored=False):
    """World positions (x, y): mid-map and its offsets (xmin & 3 takes all four
    values), the map's corners, and one point 5 texels past where the crop
    origin starts to clamp on both axes (at 0 in x and at its maximum in y; with
    pad = crop that is more than crop / 2 outside the map). mirrored: also the
    opposite point (the maximum in x, 0 in y), so both clamps of both axes, and
    the last rows and columns of the byte maps, are staged."""
    mx, my = P.map_w // 2 + 0.0, P.map_h // 2 + 0.0
    lo, hi = P.crop / 2.0 - P.pad - 5.0, P.pad - P.crop / 2.0 + 5.0
    pos = [(mx, my), (mx + 1, my + 2), (mx + 2, my + 3), (mx + 3.5, my + 0.5), (3.0, 3.0),
           (P.map_w - 2.0, P.map_h - 2.0), (lo, P.map_h + hi)]
    return pos + [(P.map_w + hi, lo)] if mirrored else pos


def _serpentine(n, C):
    """n distinct integer crop points, consecutive ones adjacent, spread over the crop."""
    per = 16
    sx, sy = max(2, (C - 16) // per), max(2, (C - 16) // ((n + per - 1) // per))
    pts = []
    for i in range(n):
        r, c = divmod(i, per)
        c = c if r % 2 == 0 else per - 1 - c
        pts.append((8 + sx * c, 8 + sy * r))
    return pts


def _light(rx, ry, w, h, state):
    """A light whose painted rect is exactly (rx, ry, w, h) in padded-map texels."""
    return TrafficLightSpec(x=rx + w / 2.0, y=ry + h / 2.0, orientation="horizontal", state=state, width=float(h),
                            length=float(w))


def _still(kind, wx, wy):
    """An actor standing at world (wx, wy): a two-point route, speed 0, no jitter."""
    return ActorSpec(kind=kind, rx=[wx, wx + 2.0], ry=[wy, wy], speed_mps=0.0, jitter=False)


def painted_scene(P, xm, ym, k=0):
    """A scene placed relative to the crop origin (xm, ym) (padded-map texels).
    Draw order is vehicles, pedestrians, targets, lights; later wins.
      vehicle 0 covers crop texel (0, 0); pedestrian 0 lies partly over it, and
        over (0, 0) too in every other env
      vehicles straddle the crop's right and bottom edges; one vehicle and one
        pedestrian near the centre
      a 128-point ego route over the crop (every fifth target bit is cleared by
        the caller)
      lights: one over crop (0, 0) (moved one texel right in every fourth env, so
        the background there is the actor's colour, not the light's), two
        overlapping with different colours, one straddling the top edge"""
    C, pad = P.crop, P.pad
    w = lambda cx, cy: (xm + cx - pad + 0.0, ym + cy - pad + 0.0)  # noqa: E731  crop texel -> world
    veh = [_still("vehicle", *w(1, 1)),              # rect crop [-1, 3) x [-1, 3)
           _still("vehicle", *w(C, C // 2 + 9)),     # straddles the right edge
           _still("vehicle", *w(C // 3, C)),         # straddles the bottom edge
           _still("vehicle", *w(C // 2 + 7, C // 2 - 6))]
    ped = [_still("pedestrian", *(w(1, 1) if k % 2 else w(3, 3))),  # rect [0, 2)^2 or [2, 4)^2
           _still("pedestrian", *w(C // 2 - 9, C // 2 + 5))]
    route = _serpentine(128, C)
    lx = 1 if k % 4 == 3 else -1
    pair = (("green", "yellow"), ("yellow", "red"), ("red", "green"))[k % 3]
    lights = [_light(xm + lx, ym - 1, 6, 3, "red"),
              _light(xm + C // 2 + 8, ym + C // 2 - 12, 9, 4, pair[0]),
              _light(xm + C // 2 + 12, ym + C // 2 - 14, 4, 9, pair[1]),
              _light(xm + 2 * C // 3, ym - 2, 3, 7, "yellow")]
    return SceneSpec(agent_rx=[xm + p[0] - pad for p in route], agent_ry=[ym + p[1] - pad for p in route],
                     vehicles=veh, pedestrians=ped, traffic_lights=lights, hero_jitter_seed=k, actor_jitter_seed=k)


def clear_every_fifth_target(view):
    for i in range(0, view.i("NROUTE"), 5):
        view.vis[i >> 5] &= np.uint32(~(1 << (i & 31)) & 0xFFFFFFFF)


def raster_cases(P, step_deg=1.5, mirrored=False):
    """(angle, x, y) per env: all headings at the first position, every fifth at the others."""
    heads, pos = raster_headings(step_deg), raster_positions(P, mirrored)
    cases = [(a, *pos[0]) for a in heads]
    for p in pos[1:]:
        cases += [(a, *p) for a in heads[::5]]
    return cases


def yaw_of_angle(a):
    """The yaw whose render angle (float)(degrees(yaw) + 90) is the float32 a."""
    return math.radians(float(a) - 90.0)


def raster_step_deg(size):
    """The heading grid: 1.5 degrees, 3 at size 256 (its oracle frames cost four times as much)."""
    return 3.0 if size >= 256 else 1.5


def reduced_step_deg(size):
    """The reduced-crop geometries' heading grid: 6 degrees, 12 at size 256."""
    return 12.0 if size >= 256 else 6.0


def raster_batch(size, anchor_y, step_deg=None, world=None):
    """(P, padded, caps, recs, layout, acts): the raster matrix of one geometry.
    acts: action 0 (nothing pressed), then gas. world: the (P, padded map) of a
    reduced-crop geometry (reduced_world) instead of authored_world's; its matrix
    takes the coarser grid and the mirrored clamp position as well."""
    P, padded = authored_world(size, anchor_y)[:2] if world is None else world
    if step_deg is None:
        step_deg = raster_step_deg(size) if world is None else reduced_step_deg(size)
    cases = raster_cases(P, step_deg, mirrored=world is not None)
    specs = []
    for k, (a, x, y) in enumerate(cases):
        xm, ym = raster_ref.crop_origin(P, x, y)
        specs.append(painted_scene(P, xm, ym, k))
    recs, layout, views = pack_records(specs, size, CAPS_RASTER)
    for v, (a, x, y) in zip(views, cases):
        assert v.i("NROUTE") == 128
        set_pose(v, x, y, yaw_of_angle(a))
        clear_every_fifth_target(v)
    acts = np.zeros((2, len(cases)), np.int32)
    acts[1] = 1
    return P, padded, CAPS_RASTER, recs, layout, acts


def many_actor_batch():
    """Size 128, one env per heading: 70 vehicles and 10 pedestrians inside one crop."""
    P, padded, _ = authored_world(128, 0.5)
    C, pad = P.crop, P.pad
    x, y = P.map_w // 2 + 1.0, P.map_h // 2 + 2.0
    xm, ym = raster_ref.crop_origin(P, x, y)
    w = lambda cx, cy: (xm + cx - pad + 0.0, ym + cy - pad + 0.0)  # noqa: E731
    veh = [_still("vehicle", *w(6 + 17 * (i % 10) + (i // 10), 5 + 24 * (i // 10) + 2 * (i % 10))) for i in range(70)]
    # pedestrians: some over the last vehicles (painted past thread 63), some alone
    ped = [_still("pedestrian", *w(6 + 17 * (i % 10) + 6 + (i % 3), 5 + 24 * 6 + 2 * (i % 10) + (i % 2))) for i in range(10)]
    route = _serpentine(128, C)
    spec = SceneSpec(agent_rx=[xm + p[0] - pad for p in route], agent_ry=[ym + p[1] - pad for p in route],
                     vehicles=veh, pedestrians=ped, traffic_lights=[_light(xm + 20, ym + 30, 8, 5, "red")],
                     hero_jitter_seed=1, actor_jitter_seed=1)
    angles = [np.float32(a) for a in (0.0, 90.0, 33.0, 121.5, -47.0, 200.25, 45.0, 179.5)]
    recs, layout, views = pack_records([spec] * len(angles), 128, CAPS_MANY)
    for v, a in zip(views, angles):
        assert v.i("NACT") == 80 and v.i("NVEH") == 70
        set_pose(v, x, y, yaw_of_angle(a))
        clear_every_fifth_target(v)
    acts = np.zeros((2, len(angles)), np.int32)
    acts[1] = 1
    return P, padded, CAPS_MANY, recs, layout, acts


# ------------------------------------------------------------------ raster branch classes
def _rot_setup(P, angle):
    """cbev.hip rot_setup + raster8_affine: (r90, nx, ny, isin, icos, dx00, dy00, rx0, ry0)."""
    C = P.crop
    angle = np.float32(angle)
    q = float(angle) / 90.0
    r90 = q == math.floor(q)
    if r90:
        k = int(math.fmod(math.trunc(int(angle) / 90), 4))
        k += 4 if k < 0 else 0
        isin, icos = ((0, 65536), (65536, 0), (0, -65536), (-65536, 0))[k]
        ac, ar = ((0, 0), (C - 1, 0), (C - 1, C - 1), (0, C - 1))[k]
        nx = ny = C
        dx00, dy00 = (ac << 16) + 0x8000, (ar << 16) + 0x8000
    else:
        rad = float(angle) * .01745329251994329
        s, c = math.sin(rad), math.cos(rad)
        cx, cy, sx, sy = c * C, c * C, s * C, s * C
        nx = int(max(abs(cx + sy), abs(cx - sy), abs(-cx + sy), abs(-cx - sy)))
        ny = int(max(abs(sx + cy), abs(sx - cy), abs(-sx + cy), abs(-sx - cy)))
        icy = ny // 2
        xd, yd = (C - nx) * 32768, (C - ny) * 32768
        isin, icos = int(s * 65536), int(c * 65536)
        ax = (nx << 15) - int(c * ((nx - 1) << 15))
        ay = (ny << 15) - int(s * ((nx - 1) << 15))
        dx00, dy00 = (ax + isin * icy) + xd, (ay - icos * icy) + yd
    return r90, nx, ny, isin, icos, dx00, dy00, P.anchor_x - nx // 2, P.anchor_y - ny // 2


def tile_shape(S):
    """(TC, TR) of cbev.hip Tiles (tile_cols, tile_rows): 64 x 64 at size 64, 128 x 128 at 128 and 256."""
    return (S if S < 128 else 128), (64 if S <= 64 else 128)


def raster_classes(P, x, y, yaw, NT=256):
    """The branch classes of the step raster of pose (x, y, yaw), one dict per tile
    (cbev.hip rot_setup, raster_fast, tile_window, stage_tile). Coverage accounting
    only: no expected pixel comes from here."""
    S, C = P.size, P.crop
    angle = np.float32(math.degrees(yaw) + 90)
    r90, nx, ny, isin, icos, dx00, dy00, rx0, ry0 = _rot_setup(P, angle)
    vmax = (C << 16) - 1

    def src(xx, yy):
        return dx00 + xx * icos - yy * isin, dy00 + xx * isin + yy * icos

    full = rx0 <= 0 and ry0 <= 0 and rx0 + nx >= S and ry0 + ny >= S
    fast = full
    if full and not r90:
        for c in range(4):
            dx, dy = src(((S - 1) if c & 1 else 0) - rx0, ((S - 1) if c & 2 else 0) - ry0)
            fast = fast and 0 <= dx <= vmax and 0 <= dy <= vmax
    # d_crop_origin, and whether the clamp moved it
    offx, offy = math.trunc((P.pad + x) + (-C / 2.0)), math.trunc((P.pad + y) + (-C / 2.0))
    ux, uy = int(round(offx + C / 2.0)) - C // 2, int(round(offy + C / 2.0)) - C // 2
    xmin, ymin = raster_ref.crop_origin(P, x, y)
    clamped = (ux, uy) != (xmin, ymin)
    TC, TR = tile_shape(S)
    out = []
    for oy0 in range(0, S, TR):
        for ox0 in range(0, S, TC):
            xs, ys, outside = [], [], False
            for c in range(4):
                dx, dy = src(ox0 + ((TC - 1) if c & 1 else 0) - rx0, oy0 + ((TR - 1) if c & 2 else 0) - ry0)
                outside = outside or not (0 <= dx <= vmax and 0 <= dy <= vmax)
                xs.append(dx >> 16)
                ys.append(dy >> 16)
            clipped = min(xs) < 0 or min(ys) < 0 or max(xs) > C - 1 or max(ys) > C - 1
            # the whole tile lies past one side of the crop: tile_window clamps it to one row or column of texels
            no_texel = max(xs) < 0 or max(ys) < 0 or min(xs) > C - 1 or min(ys) > C - 1
            xl, yl = min(max(min(xs), 0), C - 1), min(max(min(ys), 0), C - 1)
            xh, yh = max(min(max(xs), C - 1), xl), max(min(max(ys), C - 1), yl)
            tr = abs(isin) > abs(icos)
            ul, uh = (yl, yh) if tr else (xl, xh)
            umin = ymin if tr else xmin
            nv = ((xh - xl) if tr else (yh - yl)) + 1
            ushift = umin & 3
            c0 = (ushift + ul) >> 4
            nc = ((ushift + uh) >> 4) - c0 + 1
            dr = NT // nc
            off = dict(off_left=ox0 - rx0 < 0, off_right=ox0 + TC - 1 - rx0 >= nx, off_top=oy0 - ry0 < 0,
                       off_bottom=oy0 + TR - 1 - ry0 >= ny)  # the side of the rotated surface the tile passes
            off_surface = any(off.values())
            out.append(dict(r90=r90, near_axis=(not r90) and (isin == 0 or icos == 0), transposed=tr, fast=fast,
                            ushift=ushift, nc=nc, nv=nv, leftover=NT % nc != 0, passes_gt4=(nv + dr - 1) // dr > 4,
                            clipped=clipped, outside=outside, no_texel=no_texel, off_surface=off_surface, clamped=clamped,
                            lds=nv * (16 * nc + 4), **off))
    return out


def class_labels(tile):
    """The named classes one tile counts towards."""
    t = tile
    return ["r90" if t["r90"] else "near_axis" if t["near_axis"] else "general",
            "transposed" if t["transposed"] else "upright",
            "fast" if t["fast"] else "check",
            f"ushift{t['ushift']}",
            "nc_leftover" if t["leftover"] else "nc_divides",
            "passes_gt4" if t["passes_gt4"] else "passes_le4",
            "clipped" if t["clipped"] else "unclipped",
            "outside" if t["outside"] else "inside",
            "no_texel" if t["no_texel"] else "some_texel",
            "off_surface" if t["off_surface"] else "on_surface",
            "clamped" if t["clamped"] else "unclamped"] + [k for k in OFF_SIDES if t[k]]


OFF_SIDES = ("off_left", "off_right", "off_top", "off_bottom")
ALL_CLASSES = ("r90", "near_axis", "general", "transposed", "upright", "fast", "check", "ushift0", "ushift1", "ushift2",
               "ushift3", "nc_leftover", "nc_divides", "passes_gt4", "passes_le4", "clipped", "unclipped", "outside",
               "inside", "no_texel", "some_texel", "off_surface", "on_surface", "clamped", "unclamped") + OFF_SIDES


# ------------------------------------------------------------------ long ego routes
LONG_ROUTE_LENGTHS = (33, 64, 65, 127, 128)
PLACE_INDICES = (0, 31, 32, 63, 64, 70, -1)
PLACE_HEADINGS_DEG = (0.0, 90.0, 180.0, -90.0, 45.0, -170.0)
DRIVE_STARTS = (20, 50, 85, 100)  # 85: consumption and TIDX cross index 96 within the run
DRIVE_STEPS = 40


@lru_cache(maxsize=None)
def _road_run(size):
    """(y, x0, x1): the longest horizontal run of drivable texels on the map."""
    _, _, classes = authored_world(size)
    best = (0, 0, 0)
    for y in range(0, classes.shape[0], 2):
        d = np.concatenate(([0], (classes[y] == 1).astype(np.int8), [0]))
        edges = np.flatnonzero(np.diff(d))
        for a, b in zip(edges[::2], edges[1::2]):
            if b - a > best[2] - best[1]:
                best = (y, int(a), int(b))
    return best


def long_route_spec(n, size=128, seed=0):
    """An n-point ego route along the map's longest straight road, 3 texels a
    point (2 or 1 where the road is shorter), weaving one texel every 8 points."""
    y, x0, x1 = _road_run(size)
    sp = max(1, min(3, (x1 - x0 - 8) // (n - 1)))
    rx = [x0 + 4 + sp * i for i in range(n)]
    ry = [y + ((i // 8) % 2) for i in range(n)]
    return SceneSpec(agent_rx=rx, agent_ry=ry, initial_speed_mps=0.0, hero_jitter_seed=seed, actor_jitter_seed=seed,
                     vehicles=[_still("vehicle", rx[n // 2] + 0.0, ry[n // 2] + 9.0)],
                     pedestrians=[_still("pedestrian", rx[n // 3] + 0.0, ry[n // 3] - 7.0)])


def long_route_batch(caps, size=128):
    """(P, padded, caps, recs, layout, acts, n_place): single-step placements
    first (they are stepped with the drive envs, which is harmless), then the
    drive envs. acts: gas for DRIVE_STEPS steps."""
    P, padded, _ = authored_world(size)
    specs, edits = [], []
    for n in LONG_ROUTE_LENGTHS:
        for idx in PLACE_INDICES:
            i = n - 1 if idx < 0 else idx
            if i >= n:
                continue
            for h, deg in enumerate(PLACE_HEADINGS_DEG):
                specs.append(long_route_spec(n, size, seed=len(specs)))
                edits.append((i, math.radians(deg), 0.0, h % 2 == 0))
    n_place = len(specs)
    for n in LONG_ROUTE_LENGTHS:
        for i in DRIVE_STARTS:
            if i < n - 1:
                specs.append(long_route_spec(n, size, seed=len(specs)))
                edits.append((i, None, 30.0, True))
    recs, layout, views = pack_records(specs, size, caps)
    for v, (i, yaw, vel, set_tidx) in zip(views, edits):
        assert v.i("NROUTE") == len(np.flatnonzero(v.raw_cum)) + 1  # no point was dropped as a duplicate
        set_pose(v, v.cx[i], v.cy[i], v.cyaw[i] if yaw is None else yaw, vel)
        if set_tidx:
            v.hi[LY.HI["TIDX"]] = i
    acts = np.ones((DRIVE_STEPS, len(specs)), np.int32)
    return P, padded, caps, recs, layout, acts, n_place


# ------------------------------------------------------------------ retreats
# (cur, standing exactly on initial_route[cur]); NROUTE after the rebuild is cur + 2,
# except on the point: cur = 0 leaves one distinct point (the +1e-3 fallback, NROUTE 2)
RETREAT_CASES = ((0, False), (0, True)) + tuple((c, False) for c in range(1, 12)) + ((30, False), (61, False), (62, False))
RETREAT_DEDUP = (4, True)   # NRX 6, NROUTE 5: the duplicate first point is dropped
RETREAT_STEPS = 31          # the retreat on step 1, then 30 steps along the rebuilt route
RETREAT_ROUTE_POINTS = 63
RETREAT_P1 = 1.0


def _retreat_ped(x0, y0):
    """A yield_return pedestrian on a gently curved 63-point route, one texel a point."""
    rx = [x0 + 0.02 * i * i for i in range(RETREAT_ROUTE_POINTS)]
    ry = [y0 + 1.0 * i for i in range(RETREAT_ROUTE_POINTS)]
    return ActorSpec(kind="pedestrian", rx=rx, ry=ry, speed_mps=1.5, jitter=False,
                     behavior={"type": "yield_return", "params": {"start_delay": 0.0, "yield_duration": RETREAT_P1}})


def retreat_batch(caps, size=128):
    """(P, padded, caps, recs, layout, acts, cases): env 0 holds the sixteen
    RETREAT_CASES pedestrians (all retreat on step 1, in one wave), then one env
    per case alone, then RETREAT_DEDUP alone. cases[e] = [(slot, cur, on_point)]."""
    P, padded, _ = authored_world(size)
    y, x0, x1 = _road_run(size)
    ex, ey = x0 + 40, y

    def spec(peds, seed):
        return SceneSpec(agent_rx=[ex + 4 * i for i in range(8)], agent_ry=[ey] * 8, hero_jitter_seed=seed,
                         actor_jitter_seed=seed, pedestrians=peds)

    every = RETREAT_CASES + (RETREAT_DEDUP,)
    specs = [spec([_retreat_ped(ex + 12.0 + 3.0 * k, ey - 20.0) for k in range(len(RETREAT_CASES))], 0)]
    cases = [[(k, c, on) for k, (c, on) in enumerate(RETREAT_CASES)]]
    for k, (c, on) in enumerate(every):
        specs.append(spec([_retreat_ped(ex + 12.0 + 3.0 * k, ey - 20.0)], 1 + k))
        cases.append([(0, c, on)])
    recs, layout, views = pack_records(specs, size, caps)
    for v, cs in zip(views, cases):
        for slot, cur, on in cs:
            v.ai[LY.AI["BSTATE"], slot] = LY.BSTATE["yielding"]
            v.ad[LY.AD["STATE_ELAPSED"], slot] = RETREAT_P1 + 1.0
            v.ad[LY.AD["ELAPSED"], slot] = RETREAT_P1 + 3.0
            v.ai[LY.AI["TIDX"], slot] = cur
            dx, dy = (0.0, 0.0) if on else (0.4, 0.3)
            v.ad[LY.AD["X"], slot] = v.aix[slot, cur] + dx
            v.ad[LY.AD["Y"], slot] = v.aiy[slot, cur] + dy
    acts = np.zeros((RETREAT_STEPS, len(specs)), np.int32)
    return P, padded, caps, recs, layout, acts, cases


def retreat_raw_route(view, slot, cur):
    """[pos] + initial_route[:cur + 1][::-1] of a record before its retreat (jaywalk.py:43-54)."""
    px = [view.ad[LY.AD["X"], slot]] + list(view.aix[slot, :cur + 1][::-1])
    py = [view.ad[LY.AD["Y"], slot]] + list(view.aiy[slot, :cur + 1][::-1])
    return np.array(px), np.array(py)
