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


# ------------------------------------------------------------------ the actor target search
# calc_target_index of a scripted actor (stanley_controller.py:100-123): the
# kernel's actor_search / actor_search_win<AW> against
#     max(tid0, int(np.argmin(np.hypot(cx - fx, cy - fy))))
# in float64 NumPy (expected_tidx). Every searching actor stands still (speed 0)
# at yaw exactly 0, so a second step repeats the search from the index the
# first one chose. Its front axle is fx = x + 2.9 * cos(0) = fl(x + 2.9), fy =
# y + 2.9 * sin(0) = y: cos(0) = 1 and sin(0) = 0 exactly in every libm, 2.9 * 1
# and 2.9 * 0 are exact, and x is chosen as fl(fx - 2.9) with fl(x + 2.9) == fx
# asserted (_search_actor), so fx is the authored value with or without a fused
# multiply-add. Route coordinates lie within a factor of two of the axle's, so
# fx - cx is exact too (Sterbenz); what is left is dx * dx + dy * dy and hypot.
SEARCH_WHEELBASE = 2.9
ACTOR_NB = 18        # cbev.hip: the circles a group holds (blocks of BP points)
ACTOR_BATCH = 24     # cbev.hip: route points per lane and round of actor_search<1>
BP = LY.ACB_PTS
# g4 (32 slots; 528 points: 33 blocks, past the 32 candidate bits), narrow (64), wide (96)
CAPS_SEARCH = (LY.Caps(16, 32, 528, 1), LY.Caps(16, 64, 320, 1), LY.Caps(16, 96, 320, 1))
SEARCH_NACT = {32: (1, 2, 3, 5, 16, 17, 32), 64: (17, 33, 64), 96: (20, 40, 65, 80)}
SEARCH_F = (600.0, 500.0)
# the 20 integer lattice points at distance exactly 25
LATTICE25 = tuple((sx * a, sy * b) for a, b in ((15, 20), (20, 15), (7, 24), (24, 7)) for sx in (1, -1)
                  for sy in (1, -1)) + ((25, 0), (-25, 0), (0, 25), (0, -25))


def max_route_coordinate(size):
    """The largest coordinate of a route point on the render surface: pack_scene
    itself checks no coordinate; a point past map + pad is past the padded map's
    last texel (params.padded_map: the map blitted at (pad, pad) into a surface
    of map + 2 pad), where nothing is drawn or looked up. (x, y) limits."""
    P, _, _ = authored_world(size)
    return P.map_w + P.pad, P.map_h + P.pad


class SearchCase:
    """One actor's search: route points, front axle, previous target index."""

    def __init__(self, name, px, py, f, tid0):
        self.name, self.fx, self.fy, self.tid0 = name, float(f[0]), float(f[1]), int(tid0)
        self.px, self.py = np.asarray(px, np.float64), np.asarray(py, np.float64)
        self.n = len(self.px)
        assert self.n >= 2 and 0 <= self.tid0 <= self.n - 1

    @property
    def frozen(self):
        return self.tid0 >= self.n - 1

    def as_frozen(self):
        return SearchCase(self.name + "/frozen", self.px, self.py, (self.fx, self.fy), self.n - 1)


def expected_tidx(px, py, x, y, yaw, tid0):
    """TIDX after one Actor.step, in float64 NumPy; a frozen actor keeps its own."""
    if tid0 >= len(px) - 1:
        return int(tid0)
    fx = x + SEARCH_WHEELBASE * np.cos(yaw)
    fy = y + SEARCH_WHEELBASE * np.sin(yaw)
    return max(int(tid0), int(np.argmin(np.hypot(np.asarray(px) - fx, np.asarray(py) - fy))))


def _filler(n, f, sgn=1.0):
    """n route points far from the axle f (more than 700 px), all distances distinct."""
    j = np.arange(n)
    return f[0] + sgn * (500.0 + 2.0 * j), f[1] + sgn * (500.0 + (j % 3))


def _case(name, n, special, tid0, f=SEARCH_F, sgn=1.0):
    """A route of n filler points with the offsets special[i] = (dx, dy) from the axle at index i."""
    px, py = _filler(n, f, sgn)
    for i, (dx, dy) in special.items():
        px[i], py[i] = f[0] + dx, f[1] + dy
    return SearchCase(name, px, py, f, tid0)


@lru_cache(maxsize=None)
def near_tie_pairs(f=SEARCH_F, lim=None):
    """((near), (far)) route points whose float64 squared distances from f differ
    by 3e-14 to 1e-9 relative (above the 1e-14 band of the hypot pass and the
    one-ulp difference a fused multiply-add makes; far below float32), and whose
    float32 copies order them the other way round or not at all, with and
    without a fused multiply-add in the float32 sum. Decimal coordinates k + 0.1
    m on the circle of radius 0.5 (0.3, 0.4): equal in exact arithmetic, apart
    by the float64 rounding of the coordinates."""
    import itertools
    f32 = np.float32
    pts = sorted({(round(f[0] + sa * u, 1), round(f[1] + sb * v, 1)) for a, b in ((0.3, 0.4), (0.5, 0.0))
                  for sa in (1, -1) for sb in (1, -1) for u, v in ((a, b), (b, a))})
    if lim is not None:
        pts = [p for p in pts if p[0] <= lim[0] and p[1] <= lim[1]]

    def d64(p):
        dx, dy = f[0] - p[0], f[1] - p[1]
        return dx * dx + dy * dy

    def d32(p, fma):
        dx, dy = f32(f[0]) - f32(p[0]), f32(f[1]) - f32(p[1])
        return f32(float(dx) * float(dx) + float(f32(dy * dy))) if fma else f32(f32(dx * dx) + f32(dy * dy))

    out = []
    for p, q in itertools.combinations(pts, 2):
        a, b = d64(p), d64(q)
        if a == b or not 3e-14 <= abs(a - b) / a <= 1e-9:
            continue
        near, far = (p, q) if a < b else (q, p)
        if all(d32(near, m) >= d32(far, m) for m in (False, True)):
            out.append((near, far))
    return tuple(out)


@lru_cache(maxsize=None)
def hypot_pairs(count=4):
    """(collapsing, separate): offsets ((dx_i, dy_i), (dx_j, dy_j)) from the axle,
    multiples of 2^-18 px, with d2_j = d2_i - one ulp and both squared distances
    exact in float64: a = 2 b + 3, (a, b) and (a - 1, b + 2) give a^2 + b^2 = N
    and N - 1 (5 b^2 + 12 b + 9 and one less), with N in [2^52, 2^53), so the
    integers are the float64 significands. collapsing: np.hypot (and the
    correctly rounded square root of the exact sum) gives both the same distance,
    so np.argmin keeps i; separate: the distances differ and j wins."""
    s = 2.0 ** -18
    col, sep = [], []
    b = 30_100_003
    while len(col) < count or len(sep) < count:
        a = 2 * b + 3
        N = a * a + b * b
        assert 2 ** 52 <= N - 1 and N < 2 ** 53
        pi, pj = (a * s, b * s), ((a - 1) * s, (b + 2) * s)
        assert pi[0] * pi[0] + pi[1] * pi[1] == N * s * s and pj[0] * pj[0] + pj[1] * pj[1] == (N - 1) * s * s
        hi, hj = np.hypot(*pi), np.hypot(*pj)
        # the library's hypot agrees with the square root of the exact sum on these
        assert hi == math.sqrt(N * s * s) and hj == math.sqrt((N - 1) * s * s)
        (col if hi == hj else sep).append((pi, pj))
        b += 700_001
    return tuple(col[:count]), tuple(sep[:count])


@lru_cache(maxsize=None)
def search_cases():
    """The scenario library: one SearchCase per searched situation (see DESIGN.md
    section 4 for the table)."""
    L = LATTICE25
    A, B, C3, D4 = L[16], L[0], L[2], L[5]  # (25, 0), (15, 20), (15, -20), (-20, 15): all at distance 25
    out = []
    add = out.append
    # exact ties of two points: the lower index wins
    add(_case("tie/one-lane", 40, {3: A, 11: B}, 0))           # 8 apart: one lane's share for AW <= 8
    add(_case("tie/two-lanes", 40, {3: A, 4: B}, 0))           # neighbours: two lanes for AW >= 2
    add(_case("tie/window-blocks", 40, {3: A, 19: B}, 0))      # blocks 0 and 1 of the window
    add(_case("tie/window-blocks-late", 96, {52: A, 77: B}, 50))
    add(_case("tie/outside-earlier", 96, {5: A, 60: B}, 50))   # block 0 behind the window (blocks 3, 4): stays at 50
    add(_case("tie/outside-earlier-near", 96, {40: A, 60: B}, 50))
    add(_case("tie/outside-later", 96, {7: A, 70: B}, 2))      # block 4 ahead of the window (blocks 0, 1)
    add(_case("tie/outside-later-far", 200, {20: A, 190: B}, 3))
    add(_case("tie/outside-both", 200, {100: A, 190: B}, 3))   # both in blocks of the second round
    # exact k-way ties
    add(_case("tie3", 40, {3: A, 12: B, 21: C3}, 0))
    add(_case("tie3/one-lane", 64, {2: A, 18: B, 34: C3}, 0))
    add(_case("tie5/one-lane", 40, {1: A, 5: B, 9: C3, 13: D4, 17: L[9]}, 0))
    add(_case("tie5/blocks", 80, {1: A, 17: B, 33: C3, 49: D4, 65: L[9]}, 0))
    add(_case("tie4/behind", 80, {1: A, 5: B, 9: C3, 13: D4}, 60))
    order = [L[(7 * k + 3) % 20] for k in range(20)]            # a fixed shuffle of the 20 points
    add(SearchCase("tie20", [SEARCH_F[0] + p[0] for p in order], [SEARCH_F[1] + p[1] for p in order], SEARCH_F, 0))
    # the first of the 20 at index 17: no lane of a group of 16 or fewer visits it first
    add(_case("tie20/offset", 48, {17 + k: p for k, p in enumerate(order)}, 0))
    add(_case("tie20/offset-tid", 48, {17 + k: p for k, p in enumerate(order)}, 20))
    # near-ties that float32 cannot separate, the nearer point at the lower and at the higher index
    for k, (near, far) in enumerate(near_tie_pairs()[:6]):
        rel = lambda p: (p[0] - SEARCH_F[0], p[1] - SEARCH_F[1])  # noqa: E731
        i, j = ((3, 11), (3, 4), (6, 22), (5, 40), (2, 10), (9, 12))[k]
        add(_case(f"near{k}/low", 48, {i: rel(near), j: rel(far)}, 0))
        add(_case(f"near{k}/high", 48, {i: rel(far), j: rel(near)}, 0))
        out[-2].px[i], out[-2].py[i], out[-2].px[j], out[-2].py[j] = near[0], near[1], far[0], far[1]
        out[-1].px[i], out[-1].py[i], out[-1].px[j], out[-1].py[j] = far[0], far[1], near[0], near[1]
    # the hypot collapse: j is nearer by one ulp of the squared distance
    col, sep = hypot_pairs()
    for k, (pi, pj) in enumerate(col):
        i, j = ((4, 9), (4, 5), (7, 23), (2, 50))[k]
        add(_case(f"collapse{k}", 64, {i: pi, j: pj}, 0))
    for k, (pi, pj) in enumerate(sep):
        i, j = ((4, 9), (4, 5), (7, 23), (2, 50))[k]
        add(_case(f"separate{k}", 64, {i: pi, j: pj}, 0))
    # route lengths: the minimum on the last point, and a tie of the last two
    lengths = [2, 3, BP - 1, BP, BP + 1, 2 * BP, 2 * BP + 1, ACTOR_BATCH - 1, ACTOR_BATCH, ACTOR_BATCH + 1,
               BP * ACTOR_NB, BP * ACTOR_NB + 1, BP * (ACTOR_NB + 1), BP * (ACTOR_NB + 2), BP * 22, BP * 26, BP * 32 + 1, BP * 33]
    for n in lengths:
        add(_case(f"len{n}/last", n, {n - 1: A}, 0))
        add(_case(f"len{n}/tie-last-two", n, {n - 2: A, n - 1: B}, 0))
        if n > 2 * BP:
            add(_case(f"len{n}/tie-first-last", n, {1: A, n - 1: B}, 0))
            add(_case(f"len{n}/behind", n, {1: A}, n - 5))
    # the previous target index: the window's clamp at both ends
    for t in (0, 1, 2, 3, 62, 63):
        add(_case(f"tid{t}/ahead", 64, {40: A}, t))
        add(_case(f"tid{t}/tie", 64, {6: A, 45: B}, t))
    for t in (17, 18, 19, 33, 34, 35):  # tid0 - 2 crosses a block boundary
        add(_case(f"tid{t}/edge", 80, {t - 3: A, t + 20: B}, t))
    add(_case("behind/far", 200, {10: A}, 150))       # many blocks behind the window: stays at 150
    add(_case("behind/far-tie", 200, {10: A, 160: B}, 150))
    add(_case("behind/near-window", 200, {130: A}, 150))
    add(_case("ahead/far", 200, {180: A}, 5))         # many blocks ahead: the second round finds it
    add(_case("ahead/far-304", 304, {300: A}, 5))
    add(_case("ahead/window-decoy", 200, {8: (26.0, 0.0), 180: A}, 5))  # a point 1 px farther inside the window
    # the largest coordinates a route point can take (size 256): a near-tie pair there
    mx, my = max_route_coordinate(256)
    fbig = (mx - 1.0, my - 1.0)
    near, far = max(near_tie_pairs(fbig, (float(mx), float(my))), key=lambda pq: sum(pq[0]) + sum(pq[1]))
    for tag, (p, q) in (("low", (near, far)), ("high", (far, near))):
        c = _case(f"largest/{tag}", 48, {3: (0.0, 0.0), 11: (0.0, 0.0)}, 0, f=fbig, sgn=-1.0)
        c.px[3], c.py[3], c.px[11], c.py[11] = p[0], p[1], q[0], q[1]
        add(c)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def search_width(actor_cap, nact, slot):
    """(AW, windowed) of actor `slot` in an env of nact actors (cbev.hip
    actors_body): AW 0 is the serial path of more than 64 actors."""
    if actor_cap > 64 and nact > 64:
        return 0, False
    minaw = 4 if actor_cap <= 32 else 1
    aw = 64 if nact <= 1 else 32 if nact <= 2 else 16 if nact <= 4 else 8 if nact <= 8 else 4 if nact <= 16 \
        else 2 if nact <= 32 else 1
    aw = max(minaw, aw)
    if aw == 4 and nact > 16 and slot >= 16:
        aw = 8 if nact <= 24 else 4
    return aw, aw > 1


SEARCH_CLASSES = ("window_only", "outside_scanned", "all", "all_cq", "all_nb32", "lane3", "hypot_collapse", "never_back",
                  "tie_one_lane", "tie_two_lanes", "tie_window_blocks", "tie_outside_earlier", "tie_outside_later",
                  "unwindowed", "serial", "frozen")


def search_classes(c, aw, windowed):
    """The branch classes one search falls into: cbev.hip actor_search_win<AW> /
    actor_search<AW> restated with NumPy float32 (no fused multiply-add: the
    cases keep every predicate far from its threshold or exactly on it, see
    near_tie_pairs). Coverage accounting only, never an expected index."""
    if c.frozen:
        return {"frozen"}
    if aw == 0:
        return {"serial"}
    f32 = np.float32
    n, out = c.n, set()
    cf = np.stack([c.px, c.py], 1).astype(f32)
    dx, dy = f32(c.fx) - cf[:, 0], f32(c.fy) - cf[:, 1]
    d = dx * dx + dy * dy
    nb = (n + BP - 1) // BP
    blk = np.arange(n) // BP
    if windowed:
        kb = min(max(c.tid0 - 2, 0) // BP, max(nb - 2, 0))
        w0, w1 = kb * BP, min(kb * BP + 2 * BP, n)
        inwin = (np.arange(n) >= w0) & (np.arange(n) < w1)
        cq = (ACTOR_NB + aw - 1) // aw
        if nb > cq * aw or nb > 32:
            out.add("all")
            out.add("all_nb32" if nb > 32 else "all_cq")
            scanned = np.ones(n, bool)
        else:
            reach = np.sqrt(d[inwin].min()) + f32(0.15) + f32(0.05)
            circ = LY.acb_circles(cf)
            cand = set()
            for k in range(nb):
                if k in (kb, kb + 1):
                    continue
                bx = f32((int(circ[k, 0]) & 0xFFFF) - 32768) * f32(0.125)
                by = f32((int(circ[k, 0]) >> 16) - 32768) * f32(0.125)
                ex, ey = f32(c.fx) - bx, f32(c.fy) - by
                if np.sqrt(ex * ex + ey * ey) - f32(circ[k, 1]) * f32(0.125) <= reach:
                    cand.add(k)
            out.add("outside_scanned" if cand else "window_only")
            scanned = inwin | np.isin(blk, list(cand))
        if aw >= 32:
            lane = np.where(inwin, np.arange(n) - w0, np.arange(n) % BP)
        else:
            lane = np.arange(n) % aw
    else:
        out.add("unwindowed")
        w0, w1 = 0, n
        inwin = np.ones(n, bool)
        scanned, lane = np.ones(n, bool), np.arange(n) % aw
    thr = (np.sqrt(d[scanned].min()) + f32(0.15)) ** 2
    hits = scanned & (d <= thr)
    if np.bincount(lane[hits], minlength=64).max() >= 3:
        out.add("lane3")
    ex, ey = c.fx - c.px, c.fy - c.py
    d2 = ex * ex + ey * ey
    amin = int(np.argmin(np.hypot(ex, ey)))
    if int(np.argmin(d2)) != amin:
        out.add("hypot_collapse")
    if amin < c.tid0:
        out.add("never_back")
    tie = np.flatnonzero(d2 == d2.min())
    if len(tie) >= 2:
        i, j = int(tie[0]), int(tie[1])
        if scanned[i] and scanned[j]:
            out.add("tie_one_lane" if lane[i] == lane[j] else "tie_two_lanes")
        if windowed:
            if inwin[i] and inwin[j] and blk[i] != blk[j]:
                out.add("tie_window_blocks")
            if i < w0 and inwin[j]:
                out.add("tie_outside_earlier")
            if inwin[i] and j >= w1:
                out.add("tie_outside_later")
    return out


def _search_actor(view, slot, c):
    """SearchCase c into actor slot `slot` of a packed record: the route as
    authored (no smoothing), its float32 copy and circles as scene_pack writes
    them, the actor at rest on yaw 0 with its front axle exactly on (fx, fy)."""
    n = c.n
    x = c.fx - SEARCH_WHEELBASE
    assert x + SEARCH_WHEELBASE * 1.0 == c.fx, (c.name, "the front axle is not exact")
    assert n <= view.acx.shape[1], (c.name, n)
    view.acx[slot, :n], view.acy[slot, :n], view.acyaw[slot, :n] = c.px, c.py, 0.0
    view.acf[slot, :n, 0], view.acf[slot, :n, 1] = view.acx[slot, :n], view.acy[slot, :n]
    view.acb[slot] = 0
    view.acb[slot, :(n + BP - 1) // BP] = LY.acb_circles(view.acf[slot, :n])
    ad, ai = view.ad, view.ai
    ad[LY.AD["X"], slot], ad[LY.AD["Y"], slot], ad[LY.AD["YAW"], slot], ad[LY.AD["V"], slot] = x, c.fy, 0.0, 0.0
    assert ad[LY.AD["T_SPEED"], slot] == 0.0 and ad[LY.AD["CRUISE"], slot] == 0.0
    ai[LY.AI["NROUTE"], slot], ai[LY.AI["TIDX"], slot] = n, c.tid0


SEARCH_STEPS = 2


def actor_search_batch(caps, size=128):
    """(P, padded, caps, recs, layout, acts, cases): for every actor count of
    SEARCH_NACT[caps.actor_cap], the scenario library (those whose route fits
    caps.actor_route_cap) dealt into envs of that many actors, a frozen copy
    (TIDX on the last point) after every third, so frozen actors sit between
    live ones of one group round. cases[e] = [(slot, SearchCase, AW, windowed)].
    The hero stands on its road, far from every actor; acts: nothing pressed."""
    P, padded, _ = authored_world(size)
    y, x0, x1 = _road_run(size)
    ex, ey = x0 + 40, y
    lib_ = [c for c in search_cases() if c.n <= caps.actor_route_cap]
    deal = []
    for k, c in enumerate(lib_):
        deal.append(c)
        if k % 3 == 2:
            deal.append(c.as_frozen())
    groups = []
    for nact in SEARCH_NACT[caps.actor_cap]:
        m = (len(deal) + nact - 1) // nact
        for g in range(m):
            groups.append([deal[(g * nact + a) % len(deal)] for a in range(nact)])
    specs = [SceneSpec(agent_rx=[ex + 4 * i for i in range(8)], agent_ry=[ey] * 8, hero_jitter_seed=e,
                       actor_jitter_seed=e, vehicles=[_still("vehicle", 10.0 + a, 10.0) for a in range(len(g))])
             for e, g in enumerate(groups)]
    recs, layout, views = pack_records(specs, size, caps)
    cases = []
    for v, g in zip(views, groups):
        assert v.i("NACT") == len(g)
        row = []
        for slot, c in enumerate(g):
            _search_actor(v, slot, c)
            assert math.hypot(v.h("X") - c.fx, v.h("Y") - c.fy) > 100.0  # no collision, no actor state near the hero
            row.append((slot, c) + search_width(caps.actor_cap, len(g), slot))
        cases.append(row)
    acts = np.zeros((SEARCH_STEPS, len(specs)), np.int32)
    return P, padded, caps, recs, layout, acts, cases
