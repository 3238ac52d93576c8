"""Directed GPU parity over the authored edge cases (tests/edge_cases.py): the
device step against the C oracle on states the scene generator never produces.
The oracle's frames and rebuilt routes for these cases are themselves checked
against independent restatements, and the cases' branch coverage is counted, in
test_edge_cases_cpu.py.

Same bar as test_gpu_parity.py (run_parity): reset and step frames, whole
records, flags, rewards and info after every step, and no error flag at the end
(no CBEV_ERR_RASTER_WINDOW).
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import edge_cases as EC
from carlabev_env_amd import layout as LY
from carlabev_env_amd._lib import lib
from test_gpu_parity import run_parity

pytestmark = pytest.mark.gpu


def _run(P, padded, caps, recs, acts, **kw):
    return run_parity(None, len(recs), len(acts), caps=caps, recs=recs, world_=(P, padded), acts=acts, **kw)


@pytest.mark.parametrize("geo", EC.GEOMETRIES, ids=[f"{s}-{a}" for s, a in EC.GEOMETRIES])
def test_raster_matrix(geo):
    """Headings x positions x painted content of one geometry: reset, a step with
    nothing pressed (the pose stays), a step with gas."""
    P, padded, caps, recs, layout, acts = EC.raster_batch(*geo)
    _run(P, padded, caps, recs, acts)


def test_crop_above_400_is_refused():
    """256 with anchor_y 0.2 or 0.8 gives crop 482: cbev_create refuses it."""
    for ay in (0.2, 0.8):
        P, _, _ = EC.authored_world(256, ay)
        assert P.crop == 482
        L = lib()
        ctx = ctypes.c_void_p()
        rc = L.cbev_create(ctypes.byref(P), ctypes.byref(EC.CAPS_RASTER.c()), 0, ctypes.byref(ctx))
        assert rc != 0 and b"crop 482" in L.cbev_last_error()


def test_more_than_64_actors_painted():
    """70 vehicles and 10 pedestrians in one crop: paint_tile's actor loops past thread 63."""
    P, padded, caps, recs, layout, acts = EC.many_actor_batch()
    _run(P, padded, caps, recs, acts)


@pytest.mark.parametrize("caps", [EC.CAPS_EGO8, EC.CAPS_EGO16], ids=["ego8", "ego16"])
def test_long_ego_routes(caps):
    """Ego routes of 33 to 128 points: vis / vis_draw words 1-3, the target paint
    past thread 63, k_ego's S2 and S5 past their prefetch (16 envs per workgroup
    at the small capacities), consumption and TIDX across word boundaries."""
    P, padded, caps, recs, layout, acts, _ = EC.long_route_batch(caps)
    _run(P, padded, caps, recs, acts)


def test_long_ego_routes_64_envs_per_workgroup(monkeypatch):
    monkeypatch.setenv("CBEV_EGO_NE", "64")
    P, padded, caps, recs, layout, acts, _ = EC.long_route_batch(EC.CAPS_EGO16)
    _run(P, padded, caps, recs, acts)


@pytest.mark.parametrize("caps", EC.CAPS_RETREAT, ids=["slots32", "slots48", "slots96"])
def test_retreats_at_pinned_route_lengths(caps):
    """wave_start_retreat at NROUTE 2 to 13, 32, 63 and 64, the +1e-3 fallback, a
    dropped duplicate first point, and sixteen retreats in one wave on one step;
    then the walk along the rebuilt routes. 32, 48 and 96 actor slots:
    k_actors_g4, k_actors<false>, k_actors<true>."""
    P, padded, caps, recs, layout, acts, cases = EC.retreat_batch(caps)
    seen = {}

    def on_step(t, views, causes):
        if t == 0:
            seen["nroute"] = sorted(int(v.ai[LY.AI["NROUTE"], s]) for v, cs in zip(views, cases) for s, _, _ in cs)
            seen["state"] = {int(v.ai[LY.AI["BSTATE"], s]) for v, cs in zip(views, cases) for s, _, _ in cs}

    _run(P, padded, caps, recs, acts, on_step=on_step)
    assert seen["state"] == {LY.BSTATE["retreating"]}
    assert set(seen["nroute"]) == set(range(2, 14)) | {32, 63, 64}
