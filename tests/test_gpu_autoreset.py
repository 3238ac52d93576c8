"""Same-step autoreset: cbev_final_frames against torch indexing (alone, and
captured and replayed), make_env(cfg, autoreset="same_step") against a
"disabled" twin that runs step() then reset_terminated(), the mode with
active=, and its surface. Everything is bitwise: the new kernel copies bytes,
there is no tolerance to choose.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from carlabev_env_amd._lib import lib
from gpu_harness import P_, ptr
from gpu_scenes import EGO_ONLY, ego_only_64, eval_actions, eval_cfg, obs_world, relaid
from helpers import CAPS_FULL, bench_caps

pytestmark = pytest.mark.gpu

CBEV_EINVAL = -1
SENT, SENT_ENV, GUARD = 0xA5, -77, 64


# ---------------------------------------------------------------------- 1. the kernel alone
class Bufs:
    """ring, mask, out, out_env and out_count of one geometry; ring and mask at
    byte offsets into their stores, `out` between guard bytes."""

    def __init__(self, hw, n, F, ring_off=0, mask_off=0, seed=0):
        self.hw, self.n, self.F = hw, n, F
        nb = F * n * hw[0] * hw[1]
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.ring_store = torch.randint(0, 16, (ring_off + nb,), dtype=torch.uint8, device="cuda", generator=g)
        self.ring = self.ring_store[ring_off:].view(F, n, *hw)
        self.mask_store = torch.zeros(mask_off + n, dtype=torch.uint8, device="cuda")
        self.mask = self.mask_store[mask_off:]
        self.out_store = torch.empty(GUARD + nb + GUARD, dtype=torch.uint8, device="cuda")
        self.out = self.out_store[GUARD:GUARD + nb].view(F, n, *hw)
        self.env = torch.empty(n + 2, dtype=torch.int32, device="cuda")
        self.count = torch.empty(3, dtype=torch.int32, device="cuda")
        self.prefill()

    def prefill(self):
        self.out_store.fill_(SENT)
        self.env.fill_(SENT_ENV)
        self.count.fill_(SENT_ENV)

    def call(self, c, head, heads, stream=None):
        return lib().cbev_final_frames(c.ctx, ptr(self.ring), self.n, self.F, head, ptr(heads) if heads is not None
                                       else None, ptr(self.mask), ptr(self.out), ptr(self.env[1:]),
                                       ptr(self.count[1:]), stream)

    def expected(self, head, heads):
        """(out store, out_env, out_count) by the definition, from torch indexing."""
        n, F = self.n, self.F
        H = heads.long() % F if heads is not None else torch.full((n,), head, dtype=torch.long, device="cuda")
        sel = torch.nonzero(self.mask).reshape(-1)
        k = sel.numel()
        store = torch.full_like(self.out_store, SENT)
        out = store[GUARD:GUARD + self.out.numel()].view(self.out.shape)
        if k:
            out[:, :k] = relaid(self.ring, H)[:, sel]  # rows >= k keep the sentinel
        env = torch.full_like(self.env, SENT_ENV)
        env[1:1 + n] = -1
        env[1:1 + k] = sel.to(torch.int32)
        count = torch.full_like(self.count, SENT_ENV)
        count[1] = k
        return store, env, count

    def check(self, c, head, heads, what):
        self.prefill()
        assert self.call(c, head, heads) == 0, lib().cbev_last_error()
        torch.cuda.synchronize()
        store, env, count = self.expected(head, heads)
        assert torch.equal(self.count, count), (what, "count", self.count.tolist(), count.tolist())
        assert torch.equal(self.env, env), (what, "out_env")
        assert torch.equal(self.out_store, store), (what, "out, the unwritten rows and the guard bytes")


def _masks(n, seed):
    rng = np.random.default_rng(seed)
    z = np.zeros(n, np.uint8)
    first, last = z.copy(), z.copy()
    first[0], last[-1] = 1, 1
    rnd = (rng.random(n) < 0.07).astype(np.uint8)
    if n >= 15:
        rnd[rng.integers(0, n)] = 1
    odd = rnd.copy()
    odd[rnd != 0] = np.where(rng.random(int(rnd.sum())) < 0.5, 2, 0xFF)  # any nonzero byte selects
    odd[n // 2] = 2
    return {"empty": z, "full": z + 1, "first": first, "last": last, "random": rnd, "bytes-2-0xff": odd}


GEOMETRIES = [
    # hw, F, ring byte offset, the sizes of n
    pytest.param((128, 128), 4, 0, (1, 15, 16, 17, 257), id="128x128-F4"),
    pytest.param((96, 96), 3, 0, (1, 15, 16, 17, 257, 4097), id="96x96-F3"),
    pytest.param((84, 84), 4, 0, (17, 4097), id="84x84-F4"),
    pytest.param((84, 84), 1, 0, (16, 257), id="84x84-F1"),
    pytest.param((5, 7), 3, 0, (1, 15, 16, 17, 257, 4097), id="5x7-F3-bytes"),
    pytest.param((5, 7), 1, 0, (17,), id="5x7-F1-bytes"),
    pytest.param((96, 96), 4, 4, (17, 257), id="96x96-F4-ring-off-4"),
]


@pytest.mark.parametrize("hw,F,ring_off,sizes", GEOMETRIES)
def test_final_frames_equals_torch_indexing(hw, F, ring_off, sizes):
    c = obs_world(hw)
    for n in sizes:
        for mask_off in (0, 1):  # 1: the ranking's byte path
            b = Bufs(hw, n, F, ring_off, mask_off, seed=1000 * n + F)
            assert b.ring.data_ptr() % 16 == ring_off and b.mask.data_ptr() % 16 == mask_off
            rng = np.random.default_rng(n + 7 * F)
            h = rng.integers(0, 256, n).astype(np.uint8)
            h[n // 2] = F  # a head byte >= F is reduced modulo F
            heads = torch.from_numpy(h).cuda()
            for name, m in _masks(n, n + mask_off).items():
                b.mask.copy_(torch.from_numpy(m))
                # every global head on the random mask, one elsewhere; per-env heads on every mask
                for head in (range(F) if name == "random" else (n % F,)):
                    b.check(c, head, None, (n, mask_off, name, head))
                b.check(c, 0, heads, (n, mask_off, name, "per-env heads"))


def test_refusals_write_nothing():
    hw, n, F = (96, 96), 17, 3
    c = obs_world(hw)
    b = Bufs(hw, n, F)
    b.mask.fill_(1)
    L = lib()
    nb = b.ring.numel()

    def call(ctx=c.ctx, ring=b.ring, n_=n, F_=F, head=0, heads=None, mask=b.mask, out=b.out, env=b.env[1:],
             count=b.count[1:]):
        return L.cbev_final_frames(ctx, ptr(ring) if ring is not None else None, n_, F_, head,
                                   ptr(heads) if heads is not None else None, ptr(mask) if mask is not None else None,
                                   ptr(out) if out is not None else None, ptr(env) if env is not None else None,
                                   ptr(count) if count is not None else None, None)

    def untouched(what):
        """The full mask would fill every row: after a call that launched, no sentinel is left."""
        torch.cuda.synchronize()
        assert bool((b.out_store == SENT).all()), (what, "out")
        assert bool((b.env == SENT_ENV).all()) and bool((b.count == SENT_ENV).all()), (what, "out_env / out_count")

    def refused(word, **kw):
        assert call(**kw) == CBEV_EINVAL and word in L.cbev_last_error(), kw
        untouched(kw)

    for kw in (dict(ctx=None), dict(ring=None), dict(mask=None), dict(out=None), dict(env=None), dict(count=None)):
        refused(b"null", **kw)
    for bad in (0, 256, -1):
        refused(b"n_frames", F_=bad)
    for bad in (-1, F, 255):
        refused(b"head", head=bad)
    refused(b"exceeds", n_=(1 << 20) + 1)
    # out's byte range overlapping the ring's: from either side, and the ring itself
    both = torch.zeros(2 * nb - 16, dtype=torch.uint8, device="cuda")
    lo, hi = both[:nb].view(b.ring.shape), both[nb - 16:].view(b.ring.shape)
    for ring_, out_ in ((lo, hi), (hi, lo), (lo, lo)):
        refused(b"overlap", ring=ring_, out=out_)
        assert not bool(both.any())
    assert call(n_=0) == 0 and call(n_=-3) == 0  # nothing to do
    untouched("n <= 0")
    # the same buffers are written once a call is accepted: with heads the global head is ignored
    assert call(head=F, heads=b.mask) == 0
    torch.cuda.synchronize()
    assert int(b.count[1]) == n and not bool((b.out == SENT).all()) and bool((b.env[1:1 + n] >= 0).all())


# ---------------------------------------------------------------------- 2. captured and replayed
def test_final_frames_under_graph_capture():
    """Captured once on a side stream, replayed twice with the mask edited in
    between: each replay ranks the mask as it is then."""
    hw, n, F = (96, 96), 257, 3
    c = obs_world(hw)
    b = Bufs(hw, n, F, seed=5)
    heads = torch.from_numpy(np.random.default_rng(2).integers(0, F, n).astype(np.uint8)).cuda()
    masks = [torch.from_numpy(m).cuda() for m in (_masks(n, 31)["random"], _masks(n, 32)["bytes-2-0xff"],
                                                   _masks(n, 33)["last"])]
    assert not torch.equal(masks[1] != 0, masks[2] != 0)
    b.mask.copy_(masks[0])
    b.check(c, 0, heads, "eager")  # the kernel is loaded before the capture
    b.prefill()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            assert b.call(c, 0, heads, P_(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert bool((b.out_store == SENT).all()) and bool((b.count == SENT_ENV).all())  # the capture ran nothing
    for rep in (1, 2):
        b.prefill()
        b.mask.copy_(masks[rep])
        g.replay()
        torch.cuda.synchronize()
        store, env, count = b.expected(0, heads)
        assert int(count[1]) == int((masks[rep] != 0).sum()) > 0
        assert torch.equal(b.count, count) and torch.equal(b.env, env) and torch.equal(b.out_store, store), rep


# ---------------------------------------------------------------------- 3-5. the vector env
N, MAX_ACTIONS = 64, 8


def _make(monkeypatch, autoreset, cfg_update=None, caps=EGO_ONLY, difficulty="rt_no_traffic_v1", attach=True, n=N,
          **kw):
    """An env of the small-episode config (max_actions = 8) on the seeded reset,
    with a 16-row bank attached. Size 64 has no scene generator: its scenes are
    test_gpu_masked_step's nine authored ones, env e running scene e % 9, and
    they are the bank as well."""
    from carlabev_env_amd import RandomNavigationReset, build_random_navigation_options, make_env
    cfg = eval_cfg(monkeypatch, MAX_ACTIONS)
    if cfg_update:
        cfg = type(cfg)(**{**cfg.model_dump(), **cfg_update})
    env = make_env({"env": cfg, "num_envs": n}, num_envs=n, caps=caps, autoreset=autoreset, **kw)
    assert env.params.max_actions == MAX_ACTIONS
    if cfg.size == 64:
        nine = torch.from_numpy(ego_only_64(9)[3]).cuda()
        env.load_scenes(nine[torch.arange(n, device="cuda") % 9].contiguous())
        if attach:
            env.attach_bank(nine)
        return env
    opts = build_random_navigation_options(RandomNavigationReset(difficulty_id=difficulty))
    env.reset(seed=11, options=opts)
    if attach:
        env.attach_bank(env.build_bank(list(range(900, 916)), opts))
    return env


def _same(a, b, path=()):
    """Materialised infos, compared value by value but for infos["episode"]["t"],
    the episode's wall-clock seconds on each env's own device clock (its mask
    "_t" is compared)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(
            path + (k,) == ("episode", "t") or _same(a[k], b[k], path + (k,)) for k in a)
    if isinstance(a, np.ndarray):
        if a.dtype == object:
            return a.shape == b.shape and all(_same(x, y, path + (None,)) for x, y in zip(a.tolist(), b.tolist()))
        return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    if isinstance(a, float) and isinstance(b, float):
        return a == b or (a != a and b != b)
    return a == b


TWINS = [
    pytest.param({}, {}, id="128-ego-only-f32-F4"),
    pytest.param(dict(max_vehicles=10), dict(caps=dataclasses.asdict(CAPS_FULL), difficulty="rt_medium_v1"),
                 id="actor-slots"),
    pytest.param(dict(obs_size=(96, 96)), dict(obs_dtype="bits"), id="96x96-bits"),
    pytest.param(dict(obs_size=(84, 84), obs_mode="bev_rgb"), {}, id="84x84-gray"),
    pytest.param(dict(temporal_fusion_mode="vehicle_temporal"), dict(obs_dtype="float16"), id="float16-temporal"),
    pytest.param({}, dict(stack_heads="per_env"), id="per-env-heads"),
    pytest.param({}, dict(action_repeat=2), id="action-repeat-2"),
    pytest.param(dict(size=64, obs_size=(64, 64)), dict(caps=dataclasses.asdict(bench_caps(2))), id="size-64"),
]


@pytest.mark.parametrize("cfg_update,kw", TWINS)
def test_same_step_equals_step_then_reset_terminated(monkeypatch, cfg_update, kw):
    A = _make(monkeypatch, "same_step", cfg_update, **kw)
    B = _make(monkeypatch, "disabled", cfg_update, **kw)
    assert A.metadata["autoreset_mode"] == "same_step" and B.metadata["autoreset_mode"] == "disabled"
    assert B.auto_obs and not bool(lib().cbev_reset_pending(A._ctx))
    ar = torch.arange(N, device="cuda")

    def both(t):
        a = eval_actions(N, t)
        oa, ra, ta, ua, ia = A.step(a)
        fin, ids = A.final_obs()
        ob, rb, tb, ub, ib = B.step(a)
        obs_r = B.reset_terminated()
        assert torch.equal(oa, obs_r), (t, "the observation after the reset")
        assert torch.equal(ra, rb) and torch.equal(ta, tb) and torch.equal(ua, ub), (t, "rew / term / trunc")
        assert _same(dict(ia), dict(ib)), (t, "infos")
        assert torch.equal(ids, torch.nonzero(tb).reshape(-1)) and ids.dtype == torch.int64, (t, "final env ids")
        assert fin.dtype == ob.dtype and fin.shape == (ids.numel(), *ob.shape[1:])
        assert torch.equal(fin, ob[tb]), (t, "the terminal observations")
        assert int(A.final_count.item()) == ids.numel()
        assert torch.equal(A.final_env, torch.cat([ids.to(torch.int32), torch.full((N - ids.numel(),), -1,
                                                                                   dtype=torch.int32, device="cuda")]))
        return tb.cpu().numpy(), dict(ib)

    # ends fall on different steps whatever the dynamics do: the episode clocks of two thirds
    # of the envs are restarted at different steps before the compared loop
    t = 0
    for stop, group in ((3, 0), (5, 1)):
        while t < stop:
            both(t)
            t += 1
        m = (ar % 3 == group)
        assert torch.equal(A.reset_from_bank(m), B.reset_from_bank(m))
    ends = []
    for t in range(5, 5 + 20):
        term, infos = both(t)
        assert ("_episode" in infos) == bool(term.any())
        ends.append(term)
    ends = np.stack(ends)
    per_step = ends.sum(axis=1)
    assert (per_step == 0).any(), "no step without an end"
    assert ((per_step > 0) & (per_step < N)).any(), "no step in which some but not all envs ended"
    assert (ends.sum(axis=0) >= 2).any(), "no env ended in two different steps"
    assert torch.equal(A.records, B.records) and torch.equal(A.ring, B.ring)
    assert np.array_equal(A.reset_counts(), B.reset_counts()) and A.bank_rows_used() == B.bank_rows_used()
    if A.per_env:
        assert torch.equal(A.heads, B.heads)
    assert A.errors() == 0 and B.errors() == 0
    for env in (A, B):
        env.close()


@pytest.mark.parametrize("stack_heads", ["global", "per_env"])
def test_same_step_with_an_active_mask(monkeypatch, stack_heads):
    """An env that ended, was reset, and is then left inactive keeps its stale
    term byte: it is neither reset nor reported again; an active env that ends is."""
    A = _make(monkeypatch, "same_step", stack_heads=stack_heads)
    everyone = torch.ones(N, dtype=torch.bool, device="cuda")
    active = torch.arange(N, device="cuda") % 3 != 2  # a third stands still
    off = ~active
    t = 0
    while True:  # every env is truncated by the same step (max_actions), if not earlier
        _, _, term, _, _ = A.step(eval_actions(N, t), active=everyone)
        t += 1
        assert t <= MAX_ACTIONS
        if bool(term[off].any()):
            break
    _, ids = A.final_obs()
    just_ended = term & off
    assert torch.equal(ids, torch.nonzero(term).reshape(-1)) and bool(just_ended.any())
    counts0, recs0, ring0 = A.reset_counts(), A.records.clone(), A.ring.clone()
    seen_active_end = False
    for _ in range(MAX_ACTIONS + 1):
        obs, rew, term, _, _ = A.step(eval_actions(N, t), active=active)
        t += 1
        fin, ids = A.final_obs()
        assert bool(term[just_ended].all()), "the stale term bytes the mask has to be and-combined against"
        want = torch.nonzero(term & active).reshape(-1)
        assert torch.equal(ids, want), "reported: exactly the active envs that ended in this step"
        assert fin.shape[0] == want.numel()
        assert np.array_equal(A.reset_counts()[off.cpu().numpy()], counts0[off.cpu().numpy()])
        assert torch.equal(A.records[off], recs0[off]), "an inactive env's record"
        if stack_heads == "per_env":
            assert torch.equal(A.ring[:, off], ring0[:, off]), "an inactive env's ring slots"
        if want.numel():
            seen_active_end = True
            # reset: the observation shows the reset frame in every stack position
            fr = A.ring[:, want]
            assert torch.equal(fr, fr[:1].expand_as(fr))
            assert (A.reset_counts()[want.cpu().numpy()] > counts0[want.cpu().numpy()]).all()
    assert seen_active_end
    assert A.errors() == 0
    A.close()


def test_surface(monkeypatch):
    from carlabev_env_amd import CarlaBEVVectorEnv
    A = _make(monkeypatch, "same_step", attach=False, n=4)
    D = _make(monkeypatch, "disabled", attach=False, n=4)
    assert A.metadata["autoreset_mode"] == "same_step"
    assert D.metadata["autoreset_mode"] == "disabled" and CarlaBEVVectorEnv.metadata["autoreset_mode"] == "disabled"
    assert "metadata" not in vars(D)
    assert not hasattr(D, "_final") and not hasattr(D, "_final_env") and not hasattr(D, "_final_count")
    assert A._final.shape == A._ring.shape and A._final_env.shape == (4,) and A._final_count.shape == (1,)
    a = eval_actions(4, 0)
    with pytest.raises(RuntimeError, match="before any step"):
        A.final_obs()
    with pytest.raises(RuntimeError, match="same_step"):
        D.final_obs()
    with pytest.raises(RuntimeError, match="no scene bank"):
        A.step(a)
    rec0 = A.records.clone()
    torch.cuda.synchronize()
    assert torch.equal(A.records, rec0)  # the refused step launched nothing
    from carlabev_env_amd import RandomNavigationReset, build_random_navigation_options
    opts = build_random_navigation_options(RandomNavigationReset(difficulty_id="rt_no_traffic_v1"))
    A.attach_bank(A.build_bank([900, 901, 902], opts))
    with pytest.raises(RuntimeError, match="same_step"):
        A.reset_terminated()
    A.step(a)
    rows, ids = A.final_obs()
    k = int(A.final_count.item())
    assert rows.shape == (k, *A.single_observation_space.shape) and rows.dtype == A.obs_buf.dtype
    assert ids.shape == (k,) and ids.dtype == torch.int64 and ids.device == A.device
    with pytest.raises(RuntimeError, match="same_step"):
        A.reset_terminated()
    for env in (A, D):
        env.close()


def test_same_step_on_the_bare_rgb_observation(monkeypatch):
    """wrappers=False: a one-slot ring and the RGB expansion; obs_mode="vector"
    (read from the records the reset overwrites) is refused."""
    from carlabev_env_amd import make_env
    n = 8
    A = _make(monkeypatch, "same_step", n=n, wrappers=False)
    B = _make(monkeypatch, "disabled", n=n, wrappers=False)
    ended = 0
    for t in range(MAX_ACTIONS + 1):
        a = eval_actions(n, t)
        oa, _, ta, _, _ = A.step(a)
        fin, ids = A.final_obs()
        ob, _, tb, _, _ = B.step(a)
        obs_r = B.reset_terminated()
        assert torch.equal(oa, obs_r) and torch.equal(ta, tb)
        assert torch.equal(ids, torch.nonzero(tb).reshape(-1)) and torch.equal(fin, ob[tb])
        ended += ids.numel()
    assert ended >= n
    for env in (A, B):
        env.close()
    cfg = eval_cfg(monkeypatch, MAX_ACTIONS)
    cfg = type(cfg)(**{**cfg.model_dump(), "obs_mode": "vector"})
    with pytest.raises(ValueError, match="autoreset.*vector"):
        make_env({"env": cfg, "num_envs": 2}, num_envs=2, caps=EGO_ONLY, wrappers=False, autoreset="same_step")
