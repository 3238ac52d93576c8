"""Import selected pure-Python modules of the reference (read-only, /root/reference).

Test infrastructure only: used by `make_golden.py` in the build container to
capture golden input/output vectors from the reference's own arithmetic. It is
never imported by the product, by `-m gpu` tests or on the GPU box (the
reference tree does not exist there).

Mechanics:
- parent packages whose `__init__` pulls gymnasium/pygame
  (`CarlaBEV/__init__.py:1`, `CarlaBEV/envs/__init__.py:1`,
  `CarlaBEV/config/__init__.py` -> `config/env.py:18` -> `envs/utils.py:2`,
  `CarlaBEV/src/gui/__init__.py:1`) are registered as bare namespace modules
  so their `__init__` is skipped;
- a minimal `pygame` stand-in provides only the names the hero/actor modules
  touch at import/construction time (Sprite base class, Rect, Vector2/3,
  draw.rect). None of the captured numbers flows through it: the captured
  vectors are the bicycle/Stanley/behaviour/reward arithmetic, which is
  NumPy/math in the reference;
- for the whole-episode fixture (`make_golden_episodes.py`) the stand-ins also
  cover what `CarlaBEV.reset` / `CarlaBEV.step` touch: a bare `gymnasium`
  (`Env`, `spaces.Discrete`, `spaces.Box`) and inert `pygame.Surface`,
  `image.load`, `surfarray`, `transform`, `draw.polygon`. There one thing the
  captured values DO flow through is `Rect`: collision results and the
  `abs(distance) < 35` list come from `Rect.colliderect` and `Rect.center`. It is
  a restatement of pygame's documented integer semantics, written here, exactly
  as the oracle's `rect_world_center` / `colliderect` are; it holds no
  reference code;
- bytecode is neither written into nor read from the reference tree
  (`sys.pycache_prefix` points at a private temp dir, so any `__pycache__`
  shipped next to the reference sources is ignored).
"""
from __future__ import annotations

import sys
import tempfile
import types

REF = "/root/reference"

sys.dont_write_bytecode = True
sys.pycache_prefix = tempfile.mkdtemp(prefix="refpyc_")


def _bare_pkg(name: str, path: str) -> None:
    mod = types.ModuleType(name)
    mod.__path__ = [path]
    sys.modules[name] = mod


class _Rect:
    """pygame.Rect restated from pygame's documentation (a restatement, like the
    oracle's `orc_rect`; no pygame or reference code):

    - the four fields are integers; float arguments are truncated toward zero
      (`Rect(left, top, width, height)`, `Rect((left, top), (width, height))`,
      `Rect(rect)`);
    - `center` reads `(x + w // 2, y + h // 2)` and, when assigned, moves the
      rect so that it reads back the assigned (truncated) point;
    - `colliderect` is true when the rects overlap, edges excluded (a rect's
      right and bottom edges lie outside it), and a rect of zero width or height
      collides with nothing. Negative sizes are normalised first, as pygame does.
    """

    def __init__(self, *args):
        if len(args) == 1:
            a = args[0]
            args = (a.x, a.y, a.w, a.h) if isinstance(a, _Rect) else tuple(a)
        if len(args) == 2:
            args = (args[0][0], args[0][1], args[1][0], args[1][1])
        if len(args) == 0:
            args = (0, 0, 0, 0)
        x, y, w, h = args
        self.x, self.y, self.w, self.h = int(x), int(y), int(w), int(h)

    @property
    def center(self):
        return (self.x + self.w // 2, self.y + self.h // 2)

    @center.setter
    def center(self, c):
        self.x = int(c[0]) - self.w // 2
        self.y = int(c[1]) - self.h // 2

    centerx = property(lambda self: self.x + self.w // 2)
    centery = property(lambda self: self.y + self.h // 2)
    left = property(lambda self: self.x)
    top = property(lambda self: self.y)
    right = property(lambda self: self.x + self.w)
    bottom = property(lambda self: self.y + self.h)
    width = property(lambda self: self.w)
    height = property(lambda self: self.h)
    size = property(lambda self: (self.w, self.h))
    topleft = property(lambda self: (self.x, self.y))

    def __iter__(self):
        return iter((self.x, self.y, self.w, self.h))

    def __len__(self):
        return 4

    def __getitem__(self, i):
        return (self.x, self.y, self.w, self.h)[i]

    def __repr__(self):
        return f"Rect({self.x}, {self.y}, {self.w}, {self.h})"

    def copy(self):
        return _Rect(self.x, self.y, self.w, self.h)

    def colliderect(self, *args):
        o = args[0] if len(args) == 1 and isinstance(args[0], _Rect) else _Rect(*args)
        if self.w == 0 or self.h == 0 or o.w == 0 or o.h == 0:
            return False
        ax0, ax1 = min(self.x, self.x + self.w), max(self.x, self.x + self.w)
        ay0, ay1 = min(self.y, self.y + self.h), max(self.y, self.y + self.h)
        bx0, bx1 = min(o.x, o.x + o.w), max(o.x, o.x + o.w)
        by0, by1 = min(o.y, o.y + o.h), max(o.y, o.y + o.h)
        return ax0 < bx1 and ay0 < by1 and ax1 > bx0 and ay1 > by0


class _Vec2:
    def __init__(self, x=0.0, y=0.0):
        if not isinstance(x, (int, float)):  # Vector2((x, y)) / Vector2(vector)
            x, y = x[0], x[1]
        self.x, self.y = float(x), float(y)

    def __iter__(self):
        return iter((self.x, self.y))

    def __len__(self):
        return 2

    def __getitem__(self, i):
        return (self.x, self.y)[i]

    # component-wise float arithmetic with any pair (pygame.math.Vector2's)
    def __sub__(self, o):
        return _Vec2(self.x - float(o[0]), self.y - float(o[1]))

    def __rsub__(self, o):
        return _Vec2(float(o[0]) - self.x, float(o[1]) - self.y)

    def __add__(self, o):
        return _Vec2(self.x + float(o[0]), self.y + float(o[1]))

    __radd__ = __add__

    def __repr__(self):
        return f"Vector2({self.x}, {self.y})"


class _Vec3(_Vec2):
    def __init__(self, x=0.0, y=0.0, z=0.0):
        super().__init__(x, y)
        self.z = float(z)


def _install_pygame_stub() -> None:
    if "pygame" in sys.modules:
        return
    pg = types.ModuleType("pygame")
    sprite = types.ModuleType("pygame.sprite")

    class Sprite:  # noqa: D401 - stand-in base class
        def __init__(self, *a, **k):
            pass

    sprite.Sprite = Sprite
    pmath = types.ModuleType("pygame.math")
    pmath.Vector2 = _Vec2
    pmath.Vector3 = _Vec3
    draw = types.ModuleType("pygame.draw")
    draw.rect = lambda surf, color, rect, *a, **k: rect
    draw.polygon = lambda surf, color, points, *a, **k: None
    image = types.ModuleType("pygame.image")
    image.load = lambda *a, **k: _Surface((0, 0))
    surfarray = types.ModuleType("pygame.surfarray")
    surfarray.pixels3d = lambda surf: _inert_pixels(surf)
    surfarray.array3d = surfarray.pixels3d
    surfarray.make_surface = lambda arr: _Surface(arr.shape[:2])
    transform = types.ModuleType("pygame.transform")
    transform.rotate = lambda surf, angle: _Surface(surf.get_size())
    transform.scale = lambda surf, size, *a: _Surface(size)
    pg.sprite, pg.math, pg.draw, pg.Rect = sprite, pmath, draw, _Rect
    pg.image, pg.surfarray, pg.transform, pg.Surface, pg.SRCALPHA = image, surfarray, transform, _Surface, 0x00010000
    pg.init = pg.quit = lambda *a, **k: None
    sys.modules.update({"pygame": pg, "pygame.sprite": sprite, "pygame.math": pmath, "pygame.draw": draw,
                        "pygame.image": image, "pygame.surfarray": surfarray, "pygame.transform": transform})


class _Surface:
    """Inert pygame.Surface: it keeps its size and nothing else; every drawing
    call is a no-op. Frames are not captured through these stand-ins."""

    def __init__(self, size=(0, 0), flags=0, *a, **k):
        self._size = (int(size[0]), int(size[1]))

    def get_size(self):
        return self._size

    def get_width(self):
        return self._size[0]

    def get_height(self):
        return self._size[1]

    def get_rect(self, **kw):
        r = _Rect(0, 0, *self._size)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def fill(self, *a, **k):
        return None

    def blit(self, *a, **k):
        return None

    def subsurface(self, *a, **k):
        r = _Rect(*a) if a else _Rect(0, 0, *self._size)
        return _Surface((r.w, r.h))

    def convert(self, *a, **k):
        return self

    convert_alpha = copy = convert


def _inert_pixels(surf):
    import numpy as np
    w, h = surf.get_size()
    return np.zeros((w, h, 3), dtype=np.uint8)


def _install_gymnasium_stub() -> None:
    """A bare `gymnasium`: `Env` and the two `spaces` classes the reference
    constructs (envs/spaces.py), as plain data holders."""
    if "gymnasium" in sys.modules:
        return
    gym = types.ModuleType("gymnasium")
    spaces = types.ModuleType("gymnasium.spaces")

    class Env:
        def reset(self, *, seed=None, options=None):
            self._reset_seed = seed

        def step(self, action):
            raise NotImplementedError

        def close(self):
            pass

    class Discrete:
        def __init__(self, n, *a, **k):
            self.n = int(n)

    class Box:
        def __init__(self, low, high, shape=None, dtype=None, *a, **k):
            self.low, self.high, self.shape, self.dtype = low, high, shape, dtype

    gym.Env, gym.spaces = Env, spaces
    spaces.Discrete, spaces.Box = Discrete, Box
    sys.modules.update({"gymnasium": gym, "gymnasium.spaces": spaces})


def setup() -> None:
    _install_pygame_stub()
    _install_gymnasium_stub()
    _bare_pkg("CarlaBEV", f"{REF}/CarlaBEV")
    _bare_pkg("CarlaBEV.envs", f"{REF}/CarlaBEV/envs")
    _bare_pkg("CarlaBEV.config", f"{REF}/CarlaBEV/config")
    _bare_pkg("CarlaBEV.src", f"{REF}/CarlaBEV/src")
    _bare_pkg("CarlaBEV.src.gui", f"{REF}/CarlaBEV/src/gui")
