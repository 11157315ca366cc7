"""Line of sight on the host: ``visible`` in numpy.

``view.render_view`` is the reference's picture: a bot is handed the whole
GameState, walls or not.  With a dungeon bank the games have interior walls,
and a learner may want what a player can actually see from where it stands.
``BatchedEngine.sight`` / ``seen_view`` answer that on the GPU (``orx_sight``,
include/orx_sight.h); this module is the same rule restated for a
``snapshot()``-shaped dict -- the slow path for saved states, and the truth the
GPU tests compare against.  It needs numpy only (no torch, no built library).

The rule, relative to the viewer: window cell (j, i) has offset dx = i - R,
dy = j - R.  A cell is opaque where the view's tile bits are Wall; everything
else in the grid is transparent; cells outside the grid are never seen.

  line    n = max(|dx|, |dy|); for s = 1 .. n - 1 the intermediate cell has the
          offsets sign(d) * ((2 s |d| + n) // (2 n)) (variant "up": s |d| / n
          rounded half up) or sign(d) * ((2 s |d| + n - 1) // (2 n)) ("down":
          half down), d being dx and dy.  One variant is kept for a whole line.
  clear   the cell is in the grid and one of the two lines has no opaque
          intermediate cell (the target itself may be opaque; n <= 1: always).
  seen    a transparent cell: it is clear.  An opaque cell: it is clear, or one
          of its up to three neighbours toward the viewer, (dx - a, dy - b)
          with a in {0, sign dx}, b in {0, sign dy}, (a, b) != (0, 0), is
          transparent and clear -- the far walls of a room, which a bare
          digital line hides at grazing angles.

Among transparent cells the relation is symmetric (reversing a line swaps the
two variants), and without a bank every in-grid cell of the window is seen.
"""
from __future__ import annotations

import functools

import numpy as np

from .enums import Tile
from .view import VIEW_TILE_MASK, render_view

SIGHT_SEEN = 64   # include/orx_sight.h ORX_SIGHT_SEEN: bit 6 of a masked view cell


@functools.lru_cache(maxsize=None)
def _tables(R: int):
    """For every window cell (flat j * V + i) the flat indices of its
    intermediate cells on the two lines, [VV, 2, max(R - 1, 1)], and of its
    neighbours toward the viewer, [VV, 3]; VV (one past the window) pads."""
    V = 2 * R + 1
    VV = V * V
    lines = np.full((VV, 2, max(R - 1, 1)), VV, np.int64)
    nbrs = np.full((VV, 3), VV, np.int64)
    sign = lambda v: (v > 0) - (v < 0)
    for j in range(V):
        for i in range(V):
            dx, dy = i - R, j - R
            n = max(abs(dx), abs(dy))
            for var in (0, 1):          # 0: up (half up), 1: down (half down)
                for s in range(1, n):
                    ox = sign(dx) * ((2 * s * abs(dx) + n - var) // (2 * n))
                    oy = sign(dy) * ((2 * s * abs(dy) + n - var) // (2 * n))
                    lines[j * V + i, var, s - 1] = (R + oy) * V + R + ox
            toward = {(a, b) for a in (0, sign(dx)) for b in (0, sign(dy))} - {(0, 0)}
            for k, (a, b) in enumerate(sorted(toward)):
                nbrs[j * V + i, k] = (j - b) * V + i - a
    return lines, nbrs


def visible_of(cells) -> np.ndarray:
    """bool [B, V, V]: the seen cells of windows of view codes (``render_view``'s
    ``cells``: only the tile bits are read)."""
    cells = np.asarray(cells)
    B, V = cells.shape[0], cells.shape[1]
    R = V // 2
    lines, nbrs = _tables(R)
    tile = (cells & VIEW_TILE_MASK).reshape(B, V * V)
    pad = np.zeros((B, 1), bool)
    inside = tile != 0
    opaque = tile == int(Tile.Wall)
    opq = np.concatenate([opaque, pad], axis=1)
    blocked = opq[:, lines].any(axis=3)                  # [B, VV, 2]
    clear = inside & ~blocked.all(axis=2)
    floor = np.concatenate([clear & ~opaque, pad], axis=1)
    seen = clear | (opaque & floor[:, nbrs].any(axis=2))
    return seen.reshape(B, V, V)


def visible(snap: dict, cfg, player: int, radius: int, bank=None) -> np.ndarray:
    """bool [B, V, V]: which cells of ``render_view(snap, cfg, player, radius,
    bank)`` the player sees from the centre."""
    return visible_of(render_view(snap, cfg, player, radius, bank=bank))


def pack_rows(vis) -> np.ndarray:
    """uint32 [B, V]: bit i of row j is ``vis[b, j, i]`` (orx_sight's ``rows``)."""
    vis = np.asarray(vis, bool)
    weights = np.uint32(1) << np.arange(vis.shape[2], dtype=np.uint32)
    return (vis * weights).sum(axis=2, dtype=np.uint32)


def unpack_rows(rows, V: int) -> np.ndarray:
    """bool [B, V, V] of uint32 [B, V] row words (``pack_rows``'s inverse)."""
    rows = np.asarray(rows).astype(np.uint32)
    return ((rows[:, :, None] >> np.arange(V, dtype=np.uint32)) & 1).astype(bool)


def apply(cells, vis, health=None):
    """The masked view: a seen cell is ``code | SIGHT_SEEN``, an unseen one 0;
    with ``health`` also that plane, zero where unseen, as ``(cells, health)``."""
    vis = np.asarray(vis, bool)
    out = np.where(vis, np.asarray(cells, np.uint8) | np.uint8(SIGHT_SEEN), 0).astype(np.uint8)
    if health is None:
        return out
    return out, np.where(vis, np.asarray(health, np.uint8), 0).astype(np.uint8)
