"""The staircase distance field on the host: ``stair_field`` and ``query`` in
numpy.

The reference's StaircaseBot "rushes as quickly as possible to the staircase"
(optimax_rogue_bots/staircasebot.py:1-21) by stepping along the larger delta;
the updater turns a step into a Wall into Stay (updater.py:89-98), so on a
layout with interior walls it stops at the first one in its way.  What a
walking entity has to cover is the breadth-first distance over tiles that
``is_blocked`` lets through (world.py:41-46: in the grid and not Wall) with
``calculate_pos``'s four moves (updater.py:340-351), to the nearest
StaircaseDown -- any of them descends (updater.py:205-206).

``BatchedEngine.path`` / ``VecEnv.path`` answer that on the GPU
(``orx_path_field`` / ``orx_path_query``, include/orx_path.h); this module is
the same contract restated for layouts and a ``snapshot()``-shaped dict, and
the truth the GPU tests compare against.  It needs numpy only (no torch, no
built library).

One cell of a field (uint16): 0 on a StaircaseDown, else the number of moves
to the nearest one, ``PATH_WALL`` on a Wall tile or outside the grid,
``PATH_UNREACHABLE`` on a tile that is not Wall but has no walkable path.
"""
from __future__ import annotations

import numpy as np

from .enums import Move, Tile
from .query import (MOVE_DELTAS, bank_at, check_player, check_radius, i64, inside_grid, tile_at,
                    window_cells)

# include/orx_path.h ORX_PATH_*
PATH_WALL = 0xFFFF
PATH_UNREACHABLE = 0xFFFE


def check_path_args(player: int, radius=None, cfg=None) -> None:
    """ValueError for a player other than 0 / 1, a radius (when one is given)
    outside 1..VIEW_MAX_RADIUS, or an EmptyDungeonGenerator grid whose largest
    distance (W - 3) + (H - 3) would reach the sentinels (what orx_path_query
    refuses with ORX_EINVAL)."""
    check_player(player)
    if radius is not None:
        check_radius(radius)
    if cfg is not None and getattr(cfg, "layouts", None) is None \
            and int(cfg.width) + int(cfg.height) - 6 >= PATH_UNREACHABLE:
        raise ValueError("width + height too large for uint16 distances")


def stair_field(layouts) -> np.ndarray:
    """uint16 [L, W, H]: the field of every layout of ``layouts`` ([L, W, H] or
    [W, H] Tile codes).  A frontier breadth-first search over all layouts at
    once: each level touches only the cells it reaches, so the cost follows
    the cells (plus a few numpy calls per level), not levels x cells."""
    a = np.asarray(layouts)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("layouts must be [L, W, H] Tile codes")
    L, W, H = a.shape
    # one Wall ring around every layout: a step off the grid lands on it
    pad = np.full((L, W + 2, H + 2), int(Tile.Wall), np.uint8)
    pad[:, 1:-1, 1:-1] = a
    flat = pad.reshape(-1)
    dist = np.full(flat.shape, -1, np.int64)          # -1: not reached
    steps = np.array([-1, 1, -(H + 2), H + 2], np.int64)
    frontier = np.flatnonzero(flat == int(Tile.StaircaseDown))
    open_ = flat != int(Tile.Wall)
    dist[frontier] = 0
    d = 0
    while len(frontier):
        d += 1
        nxt = (frontier[:, None] + steps[None, :]).reshape(-1)
        nxt = nxt[open_[nxt] & (dist[nxt] < 0)]
        frontier = np.unique(nxt)
        dist[frontier] = d
    if d > PATH_UNREACHABLE:   # (cannot happen with at most 65,536 tiles)
        raise ValueError("a distance reaches the sentinels")
    out = np.where(open_, np.where(dist < 0, PATH_UNREACHABLE, dist), PATH_WALL)
    return np.ascontiguousarray(out.reshape(L, W + 2, H + 2)[:, 1:-1, 1:-1].astype(np.uint16))


def closed_form(cfg, sx, sy) -> np.ndarray:
    """uint16 [..., W, H]: the field of EmptyDungeonGenerator's dungeon
    (worldgen.py:33-43: the border is Wall, the interior open) with its
    staircase at (sx, sy) -- scalars, or arrays of one shape: PATH_WALL on the
    border, |x - sx| + |y - sy| inside.  Exact because the interior has no
    walls: the Manhattan distance is a lower bound and an L-shaped walk
    inside the interior attains it."""
    W, H = int(cfg.width), int(cfg.height)
    sx, sy = np.asarray(sx, np.int64), np.asarray(sy, np.int64)
    x = np.arange(W, dtype=np.int64)[:, None]
    y = np.arange(H, dtype=np.int64)[None, :]
    d = np.abs(x - sx[..., None, None]) + np.abs(y - sy[..., None, None])
    border = (x == 0) | (x == W - 1) | (y == 0) | (y == H - 1)
    return np.where(border, PATH_WALL, d).astype(np.uint16)


def move_toward(own, up, right, down, left) -> np.ndarray:
    """int8: the first of Up, Right, Down, Left whose target value is ``own`` -
    1; Stay where ``own`` is 0 or a sentinel (arrays of one shape)."""
    own = np.asarray(own, np.int64)
    want = own - 1
    move = np.full(own.shape, int(Move.Stay), np.int8)
    for (code, _, _), val in reversed(list(zip(MOVE_DELTAS, (up, right, down, left)))):
        move = np.where(np.asarray(val, np.int64) == want, code, move)
    return np.where((own == 0) | (own >= PATH_UNREACHABLE), int(Move.Stay), move).astype(np.int8)


def query(snap: dict, cfg, player: int, radius=None, bank=None):
    """``(dist, move)`` of ``player`` (0 / 1) of every game of a
    ``snapshot()``-shaped dict, and with a ``radius`` ``(dist, move, window)``.

    dist    int32 [B]: the value of the player's own cell, -1 where it is
            PATH_UNREACHABLE
    move    int8 [B]: the Move that gets one step closer (``move_toward``)
    window  uint16 [B, V, V], V = 2 * radius + 1: ``window[b, j, i]`` is the
            value of grid cell (px + i - radius, py + j - radius), PATH_WALL
            outside the grid (``render_view``'s geometry)

    The value of a cell is ``bank.stair_field()[p_layout[player]][x, y]`` with
    a bank (made from ``cfg.layouts`` when omitted), else ``closed_form`` with
    the staircase (st_x, st_y)[player] of the player's depth."""
    check_path_args(player, radius, cfg)
    if bank is None and getattr(cfg, "layouts", None) is not None:
        from .dungeons import DungeonBank
        bank = DungeonBank(cfg.layouts)
    p = int(player)
    px, py = i64(snap["p_x"][p]), i64(snap["p_y"][p])
    if bank is None:
        sx, sy = i64(snap["st_x"][p]), i64(snap["st_y"][p])
    else:
        field = bank.stair_field()

    def value(x, y):
        """The values of cells (x, y), arrays of shape [B, ...]."""
        if bank is None:
            g = (slice(None),) + (None,) * (x.ndim - 1)
            inside, tile = tile_at(cfg, snap, p, x, y)
            v = np.where(tile == int(Tile.Wall), PATH_WALL, np.abs(x - sx[g]) + np.abs(y - sy[g]))
        else:
            inside, v = inside_grid(cfg, x, y), bank_at(field, snap, p, x, y).astype(np.int64)
        return np.where(inside, v, PATH_WALL)

    own = value(px, py)
    dist = np.where(own == PATH_UNREACHABLE, -1, own).astype(np.int32)
    move = move_toward(own, *(value(px + dx, py + dy) for _, dx, dy in MOVE_DELTAS))
    if radius is None:
        return dist, move
    return dist, move, value(*window_cells(px, py, int(radius))).astype(np.uint16)
