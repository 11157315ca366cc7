"""What ``view.render_view``, ``path.query`` and ``moves.outcomes`` share (the
host twin of csrc/orx_query.h): the argument checks, the window's coordinates,
the tile of a cell and the NPC and item rows of a ``snapshot()``-shaped dict.
(The twin of csrc/orx_seek.h is ``path.Walk`` and its column helpers.)
"""
from __future__ import annotations

import numpy as np

from .enums import Move, StartMode, Tile, npc_alive_bits

MAX_RADIUS = 15   # include/orx_view.h ORX_VIEW_MAX_RADIUS

# calculate_pos (updater.py:340-351): Up is y - 1, Right x + 1, Down y + 1,
# Left x - 1; in the order of the Move codes 1..4
MOVE_DELTAS = ((int(Move.Up), 0, -1), (int(Move.Right), 1, 0), (int(Move.Down), 0, 1),
               (int(Move.Left), -1, 0))


def i64(a) -> np.ndarray:
    return np.asarray(a).astype(np.int64)


def check_player(player) -> None:
    if player not in (0, 1):
        raise ValueError(f"player must be 0 or 1, got {player!r}")


def check_radius(radius) -> None:
    if not isinstance(radius, (int, np.integer)) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius must be an integer in [1, {MAX_RADIUS}], got {radius!r}")


def bank_of(cfg, bank=None):
    """``bank``, or the DungeonBank made from ``cfg.layouts`` where the
    configuration has layouts and none is given; None without layouts."""
    if bank is None and getattr(cfg, "layouts", None) is not None:
        from .dungeons import DungeonBank
        bank = DungeonBank(cfg.layouts)
    return bank


def npc_depth(cfg) -> int:
    """The depth the NPCs (and their items) are on: player 1's start depth."""
    return int(cfg.p1_depth) if int(cfg.start_mode) == StartMode.Separated else 0


def window_cells(px, py, radius: int):
    """``(x, y)``, int64 [B, V, V] each: window cell [b, j, i] is grid cell
    (px + i - radius, py + j - radius) -- columns are x, rows are y."""
    off = np.arange(2 * radius + 1) - radius
    shape = (len(px), len(off), len(off))
    return (np.broadcast_to(px[:, None, None] + off[None, None, :], shape),
            np.broadcast_to(py[:, None, None] + off[None, :, None], shape))


def per_game(a, cells):   # [B] -> [B, 1, ...] against cells of shape [B, ...]
    return a[(slice(None),) + (None,) * (cells.ndim - 1)]


def inside_grid(cfg, x, y):
    return (x >= 0) & (x < int(cfg.width)) & (y >= 0) & (y < int(cfg.height))


def bank_at(planes, snap: dict, p: int, x, y):
    """``planes[layout, x, y]`` ([L, W, H]) for cells (x, y) [B, ...] clamped
    into the grid, on player row ``p``'s layout (clamped as the kernels do)."""
    L, W, H = planes.shape
    lay = np.clip(i64(snap["p_layout"][p]), 0, L - 1)
    return planes[per_game(lay, x), np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)]


def tile_at(cfg, snap: dict, p: int, x, y, layouts=None, stair_on_border: bool = False):
    """``(inside, tile)`` of cells (x, y), int64 [B, ...], on player row ``p``'s
    depth: whether the cell is in the grid, and its Tile code.  ``layouts``: a
    bank's [L, W, H]; else EmptyDungeonGenerator (worldgen.py:33-43): border
    Wall, the rest Ground but for the staircase (st_x, st_y)[p] (on a border
    cell only with ``stair_on_border``)."""
    inside = inside_grid(cfg, x, y)
    if layouts is not None:
        return inside, bank_at(np.asarray(layouts), snap, p, x, y).astype(np.int64) & 3
    W, H = int(cfg.width), int(cfg.height)
    wall = (x == 0) | (x == W - 1) | (y == 0) | (y == H - 1)
    stair = (x == per_game(i64(snap["st_x"][p]), x)) & (y == per_game(i64(snap["st_y"][p]), x))
    if not stair_on_border:
        stair = stair & ~wall
    return inside, np.where(stair, int(Tile.StaircaseDown),
                            np.where(wall, int(Tile.Wall), int(Tile.Ground)))


def npc_rows(snap: dict, K: int):
    """``(alive, x, y, health)`` [K, B] of the NPC slots (pos is x | y << 8)."""
    pos = i64(np.asarray(snap["npc_pos"]).astype(np.uint16))[:K]
    return (npc_alive_bits(np.asarray(snap["npc_alive"]).astype(np.uint32), K), pos & 0xFF,
            pos >> 8, i64(np.asarray(snap["npc_health"]).astype(np.int8))[:K])


def item_rows(snap: dict, K: int):
    """``(on_floor, x, y, kind)`` [K, B] of the item slots (EXT_ITEMS)."""
    mask = i64(np.asarray(snap["item_mask"]).astype(np.uint32))
    pos = i64(np.asarray(snap["item_pos"]).astype(np.uint16))[:K]
    k = np.arange(K)[:, None]
    return ((mask[0] >> k) & 1) == 1, pos & 0xFF, pos >> 8, (mask[1] >> k) & 1
