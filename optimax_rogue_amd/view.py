"""The egocentric map view on the host: ``render_view`` in numpy.

What a bot sees, as cell codes: the reference hands every bot the GameState
of its depth each tick (optimax_rogue_bots/main.py:118-155) and its spectator
draws it tiles first, then the entities of the viewed depth on top
(optimax_rogue_cmdspec/map.py:56-84).  ``BatchedEngine.view`` / ``VecEnv.view``
write that picture on the GPU (``orx_view``, include/orx_view.h); this module
is the same contract restated for a ``snapshot()``-shaped dict -- the slow
path for saved states and checkpoints, and the truth the GPU tests compare
against.  It needs numpy only (no torch, no built library).

One cell (uint8), for the viewer at (px, py) on depth d, window side
V = 2 * radius + 1, ``cells[b, j, i]`` = grid cell (px + i - R, py + j - R):

  bits 0-1  0 = outside the W x H grid, else the Tile code of
            dungeons[d].tiles[x, y] (1 Ground, 2 Wall, 3 StaircaseDown)
  bit 2     VIEW_PLAYER: the other player stands there (it is on depth d)
  bit 3     VIEW_NPC: an NPC still in GameState.entities stands there
  bit 4     VIEW_ITEM: EXT_ITEMS: an item lies there
  bit 5     VIEW_ITEM_KIND: that item's kind (0 damage, 1 max health)

The centre cell is the viewer's own and carries no flag for the viewer.
"""
from __future__ import annotations

import numpy as np

from .enums import EXT_ITEMS, Tile
from .query import (MAX_RADIUS, bank_of, check_player, check_radius, i64, item_rows,  # noqa: F401
                    npc_depth, npc_rows, tile_at, window_cells)

# include/orx_view.h ORX_VIEW_*
VIEW_MAX_RADIUS = MAX_RADIUS
VIEW_TILE_MASK = 3
VIEW_OUTSIDE = 0
VIEW_PLAYER = 4
VIEW_NPC = 8
VIEW_ITEM = 16
VIEW_ITEM_KIND = 32


def check_view_args(player: int, radius: int) -> None:
    """ValueError for a player other than 0 / 1 or a radius outside
    1..VIEW_MAX_RADIUS (what orx_view refuses with ORX_EINVAL)."""
    check_player(player)
    check_radius(radius)


def render_view(snap: dict, cfg, player: int, radius: int, bank=None, health: bool = False):
    """The window of ``player`` (0 / 1) of every game of a ``snapshot()``-shaped
    dict: ``cells`` uint8 [B, V, V]; with ``health`` also the uint8 [B, V, V]
    health plane (the flagged occupant's health clamped to 0..255: the other
    player's where VIEW_PLAYER is set, else the NPC's; 0 elsewhere) as
    ``(cells, health)``.  ``bank``: the DungeonBank of a configuration with
    layouts (made from ``cfg.layouts`` when omitted; the snapshot then has
    ``p_layout``)."""
    check_view_args(player, radius)
    W, H, K, R = int(cfg.width), int(cfg.height), int(cfg.n_npcs), int(radius)
    V = 2 * R + 1
    bank = bank_of(cfg, bank)
    p, q = int(player), 1 - int(player)
    px, py, d = i64(snap["p_x"][p]), i64(snap["p_y"][p]), i64(snap["p_depth"][p])
    B = len(px)
    x, y = window_cells(px, py, R)
    inside, tile = tile_at(cfg, snap, p, x, y, None if bank is None else bank.layouts,
                           stair_on_border=True)
    cells = np.where(inside, tile, VIEW_OUTSIDE).astype(np.uint8)
    hp = np.zeros((B, V, V), np.uint8)

    def mark(games, ex, ey, bits, hval=None):
        """ORs ``bits`` into the window cell of grid cell (ex, ey) of the
        ``games`` (bool [B]) where it lies inside the window and the grid."""
        i, j = ex - px + R, ey - py + R
        ok = games & (i >= 0) & (i < V) & (j >= 0) & (j < V) & (ex >= 0) & (ex < W) \
            & (ey >= 0) & (ey < H)
        g = np.flatnonzero(ok)
        cells[g, j[g], i[g]] |= np.broadcast_to(np.asarray(bits, np.uint8), (B,))[g]
        if hval is not None:
            hp[g, j[g], i[g]] = np.clip(hval[g], 0, 255).astype(np.uint8)

    on_npc_depth = d == npc_depth(cfg)
    if K and int(cfg.flags) & EXT_ITEMS and "item_mask" in snap:
        on, ix, iy, kind = item_rows(snap, K)
        for k in range(K):
            mark(on_npc_depth & on[k], ix[k], iy[k], VIEW_ITEM + VIEW_ITEM_KIND * kind[k])
    if K:
        alive, nx, ny, nhp = npc_rows(snap, K)
        for k in range(K):
            mark(on_npc_depth & alive[k], nx[k], ny[k], VIEW_NPC, nhp[k])
    # the other player last: its health takes the health byte
    mark(i64(snap["p_depth"][q]) == d, i64(snap["p_x"][q]), i64(snap["p_y"][q]), VIEW_PLAYER,
         i64(snap["p_health"][q]))
    return (cells, hp) if health else cells


def decode(cells) -> dict:
    """The planes of a window of cell codes (a numpy array or a torch tensor,
    any shape), for a learner that wants channels: ``tile`` (uint8: 0 outside
    the grid, else the Tile code) and the boolean planes ``outside``,
    ``ground``, ``wall``, ``staircase``, ``player``, ``npc``, ``item`` and
    ``item_kind``."""
    tile = cells & VIEW_TILE_MASK
    return {"tile": tile,
            "outside": tile == VIEW_OUTSIDE,
            "ground": tile == int(Tile.Ground),
            "wall": tile == int(Tile.Wall),
            "staircase": tile == int(Tile.StaircaseDown),
            "player": (cells & VIEW_PLAYER) != 0,
            "npc": (cells & VIEW_NPC) != 0,
            "item": (cells & VIEW_ITEM) != 0,
            "item_kind": (cells & VIEW_ITEM_KIND) != 0}


def encode(planes: dict) -> np.ndarray:
    """The cell codes of ``decode``'s planes (numpy; its inverse)."""
    out = np.asarray(planes["tile"]).astype(np.uint8) & VIEW_TILE_MASK
    for name, bit in (("player", VIEW_PLAYER), ("npc", VIEW_NPC), ("item", VIEW_ITEM),
                      ("item_kind", VIEW_ITEM_KIND)):
        out = out | (np.asarray(planes[name]).astype(np.uint8) * np.uint8(bit))
    return out.astype(np.uint8)
