"""The map a player remembers, on the host: ``update`` and ``seek`` in numpy.

``sight.visible`` is what a player sees this tick.  ``BatchedEngine.explore``
/ ``explore_seek`` keep what it saw earlier on the GPU (``orx_explore_update``
/ ``orx_explore_seek``, include/orx_explore.h); this module is the same
contract restated for a ``snapshot()``-shaped dict -- the truth the GPU tests
compare against.  It needs numpy only (no torch, no built library).

The map: ``memory`` uint32 [B, H, WW] with ``WW = words(W)``; bit ``x % 32`` of
``memory[b, y, x // 32]`` is set when the player has seen grid cell (x, y) on
its present depth in the present episode.  ``key`` int32 [B, 4] is {episode,
depth, tick, known}; it is *valid* for a state when ``known >= 0``, episode
and depth are the state's and its tick is not ahead of the state's.  A map
whose key is not valid is cleared by the next ``update``.

A *frontier* cell is known, Ground, and has an in-grid 4-neighbour that is not
known.  Every shortest walk to a NEAREST frontier cell passes only known Ground
cells (the cell before the first unknown one would be a nearer frontier cell),
so the explorer -- walk to the nearest frontier cell until there is none --
never uses knowledge the player lacks.
"""
from __future__ import annotations

import numpy as np

from .enums import Move, Tile
from .path import (PATH_UNREACHABLE, PATH_WALL, SEEK_ABSENT, SEEK_COLS, SEEK_UNREACHABLE,
                   move_toward, room_distance)
from .query import (MOVE_DELTAS, check_player, check_radius, i64, inside_grid, tile_at,
                    window_cells)
from .sight import SIGHT_SEEN, unpack_rows
from .view import VIEW_TILE_MASK

# include/orx_explore.h
EXPLORE_KNOWN = 128
EXPLORE_FRONTIER, EXPLORE_STAIRS = 0, 1


def words(W: int) -> int:
    """uint32 words of a map row of ``W`` cells."""
    return (int(W) + 31) // 32


def empty(B: int, W: int, H: int):
    """``(memory, key)`` of ``B`` fresh maps: all-zero memory, the key -1."""
    return np.zeros((B, H, words(W)), np.uint32), np.full((B, 4), -1, np.int32)


def valid(key, snap: dict, player: int) -> np.ndarray:
    """bool [B]: the key rows that are valid for ``player`` of ``snap``."""
    k = i64(key)
    return (k[:, 3] >= 0) & (k[:, 0] == i64(snap["episode"])) \
        & (k[:, 1] == i64(snap["p_depth"][player])) & (k[:, 2] <= i64(snap["tick"]))


def unpack(memory, W: int) -> np.ndarray:
    """bool [B, W, H]: ``known[b, x, y]`` of uint32 [B, H, WW] map words."""
    m = np.asarray(memory).astype(np.uint32)
    bits = ((m[:, :, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)
    return np.ascontiguousarray(bits.reshape(m.shape[0], m.shape[1], -1)[:, :, :W].transpose(0, 2, 1))


def pack(known) -> np.ndarray:
    """uint32 [B, H, WW] of bool [B, W, H] (``unpack``'s inverse)."""
    k = np.asarray(known, bool)
    B, W, H = k.shape
    padded = np.zeros((B, H, words(W) * 32), bool)
    padded[:, :, :W] = k.transpose(0, 2, 1)
    weights = np.uint32(1) << np.arange(32, dtype=np.uint32)
    return (padded.reshape(B, H, -1, 32) * weights).sum(axis=3, dtype=np.uint32)


def update(memory, key, snap: dict, cfg, player: int, radius: int, rows, cells=None,
           health=None) -> np.ndarray:
    """orx_explore_update on numpy arrays, in place: adds the cells that
    ``rows`` (uint32 [B, V], ``sight.pack_rows``) marks seen to ``memory`` /
    ``key`` -- a map whose key is not valid for ``snap`` is cleared first -- and
    returns ``gained`` int32 [B], the number of cells newly known.  Bits >= V
    and bits of cells outside the grid are ignored.  ``cells`` / ``health``
    (uint8 [B, V, V], ``view.render_view``'s) become the remembered view: a
    seen cell ``code | SIGHT_SEEN | EXPLORE_KNOWN`` with its health, a known
    cell not seen now ``tile | EXPLORE_KNOWN`` with health 0, any other 0."""
    check_player(player)
    check_radius(radius)
    p, R, V = int(player), int(radius), 2 * int(radius) + 1
    W = int(cfg.width)
    px, py = i64(snap["p_x"][p]), i64(snap["p_y"][p])
    B = len(px)
    memory[~valid(key, snap, p)] = 0
    known = unpack(memory, W)
    x, y = window_cells(px, py, R)
    inside = inside_grid(cfg, x, y)
    seen = unpack_rows(np.asarray(rows).astype(np.uint32).reshape(B, V), V) & inside
    b = np.broadcast_to(np.arange(B)[:, None, None], x.shape)
    before = known.sum(axis=(1, 2))
    known[b[seen], x[seen], y[seen]] = True
    after = known.sum(axis=(1, 2))
    memory[...] = pack(known)
    key[...] = np.stack([i64(snap["episode"]), i64(snap["p_depth"][p]), i64(snap["tick"]), after],
                        axis=1).astype(np.int32)
    if cells is not None:
        kn = inside & known[b, np.clip(x, 0, W - 1), np.clip(y, 0, int(cfg.height) - 1)]
        c = np.asarray(cells, np.uint8)
        cells[...] = np.where(seen, c | np.uint8(SIGHT_SEEN | EXPLORE_KNOWN),
                              np.where(kn, (c & np.uint8(VIEW_TILE_MASK)) | np.uint8(EXPLORE_KNOWN),
                                       0)).astype(np.uint8)
    if health is not None:
        health[...] = np.where(seen, np.asarray(health, np.uint8), 0).astype(np.uint8)
    return (after - before).astype(np.int32)


def frontier(known, tiles) -> np.ndarray:
    """bool [..., W, H]: the frontier cells of ``known`` (bool [..., W, H]) on
    ``tiles`` (Tile codes of the same shape): known, Ground, and an in-grid
    4-neighbour that is not known."""
    k = np.asarray(known, bool)
    un = ~k
    edge = np.zeros(k.shape, bool)
    edge[..., 1:, :] |= un[..., :-1, :]
    edge[..., :-1, :] |= un[..., 1:, :]
    edge[..., :, 1:] |= un[..., :, :-1]
    edge[..., :, :-1] |= un[..., :, 1:]
    return k & (np.asarray(tiles) == int(Tile.Ground)) & edge


def seek(memory, key, snap: dict, cfg, player: int, bank=None):
    """orx_explore_seek on numpy arrays: ``(dist, move, target)``, int32, int8
    and int32 [B, SEEK_COLS], of ``player`` (0 / 1) of every game: column
    EXPLORE_FRONTIER the nearest frontier cell of its map, EXPLORE_STAIRS the
    nearest known StaircaseDown; columns 2 and 3 pad.

    dist    the least walking distance over the column's targets --
            ``bank.pair_field()[layout, target, own]`` with a bank (made from
            ``cfg.layouts`` when omitted), else ``path.room_distance``;
            SEEK_UNREACHABLE when none can be reached, SEEK_ABSENT without a
            target, with a key that is not valid, or off the grid
    target  the flat cell ``x * H + y`` attaining it, the lowest on a tie (and
            the lowest target where none can be reached); -1 when absent
    move    the first of Up, Right, Down, Left whose neighbour cell is at
            ``dist - 1`` from the target -- a staircase neighbour only if it is
            the target; Stay when ``dist <= 0``"""
    check_player(player)
    if bank is None and getattr(cfg, "layouts", None) is not None:
        from .dungeons import DungeonBank
        bank = DungeonBank(cfg.layouts)
    p = int(player)
    W, H = int(cfg.width), int(cfg.height)
    WH = W * H
    px, py = i64(snap["p_x"][p]), i64(snap["p_y"][p])
    B = len(px)
    games = np.arange(B)
    ok = valid(key, snap, p) & inside_grid(cfg, px, py)
    known = unpack(memory, W)
    X = np.broadcast_to(np.arange(W)[None, :, None], (B, W, H))
    Y = np.broadcast_to(np.arange(H)[None, None, :], (B, W, H))
    flat = lambda u, v: np.clip(u, 0, W - 1) * H + np.clip(v, 0, H - 1)
    own = flat(px, py)
    if bank is None:
        sx, sy = i64(snap["st_x"][p]), i64(snap["st_y"][p])
        tiles = tile_at(cfg, snap, p, X, Y)[1]
        g = (slice(None), None, None)
        d = room_distance(cfg, sx[g], sy[g], px[g], py[g], X, Y).reshape(B, WH)
    else:
        pairs = bank.pair_field()
        lay = np.clip(i64(snap["p_layout"][p]), 0, len(pairs) - 1)
        tiles = bank.layouts[lay].astype(np.int64) & 3
        d = pairs[lay[:, None], np.arange(WH)[None, :], own[:, None]].astype(np.int64)
    d = np.minimum(d, PATH_UNREACHABLE)

    def between(x, y, tc):
        """From cells (x, y) to flat target cells ``tc``, int64 [B]."""
        if bank is None:
            v = room_distance(cfg, sx, sy, x, y, tc // H, tc % H)
        else:
            v = pairs[lay, tc, flat(x, y)].astype(np.int64)
        return np.where(inside_grid(cfg, x, y), v, PATH_WALL)

    def is_stair(x, y):
        return inside_grid(cfg, x, y) & (tiles[games, np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)]
                                         == int(Tile.StaircaseDown))

    dist = np.full((B, SEEK_COLS), SEEK_ABSENT, np.int32)
    move = np.full((B, SEEK_COLS), int(Move.Stay), np.int8)
    target = np.full((B, SEEK_COLS), -1, np.int32)
    columns = ((EXPLORE_FRONTIER, frontier(known, tiles)),
               (EXPLORE_STAIRS, known & (tiles == int(Tile.StaircaseDown))))
    for col, cells in columns:
        # absent above unreachable above every distance: argmin takes the lowest cell
        v = np.where(cells.reshape(B, WH) & ok[:, None], d, PATH_WALL)
        best = v.argmin(axis=1)
        here = v[games, best]
        has = here != PATH_WALL
        bx, by = best // H, best % H
        near = []
        for _, dx, dy in MOVE_DELTAS:
            x, y = px + dx, py + dy
            near.append(np.where(is_stair(x, y) & ~((x == bx) & (y == by)), PATH_WALL,
                                 between(x, y, best)))
        dist[:, col] = np.where(has, np.where(here == PATH_UNREACHABLE, SEEK_UNREACHABLE, here),
                                SEEK_ABSENT)
        move[:, col] = np.where(has, move_toward(here, *near), int(Move.Stay))
        target[:, col] = np.where(has, best, -1)
    return dist, move, target


def explorer_moves(dist, move) -> np.ndarray:
    """int8 [B], ready as ``actions``: the frontier column's move where its
    distance is > 0, else the stairs column's where its distance is > 0, else
    Stay -- explore the depth, then descend."""
    dist, move = np.asarray(dist), np.asarray(move)
    return np.where(dist[:, EXPLORE_FRONTIER] > 0, move[:, EXPLORE_FRONTIER],
                    np.where(dist[:, EXPLORE_STAIRS] > 0, move[:, EXPLORE_STAIRS],
                             int(Move.Stay))).astype(np.int8)
