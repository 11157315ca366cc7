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
from .path import PATH_UNREACHABLE, PATH_WALL, Walk, fill_column, seek_columns
from .query import bank_of, check_player, check_radius, i64, inside_grid, tile_at, window_cells
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


def remembered(memory, key, snap: dict, cfg, p: int, bank=None):
    """``(ok, known, tiles)`` of player ``p``'s map: bool [B], where the key is
    valid for ``snap`` and the player stands in the grid; ``unpack(memory)``,
    bool [B, W, H]; and the Tile codes [B, W, H] of the dungeon the player is
    in -- its layout (clamped into the bank) of ``bank``, else the empty
    room's."""
    W, H = int(cfg.width), int(cfg.height)
    ok = valid(key, snap, p) & inside_grid(cfg, i64(snap["p_x"][p]), i64(snap["p_y"][p]))
    if bank is None:
        X, Y = (np.broadcast_to(a, (len(ok), W, H)) for a in np.indices((W, H)))
        tiles = tile_at(cfg, snap, p, X, Y)[1]
    else:
        lay = np.clip(i64(snap["p_layout"][p]), 0, len(bank.layouts) - 1)
        tiles = bank.layouts[lay].astype(np.int64) & 3
    return ok, unpack(memory, W), tiles


def neighbours(cells) -> np.ndarray:
    """bool [..., W, H]: the in-grid 4-neighbours of bool [..., W, H] cells."""
    c = np.asarray(cells, bool)
    out = np.zeros(c.shape, bool)
    out[..., 1:, :] |= c[..., :-1, :]
    out[..., :-1, :] |= c[..., 1:, :]
    out[..., :, 1:] |= c[..., :, :-1]
    out[..., :, :-1] |= c[..., :, 1:]
    return out


def frontier(known, tiles) -> np.ndarray:
    """bool [..., W, H]: the frontier cells of ``known`` (bool [..., W, H]) on
    ``tiles`` (Tile codes of the same shape): known, Ground, and an in-grid
    4-neighbour that is not known."""
    k = np.asarray(known, bool)
    return k & (np.asarray(tiles) == int(Tile.Ground)) & neighbours(~k)


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
    p = int(player)
    bank = bank_of(cfg, bank)
    W, H = int(cfg.width), int(cfg.height)
    px, py = i64(snap["p_x"][p]), i64(snap["p_y"][p])
    B = len(px)
    games = np.arange(B)
    ok, known, tiles = remembered(memory, key, snap, cfg, p, bank)
    walk = Walk(cfg, snap, p, bank)
    X, Y = (np.broadcast_to(a, (B, W, H)) for a in np.indices((W, H)))
    d = np.minimum(walk.between(px[:, None, None], py[:, None, None], X, Y), PATH_UNREACHABLE)
    out = seek_columns((B,), np.int32)
    columns = ((EXPLORE_FRONTIER, frontier(known, tiles)),
               (EXPLORE_STAIRS, known & (tiles == int(Tile.StaircaseDown))))
    for col, cells in columns:
        # absent above unreachable above every distance: argmin takes the lowest cell
        v = np.where(cells & ok[:, None, None], d, PATH_WALL).reshape(B, W * H)
        best = v.argmin(axis=1)
        own = v[games, best]
        fill_column(out, col, own != PATH_WALL, own,
                    walk.first_move(px, py, best // H, best % H, own), best)
    return out


def explorer_moves(dist, move) -> np.ndarray:
    """int8 [B], ready as ``actions``: the frontier column's move where its
    distance is > 0, else the stairs column's where its distance is > 0, else
    Stay -- explore the depth, then descend."""
    dist, move = np.asarray(dist), np.asarray(move)
    return np.where(dist[:, EXPLORE_FRONTIER] > 0, move[:, EXPLORE_FRONTIER],
                    np.where(dist[:, EXPLORE_STAIRS] > 0, move[:, EXPLORE_STAIRS],
                             int(Move.Stay))).astype(np.int8)
