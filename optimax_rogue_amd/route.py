"""Walking distances over the map a player remembers, on the host: ``planes``
and ``route`` in numpy.

``BatchedEngine.explore_route`` searches the remembered map on the GPU
(``orx_route``, include/orx_route.h); this module is the same contract restated
for a ``snapshot()``-shaped dict -- the truth the GPU tests compare against.
It needs numpy only (no torch, no built library), and no pair table.

A *known walk* from the player's cell (whatever its tile, known or not) to a
cell t is a 4-connected path whose interior cells are all known and Ground; t
must be known, and Ground or StaircaseDown.  The *known distance* is the number
of moves of the shortest one.  The search below is that sentence: a set of
reached cells, dilated by one move at a time, of which only the known Ground
cells (and the source) dilate further.
"""
from __future__ import annotations

import numpy as np

from .enums import Move, Tile
from .explore import frontier, neighbours, pack, remembered
from .path import SEEK_ABSENT, SEEK_UNREACHABLE, seek_columns
from .query import MOVE_DELTAS, bank_of, check_player, i64, inside_grid

# include/orx_route.h
ROUTE_FRONTIER, ROUTE_STAIRS, ROUTE_GOAL = 0, 1, 2

_FAR = np.int64(1) << 40      # no known walk (above every distance)


def planes(layouts) -> np.ndarray:
    """orx_route_planes: uint32 [L, 2, H, WW] of Tile codes uint8 [L, W, H] --
    plane 0 the Ground bits, plane 1 the StaircaseDown bits, in the map's own
    layout (``explore.pack``)."""
    t = np.asarray(layouts).astype(np.int64) & 3
    return np.stack([pack(t == int(Tile.Ground)), pack(t == int(Tile.StaircaseDown))], axis=1)


def known_distance(source, passable, ends) -> np.ndarray:
    """int64 [B, W, H]: the known distance from the ``source`` cell of every
    game (bool [B, W, H], at most one per game; distance 0) to every cell of
    ``passable | ends`` -- walks pass ``passable`` cells only and may end on an
    ``ends`` cell -- ``_FAR`` where there is none."""
    source, passable = np.asarray(source, bool), np.asarray(passable, bool)
    allowed = passable | np.asarray(ends, bool)
    dist = np.where(source, 0, _FAR)
    wave = source
    for k in range(1, source.shape[1] * source.shape[2] + 1):   # (no walk is longer)
        if not wave.any():
            break
        new = neighbours(wave) & allowed & (dist == _FAR)
        dist[new] = k
        wave = new & passable
    return dist


def route(memory, key, snap: dict, cfg, player: int, goal=None, bank=None):
    """orx_route on numpy arrays: ``(dist, move, target)``, int32, int8 and
    int32 [B, SEEK_COLS], of ``player`` (0 / 1) of every game.  Column
    ROUTE_FRONTIER: the frontier cells of its map (``explore.frontier``);
    ROUTE_STAIRS: the known StaircaseDown cells; ROUTE_GOAL: the one cell
    ``goal[b]`` (flat ``x * H + y``; absent when ``goal`` is None or the cell is
    outside ``[0, W * H)``); column 3 pads.  The tiles are ``bank``'s layouts
    (made from ``cfg.layouts`` when omitted), else the empty room's.

    dist    the least known distance over the column's targets;
            SEEK_UNREACHABLE where targets exist but none has a known walk (a
            goal that is not known, or neither Ground nor StaircaseDown, has
            none); SEEK_ABSENT without a target, with a key that is not valid,
            or off the grid
    target  the lowest flat cell among the targets at that distance, the lowest
            target where none is reachable; -1 when absent
    move    the first of Up, Right, Down, Left whose neighbour cell is in the
            grid, is known Ground or the target itself, and is at known
            distance ``dist - 1`` from the target; Stay when ``dist <= 0``"""
    check_player(player)
    p = int(player)
    W, H = int(cfg.width), int(cfg.height)
    WH = W * H
    px, py = i64(snap["p_x"][p]), i64(snap["p_y"][p])
    B = len(px)
    games = np.arange(B)
    ok, known, tiles = remembered(memory, key, snap, cfg, p, bank_of(cfg, bank))
    X, Y = (np.broadcast_to(a, (B, W, H)) for a in np.indices((W, H)))
    passable = known & (tiles == int(Tile.Ground))
    stairs = known & (tiles == int(Tile.StaircaseDown))
    ends = passable | stairs                      # where a known walk may end

    def one(x, y):
        """bool [B, W, H]: cell (x[b], y[b]) of game b, where it is in the grid."""
        return (X == x[:, None, None]) & (Y == y[:, None, None])

    cx, cy = np.clip(px, 0, W - 1), np.clip(py, 0, H - 1)
    from_own = known_distance(one(cx, cy), passable, stairs)
    if goal is None:
        goals = np.zeros((B, W, H), bool)
    else:
        g = i64(goal)
        assert g.shape == (B,), "goal is [B]"
        gin = (g >= 0) & (g < WH)
        goals = one(np.where(gin, g // H, -1), np.where(gin, g % H, -1))

    dist, move, target = seek_columns((B,), np.int32)
    columns = ((ROUTE_FRONTIER, frontier(known, tiles)), (ROUTE_STAIRS, stairs), (ROUTE_GOAL, goals))
    for col, cells in columns:
        cells = cells & ok[:, None, None]
        # no target above no walk above every distance: argmin takes the lowest cell
        v = np.where(cells, np.where(ends, from_own, _FAR), _FAR + 1).reshape(B, WH)
        best = v.argmin(axis=1)
        here = v[games, best]
        has, reached = here <= _FAR, here < _FAR
        bx, by = best // H, best % H
        # from the chosen target: the source expands whatever its tile
        back = known_distance(one(bx, by) & reached[:, None, None], passable, passable & False)
        mv = np.full(B, int(Move.Stay), np.int64)
        for m, dx, dy in reversed(MOVE_DELTAS):
            x, y = px + dx, py + dy
            at = back[games, np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)]
            mv = np.where(reached & (here > 0) & inside_grid(cfg, x, y) & (at == here - 1), int(m), mv)
        dist[:, col] = np.where(reached, here, np.where(has, SEEK_UNREACHABLE, SEEK_ABSENT))
        move[:, col] = mv
        target[:, col] = np.where(has, best, -1)
    return dist, move, target


def router_moves(dist, move) -> np.ndarray:
    """int8 [B], ready as ``actions``: the frontier column's move where its
    distance is > 0, else the stairs column's where its distance is > 0, else
    Stay -- explore the depth through what is known, then descend."""
    dist, move = np.asarray(dist), np.asarray(move)
    return np.where(dist[:, ROUTE_FRONTIER] > 0, move[:, ROUTE_FRONTIER],
                    np.where(dist[:, ROUTE_STAIRS] > 0, move[:, ROUTE_STAIRS],
                             int(Move.Stay))).astype(np.int8)


__all__ = ["ROUTE_FRONTIER", "ROUTE_STAIRS", "ROUTE_GOAL", "planes", "known_distance", "route",
           "router_moves"]
