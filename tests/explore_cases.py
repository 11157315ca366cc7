"""The configurations tests/test_explore.py (CPU, oracle states) and
tests/test_gpu_explore.py (engine states) check the remembered map on, an
independent restatement of its rule (include/orx_explore.h) for one game in the
reference's schema, a breadth-first search over known Ground cells, and what
the coverage conditions count.

The restatement keeps, per game and player, a plain Python set of grid cells
and the (episode, depth, tick) it belongs to; what a player sees comes from
sight_cases.expected_seen (exact rationals, grid coordinates).

Cases: ``m``, sight_cases' ``wg`` bank (12 x 10, 3 layouts) with episodes of 25
ticks, a StaircaseBot that descends and a RandomBot, radius 2 -- maps are
cleared by descents and by new episodes, and cells drop out of sight while they
stay known; ``x``, a 40 x 8 bank (two map words per row) whose players cross
x = 32 inside a radius-5 window; view_cases' ``a`` (no bank) and ``e`` (4 x 4:
the window is larger than the grid).
"""
from collections import deque

import numpy as np

import sight_cases as sc
import view_cases as vc

N_GAMES = vc.N_GAMES
GROUND, WALL, STAIR = 1, 2, 3
TALLY_KEYS = ("cleared_by_depth", "cleared_by_episode", "known_unseen_cells", "gained",
              "gained_nothing", "stairs_known", "stairs_unknown")


def cases():
    """name -> dict(cfg, seed, ticks, policies, radius): ``ticks`` states -- the
    reset state and the one after each of ``ticks`` - 1 engine ticks -- the
    map updated in each."""
    from optimax_rogue_amd import DungeonBank, EnvConfig
    wg = sc.cases()["wg"]["cfg"]
    wide = DungeonBank.random(40, 8, 3, seed=5, wall_p=0.15, connected=True)
    v = vc.cases()
    return {
        "m": dict(cfg=EnvConfig(width=12, height=10, n_npcs=6, max_ticks=25, layouts=wg.layouts),
                  seed=31, ticks=60, policies=(2, 1), radius=2),
        "x": dict(cfg=EnvConfig(width=40, height=8, n_npcs=2, max_ticks=40, layouts=wide.layouts),
                  seed=32, ticks=30, policies=(1, 1), radius=5),
        "a": dict(v["a"], ticks=40, radius=2),
        "e": dict(v["e"], ticks=12, radius=5),
    }


class Memory:
    """One player's remembered map of one game, in grid coordinates."""

    def __init__(self):
        self.cells, self.where, self.tick = set(), None, None

    def update(self, gs, player, radius, episode, tick):
        """Adds what the player sees in ``gs`` (compat.GameStateView); returns
        (why the map was cleared or None, gained, seen cells)."""
        viewer = gs.iden_lookup[1 + player]
        where, why = (int(episode), int(viewer.depth)), None
        if self.where is not None:
            if where[0] != self.where[0]:
                why = "episode"
            elif where[1] != self.where[1]:
                why = "depth"
            elif tick < self.tick:
                why = "tick"
        if why:
            self.cells = set()
        self.where, self.tick = where, int(tick)
        vis = sc.expected_seen(gs, player, radius)
        seen = {(int(viewer.x) + i - radius, int(viewer.y) + j - radius)
                for j, i in zip(*np.nonzero(vis))}
        gained = len(seen - self.cells)
        self.cells |= seen
        return why, gained, seen

    def known(self, W, H):
        k = np.zeros((W, H), bool)
        for x, y in self.cells:
            k[x, y] = True
        return k


def remembered(cells, health, viewer, radius, seen, known, W, H):
    """The remembered planes of one window (uint8 [V, V] view codes and
    health), cell by cell."""
    V = 2 * radius + 1
    out, hp = np.zeros((V, V), np.uint8), np.zeros((V, V), np.uint8)
    for j in range(V):
        for i in range(V):
            x, y = int(viewer.x) + i - radius, int(viewer.y) + j - radius
            if not (0 <= x < W and 0 <= y < H):
                continue
            if (x, y) in seen:
                out[j, i], hp[j, i] = cells[j, i] | 64 | 128, health[j, i]
            elif (x, y) in known:
                out[j, i] = (cells[j, i] & 3) | 128
    return out, hp


def walk_known(tiles, known, start):
    """dict cell -> moves from ``start`` over known Ground cells only (the
    start itself whatever it is), breadth first."""
    W, H = len(tiles), len(tiles[0])
    dist, queue = {start: 0}, deque([start])
    while queue:
        x, y = queue.popleft()
        for nx, ny in ((x, y - 1), (x + 1, y), (x, y + 1), (x - 1, y)):
            if 0 <= nx < W and 0 <= ny < H and (nx, ny) not in dist and (nx, ny) in known \
                    and tiles[nx][ny] == GROUND:
                dist[nx, ny] = dist[x, y] + 1
                queue.append((nx, ny))
    return dist


def frontier_cells(tiles, known):
    """The frontier of a set of known cells, as a set."""
    W, H = len(tiles), len(tiles[0])
    return {(x, y) for x, y in known if tiles[x][y] == GROUND and any(
        0 <= nx < W and 0 <= ny < H and (nx, ny) not in known
        for nx, ny in ((x, y - 1), (x + 1, y), (x, y + 1), (x - 1, y)))}


def add_up(tallies):
    total = {k: 0 for k in TALLY_KEYS}
    for c in tallies:
        for k, v in c.items():
            total[k] += v
    return total


def tiles_of(cfg, snap, player, bank):
    """int64 [B, W, H]: the Tile codes of ``player``'s dungeon in every game."""
    from optimax_rogue_amd.query import tile_at
    B, W, H = len(snap["p_x"][player]), int(cfg.width), int(cfg.height)
    X = np.broadcast_to(np.arange(W)[None, :, None], (B, W, H))
    Y = np.broadcast_to(np.arange(H)[None, None, :], (B, W, H))
    return tile_at(cfg, snap, player, X, Y, None if bank is None else bank.layouts)[1]
