"""The configurations tests/test_sight.py (CPU, oracle states) and
tests/test_gpu_sight.py (engine states) check the line of sight on, an
independent restatement of the rule (include/orx_sight.h) for one game in the
reference's schema, and what the coverage conditions count.

The cases are view_cases' ``a``, ``c``, ``d`` and ``e`` and one more, ``w``: a
12 x 10 bank of connected layouts at wall density 0.3 (rooms and corridors),
with ``wg``, the same bank as the engine accepts it.
Seeds and ticks were picked on the CPU so that the ORACLE's states alone meet
every coverage condition test_sight.py asserts; the engine is bit-exact with
the oracle, so the GPU test sees the same states.
"""
from fractions import Fraction
from math import ceil, floor

import numpy as np

import view_cases as vc

N_GAMES = vc.N_GAMES
RADII = (1, 5, 15)
WALL, HALF = 2, Fraction(1, 2)


def cases():
    """name -> dict(cfg, seed, ticks, policies, radii), as view_cases.cases()."""
    from optimax_rogue_amd import DungeonBank, EnvConfig
    out = {k: v for k, v in vc.cases().items() if k in ("a", "c", "d", "e")}
    bank = DungeonBank.random(12, 10, 4, seed=7, wall_p=0.3, connected=True)
    out["w"] = dict(cfg=EnvConfig(width=12, height=10, n_npcs=6, layouts=bank.layouts), seed=31,
                    ticks=20, policies=(1, 1), radii=RADII)
    # wg: w's bank without the layout that ``connected`` left 2 Ground tiles (its
    # staircase sits in a pocket).  The oracle plays w as it is; BatchedEngine
    # refuses a bank with a layout of fewer than n_npcs + 2 Ground tiles, so the
    # GPU tests run wg where the CPU tests run w and wg
    roomy = bank.layouts[(bank.layouts == 1).sum(axis=(1, 2)) >= 6 + 2]
    assert len(roomy) == 3
    out["wg"] = dict(out["w"], cfg=EnvConfig(width=12, height=10, n_npcs=6, layouts=roomy))
    return out


CPU_CASES = ("a", "c", "e", "w", "wg")    # (d, 20 x 20 with 40 NPCs, is the GPU test's alone)
GPU_CASES = ("a", "c", "d", "e", "wg")


def sign(v):
    return (v > 0) - (v < 0)


def line(dx, dy, half_up):
    """The intermediate offsets of the line to (dx, dy): s |d| / n rounded half
    up or half down, with exact rationals."""
    n = max(abs(dx), abs(dy))
    rnd = (lambda q: floor(q + HALF)) if half_up else (lambda q: ceil(q - HALF))
    return [(sign(dx) * rnd(Fraction(s * abs(dx), n)), sign(dy) * rnd(Fraction(s * abs(dy), n)))
            for s in range(1, n)]


_LINES = {}


def lines(dx, dy):
    if (dx, dy) not in _LINES:
        _LINES[dx, dy] = (line(dx, dy, True), line(dx, dy, False))
    return _LINES[dx, dy]


def sees(tiles, vx, vy, x, y):
    """Whether grid cell (x, y) is clear from (vx, vy) on ``tiles`` [W, H]."""
    return any(all(tiles[vx + ox][vy + oy] != WALL for ox, oy in ln)
               for ln in lines(x - vx, y - vy))


def expected_seen(gs, player, radius):
    """bool [V, V] of ``player`` (0 / 1) of one game in the reference's schema
    (compat.GameStateView), by the header's rule in GRID coordinates: every
    cell of the viewer's dungeon within the window is looked at from the
    viewer's cell; cells outside the grid are never seen."""
    R, V = radius, 2 * radius + 1
    viewer = gs.iden_lookup[1 + player]
    tiles = np.asarray(gs.world.get_at_depth(viewer.depth).tiles).tolist()
    W, H = len(tiles), len(tiles[0])
    vx, vy = int(viewer.x), int(viewer.y)
    xs = range(max(0, vx - R), min(W, vx + R + 1))
    ys = range(max(0, vy - R), min(H, vy + R + 1))
    clear = {(x, y): sees(tiles, vx, vy, x, y) for x in xs for y in ys}
    seen = np.zeros((V, V), bool)
    for (x, y), ok in clear.items():
        if not ok and tiles[x][y] == WALL:
            sx, sy = sign(x - vx), sign(y - vy)
            ok = any(clear[x - a, y - b] and tiles[x - a][y - b] != WALL
                     for a in {0, sx} for b in {0, sy} if (a, b) != (0, 0))
        seen[y - vy + R, x - vx + R] = ok
    return seen


def tally(cells, vis):
    """The coverage counts of windows of view codes [B, V, V] and their seen
    cells: the other player and the NPCs seen / unseen, and the walls seen
    only through the neighbour rule (not clear by a line of their own)."""
    from optimax_rogue_amd import sight
    walls = (cells & 3) == WALL
    # a wall's own lines: ``clear``, recomputed from the reference's line tables
    lines_, _ = sight._tables(cells.shape[1] // 2)
    B, V = cells.shape[0], cells.shape[1]
    opq = np.concatenate([walls.reshape(B, V * V), np.zeros((B, 1), bool)], axis=1)
    clear = ~opq[:, lines_].any(axis=3).all(axis=2).reshape(B, V, V)
    return {"player_seen": int(((cells & 4) != 0)[vis].sum()),
            "player_unseen": int(((cells & 4) != 0)[~vis].sum()),
            "npc_seen": int(((cells & 8) != 0)[vis].sum()),
            "npc_unseen": int(((cells & 8) != 0)[~vis].sum()),
            "walls_by_neighbour": int((walls & vis & ~clear).sum())}


def add_up(tallies):
    total = {}
    for c in tallies:
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    return total


def sees_other(snap, vis, player, radius):
    """bool [B]: the other player is on ``player``'s depth, in its window and
    seen (numpy; what BatchedEngine.sees_other answers)."""
    p, q, R = player, 1 - player, radius
    i = np.asarray(snap["p_x"][q], np.int64) - np.asarray(snap["p_x"][p], np.int64) + R
    j = np.asarray(snap["p_y"][q], np.int64) - np.asarray(snap["p_y"][p], np.int64) + R
    near = (np.asarray(snap["p_depth"][p]) == np.asarray(snap["p_depth"][q])) \
        & (i >= 0) & (i <= 2 * R) & (j >= 0) & (j <= 2 * R)
    b = np.arange(len(i))
    return near & vis[b, np.clip(j, 0, 2 * R), np.clip(i, 0, 2 * R)]
