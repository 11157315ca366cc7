"""The banks tests/test_path.py (CPU) and tests/test_gpu_path.py check the
staircase distance field on, and an independent statement of that field.

Every bank is built by hand or by ``DungeonBank.random`` with a fixed seed;
the host field of each is computed once per process (``truth``) and shared.
"""
import functools

import numpy as np

GROUND, WALL, STAIR = 1, 2, 3


def room(W, H):
    """A W x H layout with a Wall border and an open interior (no staircase)."""
    t = np.full((W, H), GROUND, np.uint8)
    t[[0, -1], :] = WALL
    t[:, [0, -1]] = WALL
    return t


def serpentine(W=64, H=64):
    """Interior Wall columns at x = 2, 4, ..., the k-th with its one gap at
    y = 1 for even k and at y = H - 2 for odd k; the staircase at (1, H - 2).
    One corridor of (W / 2 - 1) * (H - 3) + W - 4 + 1 cells: the field needs
    that many breadth-first levels, far more than W + H."""
    t = room(W, H)
    for k, x in enumerate(range(2, W - 1, 2)):
        t[x, 1:H - 1] = WALL
        t[x, 1 if k % 2 == 0 else H - 2] = GROUND
    t[1, H - 2] = STAIR
    return t


def pocket(W=64, H=64):
    """A room with two staircases and a sealed pocket of 3 x 3 Ground tiles
    (a Wall ring around x, y in 11..13)."""
    t = room(W, H)
    t[10:15, 10:15] = WALL
    t[11:14, 11:14] = GROUND
    t[5, 5] = STAIR
    t[W - 14, H - 24] = STAIR
    return t


def long_walls(W=256, H=256):
    """A room cut by a few long walls with one gap each, alternating ends, and
    one wall along x; the staircase in a corner."""
    t = room(W, H)
    for k, x in enumerate((40, 90, 150, 200)):
        t[x, 1:H - 1] = WALL
        t[x, 3 if k % 2 == 0 else H - 4] = GROUND
    t[41:90, 128] = WALL
    t[60, 128] = GROUND
    t[2, H - 3] = STAIR
    return t


def open_room(W, H, sx, sy):
    t = room(W, H)
    t[sx, sy] = STAIR
    return t


@functools.lru_cache(maxsize=None)
def banks():
    """name -> uint8 [L, W, H] layouts: the banks the issue lists."""
    from optimax_rogue_amd import DungeonBank
    tiny = room(3, 3)
    tiny[1, 1] = STAIR
    small = room(3, 4)
    small[1, 2] = STAIR
    out = {
        "3x3": tiny[None],
        "3x4": small[None],
        "9x8": DungeonBank.random(9, 8, 16, seed=0).layouts,
        "17x5": DungeonBank.random(17, 5, 8, seed=0, wall_p=0.3, n_stairs=2).layouts,
        "64x64": np.stack([open_room(64, 64, 40, 7), serpentine(), pocket()]),
        "9x8x300": DungeonBank.random(9, 8, 300, seed=3, wall_p=0.25).layouts,
        "256x256": np.stack([open_room(256, 256, 200, 31), long_walls()]),
    }
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def truth(name):
    """``path.stair_field`` of a bank of ``banks()``, computed once."""
    from optimax_rogue_amd.path import stair_field
    f = stair_field(banks()[name])
    f.setflags(write=False)
    return f


def dijkstra_field(layout):
    """The field of one [W, H] layout by an independent route: scipy's
    Dijkstra over the grid graph (an edge of weight 1 between every two
    4-adjacent tiles that are both not Wall), from all staircases at once."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    t = np.asarray(layout)
    W, H = t.shape
    open_ = t != WALL
    idx = np.arange(W * H).reshape(W, H)
    rows, cols = [], []
    for a, b in ((np.s_[:-1, :], np.s_[1:, :]), (np.s_[:, :-1], np.s_[:, 1:])):
        ok = open_[a] & open_[b]
        rows += [idx[a][ok], idx[b][ok]]
        cols += [idx[b][ok], idx[a][ok]]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    g = coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(W * H, W * H)).tocsr()
    d = dijkstra(g, directed=False, indices=np.flatnonzero(t == STAIR), min_only=True)
    out = np.where(np.isinf(d), 0xFFFE, d).astype(np.int64).reshape(W, H)
    return np.where(open_, out, 0xFFFF).astype(np.uint16)


def walk_cfg(**kw):
    """The device walk's configuration: a 9 x 8 bank with pockets, no NPCs, a
    Separated start with player 2 far below, no time limit in reach."""
    from optimax_rogue_amd import DungeonBank, EnvConfig
    bank = DungeonBank.random(9, 8, 16, seed=0, wall_p=0.3)
    return EnvConfig(width=9, height=8, n_npcs=0, start_mode=2, p1_depth=0, p2_depth=900,
                     max_ticks=100000, layouts=bank.layouts, **kw)
