"""The states tests/test_seek.py (CPU, oracle states) and tests/test_gpu_seek.py
(engine states) check ``seek`` on, and independent statements of the walking
distance and of the query: scipy's all-pairs search over the Ground-only graph
with the staircase end cells attached afterwards, and plain loops over the
entities of one game in the reference's schema.

Seeds and tick counts were picked on the CPU so that the ORACLE's states alone
meet every coverage condition test_seek.py asserts.  The engine is bit-exact
with the oracle, so the GPU test sees the same states.
"""
import functools

import numpy as np

import moves_cases as mc
import path_cases as pc
import view_cases as vc

N_GAMES = 200
WALL_V, FAR_V = 0xFFFF, 0xFFFE
UNREACHABLE, ABSENT, STAY = -1, -2, 5
BANKS = ("c", "pockets", "17x5", "items12", "dense", "moving")    # the cases on a dungeon bank


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(cfg=EnvConfig, seed, ticks, policies=(p1, p2))."""
    from optimax_rogue_amd import DungeonBank, EnvConfig
    from optimax_rogue_amd.enums import EXT_RPG
    bank = lambda *a, **kw: DungeonBank.random(*a, **kw).layouts
    out = {name: dict(case) for name, case in vc.cases().items()}
    out["rpg"] = dict(mc.cases()["rpg"], policies=(1, 1))
    out.update({
        "pockets": dict(cfg=EnvConfig(width=9, height=8, n_npcs=6,
                                      layouts=bank(9, 8, 16, seed=0, wall_p=0.3)),
                        seed=21, ticks=20, policies=(1, 1)),
        "17x5": dict(cfg=EnvConfig(width=17, height=5, n_npcs=4,
                                   layouts=bank(17, 5, 8, seed=0, wall_p=0.3, n_stairs=2)),
                     seed=22, ticks=16, policies=(1, 1)),
        "items12": dict(cfg=EnvConfig(width=12, height=12, n_npcs=8, flags=EXT_RPG,
                                      item_drop_pct=100,
                                      layouts=bank(12, 12, 4, seed=5, wall_p=0.25, n_stairs=2)),
                        seed=23, ticks=40, policies=(1, 1)),
        "dense": dict(cfg=EnvConfig(width=12, height=10, n_npcs=24,
                                    layouts=bank(12, 10, 4, seed=6, wall_p=0.2)),
                      seed=24, ticks=16, policies=(1, 1)),
        "moving": dict(cfg=EnvConfig(width=12, height=10, n_npcs=10, npc_policy=2,
                                     layouts=bank(12, 10, 4, seed=6, wall_p=0.2)),
                       seed=25, ticks=16, policies=(1, 1)),
    })
    return out


def scipy_pairs(layout):
    """uint16 [W * H, W * H] of one [W, H] layout by an independent route:
    scipy's all-pairs shortest paths over the graph of Ground tiles alone (an
    edge between every two 4-adjacent Ground tiles); then a staircase end cell
    is one move from its nearest Ground neighbour, two adjacent staircases are
    one move apart, and a cell is 0 from itself.  Wall rows seed nothing."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import shortest_path
    t = np.asarray(layout)
    W, H = t.shape
    n = W * H
    flat = t.reshape(-1)
    ground, stair = flat == pc.GROUND, flat == pc.STAIR
    idx = np.arange(n).reshape(W, H)
    ends = []
    for a, b in ((np.s_[:-1, :], np.s_[1:, :]), (np.s_[:, :-1], np.s_[:, 1:])):
        ends += [(idx[a].reshape(-1), idx[b].reshape(-1)), (idx[b].reshape(-1), idx[a].reshape(-1))]
    src, dst = np.concatenate([e[0] for e in ends]), np.concatenate([e[1] for e in ends])
    gg = ground[src] & ground[dst]
    g = coo_matrix((np.ones(int(gg.sum())), (src[gg], dst[gg])), shape=(n, n)).tocsr()
    d = shortest_path(g, method="D", directed=False, unweighted=True)
    d[~ground, :] = np.inf
    d[:, ~ground] = np.inf
    # one staircase end: through its Ground neighbours
    one = d.copy()
    for s, q in zip(src, dst):
        if stair[s] and ground[q]:
            one[s, :] = np.minimum(one[s, :], 1 + d[q, :])
            one[:, s] = np.minimum(one[:, s], 1 + d[:, q])
    # both ends staircases: a Ground neighbour of each, or adjacent
    two = one.copy()
    for s, q in zip(src, dst):
        if stair[s] and ground[q]:
            two[s, stair] = np.minimum(two[s, stair], 1 + one[q, stair])
        if stair[s] and stair[q]:
            two[s, q] = 1
    two[np.arange(n), np.arange(n)] = 0
    out = np.where(np.isinf(two), FAR_V, two).astype(np.int64)
    out[:, flat == pc.WALL] = WALL_V      # (a Wall's own row is unreachable off the Walls)
    return out.astype(np.uint16)


def scipy_rows(layouts, layout, cell):
    """``path.source_rows``'s contract from ``scipy_pairs``."""
    layouts = np.asarray(layouts)
    L, W, H = layouts.shape
    tables = {}
    rows = []
    for l, c in zip(layout, cell):
        lc = min(max(int(l), 0), L - 1)
        if lc not in tables:
            tables[lc] = scipy_pairs(layouts[lc])
        if 0 <= l < L and 0 <= c < W * H:
            rows.append(tables[lc][c])
        else:
            rows.append(np.where(layouts[lc].reshape(-1) == pc.WALL, WALL_V, FAR_V))
    return np.stack(rows).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def pair_truth(name):
    """``path.pair_field`` of a bank of path_cases.banks(), computed once."""
    from optimax_rogue_amd.path import pair_field
    f = pair_field(pc.banks()[name])
    f.setflags(write=False)
    return f


def room_layout(W, H, sx, sy):
    """EmptyDungeonGenerator's dungeon materialised: border Wall, one staircase."""
    return pc.open_room(W, H, sx, sy)


class Distances:
    """The walking distance between two cells of game ``i``'s dungeon of
    player ``p``, by ``scipy_pairs`` (tables cached per layout or staircase)."""

    def __init__(self, cfg, snap):
        self.cfg, self.snap, self.tables = cfg, snap, {}

    def table(self, p, i):
        cfg, snap = self.cfg, self.snap
        if cfg.layouts is not None:
            key = int(snap["p_layout"][p][i])
            layout = lambda: np.asarray(cfg.layouts)[key]
        else:
            key = (int(snap["st_x"][p][i]), int(snap["st_y"][p][i]))
            layout = lambda: room_layout(int(cfg.width), int(cfg.height), *key)
        if key not in self.tables:
            lay = layout()
            self.tables[key] = (scipy_pairs(lay), scipy_pairs(np.where(lay == pc.STAIR, pc.GROUND,
                                                                       lay)), lay)
        return self.tables[key]


def expected_seek(gs, snap, i, cfg, player, dists):
    """``(dist, move, target, crossing)`` rows of four for ``player`` (0 / 1)
    of game ``i``: plain loops over the entities of ``gs`` (the game in the
    reference's schema, compat.GameStateView) and, for the items the schema
    does not carry, over the exported item slots.  ``crossing``: per column,
    whether the distance differs from the one that walks through staircases."""
    H = int(cfg.height)
    table, through, layout = dists.table(player, i)
    viewer = gs.iden_lookup[1 + player]
    npc_depth = int(cfg.p1_depth) if int(cfg.start_mode) == 2 else 0
    cell = lambda x, y: int(x) * H + int(y)
    columns = [[], [], []]
    for ent in gs.entities:
        if ent.iden == viewer.iden or ent.depth != viewer.depth:
            continue
        if ent.iden in (1, 2):
            columns[0].append((ent.iden - 1, ent.x, ent.y))
        elif viewer.depth == npc_depth:
            columns[1].append((ent.iden - 3, ent.x, ent.y))
    if snap.get("item_mask") is not None and viewer.depth == npc_depth:
        on = int(np.asarray(snap["item_mask"])[0][i]) & 0xFFFFFFFF
        for k in range(int(cfg.n_npcs)):
            if (on >> k) & 1:
                pos = int(np.asarray(snap["item_pos"])[k][i]) & 0xFFFF
                columns[2].append((k, pos & 0xFF, pos >> 8))
    dist, move, target, crossing = [ABSENT] * 4, [STAY] * 4, [-1] * 4, [False] * 4
    own = cell(viewer.x, viewer.y)
    for col, targets in enumerate(columns):
        best = None
        for slot, x, y in sorted(targets):
            d = int(table[cell(x, y)][own])
            d = d if d < FAR_V else 1 << 30
            if best is None or d < best[0]:
                best = (d, slot, x, y)
        if best is None:
            continue
        d, slot, tx, ty = best
        target[col] = slot
        dist[col] = UNREACHABLE if d == 1 << 30 else d
        plain = int(through[cell(tx, ty)][own])
        crossing[col] = (plain if plain < FAR_V else 1 << 30) != d
        if dist[col] <= 0:
            continue
        for code, (dx, dy) in enumerate(((0, -1), (1, 0), (0, 1), (-1, 0)), start=1):
            x, y = viewer.x + dx, viewer.y + dy
            if not (0 <= x < int(cfg.width) and 0 <= y < H):
                continue
            if layout[x, y] == pc.STAIR and (x, y) != (tx, ty):
                continue
            if int(table[cell(tx, ty)][cell(x, y)]) == d - 1:
                move[col] = code
                break
    return dist, move, target, crossing
