"""Cases for orx_dungeon_spawn / orx_dungeon_stairs (stairs_kernel), shared by
test_dungeon_spawn.py on the CPU and test_gpu_dungeon_spawn.py on the GPU
(numpy only, no torch, no GPU).

The entry point regenerates a dungeon of World.dungeons from (game, episode,
depth, generation).  The oracle keeps its world, so a run of the oracle says
what every dungeon's staircase (and, with a bank, layout) must be; which
generation a dungeon is follows from the players' depths alone, by the rule
above ``descend`` in orx_engine.hip (``Tracker``).
"""
from collections import namedtuple

import numpy as np

UNREACHABLE, UNUSED = 1, 2
TOGETHER, SEPARATED = 1, 2
B, TICKS, OFFSET = 96, 60, 5000

# cfg: the orx_cfg_t fields that differ from the oracle's defaults; bank: the
# layouts' count or 0; bots; seed
Case = namedtuple("Case", "name cfg bank bots seed")

_PLAYERS = dict(player_health=30, player_damage=1, player_armor=0, max_ticks=50)
CASES = (
    Case("unreachable_4x4", dict(_PLAYERS, width=4, height=4, despawn=UNREACHABLE), 0, (2, 2), 41),
    Case("unused_5x4", dict(_PLAYERS, width=5, height=4, despawn=UNUSED), 0, (2, 2), 42),
    Case("unused_sep_9x7", dict(_PLAYERS, width=9, height=7, despawn=UNUSED, start_mode=SEPARATED,
                                p1_depth=0, p2_depth=1), 0, (2, 2), 43),
    Case("unreachable_bank1_12x10", dict(_PLAYERS, width=12, height=10, despawn=UNREACHABLE), 1,
         (2, 1), 44),
    Case("unused_sep_bank6_12x10", dict(_PLAYERS, width=12, height=10, despawn=UNUSED,
                                        start_mode=SEPARATED, p1_depth=2, p2_depth=0), 6, (2, 2), 45),
    Case("unreachable_40x4", dict(_PLAYERS, width=40, height=4, despawn=UNREACHABLE, max_ticks=0),
         0, (2, 2), 46),
    Case("unused_bank3_npcs_7x8", dict(_PLAYERS, width=7, height=8, despawn=UNUSED, n_npcs=3,
                                       npc_health=2), 3, (2, 2), 47),
    Case("unreachable_sep_bank2_8x8", dict(_PLAYERS, width=8, height=8, despawn=UNREACHABLE,
                                           start_mode=SEPARATED, p1_depth=1, p2_depth=3), 2,
         (1, 2), 48),
)
CASE = {c.name: c for c in CASES}


def layouts_of(case):
    """The case's explicit-grid layouts [n, W, H] of Tile codes (1 Ground, 2
    Wall, 3 StaircaseDown), or None: a wall ring, inner walls on a diagonal
    lattice that shifts with the layout, one to three staircases."""
    if not case.bank:
        return None
    W, H = case.cfg["width"], case.cfg["height"]
    out = np.ones((case.bank, W, H), np.uint8)
    for li in range(case.bank):
        t = out[li]
        t[[0, -1], :] = 2
        t[:, [0, -1]] = 2
        for x in range(2, W - 2):
            for y in range(2, H - 2):
                if (3 * x + 5 * y + 2 * li) % 11 == 0:
                    t[x, y] = 2
        for sx, sy in ((1 + li % (W - 2), 1), (W - 2, H - 2), (W // 2, 1 + li % (H - 2)))[:1 + li % 3]:
            t[sx, sy] = 3
    return out


def starts(cfg):
    """The players' start depths."""
    if cfg.get("start_mode", TOGETHER) == SEPARATED:
        return cfg["p1_depth"], cfg["p2_depth"]
    return 0, 0


class Tracker:
    """The generation of every dungeon of every game's world, from the
    players' depths tick by tick.  When a player enters depth nd and the other
    player does not stand on it, a dungeon is made: generation 1 under the
    Unused rule where the other player already passed through nd (its start
    depth <= nd < its depth), else generation 0.  ``gen1`` lists those
    descents as (tick, game, player, nd, the other's depth).  Where both
    players descend in one tick, the order they moved in is the one that makes
    as many dungeons as the tick counted; where both do and they make
    different ones, the game is not followed for the rest of its episode
    (``unknown``)."""

    def __init__(self, cfg, n):
        self.cfg, self.n = cfg, n
        self.gens = [dict() for _ in range(n)]
        self.unknown = np.zeros(n, bool)
        self.gen1 = []
        self.descents = 0

    def see(self, t, prev, s):
        unused = self.cfg.get("despawn", UNREACHABLE) == UNUSED
        start = starts(self.cfg)
        for g in range(self.n):
            if s["episode"][g] != prev["episode"][g]:
                self.gens[g], self.unknown[g] = {}, False
                continue
            down = [p for p in (0, 1) if int(s["p_depth"][p][g]) > int(prev["p_depth"][p][g])]
            if self.unknown[g] or not down:
                continue
            self.descents += len(down)
            was = [int(prev["p_depth"][p][g]) for p in (0, 1)]
            if not unused:
                continue   # (Unreachable: generation 0 always)
            # the orders the two may have moved in that make as many dungeons
            # as the tick's spawn_dungeon calls (ORX_CNT_DUNGEON)
            n_made = int(s["counters"][2][g]) - int(prev["counters"][2][g])
            made = [m for m in (self._enter(was, order, start) for order in (down, down[::-1]))
                    if len(m) == n_made]
            assert made, (t, g, was, down, n_made)
            if any({(nd, gen) for _, nd, _, gen in m} != {(nd, gen) for _, nd, _, gen in made[0]}
                   for m in made):
                self.unknown[g] = True
                continue
            self.gens[g].update((nd, gen) for p, nd, od, gen in made[0])
            self.gen1 += [(t, g, p, nd, od) for p, nd, od, gen in made[0] if gen]

    @staticmethod
    def _enter(depths, order, start):
        """The dungeons made when the players ``order`` descend in that order:
        (player, depth entered, the other's depth then, generation) each."""
        depths, made = list(depths), []
        for p in order:
            nd, od = depths[p] + 1, depths[1 - p]
            if od != nd:   # (else the other player's dungeon, whatever its generation)
                made.append((p, nd, od, int(start[1 - p] <= nd < od)))
            depths[p] = nd
        return sorted(made)

    def gen(self, g, depth):
        return self.gens[g].get(int(depth), 0)


def new_oracle(oracle_mod, case, record_events=False):
    o = oracle_mod.Oracle(case.cfg, B, case.seed, OFFSET, layouts=layouts_of(case),
                          record_events=record_events)
    o.reset(episode=np.zeros(B, np.int32))
    return o


def run(oracle_mod, case):
    """Plays the case on the oracle: per tick (t, actions, the state after it,
    the world of every followed game as (game, episode, depth, generation, sx,
    sy, layout) rows -- layout -1 without a bank), and the tracker."""
    o = new_oracle(oracle_mod, case)
    tr = Tracker(case.cfg, B)
    prev = o.export()
    ticks = []
    for t in range(TICKS):
        a = o.policy(*case.bots)
        o.step(a)
        s = o.export()
        tr.see(t, prev, s)
        rows = []
        for g in np.flatnonzero(~tr.unknown):
            for d in o.world(int(g)):
                lay = d[3] if case.bank else -1
                rows.append((int(g), int(s["episode"][g]), d[0], tr.gen(g, d[0]), d[1], d[2], lay))
        ticks.append((t, a, s, np.array(rows, np.int64).reshape(-1, 7)))
        prev = s
    return ticks, tr


def ref_spawn(case, gid, episode, depth, gen, seed=None):
    """(sx, sy, layout) of the dungeon of global game ``gid``, ``episode``,
    ``depth``, generation ``gen``: spawn_dungeon over the dungeon's own word
    stream, as oracle/pyref.py restates it (layout -1 without a bank)."""
    from oracle import pyref
    w = pyref.Words(case.seed if seed is None else seed, int(gid), int(episode), int(depth),
                    pyref.PUR_DUNGEON, int(gen))
    layouts = layouts_of(case)
    if layouts is not None:
        k = pyref.np_randint(w, len(layouts))
        x, y = np.argwhere(layouts[k] == 3)[0]
        return int(x), int(y), int(k)
    rx = pyref.np_randint(w, 1, case.cfg["width"] - 2)
    ry = pyref.np_randint(w, 1, case.cfg["height"] - 2)
    return rx, ry, -1


def ref_rows(case, games, episodes, depths, gens, seed=None):
    """ref_spawn per request: int32 [n, 3], each distinct request drawn once."""
    memo, out = {}, np.zeros((len(games), 3), np.int32)
    for j, key in enumerate(zip(games, episodes, depths, gens)):
        key = tuple(int(v) for v in key)
        if key not in memo:
            memo[key] = ref_spawn(case, *key, seed=seed)
        out[j] = memo[key]
    return out
