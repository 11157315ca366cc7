"""The states tests/test_threat.py (CPU, oracle states) and
tests/test_gpu_threat.py (engine states) check ``threat`` on, an independent
statement of the query -- plain loops over the entities of one game in the
reference's schema, on seek_cases' scipy distances -- and the hand-built states
whose rows the CPU test writes out.

The CPU test runs over seek_cases.cases() alone: seeds and tick counts there
already make the ORACLE's states meet every coverage condition test_threat.py
asserts.  ``gpu_cases`` adds the configurations only the kernel has a reason to
care about (an NPC count at and one past the register forms' limit, a bank
without NPCs, stock seeding).
"""
import functools

import numpy as np

import path_cases as pc
import seek_cases as sc

N_GAMES = sc.N_GAMES
WALL_V, FAR_V = sc.WALL_V, sc.FAR_V
UNREACHABLE, ABSENT, STAY = sc.UNREACHABLE, sc.ABSENT, sc.STAY
RADIUS = 2                      # the window of the CPU statement
DELTAS = ((0, -1), (1, 0), (0, 1), (-1, 0))        # Up, Right, Down, Left: Moves 1..4
# flags 0 and NPCs that stand still: a flee move is all that changes a distance
PLAYOUT = ("a", "b", "c", "d", "pockets", "17x5", "dense")


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """seek_cases.cases() and: K = 0 on a bank, K = 1, 16 and 17 (the last of
    the register forms and the first dense one), stock seeding."""
    from optimax_rogue_amd import DungeonBank, EnvConfig
    bank = lambda *a, **kw: DungeonBank.random(*a, **kw).layouts
    out = dict(sc.cases())
    out.update({
        "k0bank": dict(cfg=EnvConfig(width=9, height=8, n_npcs=0,
                                     layouts=bank(9, 8, 16, seed=0, wall_p=0.3)),
                       seed=31, ticks=12, policies=(1, 1)),
        "k1": dict(cfg=EnvConfig(width=7, height=9, n_npcs=1), seed=32, ticks=10, policies=(1, 1)),
        "k16": dict(cfg=EnvConfig(width=12, height=10, n_npcs=16,
                                  layouts=bank(12, 10, 4, seed=6, wall_p=0.2)),
                    seed=33, ticks=12, policies=(1, 1)),
        "k17": dict(cfg=EnvConfig(width=11, height=13, n_npcs=17), seed=34, ticks=12,
                    policies=(1, 1)),
        "stock": dict(cfg=EnvConfig(width=8, height=8, n_npcs=4, rng=1), seed=1000, ticks=10,
                      policies=(1, 1)),
    })
    return out


def expected_threat(gs, snap, i, cfg, player, dists, radius=RADIUS):
    """``(dist, move, target, after, window, notes)`` of ``player`` (0 / 1) of
    game ``i``: rows of four, a row of eight, [V][V], by plain loops over the
    entities of ``gs`` (compat.GameStateView) and include/orx_path.h's rule.
    ``notes``: what the coverage conditions ask about the game."""
    W, H = int(cfg.width), int(cfg.height)
    table, _, layout = dists.table(player, i)
    viewer = gs.iden_lookup[1 + player]
    npc_depth = int(cfg.p1_depth) if int(cfg.start_mode) == 2 else 0
    cell = lambda x, y: int(x) * H + int(y)
    inside = lambda x, y: 0 <= x < W and 0 <= y < H
    columns = [[], [], []]                      # (iden, x, y) per column
    for ent in gs.entities:
        if ent.iden == viewer.iden or ent.depth != viewer.depth:
            continue
        if ent.iden in (1, 2):
            columns[0].append((ent.iden, ent.x, ent.y))
        elif viewer.depth == npc_depth:
            columns[1].append((ent.iden, ent.x, ent.y))
    columns[2] = sorted(columns[0] + columns[1])      # (a player's iden is below every NPC's)

    def value(threats, x, y):
        """The cell's value in the field's format."""
        if not inside(x, y) or layout[x, y] == pc.WALL:
            return WALL_V
        best = FAR_V
        for _, tx, ty in threats:
            if inside(tx, ty):
                best = min(best, int(table[cell(tx, ty)][cell(x, y)]))
        return best

    shown = lambda v: UNREACHABLE if v >= FAR_V else v
    dist, move, target, after = [ABSENT] * 4, [STAY] * 4, [-1] * 4, [ABSENT] * 8
    notes = dict(stair_excluded=False, tie_kept=False)
    x0, y0 = viewer.x, viewer.y
    for col, threats in enumerate(columns):
        if not threats or not inside(x0, y0):
            continue
        own = min(value(threats, x0, y0), FAR_V)
        dist[col] = shown(own)
        nearest = [iden for iden, tx, ty in sorted(threats)
                   if min(value([(iden, tx, ty)], x0, y0), FAR_V) == own][0]
        target[col] = nearest if col == 2 else (nearest - 1 if col == 0 else nearest - 3)
        best, tied = own, False
        for code, (dx, dy) in enumerate(DELTAS, start=1):
            x, y = x0 + dx, y0 + dy
            if not inside(x, y) or layout[x, y] != pc.GROUND:
                if col == 2 and inside(x, y) and layout[x, y] == pc.STAIR:
                    notes["stair_excluded"] = True
                continue
            v = value(threats, x, y)
            if col == 2:
                after[code] = shown(v)
            if v > best:
                best, move[col], tied = v, code, False
            elif v == best and move[col] == STAY:
                tied = True
        if col == 2:
            after[STAY] = dist[col]
            notes["tie_kept"] = tied
    V = 2 * radius + 1
    window = [[value(columns[2] if inside(x0, y0) else [], x0 + i - radius, y0 + j - radius)
               for i in range(V)] for j in range(V)]
    return dist, move, target, after, window, notes


def oracle_at(case, n_games=N_GAMES):
    """The case's oracle at the start and (a clone's state kept) after its
    ticks: [(oracle, export), (oracle, export)]."""
    from oracle.oracle import Oracle
    cfg = case["cfg"]
    ora = Oracle(cfg.to_dict(), n_games, case["seed"], layouts=cfg.layouts)
    ora.reset(episode=np.zeros(n_games, np.int32))
    first = (ora.clone(), ora.export())
    for _ in range(case["ticks"]):
        ora.step(ora.policy(*case["policies"]))
    return [first, (ora, ora.export())]


# ---- hand-built states --------------------------------------------------------
#   x 0123456
# y=0 #######      the 7 x 7 layout: a dead end at (1, 1), a loop round the Wall
# y=1 #...#.#      at (2, 4) with forks at (3, 3) and (3, 5), and a staircase at
# y=2 ###.#.#      (5, 3) that cuts the corridor x = 5: (5, 1) and (5, 2) can
# y=3 #...#S#      be walked to from the staircase alone
# y=4 #.#.#.#
# y=5 #.....#
# y=6 #######
HAND_ROWS = ("#######", "#...#.#", "###.#.#", "#...#S#", "#.#.#.#", "#.....#", "#######")


def hand_layout():
    code = {"#": pc.WALL, ".": pc.GROUND, "S": pc.STAIR}
    return np.array([[code[HAND_ROWS[y][x]] for y in range(7)] for x in range(7)], np.uint8)


def hand_snap(games, bank: bool):
    """A ``snapshot()``-shaped dict of hand-placed games, player 1 the viewer:
    each ``dict(me=(x, y), other=(x, y) or None, npcs=[(x, y) or None, ...],
    stair=(x, y))`` -- ``other`` None: player 2 is on another depth; an NPC
    None: its slot is dead."""
    B, K = len(games), len(games[0]["npcs"])
    snap = dict(p_x=np.zeros((2, B), np.int32), p_y=np.zeros((2, B), np.int32),
                p_depth=np.zeros((2, B), np.int32), st_x=np.zeros((2, B), np.int32),
                st_y=np.zeros((2, B), np.int32), npc_pos=np.zeros((K, B), np.uint16),
                npc_health=np.zeros((K, B), np.int8), npc_alive=np.zeros(B, np.uint32))
    if bank:
        snap["p_layout"] = np.zeros((2, B), np.int16)
    for b, g in enumerate(games):
        snap["p_x"][0, b], snap["p_y"][0, b] = g["me"]
        snap["p_x"][1, b], snap["p_y"][1, b] = g["other"] or (1, 1)
        snap["p_depth"][1, b] = 0 if g["other"] else 1
        snap["st_x"][:, b], snap["st_y"][:, b] = g.get("stair", (0, 0))
        for k, pos in enumerate(g["npcs"]):
            if pos is not None:
                snap["npc_pos"][k, b] = pos[0] | pos[1] << 8
                snap["npc_health"][k, b] = 3
                snap["npc_alive"][b] |= 1 << k
    return snap
