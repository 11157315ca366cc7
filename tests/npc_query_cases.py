"""Shared by tests/test_npc_query.py (CPU) and tests/test_gpu_npc_query.py: the
configurations the enemies' queries (include/orx_npc_query.h) are checked on,
the hand-built states with one expectation per row of the header's rule table,
and the comparison of one predicted column against what a tick of the CPU
restatement (npc_given_cases.GivenGame) then did."""
import copy

import numpy as np

from npc_given_cases import BASE_CFG, GivenGame, bank, random_table

STAY = 5
DELTAS = {1: (0, -1), 2: (1, 0), 3: (0, 1), 4: (-1, 0), 5: (0, 0)}


def env_config(cfg: dict, layouts=None):
    from optimax_rogue_amd import EnvConfig
    return EnvConfig.from_dict({k: v for k, v in cfg.items() if k != "policy"}, layouts=layouts)


def given_runs():
    """name -> dict(cfg, layouts, G, T, seed): the GivenGame runs of the CPU
    tests -- NPCs in registers, dense NPCs and a bank with interior walls, all
    Together (the guards of tests/npc_given_cases.guarded then read the very
    dungeon the queries read)."""
    return {
        "regs": dict(cfg=dict(BASE_CFG), layouts=None, G=24, T=36, seed=11),
        "dense": dict(cfg=dict(BASE_CFG, width=12, height=12, n_npcs=20), layouts=None, G=8, T=30,
                      seed=12),
        "bank": dict(cfg=dict(BASE_CFG, width=9, height=8, n_npcs=5), layouts=bank(9, 8, 3, 7),
                     G=24, T=36, seed=13),
    }


def start_run(run):
    """The run's games and its random table [T, K, G]."""
    cfg = dict(run["cfg"], policy=(1, 1))
    table = random_table(run["T"], int(cfg["n_npcs"]), run["G"], run["seed"])
    games = [GivenGame(cfg, run["seed"], g, table, g, layouts=run["layouts"])
             for g in range(run["G"])]
    return games, table


def play_one(game, k, m):
    """A deep copy of ``game`` stepped once with both players on Stay and an
    all-Stay table but for NPC slot ``k`` playing ``m``; returns the copy."""
    g = copy.deepcopy(game)
    K = int(g.cfg["n_npcs"])
    g.table = np.full((1, K, 1), STAY, np.int8)
    g.table[0, k, 0] = m
    g.t, g.g = 0, 0
    g.step(STAY, STAY)
    return g


def check_outcome(before, after, k, m, kind, target, amount):
    """Asserts that ``after`` (``play_one(before, k, m)``) is what column ``m``
    of NPC ``k``'s prediction said; returns the names it counted."""
    from optimax_rogue_amd import enums as E
    iden = 3 + k
    out, lethal = int(kind) & E.NPC_OUT_MASK, bool(int(kind) & E.NPC_OUT_LETHAL)
    was = {e.iden: (e.depth, e.x, e.y, e.health) for e in before.gs.entities}
    now = {e.iden: (e.depth, e.x, e.y, e.health) for e in after.gs.entities}
    d, x, y, hp = was[iden]
    dx, dy = DELTAS[m]
    hit = int(target) if out in (E.NPC_OUT_ATTACK_NPC, E.NPC_OUT_ATTACK_PLAYER) else None
    names = [E.NPC_OUT_NAMES[out]] + (["LETHAL"] if lethal else [])
    assert (int(target) >= 0) == (hit is not None), names
    if hit is None:
        assert int(amount) == 0 and not lethal, names
    # nobody but the predicted target changes; nobody else moves or leaves
    for i, rec in was.items():
        if i == iden or i == hit:
            continue
        assert now.get(i) == rec, (names, i)
    if out == E.NPC_OUT_STAIRS:
        assert iden not in now, names
    elif out == E.NPC_OUT_STEP:
        assert now[iden] == (d, x + dx, y + dy, hp), names
    else:
        assert now[iden] == (d, x, y, hp), names
    if hit is not None:
        hd, hx, hy, hhp = was[hit]
        assert (hd, hx, hy) == (d, x + dx, y + dy), names
        assert int(amount) == max(int(before.cfg["npc_damage"]) - int(before.cfg["npc_armor"]), 0)
        assert lethal == (hhp > 0 and int(amount) >= hhp), names
        left = hhp - int(amount)
        if hit >= 3 and left <= 0:      # swept at the end of the tick
            assert hit not in now, names
        else:
            assert now[hit] == (hd, hx, hy, left), names
    return names


# --------------------------------------------------------------------------
# hand-built states: one game each, stacked per configuration
# --------------------------------------------------------------------------
def _state(games, K):
    """An engine-layout snapshot from a list of game dicts: ``p`` ((x, y,
    depth, health) of the two players), ``st`` (their staircases), ``npcs``
    ((x, y, health, alive) per slot)."""
    B = len(games)
    snap = {f: np.zeros((2, B), np.int32) for f in ("p_x", "p_y", "p_depth", "p_health", "st_x",
                                                     "st_y")}
    snap["npc_pos"] = np.zeros((K, B), np.uint16)
    snap["npc_health"] = np.zeros((K, B), np.int8)
    snap["npc_alive"] = np.zeros(B, np.uint32)
    for b, g in enumerate(games):
        for p in (0, 1):
            (snap["p_x"][p, b], snap["p_y"][p, b], snap["p_depth"][p, b],
             snap["p_health"][p, b]) = g["p"][p]
            snap["st_x"][p, b], snap["st_y"][p, b] = g["st"][p]
        for k, (x, y, hp, alive) in enumerate(g["npcs"]):
            snap["npc_pos"][k, b] = x | y << 8
            snap["npc_health"][k, b] = hp
            snap["npc_alive"][b] |= np.uint32(int(alive) << k)
    snap["status"] = np.ones(B, np.int32)
    snap["tick"] = np.full(B, 3, np.int32)
    return snap


def hand_states():
    """name -> dict(cfg, snap, where, expect): ``expect`` maps (game, slot,
    move) to (kind, target, amount), ``where`` is the depth state per game.
    The numbers are written from include/orx_npc_query.h's rule table, not
    taken from any implementation."""
    from optimax_rogue_amd import enums as E
    N, R, BL, ST, SR, AN, AP, FR, L = (E.NPC_OUT_NONE, E.NPC_OUT_REST, E.NPC_OUT_BLOCKED,
                                       E.NPC_OUT_STEP, E.NPC_OUT_STAIRS, E.NPC_OUT_ATTACK_NPC,
                                       E.NPC_OUT_ATTACK_PLAYER, E.NPC_OUT_FROZEN,
                                       E.NPC_OUT_LETHAL)
    # 6 x 5, Together, three slots, an attack takes 2 (interior: x 1..4, y 1..3)
    room = dict(BASE_CFG, width=6, height=5, n_npcs=3, npc_damage=3, npc_armor=1)
    games, expect = [], {}
    # 0: the rule table.  NPC 0 between a wall, a dead slot's stale cell, NPC 1
    # (health == amount) and player 1; NPC 1 under NPC 0 (health == amount + 1)
    # and above player 2 (health == amount)
    games.append(dict(p=((1, 1, 0, 10), (2, 3, 0, 2)), st=((4, 3), (4, 3)),
                      npcs=((2, 1, 3, 1), (2, 2, 2, 1), (3, 1, 3, 0))))
    expect.update({(0, 0, 1): (BL, -1, 0), (0, 0, 2): (ST, -1, 0), (0, 0, 3): (AN | L, 4, 2),
                   (0, 0, 4): (AP, 1, 2), (0, 0, 5): (R, -1, 0),
                   (0, 1, 1): (AN, 3, 2), (0, 1, 2): (ST, -1, 0), (0, 1, 3): (AP | L, 2, 2),
                   (0, 1, 4): (ST, -1, 0), (0, 1, 5): (R, -1, 0)})
    expect.update({(0, 2, m): (N, -1, 0) for m in range(8)})   # the dead slot's row
    # 1: an occupant standing on a staircase is attacked (occupancy before the tile)
    games.append(dict(p=((1, 1, 0, 10), (1, 3, 0, 10)), st=((3, 2), (3, 2)),
                      npcs=((2, 2, 3, 1), (3, 2, 3, 1), (4, 3, 3, 1))))
    expect.update({(1, 0, 2): (AN, 4, 2), (1, 0, 1): (ST, -1, 0), (1, 1, 4): (AN, 3, 2),
                   (1, 2, 1): (ST, -1, 0), (1, 2, 2): (BL, -1, 0), (1, 2, 3): (BL, -1, 0)})
    # 2: a free staircase removes the NPC
    games.append(dict(p=((1, 1, 0, 10), (1, 3, 0, 10)), st=((3, 2), (3, 2)),
                      npcs=((2, 2, 3, 1), (3, 1, 3, 1), (4, 3, 3, 0))))
    expect.update({(2, 0, 2): (SR, -1, 0), (2, 1, 3): (SR, -1, 0), (2, 1, 1): (BL, -1, 0)})
    # 3: player 2 (health 0: whatever its health) next to the staircase: frozen
    games.append(dict(p=((1, 1, 0, 10), (3, 3, 0, 0)), st=((3, 2), (3, 2)),
                      npcs=((2, 2, 3, 1), (1, 2, 3, 1), (4, 1, 3, 0))))
    expect.update({(3, k, m): (FR, -1, 0) for k in (0, 1) for m in (1, 2, 3, 4)})
    expect.update({(3, 0, 5): (R, -1, 0), (3, 2, 5): (N, -1, 0), (3, 2, 1): (N, -1, 0)})
    # 4: player 2 next to the staircase of ANOTHER depth: nothing freezes, and
    # its cell is free ground on the NPCs' depth
    games.append(dict(p=((1, 1, 0, 10), (2, 2, 1, 10)), st=((4, 3), (3, 2)),
                      npcs=((2, 1, 3, 1), (3, 3, 3, 1), (4, 1, 3, 0))))
    expect.update({(4, 0, 3): (ST, -1, 0), (4, 0, 4): (AP, 1, 2), (4, 1, 2): (SR, -1, 0),
                   (4, 1, 3): (BL, -1, 0)})
    out = {"room": dict(cfg=room, snap=_state(games, 3), expect=expect,
                        where=[E.NPC_DEPTH_WATCHED] * 5)}
    # 8 x 8, Separated with player 2 starting above player 1: player 1 has left
    # the NPCs' depth 2.  Unreachable keeps the dungeon (UNWATCHED), Unused
    # drops it (GONE); game 1: player 2 has come down to it (WATCHED by it alone)
    sep = dict(BASE_CFG, start_mode=2, p1_depth=2, p2_depth=1, n_npcs=2)
    games = [dict(p=((2, 2, 3, 10), (5, 5, 1, 10)), st=((6, 6), (3, 3)),
                  npcs=((4, 4, 3, 1), (1, 1, 3, 0))),
             dict(p=((2, 2, 3, 10), (4, 5, 2, 10)), st=((6, 6), (2, 5)),
                  npcs=((4, 4, 3, 1), (1, 1, 3, 0)))]
    gone = {(0, 0, m): (FR, -1, 0) for m in (1, 2, 3, 4)}
    none = {(0, 0, m): (N, -1, 0) for m in (1, 2, 3, 4)}
    both = {(0, 0, 5): (R, -1, 0), (0, 1, 5): (N, -1, 0),
            (1, 0, 3): (AP, 2, 1), (1, 0, 1): (ST, -1, 0), (1, 0, 5): (R, -1, 0)}
    out["unwatched"] = dict(cfg=dict(sep, despawn=1), snap=_state(games, 2),
                            expect={**none, **both},
                            where=[E.NPC_DEPTH_UNWATCHED, E.NPC_DEPTH_WATCHED])
    out["gone"] = dict(cfg=dict(sep, despawn=2), snap=_state(games, 2), expect={**gone, **both},
                       where=[E.NPC_DEPTH_GONE, E.NPC_DEPTH_WATCHED])
    return out


# what seek answers on the hand-built states: (state, game, slot) -> the
# (dist, move, target) of columns P1, P2 and NEAREST
ABSENT = (-2, 5, -1)


def hand_seek():
    return {
        # NPC 0 at (2, 1): player 1 at (1, 1) is 1 Left; player 2 at (2, 3) is
        # 2 Down -- the walk is straight down column 2 (the staircase is (4, 3))
        ("room", 0, 0): ((1, 4, 1), (2, 3, 2), (1, 4, 1)),
        ("room", 0, 2): (ABSENT, ABSENT, ABSENT),               # a dead slot
        # game 2, NPC 0 at (2, 2), staircase (3, 2): both players are 2 away
        # (player 1 wins the tie); Up is the first move that gets closer to
        # (1, 1), Down to (1, 3)
        ("room", 2, 0): ((2, 1, 1), (2, 3, 2), (2, 1, 1)),
        # game 2, NPC 1 at (3, 1): player 1 at (1, 1), two Left; player 2 at
        # (1, 3), four away: Down is the staircase (3, 2), so Left comes first
        ("room", 2, 1): ((2, 4, 1), (4, 4, 2), (2, 4, 1)),
        # game 4: player 2 is on another depth
        ("room", 4, 0): ((1, 4, 1), ABSENT, (1, 4, 1)),
        ("unwatched", 0, 0): (ABSENT, ABSENT, ABSENT),
        ("gone", 0, 0): (ABSENT, ABSENT, ABSENT),
        # watched by player 2 alone, at (4, 5) under the NPC at (4, 4)
        ("gone", 1, 0): (ABSENT, (1, 3, 2), (1, 3, 2)),
    }
