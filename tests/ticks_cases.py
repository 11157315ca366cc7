"""What tests/test_ticks.py (CPU, oracle states) and tests/test_gpu_ticks.py
(engine states) share: the configurations, an independent restatement of
include/orx_path.h's orx_path_ticks -- a per-game heapq Dijkstra written from
the header's sentences -- the play-out that checks the answer against the game
itself, and the hand-built states, one per sentence of the definition.

The five configurations of the table (bank, bank_weak, room, room_weak,
room_strong) start the players on different depths, so that the other player
is out of the way; ``together``, ``p2`` and ``off_depth`` are the three more
the restatement is compared on.
"""
import functools
import heapq

import numpy as np

WALL_V, FAR_V = 0xFFFF, 0xFFFE
GROUND, WALL, STAIR = 1, 2, 3
UP, RIGHT, DOWN, LEFT, STAY = 1, 2, 3, 4, 5
DELTAS = ((0, -1), (1, 0), (0, 1), (-1, 0))        # Up, Right, Down, Left: Moves 1..4
N_GAMES = 300
WARMUP = 3                                          # RandomBot ticks before the first question
RADII = (1, 5, 15)
SEP = dict(start_mode=2, p1_depth=0, p2_depth=1, max_ticks=0)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(cfg, seed, player): the asker is ``player``."""
    import sight_cases
    from optimax_rogue_amd import EnvConfig
    wg = sight_cases.cases()["wg"]["cfg"].layouts
    bank = lambda **kw: EnvConfig(width=12, height=10, n_npcs=6, layouts=wg, **SEP, **kw)
    room = lambda **kw: EnvConfig(width=8, height=7, n_npcs=10, **SEP, **kw)
    return {
        "bank": dict(cfg=bank(), seed=31, player=0),
        "bank_weak": dict(cfg=bank(player_damage=1), seed=31, player=0),
        "bank_strong": dict(cfg=bank(npc_health=5, player_damage=3), seed=32, player=0),
        "room": dict(cfg=room(), seed=5, player=0),
        "room_weak": dict(cfg=room(player_damage=1), seed=5, player=0),
        "room_strong": dict(cfg=room(player_damage=4), seed=6, player=0),
        # both players on the NPCs' depth; player 2 asking there; the asker a depth below
        "together": dict(cfg=EnvConfig(width=9, height=8, n_npcs=8, max_ticks=0), seed=7, player=0),
        "p2": dict(cfg=EnvConfig(width=12, height=10, n_npcs=6, layouts=wg, max_ticks=0), seed=8,
                   player=1),
        "off_depth": dict(cfg=bank(), seed=31, player=1),
    }


TABLE = ("bank", "bank_weak", "room", "room_weak", "room_strong")
PLAYOUT = ("bank", "room", "room_strong", "bank_strong")
# the issue's counts over the games on the NPCs' depth in the first state: ticks
# above the plain distance, first move differs, first move is an attack, and
# (weak) unreachable where the tiles alone reach
COUNTS = dict(bank=(72, 42, 25, 0), bank_weak=(26, 44, 0, 47), room=(112, 92, 49, 0),
              room_weak=(44, 84, 0, 69), room_strong=(86, 42, 21, 0))


def bank_of(cfg):
    from optimax_rogue_amd import DungeonBank
    return None if cfg.layouts is None else DungeonBank(cfg.layouts)


def oracle_after_warmup(case, n_games=N_GAMES):
    from oracle.oracle import Oracle
    cfg = case["cfg"]
    ora = Oracle(cfg.to_dict(), n_games, case["seed"], layouts=cfg.layouts)
    ora.reset(episode=np.zeros(n_games, np.int32))
    for _ in range(WARMUP):
        ora.step(ora.policy(1, 1))
    return ora


def tiles_of(cfg, snap, player, b):
    """int [W, H]: the Tile codes of the asker's depth in game ``b``."""
    W, H = int(cfg.width), int(cfg.height)
    if cfg.layouts is not None:
        lay = min(max(int(snap["p_layout"][player][b]), 0), len(cfg.layouts) - 1)
        return np.asarray(cfg.layouts[lay]).astype(int)
    t = np.full((W, H), GROUND)
    t[0, :] = t[-1, :] = t[:, 0] = t[:, -1] = WALL
    sx, sy = int(snap["st_x"][player][b]), int(snap["st_y"][player][b])
    if 1 <= sx <= W - 2 and 1 <= sy <= H - 2:
        t[sx, sy] = STAIR
    return t


def expected_ticks(cfg, snap, player, b, radius):
    """``(ticks, move, window)`` of game ``b`` from the header's sentences: the
    graph, enter(c) = 1 + hits(c), and T by Dijkstra from the staircases over
    reversed steps."""
    W, H, K = int(cfg.width), int(cfg.height), int(cfg.n_npcs)
    tiles = tiles_of(cfg, snap, player, b)
    inside = lambda x, y: 0 <= x < W and 0 <= y < H
    npc_depth = int(cfg.p1_depth) if int(cfg.start_mode) == 2 else 0
    damage = int(cfg.player_damage)
    if int(cfg.flags) & 124:
        damage = int(snap["p_rpg"][2][player][b])
    a = max(damage - int(cfg.player_armor), 0)
    hits = {}                                   # held cell -> hits, None: cannot be entered
    if int(snap["p_depth"][player][b]) == npc_depth:
        alive = np.asarray(snap["npc_alive"]).reshape(-1, np.asarray(snap["npc_alive"]).shape[-1])
        for k in range(K):
            if not (int(alive[k // 32][b]) >> (k % 32)) & 1:
                continue
            pos = int(snap["npc_pos"][k][b])
            c = (pos & 0xFF, pos >> 8)
            if not inside(*c):
                continue
            h = None if a == 0 else -(-max(int(snap["npc_health"][k][b]), 1) // a)
            hits[c] = h if c not in hits or h is None or hits[c] is None else min(hits[c], h)

    def enter(c):
        if c in hits:
            return None if hits[c] is None else 1 + hits[c]
        return 1

    T, heap = {}, []
    for x in range(W):
        for y in range(H):
            if tiles[x, y] == STAIR:
                T[x, y] = 0
                heap.append((0, (x, y)))
    heapq.heapify(heap)
    done = set()
    while heap:
        t, c = heapq.heappop(heap)
        if c in done:
            continue
        done.add(c)
        # a walk from a neighbour n steps onto c first: c is a staircase (the
        # walk ends) or Ground (an interior cell), and can be entered
        if enter(c) is None or (tiles[c] != GROUND and tiles[c] != STAIR):
            continue
        for dx, dy in DELTAS:
            n = (c[0] + dx, c[1] + dy)
            if inside(*n) and tiles[n] == GROUND and t + enter(c) < T.get(n, 1 << 60):
                T[n] = t + enter(c)
                heapq.heappush(heap, (T[n], n))

    x0, y0 = int(snap["p_x"][player][b]), int(snap["p_y"][player][b])
    ticks = T.get((x0, y0), -1) if inside(x0, y0) else -1
    move = STAY
    if ticks > 0:
        for code, (dx, dy) in enumerate(DELTAS, start=1):
            n = (x0 + dx, y0 + dy)
            if inside(*n) and n in T and enter(n) is not None and enter(n) + T[n] == ticks:
                move = code
                break
    V = 2 * radius + 1
    window = np.full((V, V), WALL_V, np.int64)
    for j in range(V):
        for i in range(V):
            c = (x0 + i - radius, y0 + j - radius)
            if inside(*c) and tiles[c] != WALL:
                window[j, i] = T.get(c, FAR_V)
    return ticks, move, window


def attacks(cfg, snap, player, move):
    """bool [B]: the move steps onto a cell a live NPC of the depth holds."""
    from optimax_rogue_amd.query import npc_depth, npc_rows
    alive, nx, ny, _ = npc_rows(snap, int(cfg.n_npcs))
    dx = np.array([0, 0, 1, 0, -1, 0])[np.asarray(move)]
    dy = np.array([0, -1, 0, 1, 0, 0])[np.asarray(move)]
    x, y = snap["p_x"][player] + dx, snap["p_y"][player] + dy
    on = alive & (snap["p_depth"][player] == npc_depth(cfg))[None] & (nx == x[None]) & (ny == y[None])
    return on.any(axis=0) & (np.asarray(move) != STAY)


def play_out(ask, step, max_ticks=400):
    """Plays ``move`` for player 1 and Stay for player 2 in every game whose
    players are on different depths, re-asking each tick.  ``ask()`` ->
    ``(ticks, move, depth of player 1, depth of player 2, attack)`` arrays [B],
    ``step(actions)`` plays int8 [B] for player 1.  Asserts the definition's two
    properties -- ``ticks`` drops by exactly one per tick, and the depth changes
    exactly in the tick where it was 1 -- and returns ``(played, descended,
    stood)``: the games played, those that descended, and the ticks the player
    stood still attacking."""
    ticks, move, d0, d1, hit = ask()
    playing = d0 != d1
    assert (ticks[playing] > 0).all(), "a played game with no way down, or on a staircase"
    played, descended, stood = int(playing.sum()), 0, 0
    for _ in range(max_ticks):
        if not playing.any():
            break
        stood += int((hit & playing).sum())
        step(np.where(playing, move, STAY).astype(np.int8))
        now, nmove, n0, _, nhit = ask()
        last, rest = playing & (ticks == 1), playing & (ticks > 1)
        assert (n0[last] == d0[last] + 1).all(), "did not descend in the tick where ticks was 1"
        assert (n0[rest] == d0[rest]).all(), "the depth changed before ticks was 1"
        assert (now[rest] == ticks[rest] - 1).all(), "ticks did not drop by exactly one"
        descended += int(last.sum())
        playing, ticks, move, hit, d0 = rest, now, nmove, nhit, n0
    assert not playing.any(), "games still walking"
    return played, descended, stood


# ---- hand-built states --------------------------------------------------------
#   x 0123456789
# y=0 ##########     the 10 x 7 layout: a one-wide corridor y = 1 from (1, 1) to
# y=1 #......S.#     the staircase at (7, 1), one cell behind it, and an open
# y=2 #.######.#     room below that joins the corridor's two ends the long way
# y=3 #........#     round (x = 1 and x = 8)
# y=4 #........#
# y=5 #........#
# y=6 ##########
HAND_ROWS = ("##########", "#......S.#", "#.######.#", "#........#", "#........#", "#........#",
             "##########")


def hand_layout():
    code = {"#": WALL, ".": GROUND, "S": STAIR}
    W, H = len(HAND_ROWS[0]), len(HAND_ROWS)
    return np.array([[code[HAND_ROWS[y][x]] for y in range(H)] for x in range(W)], np.uint8)


def hand_cfg(K, **kw):
    from optimax_rogue_amd import EnvConfig
    return EnvConfig(width=10, height=7, n_npcs=K, layouts=hand_layout()[None], max_ticks=0, **kw)


def hand_snap(games, K):
    """A ``snapshot()``-shaped dict of hand-placed games on the bank above,
    player 1 the asker on depth 0, player 2 a depth below: each ``dict(me=(x,
    y), npcs=[(x, y, health, alive), ...])`` with at most K NPCs."""
    B = len(games)
    snap = dict(p_x=np.ones((2, B), np.int32), p_y=np.ones((2, B), np.int32),
                p_depth=np.zeros((2, B), np.int32), st_x=np.zeros((2, B), np.int32),
                st_y=np.zeros((2, B), np.int32), npc_pos=np.zeros((K, B), np.uint16),
                npc_health=np.zeros((K, B), np.int8), npc_alive=np.zeros(B, np.uint32),
                p_layout=np.zeros((2, B), np.int16))
    snap["p_depth"][1] = 1
    for b, g in enumerate(games):
        snap["p_x"][0, b], snap["p_y"][0, b] = g["me"]
        for k, (x, y, health, alive) in enumerate(g["npcs"]):
            snap["npc_pos"][k, b] = x | y << 8
            snap["npc_health"][k, b] = health
            snap["npc_alive"][b] |= int(alive) << k
    return snap


# One game per sentence of the definition, with a = 1 (player_damage 2, armor 1)
# unless the row says otherwise: (what, me, npcs, ticks, move).
HAND = [
    ("no NPC: the plain distance", (1, 1), [], 6, RIGHT),
    ("the player on a staircase", (7, 1), [], 0, STAY),
    ("an NPC on the staircase tile: 1 + hits to step on it", (6, 1), [(7, 1, 3, 1)], 4, RIGHT),
    ("a dead end behind the staircase: the held staircase is the one way", (8, 1),
     [(7, 1, 2, 1)], 3, LEFT),
    ("a one-wide corridor forces the fight when the way round is longer", (5, 1),
     [(6, 1, 2, 1)], 4, RIGHT),
    ("two NPCs in a row", (4, 1), [(5, 1, 1, 1), (6, 1, 2, 1)], 6, RIGHT),
    ("health 127 against a = 1: round the long way (x = 1, the room, x = 8)", (5, 1),
     [(6, 1, 127, 1)], 16, LEFT),
    ("a stale cell with a clear alive bit is ignored", (5, 1), [(6, 1, 3, 0)], 2, RIGHT),
    ("the asker on a Wall", (3, 2), [], -1, STAY),
    # from (4, 3): Right to (8, 3), up to (8, 1), Left onto the staircase = 7;
    # and an NPC of 2 health at (5, 3) is worth walking round through row 4 (2
    # more moves, the fight costs 2): a tie, which the move order decides --
    # Right (the fight) comes before Down (the way round)
    ("an exact tie between fighting and going round", (4, 3), [(5, 3, 2, 1)], 9, RIGHT),
]
# a == 0 (player_damage 1): the held corridor cell cannot be entered, the way
# round it is taken; an NPC on the staircase of the dead end leaves no way
HAND_WEAK = [
    ("a == 0: round the NPC", (5, 1), [(6, 1, 1, 1)], 16, LEFT),
    ("a == 0: the staircase itself is held, and still T = 0 on it", (7, 1), [(7, 1, 1, 1)], 0, STAY),
    ("a == 0: no way onto a held staircase", (8, 1), [(7, 1, 1, 1)], -1, STAY),
]
