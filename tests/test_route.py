"""CPU: walking distances over the remembered map (optimax_rogue_amd.route,
include/orx_route.h) without a GPU.

``route.route`` (numpy: repeated dilation of boolean arrays) is checked against
a per-game search that restates the rule on its own -- a deque over a set of
known cells -- on the oracle runs of explore_cases' four cases, with goals of
four classes.  The header's properties P1 and P2 are checked against
``explore.seek`` on the same states and along explorer runs on random connected
banks; a router run follows ``route.router_moves`` to its end; hand-built
states pin the corners of the rule.  Then the header against the export table
and the library, the build id, the host-side refusals from a plain C consumer,
and the engine's argument checks.

The coverage conditions (conditions, not measurements) as this file computes
them: on the 12 x 10 radius-1 explorer run, state-games whose stairs distance
exceeds the seek's; state-games with no frontier left to walk to and a
staircase known; every goal class hit on the oracle runs.
"""
import os
import re
import subprocess
from collections import deque

import numpy as np
import pytest

import explore_cases as ec
import route_cases as rc
import view_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ec.cases()
EVERY, GAMES = 4, 40                # the checks: every 4th tick, the first 40 games
GOAL_CLASSES = rc.GOAL_CLASSES
NEIGHBOURS = ((1, 0, -1), (2, 1, 0), (3, 0, 1), (4, -1, 0))     # Move, dx, dy: Up, Right, Down, Left
TALLY = {}                          # what the runs saw (coverage)


def count(name, n=1):
    TALLY[name] = TALLY.get(name, 0) + int(n)


def walk_route(tiles, known, start):
    """dict cell -> moves of the shortest known walk from ``start`` (whatever
    it is): explore_cases.walk_known, and a known staircase next to the walk
    ends it (it is reached, never walked through)."""
    W, H = len(tiles), len(tiles[0])
    dist, queue = {start: 0}, deque([start])
    while queue:
        x, y = queue.popleft()
        for nx, ny in ((x, y - 1), (x + 1, y), (x, y + 1), (x - 1, y)):
            if 0 <= nx < W and 0 <= ny < H and (nx, ny) not in dist and (nx, ny) in known:
                if tiles[nx][ny] == ec.GROUND:
                    dist[nx, ny] = dist[x, y] + 1
                    queue.append((nx, ny))
                elif tiles[nx][ny] == ec.STAIR:
                    dist[nx, ny] = dist[x, y] + 1
    return dist


def expected_row(t, known, own, targets):
    """(dist, move, target) of one column of one game by the per-game search:
    ``targets`` is a set of cells (None: the column is absent)."""
    W, H = len(t), len(t[0])
    if not targets:
        return -2, 5, -1
    ends = lambda c: c in known and t[c[0]][c[1]] in (ec.GROUND, ec.STAIR)
    walk = walk_route(t, known, own)
    reach = sorted((walk[c], c[0] * H + c[1]) for c in targets if c in walk and ends(c))
    if not reach:
        return -1, 5, min(x * H + y for x, y in targets)
    d, tc = reach[0]
    cell = (tc // H, tc % H)
    for m, dx, dy in NEIGHBOURS if d > 0 else ():
        n = (own[0] + dx, own[1] + dy)
        if not (0 <= n[0] < W and 0 <= n[1] < H):
            continue
        if n != cell and not (n in known and t[n[0]][n[1]] == ec.GROUND):
            continue
        if walk_route(t, known, n).get(cell) == d - 1:
            return d, m, tc
    assert d == 0, "a known walk has a first step"
    return 0, 5, tc


def cells_of(known_b):
    return set(zip(*(a.tolist() for a in np.nonzero(known_b))))


def check_route(cfg, bank, snap, p, memory, key, goal, games, what):
    """route.route of one state against the per-game search."""
    from optimax_rogue_amd import explore, route
    W, H = int(cfg.width), int(cfg.height)
    dist, move, target = route.route(memory, key, snap, cfg, p, goal=goal, bank=bank)
    assert dist.dtype == np.int32 and move.dtype == np.int8 and target.dtype == np.int32
    assert dist.shape == move.shape == target.shape == (len(memory), 4)
    assert (dist[:, 3] == -2).all() and (move[:, 3] == 5).all() and (target[:, 3] == -1).all()
    tiles = ec.tiles_of(cfg, snap, p, bank)
    known = explore.unpack(memory, W)
    ok = explore.valid(key, snap, p)
    for i in games:
        t, kn = tiles[i].tolist(), cells_of(known[i])
        own = (int(snap["p_x"][p][i]), int(snap["p_y"][p][i]))
        g = -1 if goal is None else int(goal[i])
        columns = (ec.frontier_cells(t, kn), {c for c in kn if t[c[0]][c[1]] == ec.STAIR},
                   {(g // H, g % H)} if 0 <= g < W * H else None)
        for col, targets in enumerate(columns):
            want = expected_row(t, kn, own, targets) if ok[i] else (-2, 5, -1)
            got = tuple(int(a[i, col]) for a in (dist, move, target))
            assert got == want, (what, i, col, got, want)
    return dist, move, target


def draw_goals(rs, tiles, known, H):
    """route_cases.draw_goals, counted by class."""
    goal, classes = rc.draw_goals(rs, tiles, known, H)
    for cls in classes:
        count("goal_" + cls)
    return goal


def check_properties(route_rows, seek_rows, what):
    """P1 and P2 of include/orx_route.h, and the stairs column's bound."""
    (rd, rm, rt), (sd, sm, st) = route_rows, seek_rows
    assert np.array_equal(rd[:, 0], sd[:, 0]) and np.array_equal(rm[:, 0], sm[:, 0]) \
        and np.array_equal(rt[:, 0], st[:, 0]), (what, "P1")
    done = rd[:, 0] < 0
    for a, b in ((rd, sd), (rm, sm), (rt, st)):
        assert np.array_equal(a[done, 1], b[done, 1]), (what, "P2")
    r1, s1 = rd[:, 1].astype(np.int64), sd[:, 1].astype(np.int64)
    assert ((r1 == -2) == (s1 == -2)).all(), what
    assert ((r1 >= s1) | ((r1 == -1) & (s1 >= 0))).all(), what
    return int(((s1 >= 0) & ((r1 > s1) | (r1 == -1))).sum()), int((done & (s1 != -2)).sum())


@pytest.mark.parametrize("name", sorted(CASES))
def test_route_matches_the_per_game_search(oracle_lib, name):
    from optimax_rogue_amd import explore, route, sight, view
    from oracle.oracle import Oracle
    case = CASES[name]
    cfg, bank, R = case["cfg"], vc.bank_of(case["cfg"]), case["radius"]
    W, H, N = int(cfg.width), int(cfg.height), GAMES
    ora = Oracle(cfg.to_dict(), N, case["seed"], layouts=cfg.layouts)
    ora.reset(episode=np.zeros(N, np.int32))
    maps = [explore.empty(N, W, H) for _ in (0, 1)]
    rs = np.random.RandomState(len(name) + W)
    for tick in range(case["ticks"]):
        if tick:
            ora.step(ora.policy(*case["policies"]))
        snap = ora.export()
        for p in (0, 1):
            memory, key = maps[p]
            if tick % EVERY == EVERY - 1:
                # the map of the state before: some keys are stale (ABSENT rows)
                check_route(cfg, bank, snap, p, memory, key, None, range(N), (name, tick, p, "before"))
            rows = sight.pack_rows(sight.visible_of(view.render_view(snap, cfg, p, R, bank=bank)))
            explore.update(memory, key, snap, cfg, p, R, rows)
            if tick % EVERY != EVERY - 1:
                continue
            tiles = ec.tiles_of(cfg, snap, p, bank)
            goal = draw_goals(rs, tiles, explore.unpack(memory, W), H)
            got = check_route(cfg, bank, snap, p, memory, key, goal, range(N), (name, tick, p))
            for col in range(3):
                count(f"{name}_col{col}_reached", (got[0][:, col] >= 0).sum())
                count(f"{name}_col{col}_unreachable", (got[0][:, col] == -1).sum())
            stairs_gap, done = check_properties(got, explore.seek(memory, key, snap, cfg, p, bank=bank),
                                                (name, tick, p))
            count("oracle_stairs_gap", stairs_gap)
            assert np.array_equal(route.router_moves(got[0], got[1]),
                                  explore.explorer_moves(got[0], got[1]))


def test_every_goal_class_is_hit(oracle_lib):
    for name in sorted(CASES):          # (a case that did not run in this process is run here)
        if f"{name}_col0_reached" not in TALLY:
            test_route_matches_the_per_game_search(oracle_lib, name)
    assert all(TALLY.get("goal_" + c, 0) > 0 for c in GOAL_CLASSES), TALLY
    assert TALLY["m_col2_reached"] > 0 and TALLY["m_col2_unreachable"] > 0, TALLY


# ---- along the explorer ----------------------------------------------------------------
def state(xs, ys, layout=None, st=(1, 1)):
    """A snapshot()-shaped dict with player 1 of game b at (xs[b], ys[b])."""
    B = len(xs)
    z = lambda: np.zeros((2, B), np.int32)
    snap = {"p_x": z(), "p_y": z(), "p_depth": z(), "p_health": z() + 10, "st_x": z() + st[0],
            "st_y": z() + st[1],
            "episode": np.zeros(B, np.int32), "tick": np.zeros(B, np.int32) + 3}
    snap["p_x"][:], snap["p_y"][:] = xs, ys
    if layout is not None:
        snap["p_layout"] = np.zeros((2, B), np.int16) + layout
    return snap


def random_start(W, H, radius):
    """test_explore.py's recipe: a roomy random connected bank and B = 12 games
    on random Ground cells of it."""
    from optimax_rogue_amd import DungeonBank, EnvConfig
    B, L = 12, 4
    drawn = DungeonBank.random(W, H, 3 * L, seed=W * 100 + H + radius, wall_p=0.3, connected=True)
    roomy = drawn.layouts[(drawn.layouts == ec.GROUND).sum(axis=(1, 2)) >= W * H // 3]
    assert len(roomy) >= L
    bank = DungeonBank(roomy[:L])
    cfg = EnvConfig(width=W, height=H, n_npcs=0, layouts=bank.layouts)
    rs = np.random.RandomState(W + H + radius)
    lay = rs.randint(0, L, B)
    starts = [np.argwhere(bank.layouts[l] == ec.GROUND) for l in lay]
    xy = np.array([s[rs.randint(len(s))] for s in starts])
    return cfg, bank, lay, state(xy[:, 0], xy[:, 1], lay)


DELTAS = np.array([(0, 0), (0, -1), (1, 0), (0, 1), (-1, 0), (0, 0)])


def walk(snap, moves):
    step = DELTAS[moves]
    snap["p_x"][0] += step[:, 0].astype(np.int32)
    snap["p_y"][0] += step[:, 1].astype(np.int32)
    snap["tick"] += 1


@pytest.mark.parametrize("radius", (1, 2))
@pytest.mark.parametrize("W,H", ((12, 10), (24, 20)))
def test_p1_and_p2_along_the_explorer(W, H, radius):
    """Following the SEEK's frontier move (test_explore.py's explorer): in every
    state P1 and P2 hold, and the stairs column is never below the seek's."""
    from optimax_rogue_amd import explore, route, sight
    cfg, bank, lay, snap = random_start(W, H, radius)
    B = len(lay)
    memory, key = explore.empty(B, W, H)
    longer = done_with_stairs = 0
    for moves in range(4 * W * H + 1):
        rows = sight.pack_rows(sight.visible(snap, cfg, 0, radius, bank=bank))
        explore.update(memory, key, snap, cfg, 0, radius, rows)
        seek = explore.seek(memory, key, snap, cfg, 0, bank=bank)
        got = route.route(memory, key, snap, cfg, 0, bank=bank)
        a, b = check_properties(got, seek, (W, H, radius, moves))
        longer, done_with_stairs = longer + a, done_with_stairs + b
        if moves % 8 == 0:
            check_route(cfg, bank, snap, 0, memory, key, None, range(3), (W, H, radius, moves))
        go = seek[0][:, 0] > 0
        if not go.any():
            break
        walk(snap, np.where(go, seek[1][:, 0], 5))
    else:
        raise AssertionError("the explorer did not end")
    print(f"route along the explorer {W}x{H} radius {radius}: stairs longer than the seek's in "
          f"{longer} state-games, no frontier left and a staircase known in {done_with_stairs}")
    if (W, H, radius) == (12, 10, 1):
        # conditions: the stairs column is not the seek's, and P2 had something to hold on
        assert longer > 0 and done_with_stairs > 0


@pytest.mark.parametrize("radius", (1, 2))
@pytest.mark.parametrize("W,H", ((12, 10), (24, 20)))
def test_the_router_ends_with_everything_reachable_known(W, H, radius):
    """Following ``router_moves`` while a frontier cell is left: within 4 * W *
    H moves none can be walked to any more and every cell at finite pair
    distance from the start is known.  ``route`` takes no pair table: the
    bank's is read only to judge the end."""
    from optimax_rogue_amd import explore, route, sight
    from optimax_rogue_amd.path import PATH_UNREACHABLE
    cfg, bank, lay, snap = random_start(W, H, radius)
    B = len(lay)
    start = snap["p_x"][0].astype(np.int64) * H + snap["p_y"][0]
    tiles = ec.tiles_of(cfg, snap, 0, bank)
    memory, key = explore.empty(B, W, H)
    for moves in range(4 * W * H + 1):
        rows = sight.pack_rows(sight.visible(snap, cfg, 0, radius, bank=bank))
        explore.update(memory, key, snap, cfg, 0, radius, rows)
        dist, move, _ = route.route(memory, key, snap, cfg, 0, bank=bank)
        go = dist[:, 0] > 0
        if not go.any():
            break
        chosen = route.router_moves(dist, move)
        assert np.array_equal(chosen[go], move[go, 0])
        walk(snap, np.where(go, chosen, 5))
        assert (tiles[np.arange(B), snap["p_x"][0], snap["p_y"][0]] == ec.GROUND).all()
    else:
        raise AssertionError(f"the router did not end within {4 * W * H} moves")
    assert (dist[:, 0] < 0).all()
    known = explore.unpack(memory, W)
    reachable = (bank.pair_field()[lay, start] < PATH_UNREACHABLE).reshape(B, W, H)
    assert reachable.any() and not (reachable & ~known).any()


# ---- hand-built states -------------------------------------------------------------------
def ask(cfg, bank, known, snap, goal=None, key=None, memory=None):
    from optimax_rogue_amd import explore, route
    key = np.array([[0, 0, 3, known.sum()]], np.int32) if key is None else key
    memory = explore.pack(known) if memory is None else memory
    d, m, t = route.route(memory, key, snap, cfg, 0, goal=None if goal is None else np.array([goal]),
                          bank=bank)
    return d[0].tolist(), m[0].tolist(), t[0].tolist()


def test_the_corridor_cut_by_a_staircase():
    from optimax_rogue_amd import DungeonBank, EnvConfig, explore
    # a one-wide corridor along y = 2, cut by a staircase at x = 4; the player at x = 2
    lay = np.full((9, 5), ec.WALL, np.uint8)
    lay[1:8, 2] = ec.GROUND
    lay[4, 2] = ec.STAIR
    bank = DungeonBank(lay[None])
    cfg = EnvConfig(width=9, height=5, n_npcs=0, layouts=bank.layouts)
    known = np.zeros((1, 9, 5), bool)
    known[0, :5, :] = True
    known[0, 6, :] = True           # the far column known: a frontier cell beyond the staircase
    snap = state([2], [2], 0)
    beyond, on = 6 * 5 + 2, 4 * 5 + 2
    assert ask(cfg, bank, known, snap, beyond) == ([-1, 2, -1, -2], [5, 2, 5, 5], [beyond, on, beyond, -1])
    assert ask(cfg, bank, known, snap, on) == ([-1, 2, 2, -2], [5, 2, 2, 5], [beyond, on, on, -1])
    # the goal: the player's own cell, a Wall, outside the grid, not known
    own = 2 * 5 + 2
    assert [ask(cfg, bank, known, snap, g)[i][2] for g in (own, 2 * 5 + 1, 45, -1, 5 * 5 + 2)
            for i in (0, 1, 2)] == [0, 5, own, -1, 5, 2 * 5 + 1, -2, 5, -1, -2, 5, -1, -1, 5, 5 * 5 + 2]
    # a goal one step back: Left
    assert [a[2] for a in ask(cfg, bank, known, snap, 1 * 5 + 2)] == [1, 4, 1 * 5 + 2]
    # the five invalid keys: every column absent
    for bad in ([-1, -1, -1, -1], [1, 0, 3, 5], [0, 1, 3, 5], [0, 0, 4, 5], [0, 0, 3, -1]):
        assert ask(cfg, bank, known, snap, on, key=np.array([bad], np.int32)) \
            == ([-2] * 4, [5] * 4, [-1] * 4), bad
    # the player's own cell not known: it is still where the walk starts; as a goal it has no walk
    known[0, 2, 2] = False
    # (its known neighbours are frontier cells now, the lower one to the Left)
    assert ask(cfg, bank, known, snap, own) == ([1, 2, -1, -2], [4, 2, 5, 5], [1 * 5 + 2, on, own, -1])
    known[0, 3, 2] = False          # ... and the next cell neither: nowhere to go, but the frontier is seen
    d, m, t = ask(cfg, bank, known, snap, 1 * 5 + 2)
    assert (d, m) == ([1, -1, 1, -2], [4, 5, 4, 5]) and t[:3] == [1 * 5 + 2, on, 1 * 5 + 2]
    # off the grid: absent
    assert ask(cfg, bank, known, state([9], [2], 0), on) == ([-2] * 4, [5] * 4, [-1] * 4)
    # bits at x >= W are ignored, whatever they are
    known[0, 2:4, 2] = True
    memory = explore.pack(known)
    dirty = memory | ~np.uint32((1 << 9) - 1)
    assert ask(cfg, bank, known, snap, beyond, memory=dirty) == ask(cfg, bank, known, snap, beyond)


def test_a_staircase_seen_across_a_wall():
    """The seek walks through the cells the player has not seen; the route does
    not, until the detour is known."""
    from optimax_rogue_amd import DungeonBank, EnvConfig, explore
    lay = np.full((9, 7), ec.WALL, np.uint8)
    lay[1:8, 1:6] = ec.GROUND
    lay[4, 1:5] = ec.WALL            # a wall down x = 4, open at y = 5
    lay[6, 2] = ec.STAIR
    bank = DungeonBank(lay[None])
    cfg = EnvConfig(width=9, height=7, n_npcs=0, layouts=bank.layouts)
    snap = state([2], [2], 0)
    known = np.zeros((1, 9, 7), bool)
    known[0, :5, :4] = True          # the player's side down to y = 3, the wall ...
    known[0, 6, 2] = True            # ... and the staircase (seen through a gap since closed, say)
    key = np.array([[0, 0, 3, known.sum()]], np.int32)
    seek = explore.seek(explore.pack(known), key, snap, cfg, 0, bank=bank)
    d, m, t = ask(cfg, bank, known, snap)
    assert seek[0][0, 1] == 3 + 4 + 3 and (d[1], m[1], t[1]) == (-1, 5, 6 * 7 + 2)
    known[0, :, :] = True            # the detour known: its length
    d, m, t = ask(cfg, bank, known, snap)
    assert (d[1], m[1], t[1]) == (10, 2, 6 * 7 + 2) and d[0] == -2     # (Right, then down: as short)


@pytest.mark.parametrize("W", (32, 33, 64))
def test_walks_cross_the_word_boundary(W):
    """A corridor along the whole row, the target reached only by crossing
    x = 31 | 32 (where the grid has it) in each direction."""
    from optimax_rogue_amd import DungeonBank, EnvConfig
    lay = np.full((W, 5), ec.WALL, np.uint8)
    lay[1:W - 1, 2] = ec.GROUND
    lay[3, 0] = ec.STAIR             # (a bank needs one: walled in, known, never reached)
    bank = DungeonBank(lay[None])
    cfg = EnvConfig(width=W, height=5, n_npcs=0, layouts=bank.layouts)
    known = np.ones((1, W, 5), bool)
    for a, b, mv in ((1, W - 2, 2), (W - 2, 1, 4)):
        d, m, t = ask(cfg, bank, known, state([a], [2], 0), b * 5 + 2)
        assert (d[2], m[2], t[2]) == (W - 3, mv, b * 5 + 2) and (d[0], d[1]) == (-2, -1)
    known[0, 30, :] = False          # one unknown column: the far side has no known walk
    d, m, t = ask(cfg, bank, known, state([1], [2], 0), (W - 2) * 5 + 2)
    assert (d[2], t[2]) == (-1, (W - 2) * 5 + 2) and (d[0], m[0], t[0]) == (28, 2, 29 * 5 + 2)


def test_four_by_four_and_the_empty_room():
    from optimax_rogue_amd import EnvConfig, path
    # 4 x 4: two by two Ground cells, one of them the staircase
    cfg = EnvConfig(width=4, height=4, n_npcs=0)
    known = np.ones((1, 4, 4), bool)
    snap = state([1], [1], st=(2, 2))
    assert ask(cfg, None, known, snap, 2 * 4 + 2) == ([-2, 2, 2, -2], [5, 2, 2, 5], [-1, 10, 10, -1])
    # no bank, fully known: path.room_distance to every cell a walk may end on
    cfg = EnvConfig(width=9, height=7, n_npcs=0)
    known = np.ones((1, 9, 7), bool)
    snap = state([2], [3], st=(4, 3))
    for g in range(9 * 7):
        gx, gy = g // 7, g % 7
        want = int(path.room_distance(cfg, 4, 3, 2, 3, gx, gy))
        d, m, t = ask(cfg, None, known, snap, g)
        assert d[2] == (want if want < path.PATH_UNREACHABLE else -1) and t[2] == g, (g, d, want)
        assert (d[0], d[1], t[1]) == (-2, 2, 4 * 7 + 3)


@pytest.mark.parametrize("W,H", ((12, 10), (34, 8), (8, 12)))
def test_the_serpentine_is_as_long_as_its_construction_says(W, H):
    """route_cases.serpentine (the GPU suite's largest grid) at sizes the
    reference walks in no time: the distance is the construction's."""
    from optimax_rogue_amd import DungeonBank, EnvConfig
    lay, start, end, moves = rc.serpentine(W, H)
    bank = DungeonBank(lay[None])
    cfg = EnvConfig(width=W, height=H, n_npcs=0, layouts=bank.layouts)
    known = np.ones((1, W, H), bool)
    d, m, t = ask(cfg, bank, known, state([start[0]], [start[1]], 0), end[0] * H + end[1])
    assert (d, m, t) == ([-2, moves, moves, -2], [5, 2, 2, 5], [-1, t[2], t[2], -1]) and t[2] == end[0] * H + end[1]


def test_planes_are_the_layouts_bits():
    from optimax_rogue_amd import DungeonBank, explore, route
    bank = DungeonBank.random(40, 8, 3, seed=5, wall_p=0.15, connected=True)
    pl = route.planes(bank.layouts)
    assert pl.dtype == np.uint32 and pl.shape == (3, 2, 8, 2)
    assert np.array_equal(explore.unpack(pl[:, 0], 40), bank.layouts == ec.GROUND)
    assert np.array_equal(explore.unpack(pl[:, 1], 40), bank.layouts == ec.STAIR)
    assert not (pl[:, :, :, 1] >> np.uint32(8)).any()


# ---- header, exports, build id, refusals ----------------------------------------------
def test_header_is_the_export_table():
    import optimax_rogue_amd
    from optimax_rogue_amd import _lib, route
    with open(os.path.join(ROOT, "include", "orx_route.h")) as f:
        text = f.read()
    for name, value in (("FRONTIER", route.ROUTE_FRONTIER), ("STAIRS", route.ROUTE_STAIRS),
                        ("GOAL", route.ROUTE_GOAL)):
        assert int(re.search(rf"#define ORX_ROUTE_{name} +(\d+)", text).group(1)) == value
    assert (route.ROUTE_FRONTIER, route.ROUTE_STAIRS, route.ROUTE_GOAL) == (0, 1, 2)
    assert '#include "orx_explore.h"' in text and "P1." in text and "P2." in text
    decl = sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(orx_\w+)\s*\(", text, re.M)))
    assert decl == sorted(_lib.ROUTE_EXPORTS) == ["orx_route", "orx_route_build_id", "orx_route_planes"]
    for hdr in ("orx.h", "orx_view.h", "orx_explore.h"):
        with open(os.path.join(ROOT, "include", hdr)) as f:
            assert "orx_route" not in f.read()
    assert _lib.ABI_VERSION == 7 and optimax_rogue_amd.route is route


def test_route_header_in_a_plain_c_consumer(engine_lib, tmp_path):
    """include/orx_route.h compiles as C99 and every refusal of both entry
    points comes back from the host, before any launch (no GPU calls)."""
    exe = tmp_path / "route_abi_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "route_abi_check.c"), "-o", str(exe),
                    "-L", os.path.join(ROOT, "optimax_rogue_amd"), "-lorx",
                    "-Wl,-rpath," + os.path.join(ROOT, "optimax_rogue_amd")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orx_route_planes refusals: 6 of 6" in r.stdout
    assert "orx_route refusals: 31 of 31" in r.stdout


def test_engine_route_checks_come_before_the_library():
    """BatchedEngine.explore_route / explore_route_moves refuse a bad player,
    ``goal`` or ``out`` before any launch or allocation (an engine-shaped
    stand-in: no GPU here)."""
    import torch
    from optimax_rogue_amd import EnvConfig
    from optimax_rogue_amd.engine import BatchedEngine

    class Lib:
        def orx_route(self, *a):
            raise AssertionError("launched")
        orx_route_planes = orx_explore_update = orx_path_rows = orx_route

    eng = BatchedEngine.__new__(BatchedEngine)
    eng.lib, eng.B, eng.device = Lib(), 6, torch.device("cpu")
    eng.cfg, eng.bank = EnvConfig(width=10, height=8, n_npcs=0), None
    i32 = torch.int32
    row = lambda dt: torch.empty((6, 4), dtype=dt)
    for kw in (dict(player=2), dict(player=-1),
               dict(out=(row(i32), row(torch.int8))),
               dict(out=(row(i32), row(torch.int8), row(torch.int16))),
               dict(out=(row(i32), row(torch.int8), torch.empty((5, 4), dtype=i32))),
               dict(goal=[1, 2, 3, 4, 5, 6]),
               dict(goal=torch.zeros(5, dtype=i32)),
               dict(goal=torch.zeros((6, 1), dtype=i32)),
               dict(goal=torch.zeros(6, dtype=torch.float32))):
        with pytest.raises(ValueError):
            eng.explore_route(**kw)
    for player in (2, -1):
        with pytest.raises(ValueError):
            eng.explore_route_moves(player)
    assert eng.route_planes is None and not getattr(eng, "_explore_maps", None)
    assert getattr(eng, "_pair_field", None) is None
