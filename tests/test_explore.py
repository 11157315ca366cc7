"""CPU: the remembered map (optimax_rogue_amd.explore, include/orx_explore.h)
without a GPU.

``explore.update`` (vectorised, bit words) is checked every tick of ORACLE runs
against an independent restatement (explore_cases.Memory: a Python set of grid
cells per game, fed by sight_cases.expected_seen): the map, ``gained``, the key
and the remembered planes.  ``explore.seek`` is checked against a breadth-first
search over known Ground cells (the frontier column: the search never leaves
what the player knows), ``path.source_rows`` (the stairs column) and
``path.room_distance`` (no bank), and on hand-built layouts.  The explorer --
follow the frontier move -- is run to its end on random connected banks.  Then
the header against the export table and the library, the build id, the
host-side refusals from a plain C consumer, and the engine's argument checks.

The coverage counts of case ``m`` on the oracle's states (200 games, 60 ticks,
both players, radius 2), as this file computes them: maps cleared by a depth
change 916, by an episode change 800; known-but-unseen window cells 12,504;
updates that gained something 7,348, nothing 16,652; staircase known 12,084,
not yet known 11,916.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import explore_cases as ec
import view_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ec.cases()
SEEK_EVERY, SEEK_GAMES = 4, 40      # the seek checks: every 4th tick, the first 40 games
RUNS = {}                           # case -> tally


def check_seek(cfg, bank, snap, p, memory, key, games, mems):
    """explore.seek of one state against the searches, game by game."""
    from optimax_rogue_amd import explore, path
    from optimax_rogue_amd.path import SEEK_ABSENT, SEEK_UNREACHABLE
    W, H = int(cfg.width), int(cfg.height)
    dist, move, target = explore.seek(memory, key, snap, cfg, p, bank=bank)
    assert dist.dtype == np.int32 and move.dtype == np.int8 and target.dtype == np.int32
    assert (dist[:, 2:] == SEEK_ABSENT).all() and (move[:, 2:] == 5).all() and (target[:, 2:] == -1).all()
    tiles = ec.tiles_of(cfg, snap, p, bank)
    deltas = {1: (0, -1), 2: (1, 0), 3: (0, 1), 4: (-1, 0)}
    for i in games:
        t = tiles[i].tolist()
        known = mems[i].cells
        own = (int(snap["p_x"][p][i]), int(snap["p_y"][p][i]))
        # the frontier column: a search that never leaves the known Ground cells
        walk = ec.walk_known(t, known, own)
        front = ec.frontier_cells(t, known)
        reach = sorted((walk[c], c[0] * H + c[1]) for c in front if c in walk)
        d, m, tc = (int(a[i, 0]) for a in (dist, move, target))
        if not front:
            assert (d, m, tc) == (SEEK_ABSENT, 5, -1), (i, d, m, tc)
        elif not reach:
            assert (d, m, tc) == (SEEK_UNREACHABLE, 5, min(x * H + y for x, y in front)), (i, d)
        else:
            assert (d, tc) == reach[0], (i, d, tc, reach[0])
            assert d > 0 and m in deltas, (i, d, m)
            nxt = (own[0] + deltas[m][0], own[1] + deltas[m][1])
            assert nxt in known and t[nxt[0]][nxt[1]] == ec.GROUND, (i, nxt)
            # ... and one step closer to that very cell
            assert ec.walk_known(t, known, nxt).get((tc // H, tc % H)) == d - 1, (i, nxt)
        # the stairs column: the layout's true distance to the nearest known staircase
        stairs = sorted(x * H + y for x, y in known if t[x][y] == ec.STAIR)
        d, m, tc = (int(a[i, 1]) for a in (dist, move, target))
        if not stairs:
            assert (d, m, tc) == (SEEK_ABSENT, 5, -1), (i, d, m, tc)
            continue
        if bank is None:
            sx, sy = int(snap["st_x"][p][i]), int(snap["st_y"][p][i])
            ds = [int(path.room_distance(cfg, sx, sy, own[0], own[1], c // H, c % H)) for c in stairs]
        else:
            lay = int(snap["p_layout"][p][i])
            row = path.source_rows(bank.layouts, [lay], [own[0] * H + own[1]])[0]
            ds = [int(row[c]) for c in stairs]
        best = min(zip(ds, stairs))
        if best[0] >= path.PATH_UNREACHABLE:
            assert (d, m, tc) == (SEEK_UNREACHABLE, 5, stairs[0]), (i, d, m, tc)
        else:
            assert (d, tc) == best, (i, d, tc, best)
            assert (m == 5) == (d == 0), (i, d, m)


def run_case(name):
    """One case on the oracle, tick by tick: every assertion of the update and
    the sampled ones of the seek; returns the coverage tally."""
    from optimax_rogue_amd import compat, explore, sight, view
    from oracle.oracle import Oracle
    case = CASES[name]
    cfg, bank, R = case["cfg"], vc.bank_of(case["cfg"]), case["radius"]
    W, H, N = int(cfg.width), int(cfg.height), ec.N_GAMES
    ora = Oracle(cfg.to_dict(), N, case["seed"], layouts=cfg.layouts)
    ora.reset(episode=np.zeros(N, np.int32))
    maps = [explore.empty(N, W, H) for _ in (0, 1)]
    rest = [[ec.Memory() for _ in range(N)] for _ in (0, 1)]
    tally = {k: 0 for k in ec.TALLY_KEYS}
    for tick in range(case["ticks"]):
        if tick:
            ora.step(ora.policy(*case["policies"]))
        snap = ora.export()
        games = [compat.game_state(snap, i, cfg, None, bank=bank) for i in range(N)]
        for p in (0, 1):
            cells, hp = view.render_view(snap, cfg, p, R, bank=bank, health=True)
            rows = sight.pack_rows(sight.visible_of(cells))
            memory, key = maps[p]
            got_c, got_h = cells.copy(), hp.copy()
            gained = explore.update(memory, key, snap, cfg, p, R, rows, got_c, got_h)
            assert gained.dtype == np.int32 and memory.dtype == np.uint32 and key.dtype == np.int32
            known = explore.unpack(memory, W)
            assert np.array_equal(explore.pack(known), memory)
            assert explore.valid(key, snap, p).all()
            tiles = ec.tiles_of(cfg, snap, p, bank)
            for i, gs in enumerate(games):
                mem = rest[p][i]
                why, g, seen = mem.update(gs, p, R, snap["episode"][i], snap["tick"][i])
                viewer = gs.iden_lookup[1 + p]
                what = (name, tick, p, i)
                assert gained[i] == g, what
                assert np.array_equal(known[i], mem.known(W, H)), what
                assert key[i].tolist() == [snap["episode"][i], viewer.depth, snap["tick"][i],
                                           len(mem.cells)], what
                want_c, want_h = ec.remembered(cells[i], hp[i], viewer, R, seen, mem.cells, W, H)
                assert np.array_equal(got_c[i], want_c) and np.array_equal(got_h[i], want_h), what
                tally["cleared_by_depth"] += why == "depth"
                tally["cleared_by_episode"] += why == "episode"
                tally["gained" if g else "gained_nothing"] += 1
            tally["known_unseen_cells"] += int(((got_c & 128 != 0) & (got_c & 64 == 0)).sum())
            has = (known & (tiles == ec.STAIR)).any(axis=(1, 2))
            tally["stairs_known"] += int(has.sum())
            tally["stairs_unknown"] += int((~has).sum())
            if tick % SEEK_EVERY == SEEK_EVERY - 1:
                check_seek(cfg, bank, snap, p, memory, key, range(min(N, SEEK_GAMES)), rest[p])
    return tally


@pytest.mark.parametrize("name", sorted(CASES))
def test_update_and_seek_match_the_restatement(oracle_lib, name):
    RUNS[name] = run_case(name)
    print("explore coverage", name, RUNS[name])


def test_oracle_states_cover_the_map(oracle_lib):
    """A test that passes where nothing is forgotten or hidden proves nothing:
    in case m maps are cleared by descents and by new episodes, cells stay
    known out of sight, updates gain and do not, the staircase is known and
    not yet known."""
    if "m" not in RUNS:
        RUNS["m"] = run_case("m")
    assert all(RUNS["m"][k] > 0 for k in ec.TALLY_KEYS), RUNS["m"]


# ---- hand-built layouts ----------------------------------------------------------
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


def test_seek_on_hand_built_layouts():
    from optimax_rogue_amd import DungeonBank, EnvConfig, explore
    from optimax_rogue_amd.path import SEEK_ABSENT, SEEK_UNREACHABLE
    # a one-wide corridor along y = 2, cut by a staircase at x = 4; the player at x = 2
    lay = np.full((9, 5), ec.WALL, np.uint8)
    lay[1:8, 2] = ec.GROUND
    lay[4, 2] = ec.STAIR
    bank = DungeonBank(lay[None])
    cfg = EnvConfig(width=9, height=5, n_npcs=0, layouts=bank.layouts)
    known = np.zeros((1, 9, 5), bool)
    known[0, :5, :] = True          # everything up to the staircase ...
    known[0, 6, :] = True           # ... and one column beyond it, its neighbours unknown
    key = np.array([[0, 0, 3, known.sum()]], np.int32)
    snap = state([2], [2], 0)
    assert np.argwhere(explore.frontier(known, lay[None])[0]).tolist() == [[6, 2]]
    dist, move, target = explore.seek(explore.pack(known), key, snap, cfg, 0, bank=bank)
    assert dist[0].tolist() == [SEEK_UNREACHABLE, 2, SEEK_ABSENT, SEEK_ABSENT]
    assert move[0].tolist() == [5, 2, 5, 5] and target[0].tolist() == [6 * 5 + 2, 4 * 5 + 2, -1, -1]
    assert explore.explorer_moves(dist, move).tolist() == [2]
    # the same corridor seen only up to x = 3: the frontier is its known end
    known[:] = False
    known[0, :4, :] = True
    key[0, 3] = known.sum()
    dist, move, target = explore.seek(explore.pack(known), key, snap, cfg, 0, bank=bank)
    assert dist[0].tolist() == [1, SEEK_ABSENT, SEEK_ABSENT, SEEK_ABSENT]
    assert move[0].tolist() == [2, 5, 5, 5] and target[0, 0] == 3 * 5 + 2
    # an invalid key (every way): both columns absent
    for bad in ([-1, -1, -1, -1], [1, 0, 3, 5], [0, 1, 3, 5], [0, 0, 4, 5], [0, 0, 3, -1]):
        dist, move, target = explore.seek(explore.pack(known), np.array([bad], np.int32), snap, cfg,
                                          0, bank=bank)
        assert (dist == SEEK_ABSENT).all() and (move == 5).all() and (target == -1).all(), bad
    # a fully explored room without a bank: no frontier; the staircase by the room form
    cfg = EnvConfig(width=7, height=6, n_npcs=0)
    known = np.ones((1, 7, 6), bool)
    key = np.array([[0, 0, 3, 42]], np.int32)
    snap = state([1], [4], st=(5, 4))
    dist, move, target = explore.seek(explore.pack(known), key, snap, cfg, 0)
    assert dist[0].tolist() == [SEEK_ABSENT, 4, SEEK_ABSENT, SEEK_ABSENT]
    assert move[0].tolist() == [5, 2, 5, 5] and target[0].tolist() == [-1, 5 * 6 + 4, -1, -1]
    assert explore.explorer_moves(dist, move).tolist() == [2]
    known[0, 5, 4] = False           # the staircase not seen yet: its neighbours are the frontier
    dist, move, target = explore.seek(explore.pack(known), key, snap, cfg, 0)
    assert dist[0].tolist() == [3, SEEK_ABSENT, SEEK_ABSENT, SEEK_ABSENT]
    assert target[0, 0] == 4 * 6 + 4 and move[0, 0] == 2


def test_update_ignores_bits_outside_the_window_and_the_grid():
    from optimax_rogue_amd import EnvConfig, explore
    cfg = EnvConfig(width=40, height=6, n_npcs=0)
    snap = state([1, 33, 38], [0, 3, 5])
    memory, key = explore.empty(3, 40, 6)
    rows = np.full((3, 5), 0xFFFFFFFF, np.uint32)
    gained = explore.update(memory, key, snap, cfg, 0, 2, rows)
    assert gained.tolist() == [4 * 3, 5 * 5, 4 * 3] and key[:, 3].tolist() == gained.tolist()
    known = explore.unpack(memory, 40)
    assert known[0, :4, :3].all() and known[1, 31:36, 1:6].all() and known[2, 36:, 3:].all()
    assert known.sum() == gained.sum()
    assert not (memory[:, :, 1] >> np.uint32(8)).any()        # bits at x >= W stay zero
    assert explore.words(40) == 2 and explore.words(32) == 1 and explore.words(33) == 2
    # the same call again gains nothing; a tick that ran backwards clears
    assert explore.update(memory, key, snap, cfg, 0, 2, rows).tolist() == [0, 0, 0]
    snap["tick"][:] = 1
    assert explore.update(memory, key, snap, cfg, 0, 2, rows * 0).tolist() == [0, 0, 0]
    assert not memory.any() and key[:, 3].tolist() == [0, 0, 0] and key[:, 2].tolist() == [1, 1, 1]


# ---- the explorer ends --------------------------------------------------------------
@pytest.mark.parametrize("radius", (1, 2, 5))
@pytest.mark.parametrize("W,H", ((12, 10), (9, 8), (24, 20), (16, 16)))
def test_the_explorer_ends_with_everything_reachable_known(W, H, radius):
    """From random Ground cells of random connected banks, following the
    frontier move: within 4 * W * H moves (a condition, not a measurement) no
    frontier cell can be walked to any more, and every cell at finite pair
    distance from the start is known.  Every step's distance equals the
    search over known Ground cells (the first games of the batch)."""
    from optimax_rogue_amd import DungeonBank, EnvConfig, explore, sight
    from optimax_rogue_amd.path import PATH_UNREACHABLE
    B, L = 12, 4
    drawn = DungeonBank.random(W, H, 3 * L, seed=W * 100 + H + radius, wall_p=0.3, connected=True)
    # (``connected`` can leave a layout a pocket round its staircase: the roomy ones)
    roomy = drawn.layouts[(drawn.layouts == ec.GROUND).sum(axis=(1, 2)) >= W * H // 3]
    assert len(roomy) >= L
    bank = DungeonBank(roomy[:L])
    cfg = EnvConfig(width=W, height=H, n_npcs=0, layouts=bank.layouts)
    rs = np.random.RandomState(W + H + radius)
    lay = rs.randint(0, L, B)
    starts = [np.argwhere(bank.layouts[l] == ec.GROUND) for l in lay]
    xy = np.array([s[rs.randint(len(s))] for s in starts])
    snap = state(xy[:, 0], xy[:, 1], lay)
    start = xy[:, 0] * H + xy[:, 1]
    memory, key = explore.empty(B, W, H)
    deltas = np.array([(0, 0), (0, -1), (1, 0), (0, 1), (-1, 0), (0, 0)])
    tiles = ec.tiles_of(cfg, snap, 0, bank)
    most = 0
    for moves in range(4 * W * H + 1):
        rows = sight.pack_rows(sight.visible(snap, cfg, 0, radius, bank=bank))
        explore.update(memory, key, snap, cfg, 0, radius, rows)
        dist, move, target = explore.seek(memory, key, snap, cfg, 0, bank=bank)
        known = explore.unpack(memory, W)
        for i in range(3):
            cells = set(zip(*np.nonzero(known[i])))
            own = (int(snap["p_x"][0][i]), int(snap["p_y"][0][i]))
            walk = ec.walk_known(tiles[i].tolist(), cells, own)
            reach = [walk[c] for c in ec.frontier_cells(tiles[i].tolist(), cells) if c in walk]
            assert (min(reach) if reach else -1) == max(int(dist[i, 0]), -1), (moves, i)
        go = dist[:, 0] > 0
        if not go.any():
            break
        most = moves + 1
        step = deltas[np.where(go, move[:, 0], 5)]
        snap["p_x"][0] += step[:, 0].astype(np.int32)
        snap["p_y"][0] += step[:, 1].astype(np.int32)
        snap["tick"] += 1
        assert (tiles[np.arange(B), snap["p_x"][0], snap["p_y"][0]] == ec.GROUND).all()
    else:
        raise AssertionError(f"the explorer did not end within {4 * W * H} moves")
    assert (dist[:, 0] < 0).all()
    pairs = bank.pair_field()
    reachable = (pairs[lay, start] < PATH_UNREACHABLE).reshape(B, W, H)
    assert reachable.any() and not (reachable & ~known).any()
    print(f"explorer {W}x{H} radius {radius}: at most {most} moves of {W * H} cells")


# ---- header, exports, build id, refusals ----------------------------------------------
def test_header_is_the_export_table():
    from optimax_rogue_amd import _lib, explore
    with open(os.path.join(ROOT, "include", "orx_explore.h")) as f:
        text = f.read()
    assert int(re.search(r"#define ORX_EXPLORE_KNOWN (\d+)", text).group(1)) \
        == explore.EXPLORE_KNOWN == 128
    assert int(re.search(r"#define ORX_EXPLORE_FRONTIER (\d+)", text).group(1)) \
        == explore.EXPLORE_FRONTIER == 0
    assert int(re.search(r"#define ORX_EXPLORE_STAIRS +(\d+)", text).group(1)) \
        == explore.EXPLORE_STAIRS == 1
    assert '#include "orx_sight.h"' in text and '#include "orx_path.h"' in text
    decl = sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(orx_\w+)\s*\(", text, re.M)))
    assert decl == sorted(_lib.EXPLORE_EXPORTS) \
        == ["orx_explore_build_id", "orx_explore_seek", "orx_explore_update"]
    for hdr in ("orx.h", "orx_view.h"):
        with open(os.path.join(ROOT, "include", hdr)) as f:
            assert "orx_explore" not in f.read()
    assert _lib.ABI_VERSION == 7


def test_explore_header_in_a_plain_c_consumer(engine_lib, tmp_path):
    """include/orx_explore.h compiles as C99 and every refusal of both entry
    points comes back from the host, before any launch (no GPU calls)."""
    exe = tmp_path / "explore_abi_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "explore_abi_check.c"), "-o", str(exe),
                    "-L", os.path.join(ROOT, "optimax_rogue_amd"), "-lorx",
                    "-Wl,-rpath," + os.path.join(ROOT, "optimax_rogue_amd")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orx_explore_update refusals: 24 of 24" in r.stdout
    assert "orx_explore_seek refusals: 29 of 29" in r.stdout


def test_engine_explore_checks_come_before_the_library():
    """BatchedEngine.explore / explore_seek / explore_forget / explore_map refuse
    a bad radius, player or ``out`` before any launch or allocation (an
    engine-shaped stand-in: no GPU here)."""
    import torch
    from optimax_rogue_amd import EnvConfig
    from optimax_rogue_amd.engine import BatchedEngine

    class Lib:
        def orx_view(self, *a):
            raise AssertionError("launched")
        orx_sight = orx_explore_update = orx_explore_seek = orx_path_rows = orx_view

    eng = BatchedEngine.__new__(BatchedEngine)
    eng.lib, eng.B, eng.device = Lib(), 6, torch.device("cpu")
    eng.cfg, eng.bank = EnvConfig(width=10, height=8, n_npcs=0), None
    i32, u8 = torch.int32, torch.uint8
    gained, plane = torch.empty(6, dtype=i32), torch.empty((6, 11, 11), dtype=u8)
    for kw in (dict(radius=0), dict(radius=16), dict(radius=5, player=2), dict(radius=5, player=-1),
               dict(radius=5, health=True),
               dict(radius=5, out=torch.empty(5, dtype=i32)),
               dict(radius=5, out=torch.empty(6, dtype=torch.int64)),
               dict(radius=5, out=(gained, plane)),
               dict(radius=5, view=True, out=gained),
               dict(radius=5, view=True, out=(gained, torch.empty((6, 11, 12), dtype=u8))),
               dict(radius=5, view=True, health=True, out=(gained, plane)),
               dict(radius=5, view=True, health=True, out=(gained, plane, plane))):
        with pytest.raises(ValueError):
            eng.explore(**kw)
    row = lambda dt: torch.empty((6, 4), dtype=dt)
    for kw in (dict(player=2), dict(player=-1),
               dict(out=(row(i32), row(torch.int8))),
               dict(out=(row(i32), row(torch.int8), row(torch.int16))),
               dict(out=(row(i32), row(torch.int8), torch.empty((5, 4), dtype=i32)))):
        with pytest.raises(ValueError):
            eng.explore_seek(**kw)
    for player in (2, -1, "a"):
        with pytest.raises(ValueError):
            eng.explore_forget(player)
        with pytest.raises(ValueError):
            eng.explore_map(player)
    eng.explore_forget()              # (no map yet: nothing to clear, nothing allocated)
    assert not getattr(eng, "_explore_maps", None)
