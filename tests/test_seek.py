"""CPU: the pair table's and the seek query's host statements
(optimax_rogue_amd.path: ``source_rows``, ``pair_field``, ``room_distance``,
``seek``) against independent ones -- scipy's all-pairs search over the
Ground-only graph with the staircase ends attached afterwards, the closed form
against the table of the materialised room, a walk that follows ``move`` cell
by cell, and per-game loops over the oracle's states in the reference's schema
-- plus the header's constants and the two entry points' refusals from a
plain-C consumer.  Integers compared exactly; nothing here needs a GPU.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import path_cases as pc
import seek_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sc.cases()
SMALL_BANKS = ("3x3", "3x4", "9x8", "17x5")


@pytest.mark.parametrize("name", SMALL_BANKS)
def test_pair_field_is_scipys(name):
    from optimax_rogue_amd import DungeonBank
    from optimax_rogue_amd.path import PATH_WALL, source_rows
    layouts, got = pc.banks()[name], sc.pair_truth(name)
    L, W, H = layouts.shape
    assert got.dtype == np.uint16 and got.shape == (L, W * H, W * H)
    for li in range(L):
        assert np.array_equal(got[li], sc.scipy_pairs(layouts[li])), (name, li)
        tiles = layouts[li].reshape(-1)
        t = got[li].astype(np.int64)
        # symmetric wherever both cells can be stood on (a Wall's own row seeds
        # nothing: UNREACHABLE off the Walls, while its column is WALL), 0 on
        # the diagonal, and the Walls' columns and rows as the header has them
        o = tiles != pc.WALL
        assert np.array_equal(t[np.ix_(o, o)], t[np.ix_(o, o)].T), (name, li)
        assert (np.diag(t)[o] == 0).all() and (t[:, ~o] == PATH_WALL).all()
        assert (t[np.ix_(~o, o)] == sc.FAR_V).all()
        # the nearest staircase's row is the staircase field
        stairs = np.flatnonzero(tiles == pc.STAIR)
        assert np.array_equal(got[li][stairs].min(axis=0).reshape(W, H), pc.truth(name)[li])
    # every source through source_rows' own arguments, in another order
    rs = np.random.RandomState(3)
    lay, cell = rs.randint(0, L, 50), rs.randint(0, W * H, 50)
    assert np.array_equal(source_rows(layouts, lay, cell), got[lay, cell])
    bank = DungeonBank(np.array(layouts))
    assert np.array_equal(bank.pair_field(), got) and bank.pair_field() is bank.pair_field()


def test_hand_built_layouts():
    from optimax_rogue_amd.path import source_rows
    F, WL = sc.FAR_V, sc.WALL_V
    # a one-wide corridor with a staircase in the middle: (1, 1) .. (5, 1)
    cut = pc.room(7, 3)
    cut[3, 1] = pc.STAIR
    # two adjacent staircases in a 5 x 4 room
    twin = pc.room(5, 4)
    twin[1, 1] = twin[2, 1] = pc.STAIR
    bank = np.stack([np.pad(cut, ((0, 0), (0, 1)), constant_values=pc.WALL),
                     np.pad(twin, ((0, 2), (0, 0)), constant_values=pc.WALL)])   # [2, 7, 4]
    H = 4
    c = lambda x, y: x * H + y
    layout = [0, 0, 0, 1, 1, 1, 0, 2, -1, 0, 0]
    cell = [c(1, 1), c(3, 1), c(5, 1), c(1, 1), c(2, 1), c(3, 2), c(0, 0), c(1, 1), c(1, 1), 28, -1]
    got = source_rows(bank, layout, cell)
    assert got.dtype == np.uint16 and got.shape == (11, 28)
    assert np.array_equal(got, sc.scipy_rows(bank, layout, cell))
    row = lambda i: got[i].reshape(7, 4)
    # the corridor: each side ends at the staircase and cannot see the other
    assert row(0)[1:6, 1].tolist() == [0, 1, 2, F, F]
    assert row(2)[1:6, 1].tolist() == [F, F, 2, 1, 0]
    assert row(1)[1:6, 1].tolist() == [2, 1, 0, 1, 2]            # a source on the staircase
    # adjacent staircases are 1 apart; from Ground each is an end of its own
    assert row(3)[2, 1] == 1 and row(4)[1, 1] == 1 and row(3)[1, 2] == 1
    assert row(5)[1, 1] == 3 and row(5)[2, 1] == 2 and row(5)[3, 1] == 1
    assert row(3)[3, 1] == 4                                       # around, not through (2, 1)
    # a Wall source and the indices outside the bank seed nothing
    for i, lay in ((6, 0), (7, 1), (8, 0), (9, 0), (10, 0)):
        assert np.array_equal(got[i], np.where(bank[lay].reshape(-1) == pc.WALL, WL, F)), i


@pytest.mark.parametrize("W,H", [(4, 4), (5, 7), (8, 8)])
def test_closed_form_is_the_rooms_table(W, H):
    """``room_distance`` against ``pair_field`` of the materialised room, for
    every staircase position and every pair of interior cells."""
    from optimax_rogue_amd import EnvConfig
    from optimax_rogue_amd.path import PATH_WALL, pair_field, room_distance
    cfg = EnvConfig(width=W, height=H)
    x, y = [a.reshape(-1) for a in np.meshgrid(np.arange(W), np.arange(H), indexing="ij")]
    inner = (x >= 1) & (x <= W - 2) & (y >= 1) & (y <= H - 2)
    changed = 0
    for sx in range(1, W - 1):
        for sy in range(1, H - 1):
            table = pair_field(sc.room_layout(W, H, sx, sy))[0].astype(np.int64)
            got = room_distance(cfg, sx, sy, x[:, None], y[:, None], x[None, :], y[None, :])
            assert got.shape == table.shape
            assert np.array_equal(got[np.ix_(inner, inner)], table[np.ix_(inner, inner)]), (sx, sy)
            assert (got[~inner] == PATH_WALL).all() and (got[:, ~inner] == PATH_WALL).all()
            manhattan = np.abs(x[:, None] - x[None, :]) + np.abs(y[:, None] - y[None, :])
            changed += int((got != manhattan)[np.ix_(inner, inner)].sum())
    if (W, H) != (4, 4):      # (a 2 x 2 interior has no cell between two others)
        assert changed >= 1


@pytest.mark.parametrize("name", ["9x8", "17x5"])
def test_following_move_reaches_the_target_in_dist_steps(name):
    """Every (cell, target) pair of every layout as one game of a hand-made
    state: player 1 on the cell, player 2 on the target.  ``seek``'s move,
    played until Stay, arrives in exactly ``dist`` steps, and no step before
    the last lands on a staircase or a Wall."""
    from optimax_rogue_amd import DungeonBank, EnvConfig
    from optimax_rogue_amd.path import MOVE_DELTAS, seek
    layouts = np.array(pc.banks()[name])
    L, W, H = layouts.shape
    bank = DungeonBank(layouts)
    cfg = EnvConfig(width=W, height=H, n_npcs=0, layouts=layouts)
    lay, c, t = [a.reshape(-1) for a in np.meshgrid(np.arange(L), np.arange(W * H),
                                                     np.arange(W * H), indexing="ij")]
    table = sc.pair_truth(name).astype(np.int64)
    keep = (layouts.reshape(L, -1)[lay, c] != pc.WALL) & (layouts.reshape(L, -1)[lay, t] != pc.WALL)
    lay, c, t = lay[keep], c[keep], t[keep]
    x, y = c // H, c % H
    tx, ty = t // H, t % H
    n = len(lay)
    snap = dict(p_x=np.stack([x, tx]), p_y=np.stack([y, ty]), p_depth=np.zeros((2, n), np.int64),
                p_layout=np.stack([lay, lay]).astype(np.int16))
    dist, move, target = seek(snap, cfg, 0, bank=bank)
    start = table[lay, t, c]
    assert np.array_equal(dist[:, 0], np.where(start == sc.FAR_V, -1, start))
    assert (target[:, 0] == 1).all() and (dist[:, 1:] == sc.ABSENT).all()
    assert (start == sc.FAR_V).sum() > 0 and (start == 0).sum() > 0
    left = dist[:, 0].copy()
    delta = {code: (dx, dy) for code, dx, dy in MOVE_DELTAS}
    for step in range(int(left.max())):
        moving = left > 0
        assert np.array_equal(move[:, 0] != 5, moving), step
        for code, (dx, dy) in delta.items():
            sel = move[:, 0] == code
            x[sel] += dx
            y[sel] += dy
        tile = layouts[lay, x, y]
        arrived = (x == tx) & (y == ty)
        assert ((tile == pc.GROUND) | arrived)[moving].all(), step
        snap["p_x"], snap["p_y"] = np.stack([x, tx]), np.stack([y, ty])
        dist, move, _ = seek(snap, cfg, 0, bank=bank)
        assert np.array_equal(dist[:, 0], np.where(moving, left - 1, left)), step
        left = dist[:, 0].copy()
    reached = start != sc.FAR_V
    assert ((x == tx) & (y == ty))[reached].all() and (left[reached] == 0).all()
    assert (move[:, 0] == 5).all()
    assert ((x == c // H) & (y == c % H))[~reached].all()      # unreachable: stayed put


# ---- path.seek on oracle states ---------------------------------------------
@pytest.fixture(scope="module")
def truths(oracle_lib):
    """case -> [(snap, {player: (dist, move, target, crossing)}) at the start
    and after the case's ticks], the per-game restatement computed once."""
    from optimax_rogue_amd import compat
    out = {}
    for name, case in CASES.items():
        cfg, bank = case["cfg"], sc.vc.bank_of(case["cfg"])
        per_state = []
        for snap in sc.vc.oracle_states(case, sc.N_GAMES):
            dists = sc.Distances(cfg, snap)
            games = [compat.game_state(snap, i, cfg, None, bank=bank) for i in range(sc.N_GAMES)]
            want = {}
            for player in (0, 1):
                rows = [sc.expected_seek(gs, snap, i, cfg, player, dists)
                        for i, gs in enumerate(games)]
                want[player] = tuple(np.array([r[k] for r in rows]) for k in range(4))
            per_state.append((snap, want))
        out[name] = per_state
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_seek_matches_the_reference_schema(truths, name):
    from optimax_rogue_amd.path import seek
    case = CASES[name]
    bank = sc.vc.bank_of(case["cfg"])
    for snap, want in truths[name]:
        for player in (0, 1):
            dist, move, target = seek(snap, case["cfg"], player, bank=bank)
            assert dist.dtype == np.int32 and move.dtype == np.int8 and target.dtype == np.int16
            assert dist.shape == move.shape == target.shape == (sc.N_GAMES, 4)
            for got, exp, what in zip((dist, move, target), want[player],
                                      ("dist", "move", "target")):
                bad = np.argwhere(got != exp)
                assert len(bad) == 0, (name, player, what, bad[:5].tolist())
            assert (dist[:, 3] == sc.ABSENT).all() and (move[:, 3] == 5).all()
            assert (target[:, 3] == -1).all()


def test_oracle_states_cover_the_seek(truths):
    """A test that passes on absent targets proves nothing: over the oracle
    states, summed over both players and both states, every kind of answer
    occurs.  Asserted on the truth alone."""
    def count(name, fn):
        return sum(int(fn(*want[p], snap, p).sum()) for snap, want in truths[name] for p in (0, 1))

    for name in ("pockets", "17x5"):
        assert count(name, lambda d, m, t, c, s, p: d[:, 0] == sc.ABSENT) >= 20, name
        assert count(name, lambda d, m, t, c, s, p: d[:, 0] == sc.UNREACHABLE) >= 20, name
        assert count(name, lambda d, m, t, c, s, p: d[:, 0] >= 0) >= 50, name
        assert count(name, lambda d, m, t, c, s, p: d[:, 1] == sc.UNREACHABLE) >= 10, name

    K = int(CASES["dense"]["cfg"].n_npcs)

    def npc_dists(snap, p):
        """int64 [K, B]: every live NPC's distance (big: dead or unreachable)."""
        from optimax_rogue_amd.query import npc_rows
        alive, nx, ny, _ = npc_rows(snap, K)
        dists = sc.Distances(CASES["dense"]["cfg"], snap)
        H = int(CASES["dense"]["cfg"].height)
        out = np.full((K, sc.N_GAMES), 1 << 30, np.int64)
        for i in range(sc.N_GAMES):
            table = dists.table(p, i)[0]
            own = int(snap["p_x"][p][i]) * H + int(snap["p_y"][p][i])
            for k in range(K):
                if alive[k, i] and table[int(nx[k, i]) * H + int(ny[k, i])][own] < sc.FAR_V:
                    out[k, i] = table[int(nx[k, i]) * H + int(ny[k, i])][own]
        return alive, out

    def tied(d, m, t, c, snap, p):
        _, nd = npc_dists(snap, p)
        return (d[:, 1] >= 0) & ((nd == d[:, 1][None, :]).sum(axis=0) >= 2)

    def not_first(d, m, t, c, snap, p):
        alive, _ = npc_dists(snap, p)
        return (d[:, 1] >= 0) & (t[:, 1] != alive.argmax(axis=0))

    assert count("dense", tied) >= 50
    assert count("dense", not_first) >= 100
    assert count("rpg", lambda d, m, t, c, s, p: d[:, 2] > 0) >= 50
    assert count("rpg", lambda d, m, t, c, s, p: d[:, 2] == 0) >= 1
    crossing = lambda d, m, t, c, s, p: c.any(axis=1)
    assert sum(count(name, crossing) for name in sc.BANKS) >= 10
    assert sum(count(name, crossing) for name in CASES if name not in sc.BANKS) >= 1
    for name in ("a", "c", "d"):
        seen = set()
        for snap, want in truths[name]:
            for p in (0, 1):
                seen |= set(want[p][1][:, 0].tolist()) | set(want[p][1][:, 1].tolist())
        assert {1, 2, 3, 4} <= seen, (name, seen)


# ---- header and library -------------------------------------------------------
def test_header_constants_are_the_modules():
    from optimax_rogue_amd import _lib, path
    with open(os.path.join(ROOT, "include", "orx_path.h")) as f:
        text = f.read()
    defs = dict(re.findall(r"#define\s+(ORX_SEEK_\w+)\s+\(?(-?\d+)\)?", text))
    assert {k: int(v) for k, v in defs.items()} == {
        "ORX_SEEK_PLAYER": path.SEEK_PLAYER, "ORX_SEEK_NPC": path.SEEK_NPC,
        "ORX_SEEK_ITEM": path.SEEK_ITEM, "ORX_SEEK_COLS": path.SEEK_COLS,
        "ORX_SEEK_UNREACHABLE": path.SEEK_UNREACHABLE, "ORX_SEEK_ABSENT": path.SEEK_ABSENT}
    assert (path.SEEK_PLAYER, path.SEEK_NPC, path.SEEK_ITEM) == (0, 1, 2)
    assert (path.SEEK_UNREACHABLE, path.SEEK_ABSENT) == (-1, -2)
    assert {"orx_path_rows", "orx_path_seek"} <= set(_lib.PATH_EXPORTS)
    for name in ("orx_path_rows", "orx_path_seek"):
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), name
    with open(os.path.join(ROOT, "include", "orx.h")) as f:
        orx_h = f.read()
    assert "orx_path" not in orx_h and "ORX_SEEK" not in orx_h
    assert "#define ORX_ABI_VERSION 7" in orx_h and _lib.ABI_VERSION == 7


def test_seek_symbols(engine_lib):
    from optimax_rogue_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert {"orx_path_rows", "orx_path_seek"} <= set(re.findall(r" T (orx_\w+)", out))
    for name in ("orx_path_rows", "orx_path_seek"):
        assert hasattr(engine_lib, name)


def test_seek_header_in_a_plain_c_consumer(engine_lib, tmp_path):
    """include/orx_path.h's new declarations compile as C99 and every refusal
    of the two entry points comes back from the host, before any launch (no
    GPU calls)."""
    exe = tmp_path / "seek_abi_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "seek_abi_check.c"), "-o", str(exe),
                    "-L", os.path.join(ROOT, "optimax_rogue_amd"), "-lorx",
                    "-Wl,-rpath," + os.path.join(ROOT, "optimax_rogue_amd")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orx_path_seek refusals: 27 of 27" in r.stdout
