"""CPU: the danger field's host statement (optimax_rogue_amd.path.threat)
against independent ones -- per-game loops over the oracle's states in the
reference's schema on scipy's all-pairs distances, ``seek``'s two columns it
must repeat (T1), its own window (T2), a play-out on the oracle that collects
what ``after`` promised, and hand-built states whose rows are written out from
include/orx_path.h's rule -- plus the header's constants and the entry point's
refusals from a plain-C consumer.  Integers compared exactly; nothing here
needs a GPU.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import seek_cases as sc
import threat_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sc.cases()
A, F, W_ = tc.ABSENT, tc.FAR_V, tc.WALL_V
UP, RIGHT, DOWN, LEFT, STAY = 1, 2, 3, 4, 5


@pytest.fixture(scope="module")
def states(oracle_lib):
    """case -> [(oracle, snap)] at the start and after the case's ticks."""
    return {name: tc.oracle_at(case) for name, case in CASES.items()}


@pytest.fixture(scope="module")
def truths(states):
    """case -> [(snap, {player: (dist, move, target, after, window, notes)})],
    the per-game restatement computed once."""
    from optimax_rogue_amd import compat
    out = {}
    for name, case in CASES.items():
        cfg, bank = case["cfg"], sc.vc.bank_of(case["cfg"])
        per_state = []
        for _, snap in states[name]:
            dists = sc.Distances(cfg, snap)
            games = [compat.game_state(snap, i, cfg, None, bank=bank) for i in range(tc.N_GAMES)]
            want = {}
            for player in (0, 1):
                rows = [tc.expected_threat(gs, snap, i, cfg, player, dists)
                        for i, gs in enumerate(games)]
                want[player] = tuple(np.array([r[k] for r in rows]) for k in range(5)) \
                    + ([r[5] for r in rows],)
            per_state.append((snap, want))
        out[name] = per_state
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_threat_matches_the_reference_schema(truths, name):
    from optimax_rogue_amd.path import threat
    case = CASES[name]
    bank = sc.vc.bank_of(case["cfg"])
    V = 2 * tc.RADIUS + 1
    for snap, want in truths[name]:
        for player in (0, 1):
            got = threat(snap, case["cfg"], player, tc.RADIUS, bank=bank)
            dist, move, target, after, window = got
            assert [a.dtype for a in got] == [np.int32, np.int8, np.int16, np.int32, np.uint16]
            assert dist.shape == move.shape == target.shape == (tc.N_GAMES, 4)
            assert after.shape == (tc.N_GAMES, 8) and window.shape == (tc.N_GAMES, V, V)
            for g, exp, what in zip(got, want[player], ("dist", "move", "target", "after",
                                                        "window")):
                bad = np.argwhere(g != exp)
                assert len(bad) == 0, (name, player, what, bad[:5].tolist())
            assert (dist[:, 3] == A).all() and (move[:, 3] == STAY).all()
            assert (target[:, 3] == -1).all() and (after[:, [0, 6, 7]] == A).all()
            # without a radius: the same rows and no window
            rows = threat(snap, case["cfg"], player, bank=bank)
            assert rows[4] is None and all(np.array_equal(a, b) for a, b in zip(rows[:4], got))


@pytest.mark.parametrize("name", sorted(CASES))
def test_t1_and_t2(states, name):
    """T1: columns PLAYER and NPC of dist and target are ``seek``'s.  T2: the
    window's centre is dist[ANY] and its four neighbours are ``after``'s values
    wherever those moves are candidates -- on every state."""
    from optimax_rogue_amd.path import MOVE_DELTAS, seek, threat
    case = CASES[name]
    bank = sc.vc.bank_of(case["cfg"])
    for _, snap in states[name]:
        for player in (0, 1):
            for R in (1, 4):
                dist, move, target, after, window = threat(snap, case["cfg"], player, R, bank=bank)
                sdist, _, starget = seek(snap, case["cfg"], player, bank=bank)
                assert np.array_equal(dist[:, :2], sdist[:, :2])
                assert np.array_equal(target[:, :2], starget[:, :2])
                shown = np.where(window >= F, -1, window.astype(np.int64))
                has = dist[:, 2] != A
                assert np.array_equal(shown[has, R, R], dist[has, 2])
                assert (window[~has, R, R] >= F).all()
                assert np.array_equal(after[:, STAY], dist[:, 2])
                for code, dx, dy in MOVE_DELTAS:
                    cand = after[:, code] != A
                    assert np.array_equal(shown[cand, R + dy, R + dx], after[cand, code])
                    assert not (cand & ~has).any()
                # a move that is taken is a candidate, and strictly gains
                ahead = after[np.arange(len(move)), move[:, 2]].astype(np.int64)
                own = dist[:, 2].astype(np.int64)
                rank = lambda v: np.where(v == -1, 1 << 20, v)
                moving = move[:, 2] != STAY
                assert (ahead[moving] != A).all()
                assert (rank(ahead[moving]) > rank(own[moving])).all()


@pytest.mark.parametrize("name", tc.PLAYOUT)
def test_playing_the_move_gets_what_after_promised(states, name):
    """Flags 0 and NPCs that stand still: the viewer plays move[ANY], the other
    player Stays, on a copy of the oracle.  In the games still in progress on
    the same depth and episode, the new dist[ANY] is the old after[move]."""
    from optimax_rogue_amd.path import threat
    case = CASES[name]
    cfg, bank = case["cfg"], sc.vc.bank_of(case["cfg"])
    assert int(cfg.flags) == 0 and int(cfg.npc_policy) == 0
    held = moved = 0
    for ora, snap in states[name]:
        for player in (0, 1):
            dist, move, _, after, _ = threat(snap, cfg, player, bank=bank)
            promised = after[np.arange(tc.N_GAMES), move[:, 2]]
            actions = np.full((tc.N_GAMES, 2), STAY, np.int8)
            actions[:, player] = move[:, 2]
            twin = ora.clone()
            twin.step(actions)
            then = twin.export()
            same = (np.asarray(snap["status"]) == 1) & (np.asarray(then["status"]) == 1) \
                & (then["p_depth"][player] == snap["p_depth"][player]) \
                & (then["episode"] == snap["episode"])
            now = threat(then, cfg, player, bank=bank)[0][:, 2]
            bad = np.flatnonzero(same & (now != promised))
            assert len(bad) == 0, (name, player, bad[:5].tolist())
            held += int(same.sum())
            moved += int((same & (move[:, 2] != STAY)).sum())
    assert held >= 2 * tc.N_GAMES and moved >= 20, (held, moved)


def test_oracle_states_cover_the_threat(truths):
    """A test that passes on absent threats proves nothing: over the oracle's
    states, both players and both states, every kind of answer occurs.
    Asserted on the truth alone."""
    def count(names, fn):
        return sum(int(np.sum(fn(*want[p]))) for name in names for _, want in truths[name]
                   for p in (0, 1))

    everywhere = sorted(CASES)
    for code in (UP, RIGHT, DOWN, LEFT, STAY):
        assert count(everywhere, lambda d, m, t, a, w, n: m[:, 2] == code) >= 50, code
        assert count(sc.BANKS, lambda d, m, t, a, w, n: m[:, 2] == code) >= 20, code
    assert count(everywhere, lambda d, m, t, a, w, n: d[:, 2] == A) >= 50
    assert count(["pockets"], lambda d, m, t, a, w, n: d[:, 2] == tc.UNREACHABLE) >= 10
    assert count(["pockets"], lambda d, m, t, a, w, n: (d[:, :2] == tc.UNREACHABLE).any(1)
                 & (d[:, 2] >= 0)) >= 10           # one column cut off, the other not
    assert count(everywhere, lambda d, m, t, a, w, n: [x["stair_excluded"] for x in n]) >= 20
    assert count(everywhere, lambda d, m, t, a, w, n: [x["tie_kept"] for x in n]) >= 20
    assert count(everywhere, lambda d, m, t, a, w, n: (t[:, 2] >= 1) & (t[:, 2] <= 2)) >= 50
    assert count(everywhere, lambda d, m, t, a, w, n: t[:, 2] >= 3) >= 50
    # the player wins a tie with an NPC, and loses where the NPC is nearer
    assert count(everywhere, lambda d, m, t, a, w, n: (d[:, 0] == d[:, 1]) & (d[:, 0] >= 0)
                 & (t[:, 2] <= 2)) >= 5
    # a Separated start: the NPCs hunt the player on their depth, not the other
    assert count(["b"], lambda d, m, t, a, w, n: d[:, 1] == A) >= 100
    assert count(["b"], lambda d, m, t, a, w, n: d[:, 1] >= 0) >= 100
    # the window shows Walls, cells off the grid and cells nothing can reach
    assert count(sc.BANKS, lambda d, m, t, a, w, n: w == F) >= 100
    assert count(everywhere, lambda d, m, t, a, w, n: w == W_) >= 1000
    assert count(everywhere, lambda d, m, t, a, w, n: w == 0) >= 100


# ---- hand-built states --------------------------------------------------------
def run_hand(games, bank):
    from optimax_rogue_amd import DungeonBank, EnvConfig
    from optimax_rogue_amd.path import threat
    K = len(games[0]["npcs"])
    if bank:
        layouts = tc.hand_layout()[None]
        cfg, bank = EnvConfig(width=7, height=7, n_npcs=K, layouts=layouts), DungeonBank(layouts)
    else:
        cfg, bank = EnvConfig(width=8, height=8, n_npcs=K), None
    return threat(tc.hand_snap(games, bank is not None), cfg, 0, 3, bank=bank)


def assert_rows(got, want):
    for b, row in enumerate(want):
        for g, w, what in zip(got, row, ("dist", "move", "target", "after")):
            assert g[b].tolist() == w, (b, what, g[b].tolist(), w)


def test_hand_built_room():
    """The 8 x 8 room, player 1 the viewer.  Column 3 pads; after is [-, Up,
    Right, Down, Left, Stay, -, -]."""
    games = [
        # next to the staircase, the other player two cells to the left: Right
        # would be the staircase (no candidate), Up gains first
        dict(me=(3, 4), other=(1, 4), npcs=[None], stair=(4, 4)),
        # the threat stands on the staircase: an end cell, no detour
        dict(me=(4, 2), other=(4, 4), npcs=[None], stair=(4, 4)),
        # the staircase strictly between the two in one column: two moves round it
        dict(me=(4, 2), other=(4, 6), npcs=[None], stair=(4, 4)),
        # a corner: both open moves lose, Stay
        dict(me=(1, 1), other=(6, 6), npcs=[None], stair=(6, 1)),
        # nothing hunts: the other player is a depth away, the NPC dead
        dict(me=(3, 3), other=None, npcs=[None], stair=(6, 1)),
        # the other player and the NPC both two away: the player wins the tie
        dict(me=(3, 3), other=(3, 5), npcs=[(5, 3)], stair=(6, 1)),
    ]
    want = [
        ([2, A, 2, A], [UP, STAY, UP, STAY], [1, -1, 2, -1], [A, 3, A, 3, 1, 2, A, A]),
        ([2, A, 2, A], [UP, STAY, UP, STAY], [1, -1, 2, -1], [A, 3, 3, 1, 3, 2, A, A]),
        ([6, A, 6, A], [UP, STAY, UP, STAY], [1, -1, 2, -1], [A, 7, 5, 5, 5, 6, A, A]),
        ([10, A, 10, A], [STAY] * 4, [1, -1, 2, -1], [A, A, 9, 9, A, 10, A, A]),
        ([A] * 4, [STAY] * 4, [-1] * 4, [A] * 8),
        ([2, 2, 2, A], [UP, UP, UP, STAY], [1, 0, 2, -1], [A, 3, 1, 1, 3, 2, A, A]),
    ]
    got = run_hand(games, bank=False)
    assert_rows(got, want)
    # no threat: the window is the room's Walls and "nothing can come"
    window = got[4][4].astype(np.int64)                  # cells (0..6, 0..6), rows y
    assert (window[0] == W_).all() and (window[:, 0] == W_).all() and (window[1:, 1:] == F).all()
    # game 0's row y = 4: the other player at x = 1, the staircase an end cell
    # at x = 4 and two moves of detour behind it
    assert got[4][0][3].tolist() == [W_, 0, 1, 2, 3, 6, 7]


def test_hand_built_bank():
    """The 7 x 7 layout of threat_cases.HAND_ROWS, two NPC slots."""
    games = [
        # the dead end (1, 1), the threat three moves up the corridor: the one
        # open move loses, greedy stays put
        dict(me=(1, 1), other=(3, 2), npcs=[None, None]),
        # the fork (3, 3), NPC 1 two cells up: Down and Left both gain, Down is first
        dict(me=(3, 3), other=None, npcs=[None, (3, 1)]),
        # the other player behind the Wall and the staircase: unreachable, its
        # column stays put on a tie of unreachables; NPC 0 four moves away
        dict(me=(3, 3), other=(5, 2), npcs=[(1, 5), None]),
        # the threat on the staircase, the viewer below it: Up is no candidate
        dict(me=(5, 4), other=(5, 3), npcs=[None, None]),
        # next to the staircase, the one place that would gain: Stay
        dict(me=(5, 4), other=None, npcs=[(3, 5), None]),
        # NPC 0 one move to the left, NPC 1 two to the right: a step right ties, Stay
        dict(me=(2, 5), other=None, npcs=[(1, 5), (4, 5)]),
    ]
    want = [
        ([3, A, 3, A], [STAY] * 4, [1, -1, 2, -1], [A, A, 2, A, A, 3, A, A]),
        ([A, 2, 2, A], [STAY, DOWN, DOWN, STAY], [-1, 1, 4, -1], [A, 1, A, 3, 3, 2, A, A]),
        ([-1, 4, 4, A], [STAY, UP, UP, STAY], [1, 0, 3, -1], [A, 5, A, 3, 3, 4, A, A]),
        ([1, A, 1, A], [DOWN, STAY, DOWN, STAY], [1, -1, 2, -1], [A, A, A, 2, A, 1, A, A]),
        ([A, 3, 3, A], [STAY] * 4, [-1, 0, 3, -1], [A, A, A, 2, A, 3, A, A]),
        ([A, 1, 1, A], [STAY] * 4, [-1, 0, 3, -1], [A, A, 1, A, 0, 1, A, A]),
    ]
    got = run_hand(games, bank=True)
    assert_rows(got, want)
    # game 3, radius 3 around (5, 4): column x = 5 is cut by the staircase the
    # threat stands on -- it reaches (5, 2) and (5, 1) from there
    column = got[4][3][:, 3].tolist()                    # x = 5, y = 1 .. 7
    assert column == [2, 1, 0, 1, 2, W_, W_]
    # game 4: NPC 0 at (3, 5) cannot cross the staircase: (5, 2), (5, 1) unreachable
    assert got[4][4][:, 3].tolist() == [F, F, 4, 3, 2, W_, W_]


# ---- header and library -------------------------------------------------------
def test_header_constants_are_the_modules():
    from optimax_rogue_amd import _lib, path
    with open(os.path.join(ROOT, "include", "orx_path.h")) as f:
        text = f.read()
    defs = dict(re.findall(r"#define\s+(ORX_THREAT_\w+)\s+\(?(-?\d+)\)?", text))
    assert {k: int(v) for k, v in defs.items()} == {
        "ORX_THREAT_PLAYER": path.THREAT_PLAYER, "ORX_THREAT_NPC": path.THREAT_NPC,
        "ORX_THREAT_ANY": path.THREAT_ANY, "ORX_THREAT_AFTER_COLS": path.THREAT_AFTER_COLS}
    assert (path.THREAT_PLAYER, path.THREAT_NPC, path.THREAT_ANY) == (0, 1, 2)
    assert (path.THREAT_PLAYER, path.THREAT_NPC) == (path.SEEK_PLAYER, path.SEEK_NPC)
    assert "orx_path_threat" in _lib.PATH_EXPORTS
    assert re.search(r"^int\s+orx_path_threat\s*\(", text, re.M)
    with open(os.path.join(ROOT, "include", "orx.h")) as f:
        orx_h = f.read()
    assert "orx_path" not in orx_h and "ORX_THREAT" not in orx_h
    assert "#define ORX_ABI_VERSION 7" in orx_h and _lib.ABI_VERSION == 7
    assert np.array_equal(path.flee_moves(np.arange(12).reshape(3, 4)), [2, 6, 10])


def test_threat_symbol(engine_lib):
    from optimax_rogue_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert "orx_path_threat" in set(re.findall(r" T (orx_\w+)", out))
    assert hasattr(engine_lib, "orx_path_threat")


def test_threat_header_in_a_plain_c_consumer(engine_lib, tmp_path):
    """include/orx_path.h's new declaration compiles as C99 and every refusal
    of the entry point comes back from the host, before any launch (no GPU
    calls)."""
    exe = tmp_path / "threat_abi_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "threat_abi_check.c"), "-o", str(exe),
                    "-L", os.path.join(ROOT, "optimax_rogue_amd"), "-lorx",
                    "-Wl,-rpath," + os.path.join(ROOT, "optimax_rogue_amd")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orx_path_threat refusals: 27 of 27" in r.stdout
