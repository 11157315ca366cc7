"""CPU: the host statement of orx_path_ticks (optimax_rogue_amd.path.ticks)
against an independent one -- a per-game heapq Dijkstra written from
include/orx_path.h's sentences (ticks_cases.expected_ticks) -- on the oracle's
states; against the game itself, played out on the oracle; its properties
beside ``path.query``; hand-built states, one per sentence of the definition;
and the header from a plain-C consumer.  Integers compared exactly; nothing
here needs a GPU.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import ticks_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = tc.cases()


@pytest.fixture(scope="module")
def states(oracle_lib):
    """case -> (oracle, snapshot) after the warm-up."""
    out = {}
    for name, case in CASES.items():
        ora = tc.oracle_after_warmup(case)
        out[name] = (ora, ora.export())
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_ticks_matches_the_restatement(states, name):
    """ticks, move and every window cell at radii 1, 5 and 15 (the restatement's
    window at 15, cropped: the geometry is the definition's)."""
    from optimax_rogue_amd.path import ticks
    case = CASES[name]
    cfg, p = case["cfg"], case["player"]
    bank, snap = tc.bank_of(cfg), states[name][1]
    R = max(tc.RADII)
    want = [tc.expected_ticks(cfg, snap, p, b, R) for b in range(tc.N_GAMES)]
    w_ticks, w_move = (np.array([w[k] for w in want]) for k in (0, 1))
    w_window = np.stack([w[2] for w in want])
    for radius in tc.RADII:
        got = ticks(snap, cfg, p, radius, bank=bank)
        assert [a.dtype for a in got] == [np.int32, np.int8, np.uint16]
        V = 2 * radius + 1
        assert got[0].shape == got[1].shape == (tc.N_GAMES,) and got[2].shape == (tc.N_GAMES, V, V)
        crop = w_window[:, R - radius:R + radius + 1, R - radius:R + radius + 1]
        for g, w, what in zip(got, (w_ticks, w_move, crop), ("ticks", "move", "window")):
            bad = np.argwhere(g != w)
            assert len(bad) == 0, (name, radius, what, bad[:5].tolist())
    rows = ticks(snap, cfg, p, bank=bank)
    assert len(rows) == 2 and np.array_equal(rows[0], w_ticks) and np.array_equal(rows[1], w_move)


@pytest.mark.parametrize("name", sorted(CASES))
def test_properties_beside_the_plain_distance(states, name):
    """ticks >= dist; both outputs equal ``path.query``'s where no NPC is alive;
    the window's centre is ticks; the neighbour of ``move`` has the value ticks
    - enter."""
    from optimax_rogue_amd.path import PATH_UNREACHABLE, query, ticks
    from optimax_rogue_amd.query import MOVE_DELTAS, npc_rows
    case = CASES[name]
    cfg, p = case["cfg"], case["player"]
    bank, snap = tc.bank_of(cfg), states[name][1]
    dist, plain = query(snap, cfg, p, bank=bank)
    got, move, window = ticks(snap, cfg, p, 2, bank=bank)
    assert ((got >= dist) | ((got == -1) & (dist >= 0))).all()
    assert (got[dist < 0] == -1).all()
    a = int(cfg.player_damage) - int(cfg.player_armor)
    assert a == 0 or not ((got == -1) & (dist >= 0)).any()
    shown = np.where(window[:, 2, 2] >= PATH_UNREACHABLE, -1, window[:, 2, 2].astype(np.int64))
    assert np.array_equal(shown, got)
    # the neighbour the move steps onto: its value is ticks - enter
    alive, nx, ny, hp = npc_rows(snap, int(cfg.n_npcs))
    on_depth = snap["p_depth"][p] == (int(cfg.p1_depth) if int(cfg.start_mode) == 2 else 0)
    for code, dx, dy in MOVE_DELTAS:
        sel = np.flatnonzero(move == code)
        x, y = snap["p_x"][p][sel] + dx, snap["p_y"][p][sel] + dy
        held = alive[:, sel] & on_depth[sel][None] & (nx[:, sel] == x[None]) & (ny[:, sel] == y[None])
        hits = np.where(held, -(-np.maximum(hp[:, sel], 1) // max(a, 1)), 1 << 20).min(axis=0)
        enter = 1 + np.where(held.any(axis=0), hits, 0)
        assert np.array_equal(window[sel, 2 + dy, 2 + dx].astype(np.int64), got[sel] - enter), code
    assert ((move == tc.STAY) == (got <= 0)).all()
    # no NPC alive: the plain distance and the plain move
    calm = dict(snap, npc_alive=np.zeros_like(snap["npc_alive"]))
    t0, m0 = ticks(calm, cfg, p, bank=bank)
    assert np.array_equal(t0, dist) and np.array_equal(m0, plain)


@pytest.mark.parametrize("name", tc.PLAYOUT)
def test_playing_the_move_descends_on_schedule(states, name):
    """Stay NPCs, player 2 a depth away: ``move`` for player 1 and Stay for
    player 2 on a copy of the oracle, re-asking each tick.  ticks drops by
    exactly one per tick, the depth changes exactly in the tick where it was 1,
    and every played game descends."""
    from optimax_rogue_amd.path import ticks
    case = CASES[name]
    cfg, bank = case["cfg"], tc.bank_of(case["cfg"])
    assert int(cfg.flags) == 0 and int(cfg.npc_policy) == 0
    twin = states[name][0].clone()

    def ask():
        snap = twin.export()
        t, m = ticks(snap, cfg, 0, bank=bank)
        return t, m, snap["p_depth"][0].copy(), snap["p_depth"][1].copy(), tc.attacks(cfg, snap, 0, m)

    def step(actions):
        twin.step(np.stack([actions, np.full_like(actions, tc.STAY)], axis=1))

    played, descended, stood = tc.play_out(ask, step)
    assert played >= 280 and descended == played, (played, descended)
    assert stood >= 40, stood       # (the games were not all walks round)


def test_oracle_states_cover_the_query(states):
    """Per configuration of the table, at least half of the counts it was
    written with, over the games on the NPCs' depth in the oracle's first
    state: ticks above the plain distance, a first move that differs from the
    plain one (counted where there is a way down: with a == 0 the games without
    one would all count, their move being Stay), a first move that is an
    attack, and, where the NPCs cannot be hurt, no way down where the tiles
    alone have one.  The recount with ``path.ticks`` gave the table's numbers
    exactly."""
    from optimax_rogue_amd.path import query, ticks
    for name in tc.TABLE:
        case = CASES[name]
        cfg, bank, snap = case["cfg"], tc.bank_of(case["cfg"]), states[name][1]
        dist, plain = query(snap, cfg, 0, bank=bank)
        got, move = ticks(snap, cfg, 0, bank=bank)
        on = snap["p_depth"][0] == int(cfg.p1_depth)
        have = (int(((got > dist) & on).sum()), int(((move != plain) & (got > 0) & on).sum()),
                int((tc.attacks(cfg, snap, 0, move) & on).sum()),
                int(((got < 0) & (dist >= 0) & on).sum()))
        assert all(2 * h >= w for h, w in zip(have, tc.COUNTS[name])), (name, have)
        if name.endswith("weak"):
            assert have[2] == 0 and have[3] > 0


# ---- hand-built states --------------------------------------------------------
@pytest.mark.parametrize("rows, damage", [(tc.HAND, 2), (tc.HAND_WEAK, 1)])
def test_hand_built_states(rows, damage):
    from optimax_rogue_amd.path import ticks
    games = [dict(me=me, npcs=npcs) for _, me, npcs, _, _ in rows]
    cfg = tc.hand_cfg(2, player_damage=damage)
    snap = tc.hand_snap(games, 2)
    got, move, window = ticks(snap, cfg, 0, 1, bank=tc.bank_of(cfg))
    for b, (what, _, _, want, mv) in enumerate(rows):
        assert (int(got[b]), int(move[b])) == (want, mv), (what, int(got[b]), int(move[b]))
        exp = tc.expected_ticks(cfg, snap, 0, b, 1)
        assert (exp[0], exp[1]) == (want, mv) and np.array_equal(exp[2], window[b]), what


def test_hand_built_window():
    """The NPC on the staircase tile: the tile still shows 0, the cell behind it
    the cost of stepping onto it, and Walls are Walls."""
    from optimax_rogue_amd.path import ticks
    cfg = tc.hand_cfg(2)
    snap = tc.hand_snap([dict(me=(7, 1), npcs=[(7, 1, 3, 1)])], 2)
    got, move, window = ticks(snap, cfg, 0, 1, bank=tc.bank_of(cfg))
    W_ = tc.WALL_V
    assert (int(got[0]), int(move[0])) == (0, tc.STAY)
    assert window[0].tolist() == [[W_, W_, W_], [4, 0, 4], [W_, W_, 5]]


# ---- header and library -------------------------------------------------------
def test_header_and_bindings():
    from optimax_rogue_amd import _lib
    with open(os.path.join(ROOT, "include", "orx_path.h")) as f:
        text = f.read()
    assert "orx_path_ticks" in _lib.PATH_EXPORTS
    assert re.search(r"^int\s+orx_path_ticks\s*\(", text, re.M)
    for word in ("EXACT", "UPPER BOUND", "ESTIMATE"):
        assert word in text
    with open(os.path.join(ROOT, "include", "orx.h")) as f:
        orx_h = f.read()
    assert "#define ORX_ABI_VERSION 7" in orx_h and _lib.ABI_VERSION == 7


def test_ticks_symbol(engine_lib):
    from optimax_rogue_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert "orx_path_ticks" in set(re.findall(r" T (orx_\w+)", out))
    assert hasattr(engine_lib, "orx_path_ticks")


def test_ticks_header_in_a_plain_c_consumer(engine_lib, tmp_path):
    """The declaration compiles as C99 and every refusal of the entry point
    comes back from the host, before any launch (no GPU calls)."""
    exe = tmp_path / "ticks_abi_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "ticks_abi_check.c"), "-o", str(exe),
                    "-L", os.path.join(ROOT, "optimax_rogue_amd"), "-lorx",
                    "-Wl,-rpath," + os.path.join(ROOT, "optimax_rogue_amd")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orx_path_ticks refusals: 28 of 28" in r.stdout
