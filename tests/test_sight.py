"""CPU: line of sight (optimax_rogue_amd.sight, include/orx_sight.h) without a
GPU.

``sight.visible`` (vectorised, window coordinates, integer roundings) is
checked on ORACLE states against an independent restatement in the reference's
schema (sight_cases.expected_seen: per game and per grid cell, from
``world.get_at_depth(depth).tiles``, the roundings with exact rationals), over
every game, both players, radii 1 / 5 / 15, and over the query sweep's 96
draws on a capped sample of games.  The coverage tests assert, on the oracle's
states alone, that walls hide players and NPCs, that they leave others in
sight, and that the neighbour rule lights walls.  The two properties of the
rule -- symmetry among floor cells, and everything seen without a bank -- are
checked exhaustively on small boards; then the row packing, the header against
the export table and the library, the build id, and the host-side refusals
from a plain C consumer.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import query_sweep as qs
import sight_cases as sc
import view_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sc.cases()
SWEEP_GAMES = 12          # games per draw (the first ones) the restatement is run on
SWEEP = {}                # draw -> (tally, asymmetric games at radius 15)


@pytest.fixture(scope="module")
def states(oracle_lib):
    """case -> the oracle's state after the case's ticks, computed once."""
    return {name: vc.oracle_states(CASES[name])[1] for name in sc.CPU_CASES}


def views(states, name, player, radius):
    """(cells, vis) of one case, player and radius."""
    from optimax_rogue_amd import sight, view
    case = CASES[name]
    cells = view.render_view(states[name], case["cfg"], player, radius,
                             bank=vc.bank_of(case["cfg"]))
    return cells, sight.visible(states[name], case["cfg"], player, radius,
                                bank=vc.bank_of(case["cfg"]))


@pytest.mark.parametrize("name", sc.CPU_CASES)
def test_visible_matches_the_restatement(states, name):
    from optimax_rogue_amd import compat
    case = CASES[name]
    cfg, bank, snap = case["cfg"], vc.bank_of(case["cfg"]), states[name]
    games = [compat.game_state(snap, i, cfg, None, bank=bank) for i in range(sc.N_GAMES)]
    for radius in case["radii"]:
        V = 2 * radius + 1
        for player in (0, 1):
            cells, vis = views(states, name, player, radius)
            assert vis.dtype == bool and vis.shape == (sc.N_GAMES, V, V)
            for i, gs in enumerate(games):
                want = sc.expected_seen(gs, player, radius)
                assert np.array_equal(vis[i], want), (name, radius, player, i)
            assert vis[:, radius, radius].all()             # the viewer's own cell
            assert not vis[(cells & 3) == 0].any()          # nothing outside the grid


@pytest.mark.parametrize("name", ("c", "w", "wg"))
def test_oracle_states_cover_sight(states, name):
    """A test that passes where nothing is hidden proves nothing: at radius 5
    the oracle's states have the other player and NPCs both in sight and
    hidden, and walls lit by the neighbour rule alone."""
    total = sc.add_up(sc.tally(*views(states, name, p, 5)) for p in (0, 1))
    assert all(v > 0 for v in total.values()) and len(total) == 5, total


def room_snapshot(xs, ys, layout=None):
    """A snapshot()-shaped dict with player 1 of game b at (xs[b], ys[b])."""
    B = len(xs)
    z = lambda: np.zeros((2, B), np.int32)
    snap = {"p_x": z(), "p_y": z(), "p_depth": z(), "p_health": z() + 10, "st_x": z() + 1,
            "st_y": z() + 1}
    snap["p_x"][:], snap["p_y"][:] = xs, ys
    if layout is not None:
        snap["p_layout"] = np.zeros((2, B), np.int16) + layout
    return snap


@pytest.mark.parametrize("wall_p", (0.15, 0.3))
def test_sight_is_symmetric_among_floor_cells(wall_p):
    """(a) On random 12 x 10 layouts every pair of transparent cells: A sees B
    exactly when B sees A (radius 15 covers the board from every cell)."""
    from optimax_rogue_amd import DungeonBank, EnvConfig, sight
    bank = DungeonBank.random(12, 10, 6, seed=int(wall_p * 100), wall_p=wall_p)
    cfg = EnvConfig(width=12, height=10, n_npcs=0, layouts=bank.layouts)
    pairs = hidden = 0
    for lay in range(len(bank)):
        xs, ys = np.nonzero(bank.layouts[lay] != sc.WALL)
        vis = sight.visible(room_snapshot(xs, ys, lay), cfg, 0, 15, bank=bank)
        k = np.arange(len(xs))
        # sees[a, b]: from floor cell a, floor cell b
        sees = vis[k[:, None], ys[None, :] - ys[:, None] + 15, xs[None, :] - xs[:, None] + 15]
        assert np.array_equal(sees, sees.T), (wall_p, lay)
        assert sees.diagonal().all()
        pairs += sees.size
        hidden += int((~sees).sum())
    assert pairs > 10000 and hidden > 1000, (pairs, hidden)


@pytest.mark.parametrize("name", ("c", "w", "wg"))
def test_the_players_see_each_other_or_neither_does(states, name):
    snap = states[name]
    a, b = (sc.sees_other(snap, views(states, name, p, 15)[1], p, 15) for p in (0, 1))
    assert np.array_equal(a, b) and a.any() and not a.all()


@pytest.mark.parametrize("W,H", ((4, 4), (10, 8), (31, 17)))
def test_without_a_bank_the_whole_room_is_seen(W, H):
    """(b) EmptyDungeonGenerator's room from every interior cell: every cell
    of the window that lies in the grid is seen, the border walls included."""
    from optimax_rogue_amd import EnvConfig, sight, view
    cfg = EnvConfig(width=W, height=H, n_npcs=0)
    xs, ys = (a.ravel() for a in np.meshgrid(np.arange(1, W - 1), np.arange(1, H - 1)))
    snap = room_snapshot(xs, ys)
    for radius in (1, 5, 15):
        cells = view.render_view(snap, cfg, 0, radius)
        assert np.array_equal(sight.visible(snap, cfg, 0, radius), (cells & 3) != 0)


def test_rows_and_apply(states):
    from optimax_rogue_amd import sight, view
    case = CASES["w"]
    for radius in sc.RADII:
        V = 2 * radius + 1
        cells, hp = view.render_view(states["w"], case["cfg"], 0, radius,
                                     bank=vc.bank_of(case["cfg"]), health=True)
        vis = sight.visible_of(cells)
        rows = sight.pack_rows(vis)
        assert rows.dtype == np.uint32 and rows.shape == (sc.N_GAMES, V)
        assert not (rows >> np.uint32(V)).any()
        assert np.array_equal(sight.unpack_rows(rows, V), vis)
        masked, mhp = sight.apply(cells, vis, hp)
        assert masked.dtype == np.uint8 and mhp.dtype == np.uint8
        assert np.array_equal(masked, sight.apply(cells, vis))
        assert ((masked == 0) | (masked & sight.SIGHT_SEEN != 0)).all()
        assert np.array_equal(masked != 0, vis) and np.array_equal(masked[vis] & 63, cells[vis])
        assert not mhp[~vis].any() and np.array_equal(mhp[vis], hp[vis])
        again, hp2 = sight.apply(masked, vis, mhp)           # idempotent
        assert np.array_equal(again, masked) and np.array_equal(hp2, mhp)
    every = np.zeros((1, 3, 3), bool)
    every[0, 1, :] = True
    assert sight.pack_rows(every).tolist() == [[0, 7, 0]]


# ---- the sweep ----------------------------------------------------------------
def sweep_case(case):
    """One draw: the reference against the restatement on the first
    SWEEP_GAMES games of the oracle's state at the draw's own batch, with the
    draw's radii; returns (tally over all games, asymmetric games at R = 15)."""
    from optimax_rogue_amd import compat, sight, view
    d = qs.draw(case)
    cfg, bank = qs.env_config(d), qs.bank_of(d)
    snap = qs.rolled_oracle(d).export()
    n = min(d.B, SWEEP_GAMES)
    games = [compat.game_state(snap, i, cfg, None, bank=bank) for i in range(n)]
    tallies = []
    for p in (0, 1):
        R = d.radius[p]
        cells = view.render_view(snap, cfg, p, R, bank=bank)
        vis = sight.visible_of(cells)
        for i, gs in enumerate(games):
            assert np.array_equal(vis[i], sc.expected_seen(gs, p, R)), (qs.where(d), p, i)
        tallies.append(sc.tally(cells, vis))
    a, b = (sc.sees_other(snap, sight.visible(snap, cfg, p, 15, bank=bank), p, 15) for p in (0, 1))
    total = sc.add_up(tallies)
    total["banks"] = int(d.layouts is not None)
    return total, int((a != b).sum())


@pytest.mark.parametrize("case", range(qs.N_CASES))
def test_sweep_visible_matches_the_restatement(oracle_lib, case):
    SWEEP[case] = sweep_case(case)


def test_sweep_coverage(oracle_lib):
    """Conditions on the oracle's states alone, summed over the sweep."""
    if qs.N_CASES < 96:
        pytest.skip("the coverage conditions are those of the whole sweep")
    for case in range(qs.N_CASES):
        if case not in SWEEP:
            SWEEP[case] = sweep_case(case)
    total = sc.add_up(t for t, _ in SWEEP.values())
    print("sight sweep coverage:", total)
    assert total["banks"] >= 10, total
    for k in ("player_seen", "player_unseen", "npc_seen", "npc_unseen"):
        assert total[k] > 0, total
    assert sum(n for _, n in SWEEP.values()) == 0


# ---- header, exports, build id, refusals -----------------------------------------
def test_header_is_the_export_table():
    from optimax_rogue_amd import _lib, sight
    with open(os.path.join(ROOT, "include", "orx_sight.h")) as f:
        text = f.read()
    assert int(re.search(r"#define ORX_SIGHT_SEEN (\d+)", text).group(1)) == sight.SIGHT_SEEN == 64
    decl = sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(orx_\w+)\s*\(", text, re.M)))
    assert decl == sorted(_lib.SIGHT_EXPORTS) == ["orx_sight", "orx_sight_build_id"]
    for hdr in ("orx.h", "orx_view.h"):
        with open(os.path.join(ROOT, "include", hdr)) as f:
            assert "orx_sight" not in f.read()
    assert _lib.ABI_VERSION == 7


def test_sight_header_in_a_plain_c_consumer(engine_lib, tmp_path):
    """include/orx_sight.h compiles as C99 and every refusal of orx_sight comes
    back from the host, before any launch (no GPU calls)."""
    exe = tmp_path / "sight_abi_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "sight_abi_check.c"), "-o", str(exe),
                    "-L", os.path.join(ROOT, "optimax_rogue_amd"), "-lorx",
                    "-Wl,-rpath," + os.path.join(ROOT, "optimax_rogue_amd")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orx_sight refusals: 17 of 17" in r.stdout


def test_engine_sight_checks_come_before_the_library():
    """BatchedEngine.sight / seen_view refuse a bad radius, player or ``out``
    before any launch (an engine-shaped stand-in: no GPU here)."""
    import torch
    from optimax_rogue_amd.engine import BatchedEngine

    class Lib:
        def orx_view(self, *a):
            raise AssertionError("launched")
        orx_sight = orx_view

    eng = BatchedEngine.__new__(BatchedEngine)
    eng.lib, eng.B, eng.device = Lib(), 6, torch.device("cpu")
    good = torch.empty((6, 11, 11), dtype=torch.uint8)
    for kw in (dict(radius=0), dict(radius=16), dict(radius=5, player=2),
               dict(radius=5, out=torch.empty((6, 11), dtype=torch.int32)),
               dict(radius=5, out=torch.empty((6, 12), dtype=torch.uint32)),
               dict(radius=5, out=torch.empty((5, 11), dtype=torch.uint32)),
               dict(radius=5, out=(torch.empty((6, 11), dtype=torch.uint32),) * 2)):
        with pytest.raises(ValueError):
            eng.sight(**kw)
    for kw in (dict(radius=0), dict(radius=16), dict(radius=5, player=-1),
               dict(radius=5, out=torch.empty((6, 11, 12), dtype=torch.uint8)),
               dict(radius=5, health=True, out=good),
               dict(radius=5, health=True, out=(good, good))):
        with pytest.raises(ValueError):
            eng.seen_view(**kw)
    for radius, player in ((0, 0), (16, 1), (5, 2)):
        with pytest.raises(ValueError):
            eng.sees_other(radius, player)
