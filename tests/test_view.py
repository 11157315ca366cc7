"""CPU: the egocentric map view's host reference (optimax_rogue_amd.view) and
its C-ABI surface.

``render_view`` is checked on ORACLE states against an independent
restatement in the reference's schema (view_cases.expected_window: the tiles
of the viewer's depth, then the entities of that depth on top, as
optimax_rogue_cmdspec/map.py:56-84 draws them), over every game, both
players, radii 1 / 5 / 15, with and without the health plane.  The coverage
test asserts that those states are not empty windows.  Items do not exist in
the reference's schema: they are checked against item_pos / item_mask on a
hand-built snapshot.  No GPU.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import view_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = vc.cases()


@pytest.fixture(scope="module")
def states(oracle_lib):
    """case -> (state after reset, state after the case's ticks), computed once."""
    return {name: vc.oracle_states(case) for name, case in CASES.items()}


def windows(states, name, player, radius):
    from optimax_rogue_amd.view import render_view
    case = CASES[name]
    return render_view(states[name][1], case["cfg"], player, radius, bank=vc.bank_of(case["cfg"]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_render_view_matches_the_reference_schema(states, name):
    from optimax_rogue_amd import compat
    from optimax_rogue_amd.view import render_view
    case = CASES[name]
    cfg, bank = case["cfg"], vc.bank_of(case["cfg"])
    snap = states[name][1]
    games = [compat.game_state(snap, i, cfg, None, bank=bank) for i in range(vc.N_GAMES)]
    for radius in case["radii"]:
        for player in (0, 1):
            cells = render_view(snap, cfg, player, radius, bank=bank)
            cells2, health = render_view(snap, cfg, player, radius, bank=bank, health=True)
            V = 2 * radius + 1
            assert cells.dtype == np.uint8 and cells.shape == (vc.N_GAMES, V, V)
            assert health.dtype == np.uint8 and health.shape == cells.shape
            assert np.array_equal(cells, cells2)
            for i, gs in enumerate(games):
                want_c, want_h = vc.expected_window(gs, player, radius)
                assert np.array_equal(cells[i], want_c), (name, radius, player, i)
                assert np.array_equal(health[i], want_h), (name, radius, player, i)
            assert not (cells & 0xC0).any()
            assert not health[(cells & 12) == 0].any()


def test_oracle_states_cover_the_view(states):
    """A test that passes on empty windows proves nothing: over the oracle
    states of view_cases, every kind of cell occurs."""
    from optimax_rogue_amd.enums import npc_alive_bits
    from optimax_rogue_amd.view import npc_depth
    npc = player = stairs = False
    sides = [False] * 4
    for name, case in CASES.items():
        for p in (0, 1):
            for R in case["radii"]:
                c = windows(states, name, p, R)
                npc |= bool((c & 8).any())
                player |= bool((c & 4).any())
                stairs |= bool(((c & 3) == 3).any())
                out = (c & 3) == 0
                for k, edge in enumerate((out[:, 0, R], out[:, -1, R], out[:, R, 0], out[:, R, -1])):
                    sides[k] |= bool(edge.any())   # above, below, left of, right of the viewer
    assert npc and player and stairs and all(sides)

    # a dead NPC (static NPCs, episode 0: it died where it was spawned) whose
    # last cell lies inside the viewer's window shows no NPC bit
    name, R = "a", 5
    first, last = states[name]
    cfg = CASES[name]["cfg"]
    alive = npc_alive_bits(last["npc_alive"], cfg.n_npcs)
    c = windows(states, name, 0, R)
    found = 0
    for k, g in zip(*np.nonzero(~alive)):
        if last["episode"][g] != 0 or last["p_depth"][0][g] != npc_depth(cfg):
            continue
        pos = int(first["npc_pos"][k][g])
        i = (pos & 0xFF) - int(last["p_x"][0][g]) + R
        j = (pos >> 8) - int(last["p_y"][0][g]) + R
        if 0 <= i < 2 * R + 1 and 0 <= j < 2 * R + 1:
            assert not c[g, j, i] & 8
            found += 1
    assert found

    # players on different depths: the other-player bit is clear everywhere
    last = states["b"][1]
    apart = last["p_depth"][0] != last["p_depth"][1]
    assert apart.any() and not apart.all()
    for p in (0, 1):
        c = windows(states, "b", p, 15)
        assert not (c[apart] & 4).any()
        assert (c[~apart] & 4).any()
    # ... and the NPCs (depth 1, with player 1 at the start) show only there
    on = last["p_depth"][1] == npc_depth(CASES["b"]["cfg"])
    assert not (windows(states, "b", 1, 15)[~on] & 8).any()

    # the bank: some window shows a second staircase and an interior wall
    c = windows(states, "c", 0, 15)
    assert (((c & 3) == 3).sum(axis=(1, 2)) >= 2).any()
    last, cfg = states["c"][1], CASES["c"]["cfg"]
    off = np.arange(31) - 15
    x = last["p_x"][0][:, None, None] + off[None, None, :]
    y = last["p_y"][0][:, None, None] + off[None, :, None]
    interior = (x > 0) & (x < cfg.width - 1) & (y > 0) & (y < cfg.height - 1)
    assert (((c & 3) == 2) & interior).any()
    # ... and Ground on the grid's edge (the open borders)
    assert (((c & 3) == 1) & ~interior).any()


def item_snapshot():
    """Four hand-built games on a 10 x 8 board, K = 4, ORX_EXT_RPG."""
    from optimax_rogue_amd import EnvConfig
    cfg = EnvConfig(width=10, height=8, n_npcs=4, flags=4 | 8 | 16 | 32)
    B, K = 4, 4
    z = lambda *s, dt=np.int32: np.zeros(s, dt)
    snap = {"p_x": z(2, B), "p_y": z(2, B), "p_depth": z(2, B), "p_health": z(2, B) + 10,
            "st_x": z(2, B) + 8, "st_y": z(2, B) + 6, "tick": z(B) + 1, "status": z(B) + 1,
            "episode": z(B), "npc_pos": z(K, B, dt=np.uint16), "npc_health": z(K, B, dt=np.int8),
            "npc_alive": z(B, dt=np.uint32), "item_pos": z(K, B, dt=np.uint16),
            "item_mask": z(2, B, dt=np.uint32), "p_rpg": z(6, 2, B)}
    snap["p_x"][:] = [[3, 3, 3, 3], [5, 4, 5, 5]]
    snap["p_y"][:] = [[3, 3, 3, 3], [3, 4, 3, 3]]
    snap["p_depth"][1][3] = 1                     # game 3: player 2 one level down
    # game 0: items 0 (damage) at (4, 3) and 2 (max health) at (2, 2); item 1's
    # position is set but it does not lie on the floor; NPC 3 alive at (4, 4)
    snap["item_pos"][0][0] = 4 | 3 << 8
    snap["item_pos"][1][0] = 3 | 4 << 8
    snap["item_pos"][2][0] = 2 | 2 << 8
    snap["item_mask"][0][0] = 0b0101
    snap["item_mask"][1][0] = 0b0110              # kinds: item 1 and 2 max health, 0 damage
    snap["npc_pos"][3][0] = 4 | 4 << 8
    snap["npc_health"][3][0] = 3
    snap["npc_alive"][0] = 0b1000
    # game 1: player 2 stands on item 1 (its item spots are full) at (4, 4)
    snap["item_pos"][1][1] = 4 | 4 << 8
    snap["item_mask"][0][1] = 0b0010
    snap["item_mask"][1][1] = 0b0010
    snap["p_health"][1][1] = 300                  # clamped to 255 in the health plane
    # game 2: an item out of the R = 1 window at (8, 6)
    snap["item_pos"][0][2] = 8 | 6 << 8
    snap["item_mask"][0][2] = 0b0001
    # game 3: an item at (5, 3), where player 2 would stand were it on depth 0
    snap["item_pos"][0][3] = 5 | 3 << 8
    snap["item_mask"][0][3] = 0b0001
    return cfg, snap


def test_render_view_items():
    from optimax_rogue_amd.view import (VIEW_ITEM, VIEW_ITEM_KIND, VIEW_NPC, VIEW_PLAYER,
                                        render_view)
    cfg, snap = item_snapshot()
    R = 2
    c, h = render_view(snap, cfg, 0, R, health=True)
    at = lambda g, x, y: (g, y - 3 + R, x - 3 + R)     # player 1 stands at (3, 3)
    ground = 1
    assert c[at(0, 4, 3)] == ground | VIEW_ITEM
    assert c[at(0, 2, 2)] == ground | VIEW_ITEM | VIEW_ITEM_KIND
    assert c[at(0, 3, 4)] == ground                    # item 1 is not on the floor
    assert c[at(0, 4, 4)] == ground | VIEW_NPC and h[at(0, 4, 4)] == 3
    assert c[at(0, 5, 3)] == ground | VIEW_PLAYER and h[at(0, 5, 3)] == 10
    assert h[at(0, 4, 3)] == 0 and h[at(0, 2, 2)] == 0  # zero under an item alone
    assert c[at(1, 4, 4)] == ground | VIEW_PLAYER | VIEW_ITEM | VIEW_ITEM_KIND
    assert h[at(1, 4, 4)] == 255
    assert not (c[2] & (VIEW_ITEM | VIEW_ITEM_KIND)).any()
    assert c[at(3, 5, 3)] == ground | VIEW_ITEM        # player 2 is on another depth
    assert int((c & VIEW_ITEM != 0).sum()) == 4
    # player 2 of game 3 is on depth 1: not the NPCs' depth, so no item shows
    c2 = render_view(snap, cfg, 1, R)
    assert not (c2[3] & (VIEW_ITEM | VIEW_NPC | VIEW_PLAYER)).any()
    # without ORX_EXT_ITEMS the item arrays are not state
    import dataclasses
    plain = dataclasses.replace(cfg, flags=0)
    assert not (render_view(snap, plain, 0, R) & (VIEW_ITEM | VIEW_ITEM_KIND)).any()


def test_decode_round_trips(states):
    from optimax_rogue_amd import view
    _, snap = item_snapshot()
    cfg, _ = item_snapshot()
    for cells in (windows(states, "c", 0, 5), windows(states, "b", 1, 15),
                  view.render_view(snap, cfg, 0, 3)):
        planes = view.decode(cells)
        assert planes["tile"].dtype == np.uint8
        for k, v in planes.items():
            assert v.shape == cells.shape and (k == "tile" or v.dtype == bool)
        assert np.array_equal(view.encode(planes), cells)
        one_hot = planes["outside"].astype(int) + planes["ground"] + planes["wall"] \
            + planes["staircase"]
        assert (one_hot == 1).all()
    every = np.arange(64, dtype=np.uint8)
    assert np.array_equal(view.encode(view.decode(every)), every)


def test_header_constants_match():
    from optimax_rogue_amd import view
    text = open(os.path.join(ROOT, "include", "orx_view.h")).read()
    val = lambda n: int(re.search(r"#define %s (\d+)" % n, text).group(1))
    assert (view.VIEW_MAX_RADIUS, view.VIEW_TILE_MASK, view.VIEW_OUTSIDE, view.VIEW_PLAYER,
            view.VIEW_NPC, view.VIEW_ITEM, view.VIEW_ITEM_KIND) == (
        val("ORX_VIEW_MAX_RADIUS"), val("ORX_VIEW_TILE_MASK"), val("ORX_VIEW_OUTSIDE"),
        val("ORX_VIEW_PLAYER"), val("ORX_VIEW_NPC"), val("ORX_VIEW_ITEM"),
        val("ORX_VIEW_ITEM_KIND"))
    assert (view.VIEW_PLAYER, view.VIEW_NPC, view.VIEW_ITEM, view.VIEW_ITEM_KIND) == (4, 8, 16, 32)


def test_render_view_refuses_bad_arguments(states):
    from optimax_rogue_amd.view import render_view
    snap, cfg = states["a"][1], CASES["a"]["cfg"]
    for player, radius in ((0, 0), (0, 16), (2, 5), (-1, 5), (0, 2.5)):
        with pytest.raises(ValueError):
            render_view(snap, cfg, player, radius)


def test_orx_view_refuses_bad_arguments_on_the_host(engine_lib):
    """Every refusal comes before any launch (this test has no GPU): the
    arguments, then the configuration, through fail() / orx_last_error."""
    from optimax_rogue_amd import EnvConfig
    from optimax_rogue_amd._lib import OrxState
    cfg = EnvConfig(width=10, height=8, n_npcs=4).to_c()
    st = OrxState()     # all NULL: a valid call would be refused for its state, too
    buf = ctypes.create_string_buffer(16)
    call = lambda c, player, radius, cells, n: engine_lib.orx_view(
        ctypes.byref(c), ctypes.byref(st), player, radius, cells, None, n, None)
    for args, word in (((cfg, 2, 5, buf, 1), b"player"), ((cfg, -1, 5, buf, 1), b"player"),
                       ((cfg, 0, 0, buf, 1), b"radius"), ((cfg, 0, 16, buf, 1), b"radius"),
                       ((cfg, 0, 5, None, 1), b"cells"), ((cfg, 0, 5, buf, 0), b"n_games"),
                       ((cfg, 0, 5, buf, -3), b"n_games"),
                       ((EnvConfig(width=3).to_c(), 0, 5, buf, 1), b"width"),
                       ((cfg, 0, 5, buf, 1), b"state pointer")):
        assert call(*args) == -22, args[1:]
        assert word in engine_lib.orx_last_error(), (word, engine_lib.orx_last_error())
    assert engine_lib.orx_view(None, ctypes.byref(st), 0, 5, buf, None, 1, None) == -22


def test_engine_view_checks_come_before_the_library():
    """BatchedEngine.view refuses radius 0 / 16, player 2 and a wrong ``out``
    before any launch (checked on an engine-shaped stand-in: no GPU here)."""
    import torch
    from optimax_rogue_amd.engine import BatchedEngine

    class Lib:
        def orx_view(self, *a):
            raise AssertionError("launched")

    eng = BatchedEngine.__new__(BatchedEngine)
    eng.lib, eng.B, eng.device = Lib(), 6, torch.device("cpu")
    good = torch.empty((6, 11, 11), dtype=torch.uint8)
    for kw in (dict(radius=0), dict(radius=16), dict(radius=5, player=2),
               dict(radius=5, out=torch.empty((6, 11, 12), dtype=torch.uint8)),
               dict(radius=5, out=torch.empty((5, 11, 11), dtype=torch.uint8)),
               dict(radius=5, out=torch.empty((6, 11, 11), dtype=torch.int8)),
               dict(radius=5, out=torch.empty((6, 11, 22), dtype=torch.uint8)[:, :, ::2]),
               dict(radius=5, out=np.zeros((6, 11, 11), np.uint8)),
               dict(radius=5, health=True, out=good),
               dict(radius=5, health=True, out=(good, good)),
               dict(radius=5, out=(good, good.clone()))):
        with pytest.raises(ValueError):
            eng.view(**kw)


def test_view_symbol_and_export_lists(engine_lib):
    """orx_view is exported by liborx.so and bound from a list of its own;
    _lib.EXPORTS still equals what orx.h declares (the engine's build id,
    which hashes the view's two files too: tests/test_parts.py)."""
    from optimax_rogue_amd import _lib, build
    assert _lib.VIEW_EXPORTS == ("orx_view",)
    assert hasattr(engine_lib, "orx_view")
    decl = lambda path: sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(orx_\w+)\s*\(",
                                              open(path).read(), re.M)))
    assert sorted(_lib.EXPORTS) == decl(os.path.join(ROOT, "include", "orx.h"))
    assert sorted(_lib.VIEW_EXPORTS) == decl(os.path.join(ROOT, "include", "orx_view.h"))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert "orx_view" in set(re.findall(r" T (orx_\w+)", out))
    assert re.search(r"#define ORX_ABI_VERSION 7\b", open(os.path.join(ROOT, "include",
                                                                      "orx.h")).read())
    assert os.path.basename(build.PLAN_HDR) == "orx_plan.h"
    assert os.path.basename(build.QUERY_HDR) == "orx_query.h"
    assert os.path.basename(build.VIEW_SRC) == "orx_view.hip"
    assert os.path.basename(build.VIEW_HDR) == "orx_view.h"


def test_view_header_in_a_plain_c_consumer(engine_lib, tmp_path):
    exe = tmp_path / "view_abi_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "view_abi_check.c"), "-o", str(exe),
                    "-L", os.path.join(ROOT, "optimax_rogue_amd"), "-lorx",
                    "-Wl,-rpath," + os.path.join(ROOT, "optimax_rogue_amd")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orx_view refused: -22" in r.stdout
    assert "sizeof(orx_cfg_t)=116" in r.stdout
