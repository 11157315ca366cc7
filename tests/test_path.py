"""CPU: the staircase distance field's host statement (optimax_rogue_amd.path)
against independent ones -- scipy's Dijkstra on the grid graph, the closed form
against the search, and a walk that follows ``move``'s rule cell by cell --
plus DungeonBank's new methods, the header's constants, and the two entry
points' refusals from a plain-C consumer.  Integers compared exactly; nothing
here needs a GPU (the last two tests load the built library, no GPU calls).
"""
import os
import re

import numpy as np
import pytest

import path_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(pc.banks()))
def test_stair_field_is_dijkstras(name):
    layouts, got = pc.banks()[name], pc.truth(name)
    assert got.dtype == np.uint16 and got.shape == layouts.shape
    for li in range(len(layouts)):
        assert np.array_equal(got[li], pc.dijkstra_field(layouts[li])), (name, li)


@pytest.mark.parametrize("W,H,sx,sy", [(4, 4, 1, 1), (4, 4, 2, 1), (10, 8, 7, 5), (5, 9, 1, 7),
                                       (32, 32, 29, 29), (64, 7, 33, 3)])
def test_closed_form_is_the_field_of_the_empty_dungeon(W, H, sx, sy):
    from optimax_rogue_amd import EnvConfig
    from optimax_rogue_amd.path import closed_form, stair_field
    # EmptyDungeonGenerator.spawn_dungeon: Wall border, one staircase inside
    want = stair_field(pc.open_room(W, H, sx, sy))[0]
    got = closed_form(EnvConfig(width=W, height=H), sx, sy)
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    both = closed_form(EnvConfig(width=W, height=H), np.array([sx, 1]), np.array([sy, 1]))
    assert both.shape == (2, W, H) and np.array_equal(both[0], want)
    assert np.array_equal(both[1], stair_field(pc.open_room(W, H, 1, 1))[0])


def walk_all(field):
    """From every cell of a [W, H] field at once: apply ``move``'s rule until
    nobody moves; returns (steps taken, final x, final y)."""
    from optimax_rogue_amd.path import MOVE_DELTAS, PATH_WALL, move_toward
    W, H = field.shape
    pad = np.full((W + 2, H + 2), PATH_WALL, np.int64)
    pad[1:-1, 1:-1] = field
    x, y = [a.reshape(-1) for a in np.meshgrid(np.arange(W), np.arange(H), indexing="ij")]
    x, y = x.copy(), y.copy()
    steps = np.zeros(W * H, np.int64)
    delta = {code: (dx, dy) for code, dx, dy in MOVE_DELTAS}
    while True:
        m = move_toward(pad[x + 1, y + 1], pad[x + 1, y], pad[x + 2, y + 1], pad[x + 1, y + 2],
                        pad[x, y + 1])
        moving = m != 5
        if not moving.any():
            return steps, x, y
        for code, (dx, dy) in delta.items():
            sel = m == code
            x[sel] += dx
            y[sel] += dy
        steps += moving


@pytest.mark.parametrize("name", ["3x3", "3x4", "9x8", "17x5", "64x64"])
def test_following_move_reaches_a_staircase_in_d_steps(name):
    from optimax_rogue_amd.path import PATH_UNREACHABLE, PATH_WALL
    layouts, field = pc.banks()[name], pc.truth(name)
    for li in range(len(layouts)):
        f = field[li].astype(np.int64)
        steps, x, y = walk_all(field[li])
        start = f.reshape(-1)
        reach = start < PATH_UNREACHABLE
        assert np.array_equal(steps[reach], start[reach]), (name, li)
        assert (layouts[li][x[reach], y[reach]] == pc.STAIR).all(), (name, li)
        # an unreachable cell (and a Wall) stays where it is
        assert (steps[~reach] == 0).all(), (name, li)
        assert ((start == PATH_WALL) == (layouts[li].reshape(-1) == pc.WALL)).all()


def test_fixtures_show_what_they_claim():
    from optimax_rogue_amd import DungeonBank
    from optimax_rogue_amd.path import PATH_UNREACHABLE
    bank = DungeonBank(pc.banks()["64x64"])
    f = bank.stair_field()
    assert np.array_equal(f, pc.truth("64x64")) and bank.stair_field() is f   # cached
    finite = lambda a: a[a < PATH_UNREACHABLE]
    assert finite(f[1]).max() == 1952 and 1952 > 10 * (64 + 64)
    unreach = bank.unreachable_ground()
    assert unreach.tolist() == [0, 0, 9]
    assert (f[2][11:14, 11:14] == PATH_UNREACHABLE).all()
    assert (pc.banks()["64x64"][2] == pc.STAIR).sum() == 2
    b17 = DungeonBank(pc.banks()["17x5"])
    assert int(b17.unreachable_ground().sum()) == 83
    assert int((b17.layouts == pc.GROUND).sum()) == 242
    # the 256 x 256 layouts need the whole plane: both are 65,536 tiles
    assert pc.banks()["256x256"].shape == (2, 256, 256)
    assert finite(pc.truth("256x256")[1]).max() > 256 + 256


@pytest.mark.parametrize("args", [dict(width=9, height=8, n_layouts=16, seed=0, wall_p=0.3),
                                  dict(width=17, height=5, n_layouts=8, seed=0, wall_p=0.3,
                                       n_stairs=2),
                                  dict(width=64, height=64, n_layouts=4, seed=2, wall_p=0.3)])
def test_random_connected(args):
    from optimax_rogue_amd import DungeonBank
    from optimax_rogue_amd.path import PATH_UNREACHABLE
    plain = DungeonBank.random(**args)
    conn = DungeonBank.random(connected=True, **args)
    pockets = plain.stair_field() == PATH_UNREACHABLE
    assert pockets.any() and plain.unreachable_ground().sum() == pockets.sum()
    assert (conn.unreachable_ground() == 0).all()
    assert not (conn.stair_field() == PATH_UNREACHABLE).any()
    assert (conn.layouts[pockets] == pc.WALL).all() and (plain.layouts[pockets] == pc.GROUND).all()
    assert np.array_equal(conn.layouts[~pockets], plain.layouts[~pockets])
    # the reachable part keeps its distances
    assert np.array_equal(conn.stair_field()[~pockets], plain.stair_field()[~pockets])


def test_random_default_draws_what_it_drew():
    """``connected=False`` (the default) is the generator as it was: the draws
    restated here from numpy's RandomState, call for call."""
    from optimax_rogue_amd import DungeonBank
    for W, H, L, seed, wall_p, n_stairs in ((9, 8, 16, 0, 0.15, 1), (17, 5, 8, 0, 0.3, 2),
                                            (12, 20, 3, 7, 0.2, 3)):
        rs = np.random.RandomState(seed)
        want = []
        for _ in range(L):
            t = pc.room(W, H)
            inner = rs.rand(W, H) < wall_p
            inner[[0, -1], :] = False
            inner[:, [0, -1]] = False
            t[inner] = pc.WALL
            ground = np.argwhere(t == pc.GROUND)
            for j in rs.choice(len(ground), n_stairs, replace=False):
                t[tuple(ground[j])] = pc.STAIR
            want.append(t)
        got = DungeonBank.random(W, H, L, seed=seed, wall_p=wall_p, n_stairs=n_stairs)
        assert np.array_equal(got.layouts, np.stack(want))
        same = DungeonBank.random(W, H, L, seed=seed, wall_p=wall_p, n_stairs=n_stairs,
                                  connected=False)
        assert np.array_equal(same.layouts, got.layouts)


def test_query_on_a_hand_made_state():
    """``query`` on a state written out by hand: a bank layout with a pocket
    and the closed form, both players, the window's geometry."""
    from optimax_rogue_amd import EnvConfig
    from optimax_rogue_amd.path import PATH_UNREACHABLE, PATH_WALL, check_path_args, query
    t = pc.room(7, 6)
    t[3, 1:4] = pc.WALL          # a wall from the top, open at y = 4
    t[5, 4] = pc.STAIR
    t[4, 2] = pc.WALL
    t[5, 2] = pc.WALL            # seals (4, 1), (5, 1)
    cfg = EnvConfig(width=7, height=6, layouts=t[None])
    snap = dict(p_x=np.array([[1, 5, 5], [4, 2, 1]]), p_y=np.array([[1, 4, 1], [3, 4, 4]]),
                p_layout=np.zeros((2, 3), np.int16))
    dist, move = query(snap, cfg, 0)
    # (1, 1): down to y = 4 and right to x = 5 in any order left of the wall:
    # 3 + 4 moves; (2, 1) and (1, 2) are both one closer and Right comes before
    # Down; on the staircase: 0, Stay; in the pocket: -1, Stay
    assert dist.tolist() == [7, 0, -1] and move.tolist() == [2, 5, 5]
    assert dist.dtype == np.int32 and move.dtype == np.int8
    dist, move, win = query(snap, cfg, 1, radius=1)
    # (4, 3): Up is Wall, Right (5, 3) is one closer and comes before Down
    assert dist.tolist() == [2, 3, 4] and move.tolist() == [2, 2, 2]
    assert win.dtype == np.uint16 and win.shape == (3, 3, 3)
    assert win[0].tolist() == [[PATH_WALL, PATH_WALL, PATH_WALL], [PATH_WALL, 2, 1], [2, 1, 0]]
    assert win[2, :, 0].tolist() == [PATH_WALL] * 3 and win[2, 2].tolist() == [PATH_WALL] * 3
    far = query(dict(snap, p_x=np.array([[5], [5]]), p_y=np.array([[1], [1]]),
                     p_layout=np.zeros((2, 1), np.int16)), cfg, 0, radius=1)[2]
    assert far[0, 1].tolist() == [PATH_UNREACHABLE, PATH_UNREACHABLE, PATH_WALL]
    # the closed form: staircase (3, 2) for player 1, (1, 1) for player 2
    cfg0 = EnvConfig(width=6, height=5)
    snap0 = dict(p_x=np.array([[1], [4]]), p_y=np.array([[3], [3]]),
                 st_x=np.array([[3], [1]]), st_y=np.array([[2], [1]]))
    dist, move, win = query(snap0, cfg0, 0, radius=1)
    assert dist.tolist() == [3] and move.tolist() == [1]      # Up before Right
    assert win[0].tolist() == [[PATH_WALL, 2, 1], [PATH_WALL, 3, 2], [PATH_WALL] * 3]
    dist, move = query(snap0, cfg0, 1)
    assert dist.tolist() == [5] and move.tolist() == [1]
    for bad in (dict(player=2), dict(player=0, radius=0), dict(player=0, radius=16),
                dict(player=0, radius=1.5)):
        with pytest.raises(ValueError):
            check_path_args(**bad)
    with pytest.raises(ValueError):
        check_path_args(0, None, EnvConfig(width=40000, height=30000))


def test_header_constants_are_the_modules():
    from optimax_rogue_amd import _lib, path
    with open(os.path.join(ROOT, "include", "orx_path.h")) as f:
        text = f.read()
    defs = dict(re.findall(r"#define\s+(ORX_PATH_\w+)\s+(0x[0-9A-Fa-f]+)", text))
    assert int(defs["ORX_PATH_WALL"], 16) == path.PATH_WALL == 0xFFFF
    assert int(defs["ORX_PATH_UNREACHABLE"], 16) == path.PATH_UNREACHABLE == 0xFFFE
    decl = sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(orx_\w+)\s*\(", text, re.M)))
    assert decl == sorted(_lib.PATH_EXPORTS)
    # orx.h is what it was: the new entry points are not declared there
    with open(os.path.join(ROOT, "include", "orx.h")) as f:
        assert "orx_path" not in f.read()


def test_path_header_in_a_plain_c_consumer(engine_lib, tmp_path):
    """include/orx_path.h compiles as C99 and every refusal of the two entry
    points comes back from the host, before any launch (no GPU calls)."""
    import subprocess
    exe = tmp_path / "path_abi_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "path_abi_check.c"), "-o", str(exe),
                    "-L", os.path.join(ROOT, "optimax_rogue_amd"), "-lorx",
                    "-Wl,-rpath," + os.path.join(ROOT, "optimax_rogue_amd")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orx_path refusals: 17 of 17" in r.stdout
