"""GPU: orx_path_field and orx_path_query (BatchedEngine.path / VecEnv.path /
VecEnv.stair_moves) against the host statement in optimax_rogue_amd.path --
``stair_field`` for the field, ``query(eng.snapshot(), ...)`` for the query --
with exact equality over every layout, tile, game and window cell.

The banks are path_cases' (3 x 3 up to the 256 x 256 plane that fills the
LDS limit, a serpentine that needs 1,953 relaxation levels, 300 layouts for
the grid-stride); the engine states are view_cases' five configurations at the
start and after their ticks.  Batch sizes 1, 63, 65 and 200: a lone game, a
partial wave, a wave plus one game, and several workgroups whose last one is
partial, with an odd number of uint16 cells for the stream-out's tail (at
radius 15 a workgroup takes 16 games, at radius 1 and 5 it takes 64).
"""
import ctypes

import numpy as np
import pytest

import path_cases as pc
import view_cases as vc

pytestmark = pytest.mark.gpu

CASES = vc.cases()
BATCHES = (1, 63, 65, 200)
RADII = (None, 1, 5, 15)


def make_engine(case, n_games, **kw):
    from optimax_rogue_amd.engine import BatchedEngine
    return BatchedEngine(case["cfg"], n_games, seed=case["seed"], **kw)


def device_field(layouts):
    """orx_path_field on [L, W, H] layouts, through the C-ABI alone (no engine:
    the field takes banks smaller than any game configuration)."""
    import torch
    from optimax_rogue_amd import _lib
    from optimax_rogue_amd.config import OrxCfg
    lib = _lib.load()
    L, W, H = layouts.shape
    cfg = OrxCfg(width=W, height=H, n_layouts=L)
    tiles = torch.from_numpy(np.array(layouts).reshape(L, W * H)).cuda()
    field = torch.full((L, W, H), 0x7777, dtype=torch.int16, device="cuda")
    _lib.check("orx_path_field",
               lib.orx_path_field(ctypes.byref(cfg), ctypes.c_void_p(tiles.data_ptr()),
                                  ctypes.c_void_p(field.data_ptr()),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return field.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("name", sorted(pc.banks()))
def test_field_matches_stair_field(name):
    got = device_field(pc.banks()[name])
    want = pc.truth(name)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (name, len(bad), bad[:5].tolist())


def test_field_of_unaligned_layout_slices():
    """17 x 5 layouts are 170 bytes each: every second slice of the field
    starts off a 16-byte boundary (the uint16 head and tail of the stream-out);
    an engine's ``stair_field`` is the same tensor as the bank's host field."""
    import torch
    from optimax_rogue_amd import DungeonBank, EnvConfig
    from optimax_rogue_amd.engine import BatchedEngine
    bank = DungeonBank(np.array(pc.banks()["17x5"]))
    eng = BatchedEngine(EnvConfig(width=17, height=5, n_npcs=0, layouts=bank.layouts), 8, seed=1)
    f = eng.stair_field
    assert f.dtype == torch.uint16 and tuple(f.shape) == (8, 17, 5)
    assert np.array_equal(f.cpu().numpy(), bank.stair_field())
    assert eng.stair_field is f                                  # computed once
    assert make_engine(CASES["a"], 4).stair_field is None        # no bank, no field


def same(x, y):
    """torch.equal, with uint16 compared through its int16 bits."""
    import torch
    if x.dtype == torch.uint16:
        x, y = x.view(torch.int16), y.view(torch.int16)
    return torch.equal(x, y)


def check_paths(eng, case, radii=RADII):
    """Every radius and player of one engine state; returns the set of moves
    seen."""
    import torch
    from optimax_rogue_amd.path import query
    snap = eng.snapshot()
    seen = set()
    for radius in radii:
        for player in (0, 1):
            want = query(snap, case["cfg"], player, radius, bank=eng.bank)
            got = eng.path(player=player, radius=radius)
            assert len(got) == len(want) == (2 if radius is None else 3)
            assert got[0].dtype == torch.int32 and got[1].dtype == torch.int8
            assert tuple(got[0].shape) == tuple(got[1].shape) == (eng.B,)
            if radius is not None:
                V = 2 * radius + 1
                assert got[2].dtype == torch.uint16 and tuple(got[2].shape) == (eng.B, V, V)
                assert got[2].is_contiguous()
            for g, w, what in zip(got, want, ("dist", "move", "window")):
                assert np.array_equal(g.cpu().numpy(), w), (what, radius, player)
            seen |= set(want[1].tolist())
    return seen


@pytest.mark.parametrize("n_games", BATCHES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_path_matches_query(name, n_games):
    case = CASES[name]
    eng = make_engine(case, n_games)
    seen = check_paths(eng, case)                     # the start state
    vc.drive_engine(eng, case)
    seen |= check_paths(eng, case)
    if n_games == vc.N_GAMES and name != "e":
        # every direction was asked for (e: a 4 x 4 board's staircase is always
        # at (1, 1), so only Up and Left lead to it)
        assert {1, 2, 3, 4} <= seen


def test_walk_on_the_device():
    """step(stair_moves()) on a bank with pockets: every tick every game gets
    exactly one step closer, or descends from distance 1, or -- unreachable --
    stays where it is.  (Seed 5: on the C oracle's start states 26 of the 200
    games start in a pocket and the longest way down is 12 moves.)"""
    import torch
    from optimax_rogue_amd import Policy, VecEnv
    env = VecEnv(pc.walk_cfg(), 200, seed=5, opponent=Policy.Stay, check_actions=False)
    eng = env.engine
    assert int(eng.bank.unreachable_ground().sum()) > 0
    dist, move = env.path()
    started_unreachable = dist == -1
    descended = torch.zeros_like(started_unreachable)
    for tick in range(40):
        depth, x, y = eng.p_depth[0].clone(), eng.p_x[0].clone(), eng.p_y[0].clone()
        assert torch.equal(move, env.stair_moves())
        assert int((dist == 0).sum()) == 0             # nobody rests on a staircase
        obs, reward, done, status = env.step(move)
        assert not bool(done.any())
        ndist, nmove = env.path()
        same_depth = eng.p_depth[0] == depth
        closer = same_depth & (ndist == dist - 1)
        down = (dist == 1) & (eng.p_depth[0] == depth + 1)
        stuck = (dist == -1) & same_depth & (eng.p_x[0] == x) & (eng.p_y[0] == y)
        kinds = closer.int() + down.int() + stuck.int()
        assert bool((kinds == 1).all()), (tick, torch.nonzero(kinds != 1).flatten().tolist()[:5])
        assert torch.equal(move == 5, dist == -1)       # Stay only where nothing can be reached
        descended |= down
        dist, move = ndist, nmove
    assert bool(started_unreachable.any()) and bool(descended.any())
    # a game that started in a pocket is still there; the others all got down
    assert bool((dist[started_unreachable] == -1).all())
    assert not bool(descended[started_unreachable].any())
    # player 2, far below, never moved under Policy.Stay and has a path of its own
    d2, m2 = env.path(player=1)
    assert tuple(d2.shape) == (200,) and bool(((d2 >= -1) & (m2 >= 1) & (m2 <= 5)).all())


def test_path_out_reuse_and_refusals():
    import torch
    from optimax_rogue_amd import _lib
    case = CASES["c"]
    eng = make_engine(case, 65)
    vc.drive_engine(eng, case)
    dev = eng.device
    want = eng.path(radius=5)
    fresh = lambda: (torch.full((65,), -7, dtype=torch.int32, device=dev),
                     torch.full((65,), -7, dtype=torch.int8, device=dev),
                     torch.full((65, 11, 11), 7, dtype=torch.int16, device=dev).view(torch.uint16))
    out = fresh()
    got = eng.path(radius=5, out=out)
    assert all(g is o for g, o in zip(got, out))
    assert all(same(g, w) for g, w in zip(got, want))
    two = fresh()[:2]
    got = eng.path(out=two)
    assert got[0] is two[0] and got[1] is two[1]
    assert torch.equal(two[0], want[0]) and torch.equal(two[1], want[1])
    # every bad argument is refused on the host, before any launch
    d, m, w = fresh()
    for kw in (dict(player=2), dict(player=-1), dict(radius=0), dict(radius=16),
               dict(radius=2.0), dict(out=(d, m, w)), dict(radius=5, out=(d, m)),
               dict(radius=5, out=(d, m, w[:, :, :10])),
               dict(radius=5, out=(d, m, torch.empty((65, 11, 11), dtype=torch.int16, device=dev))),
               dict(radius=5, out=(d, m, torch.empty((65, 11, 11), dtype=torch.uint16))),
               dict(out=(d[:64], m)), dict(out=(d.to(torch.int64), m)), dict(out=(d, m.cpu())),
               dict(out=(m, d)), dict(out=d)):
        with pytest.raises(ValueError):
            eng.path(**kw)
    # the C codes: ORX_EINVAL from the host side of each entry point
    lib, vp = eng.lib, ctypes.c_void_p
    p = lambda t: vp(t.data_ptr())
    field, st = p(eng.stair_field), eng._stream()
    q = lambda *a: lib.orx_path_query(eng._pcfg, eng._pst, *a)
    assert q(field, 2, 5, p(d), p(m), p(w), 65, st) == -22
    assert b"player" in lib.orx_last_error()
    assert q(field, 0, 0, p(d), p(m), p(w), 65, st) == -22
    assert q(field, 0, 16, p(d), p(m), p(w), 65, st) == -22
    assert q(field, 0, 5, None, None, None, 65, st) == -22
    assert q(field, 0, 5, p(d), p(m), None, 0, st) == -22
    assert q(None, 0, 5, p(d), p(m), None, 65, st) == -22
    assert b"field" in lib.orx_last_error()
    assert lib.orx_path_query(eng._pcfg, None, field, 0, 5, p(d), p(m), None, 65, st) == -22
    assert lib.orx_path_field(eng._pcfg, None, field, st) == -22
    assert lib.orx_path_field(eng._pcfg, p(eng.bank_tiles), None, st) == -22
    nobank = make_engine(CASES["a"], 4)
    assert lib.orx_path_field(nobank._pcfg, p(eng.bank_tiles), field, st) == -22
    with pytest.raises(_lib.OrxError):
        eng._call("orx_path_query", field, 3, 0, p(d), p(m), None, 65, st)
    # radius is ignored without a window
    assert q(field, 0, 99, p(d), p(m), None, 65, st) == 0
    assert torch.equal(d, want[0]) and torch.equal(m, want[1])


def test_path_leaves_the_state_untouched():
    case = CASES["c"]
    eng = make_engine(case, 63)
    vc.drive_engine(eng, case)
    before = eng.snapshot()
    actions, tiles = eng.actions.clone(), eng.bank_tiles.clone()
    for radius in RADII:
        for player in (0, 1):
            eng.path(player=player, radius=radius)
    after = eng.snapshot()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert bool((eng.actions == actions).all()) and bool((eng.bank_tiles == tiles).all())
    # no random words either: the next ticks equal an engine's that never asked
    twin = make_engine(case, 63)
    vc.drive_engine(twin, case)
    for e in (eng, twin):
        e.step(e.policy(1, 1))
    a, b = eng.snapshot(), twin.snapshot()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_path_on_a_side_stream():
    import torch
    from optimax_rogue_amd.path import query
    case = CASES["c"]
    eng = make_engine(case, 200)
    vc.drive_engine(eng, case)
    want = query(eng.snapshot(), case["cfg"], 1, 5, bank=eng.bank)
    s = torch.cuda.Stream(device=eng.device)
    s.wait_stream(torch.cuda.current_stream(eng.device))
    with torch.cuda.stream(s):
        got = eng.path(player=1, radius=5)      # (the field is computed on this stream too)
        done = torch.cuda.Event()
        done.record(s)
    done.synchronize()
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)


def test_step_then_path_in_one_graph():
    """env.step(a) followed by env.path(radius=5) captured in one graph (a
    linear chain on the capture stream): three replays against an eager twin."""
    import torch
    from optimax_rogue_amd import VecEnv
    case = CASES["a"]
    B = 200
    mk = lambda: VecEnv(case["cfg"], B, seed=case["seed"], opponent=1, check_actions=False,
                        out_buffers=1)
    env, twin = mk(), mk()
    dev = env.device
    gen = torch.Generator().manual_seed(5)
    moves = torch.randint(1, 6, (5, B), generator=gen, dtype=torch.int64).to(dev)
    a = moves[0].clone()
    for e in (env, twin):          # (the first step settles the host-side launch blocks)
        e.step(a)
    out = (torch.zeros(B, dtype=torch.int32, device=dev),
           torch.zeros(B, dtype=torch.int8, device=dev),
           torch.zeros((B, 11, 11), dtype=torch.int16, device=dev).view(torch.uint16))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            obs, reward, done, status = env.step(a)
            env.path(radius=5, out=out)
    torch.cuda.current_stream(dev).wait_stream(s)
    for k in range(1, 4):
        a.copy_(moves[k])
        g.replay()
        t_obs, t_reward, t_done, t_status = twin.step(moves[k])
        t_out = twin.path(radius=5)
        torch.cuda.synchronize(dev)
        assert torch.equal(obs, t_obs) and torch.equal(status, t_status), k
        assert torch.equal(reward, t_reward) and torch.equal(done, t_done), k
        for x, y in zip(out, t_out):
            assert same(x, y), k
        assert int((out[0] > 0).sum()) > 0
