"""GPU: orx_path_rows and orx_path_seek (BatchedEngine.pair_field / seek,
VecEnv.seek / hunt_moves) against the host statement in optimax_rogue_amd.path
-- ``source_rows`` for the rows, ``seek(eng.snapshot(), ...)`` for the query --
with exact equality over every row, tile, game and column.

The banks are path_cases' (3 x 3 up to the 256 x 256 plane that fills the LDS
limit, 17 x 5 for rows that are not 16-byte aligned, 21,600 rows for the
grid-stride, a serpentine of 1,952 levels); the engine states are seek_cases'
configurations at the start and after their ticks, at batch sizes 1, 63, 65 and
200: a lone game, a partial wave, a wave plus one game, a workgroup's worth.
"""
import ctypes

import numpy as np
import pytest

import path_cases as pc
import seek_cases as sc

pytestmark = pytest.mark.gpu

CASES = sc.cases()
BATCHES = (1, 63, 65, 200)


def make_engine(case, n_games, **kw):
    from optimax_rogue_amd.engine import BatchedEngine
    return BatchedEngine(case["cfg"], n_games, seed=case["seed"], **kw)


def device_rows(layouts, layout, cell):
    """orx_path_rows on [L, W, H] layouts, through the C-ABI alone; the output
    is pre-filled with a pattern, so a cell the kernel left out shows."""
    import torch
    from optimax_rogue_amd import _lib
    from optimax_rogue_amd.config import OrxCfg
    lib = _lib.load()
    L, W, H = layouts.shape
    cfg = OrxCfg(width=W, height=H, n_layouts=L)
    tiles = torch.from_numpy(np.array(layouts).reshape(L, W * H)).cuda()
    lay = torch.tensor(np.asarray(layout), dtype=torch.int32, device="cuda")
    src = torch.tensor(np.asarray(cell), dtype=torch.int32, device="cuda")
    n = len(lay)
    rows = torch.full((n, W * H), 0x7777, dtype=torch.int16, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check("orx_path_rows",
               lib.orx_path_rows(ctypes.byref(cfg), p(tiles), p(lay), p(src), p(rows), n,
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return rows.cpu().numpy().view(np.uint16)


def assert_rows(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(),
                           [int(got[tuple(b)]) for b in bad[:5]])


@pytest.mark.parametrize("name", ["3x3", "3x4", "9x8", "17x5", "9x8x300"])
def test_rows_of_every_source(name):
    """Every (layout, source) of a bank in one launch: the pair table.  17 x 5
    rows are 170 bytes (the uint16 head and tail of the stream-out); 9x8x300
    is 21,600 rows, more than one launch's workgroups (the grid-stride)."""
    layouts = pc.banks()[name]
    L, W, H = layouts.shape
    lay, cell = np.divmod(np.arange(L * W * H), W * H)
    want = sc.pair_truth(name)
    got = device_rows(layouts, lay, cell)
    assert_rows(got, want.reshape(L * W * H, W * H), name)
    if name == "17x5":
        one = device_rows(layouts, [3], [42])                   # n = 1
        assert_rows(one, want[3, 42][None], "n = 1")


@pytest.mark.parametrize("li", [1, 2])
def test_rows_of_the_64x64_layouts(li):
    """The serpentine (1,952 levels) and the pocket layout of the 64 x 64 bank,
    every source: 4,096 rows of 8 KiB each."""
    from optimax_rogue_amd.path import source_rows
    layouts = pc.banks()["64x64"]
    cell = np.arange(64 * 64)
    lay = np.full(len(cell), li)
    assert_rows(device_rows(layouts, lay, cell), source_rows(layouts, lay, cell), li)


def test_rows_of_the_largest_plane():
    """256 x 256: the plane that needs the LDS limit raised.  A corner cell,
    the staircase, a Wall, cells behind the long walls, and a layout and a
    cell outside the bank."""
    from optimax_rogue_amd.path import source_rows
    layouts = pc.banks()["256x256"]
    c = lambda x, y: x * 256 + y
    lay = [1, 1, 1, 1, 1, 0, 2, 1]
    cell = [c(1, 1), c(2, 253), c(40, 100), c(254, 254), c(100, 200), c(128, 128), c(5, 5),
            256 * 256]
    assert layouts[1][2, 253] == pc.STAIR and layouts[1][40, 100] == pc.WALL
    assert_rows(device_rows(layouts, lay, cell), source_rows(layouts, lay, cell), "256x256")


def check_seek(eng, case):
    import torch
    from optimax_rogue_amd.path import seek
    snap = eng.snapshot()
    for player in (0, 1):
        want = seek(snap, case["cfg"], player, bank=eng.bank)
        got = eng.seek(player=player)
        assert len(got) == 3
        assert [g.dtype for g in got] == [torch.int32, torch.int8, torch.int16]
        for g, w, what in zip(got, want, ("dist", "move", "target")):
            assert tuple(g.shape) == (eng.B, 4) and g.is_contiguous()
            bad = np.argwhere(g.cpu().numpy() != w)
            assert len(bad) == 0, (what, player, bad[:5].tolist())


@pytest.mark.parametrize("n_games", BATCHES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_seek_matches_the_host(name, n_games):
    case = CASES[name]
    eng = make_engine(case, n_games)
    check_seek(eng, case)                     # the start state
    sc.vc.drive_engine(eng, case)
    check_seek(eng, case)
    if eng.bank is None:
        assert eng.pair_field is None
    elif n_games == 65:
        import torch
        pairs = eng.pair_field
        L, WH = len(eng.bank), eng.bank.width * eng.bank.height
        assert pairs.dtype == torch.uint16 and tuple(pairs.shape) == (L, WH, WH)
        assert eng.pair_field is pairs                           # computed once
        assert np.array_equal(pairs.cpu().numpy(), eng.bank.pair_field())


def walk_env(n_games=200, seed=5):
    from optimax_rogue_amd import EnvConfig, Policy, VecEnv
    cfg = EnvConfig(width=9, height=8, n_npcs=0, start_mode=1, max_ticks=100000,
                    layouts=pc.walk_cfg().layouts)
    return cfg, VecEnv(cfg, n_games, seed=seed, opponent=Policy.Stay, check_actions=False)


def test_walk_on_the_device():
    """step(seek's move) on a bank with pockets, both players on one depth and
    player 2 standing still: every tick a game further than one move gets
    exactly one closer on its depth; at one move it attacks, nobody moves and
    player 2's health falls by damage - armor, until Player1Win; a game whose
    player 2 cannot be reached stays put."""
    import torch
    cfg, env = walk_env()
    eng = env.engine
    hit = int(cfg.player_damage) - int(cfg.player_armor)
    dist, move, target = env.seek()
    started_unreachable = dist[:, 0] == -1
    live = torch.ones_like(started_unreachable)          # not done yet
    won = torch.zeros_like(live)
    assert bool(started_unreachable.any()) and bool((dist[:, 0] > 1).any())
    assert bool((dist[:, 0] != -2).all()) and bool((target[:, 0] == 1).all())
    for tick in range(60):
        d, m = dist[:, 0], move[:, 0]
        pos = [t.clone() for t in (eng.p_x, eng.p_y, eng.p_depth)]
        health = eng.p_health[1].clone()
        assert torch.equal(m == 5, d <= 0), tick
        obs, reward, done, status = env.step(m)
        ndist = env.seek()[0][:, 0]
        same = [(a == b) for a, b in zip(pos, (eng.p_x, eng.p_y, eng.p_depth))]
        put = same[0][0] & same[1][0] & same[2][0] & same[0][1] & same[1][1] & same[2][1]
        closer = (d > 1) & same[2][0] & ~done & (ndist == d - 1)
        attack = (d == 1) & (put | done) & ((eng.p_health[1] == health - hit) | done)
        stuck = (d == -1) & put & ~done & (ndist == -1)
        kinds = closer.int() + attack.int() + stuck.int()
        bad = live & (kinds != 1)
        assert not bool(bad.any()), (tick, torch.nonzero(bad).flatten().tolist()[:5])
        # a win is the attack that takes the last health
        assert bool((~(done & live) | ((d == 1) & (status == 2) & (health <= hit))).all()), tick
        won |= done & live & (status == 2)
        live &= ~done
        dist, move, _ = env.seek()
        if not bool((live & ~started_unreachable).any()):
            break
    assert bool(won.any()) and torch.equal(won, ~started_unreachable)
    assert bool((live == started_unreachable).all())


def test_hunt_moves_is_its_composition():
    import torch
    from optimax_rogue_amd import Policy, VecEnv
    seen = set()
    for name in ("c", "pockets"):
        case = CASES[name]
        env = VecEnv(case["cfg"], 200, seed=case["seed"], opponent=Policy.Random,
                     check_actions=False)
        for _ in range(6):
            env.step(env.hunt_moves())
        for player in (0, 1):
            dist, move, _ = env.seek(player)
            want = torch.where(dist[:, 0] > 0, move[:, 0], env.stair_moves(player))
            got = env.hunt_moves(player)
            assert got.dtype == torch.int8 and tuple(got.shape) == (200,)
            assert torch.equal(got, want)
            seen |= set((dist[:, 0] > 0).tolist())
    assert seen == {True, False}         # both branches of the composition were taken


def test_seek_out_reuse_and_refusals():
    import torch
    from optimax_rogue_amd import _lib
    case = CASES["c"]
    eng = make_engine(case, 65)
    sc.vc.drive_engine(eng, case)
    dev = eng.device
    want = eng.seek()
    fresh = lambda: (torch.full((65, 4), -7, dtype=torch.int32, device=dev),
                     torch.full((65, 4), -7, dtype=torch.int8, device=dev),
                     torch.full((65, 4), -7, dtype=torch.int16, device=dev))
    out = fresh()
    got = eng.seek(out=out)
    assert all(g is o for g, o in zip(got, out))
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    got = eng.seek(player=1, out=out)
    assert all(torch.equal(g, w) for g, w in zip(got, eng.seek(player=1)))
    # every bad argument is refused on the host, before any launch
    d, m, t = fresh()
    big = torch.zeros((65 * 4 + 8,), dtype=torch.int32, device=dev)
    for kw in (dict(player=2), dict(player=-1), dict(out=(d, m)), dict(out=d),
               dict(out=(d, m, t, t)), dict(out=(d[:64], m, t)), dict(out=(d, m, t[:, :3])),
               dict(out=(d.to(torch.int64), m, t)), dict(out=(d, t, m)), dict(out=(d, m.cpu(), t)),
               dict(out=(d, m, t.t().contiguous().t())),
               dict(out=(big[1:65 * 4 + 1].view(65, 4), m, t)),        # misaligned rows
               dict(out=(d, m, m))):
        with pytest.raises(ValueError):
            eng.seek(**kw)
    # the C codes: ORX_EINVAL from the host side of each entry point
    lib, vp = eng.lib, ctypes.c_void_p
    p = lambda x: vp(x.data_ptr())
    pairs, st = p(eng.pair_field), eng._stream()
    q = lambda *a: lib.orx_path_seek(eng._pcfg, eng._pst, *a)
    assert q(pairs, 2, p(d), p(m), p(t), 65, st) == -22
    assert b"player" in lib.orx_last_error()
    assert q(pairs, 0, None, None, None, 65, st) == -22
    assert q(pairs, 0, p(d), p(m), p(t), 0, st) == -22
    assert q(None, 0, p(d), p(m), p(t), 65, st) == -22
    assert b"pairs" in lib.orx_last_error()
    assert q(pairs, 0, vp(d.data_ptr() + 4), p(m), p(t), 65, st) == -22
    assert b"aligned" in lib.orx_last_error()
    assert q(pairs, 0, p(d), vp(m.data_ptr() + 1), p(t), 65, st) == -22
    assert q(pairs, 0, p(d), p(m), vp(t.data_ptr() + 2), 65, st) == -22
    assert lib.orx_path_seek(eng._pcfg, None, pairs, 0, p(d), p(m), p(t), 65, st) == -22
    rows = lambda *a: lib.orx_path_rows(eng._pcfg, *a)
    lay = torch.zeros(4, dtype=torch.int32, device=dev)
    buf = torch.zeros((4, 72), dtype=torch.int16, device=dev)
    assert rows(None, p(lay), p(lay), p(buf), 4, st) == -22
    assert rows(p(eng.bank_tiles), None, p(lay), p(buf), 4, st) == -22
    assert rows(p(eng.bank_tiles), p(lay), None, p(buf), 4, st) == -22
    assert rows(p(eng.bank_tiles), p(lay), p(lay), None, 4, st) == -22
    assert rows(p(eng.bank_tiles), p(lay), p(lay), p(buf), 0, st) == -22
    nobank = make_engine(CASES["a"], 4)
    assert lib.orx_path_rows(nobank._pcfg, p(eng.bank_tiles), p(lay), p(lay), p(buf), 4, st) == -22
    with pytest.raises(_lib.OrxError):
        eng._call("orx_path_seek", pairs, 3, p(d), p(m), p(t), 65, st)
    # each output alone
    assert q(pairs, 0, p(d), None, None, 65, st) == 0
    assert q(pairs, 0, None, p(m), None, 65, st) == 0
    assert q(pairs, 0, None, None, p(t), 65, st) == 0
    assert all(torch.equal(g, w) for g, w in zip((d, m, t), want))
    # a table above the limit is refused with its size; inside capture, a first use
    small = make_engine(case, 4)
    small.PAIR_FIELD_MAX_BYTES = 1000
    with pytest.raises(ValueError, match=str(2 * 4 * 72 * 72)):
        small.seek()


def test_seek_leaves_the_state_untouched():
    case = CASES["items12"]
    eng = make_engine(case, 63)
    sc.vc.drive_engine(eng, case)
    before = eng.snapshot()
    actions, tiles = eng.actions.clone(), eng.bank_tiles.clone()
    for player in (0, 1):
        eng.seek(player=player)
    after = eng.snapshot()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert bool((eng.actions == actions).all()) and bool((eng.bank_tiles == tiles).all())
    # no random words either: the next ticks equal an engine's that never asked
    twin = make_engine(case, 63)
    sc.vc.drive_engine(twin, case)
    for _ in range(3):
        eng.seek()
        for e in (eng, twin):
            e.step(e.policy(1, 1))
    a, b = eng.snapshot(), twin.snapshot()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_seek_on_a_side_stream():
    import torch
    from optimax_rogue_amd.path import seek
    case = CASES["pockets"]
    eng = make_engine(case, 200)
    sc.vc.drive_engine(eng, case)
    want = seek(eng.snapshot(), case["cfg"], 1, bank=eng.bank)
    s = torch.cuda.Stream(device=eng.device)
    s.wait_stream(torch.cuda.current_stream(eng.device))
    with torch.cuda.stream(s):
        got = eng.seek(player=1)            # (the table is built on this stream too)
        done = torch.cuda.Event()
        done.record(s)
    done.synchronize()
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)


def test_step_then_seek_in_one_graph():
    """env.step(a) followed by env.seek(out=...) captured in one graph (a
    linear chain on the capture stream): three replays against an eager twin.
    The table's first use inside a capture is refused."""
    import torch
    from optimax_rogue_amd import VecEnv
    case = CASES["pockets"]
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
    out = (torch.zeros((B, 4), dtype=torch.int32, device=dev),
           torch.zeros((B, 4), dtype=torch.int8, device=dev),
           torch.zeros((B, 4), dtype=torch.int16, device=dev))
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    refused = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(refused, stream=s):
            out[0].zero_()
            with pytest.raises(RuntimeError, match="before capturing"):
                env.seek(out=out)
    env.seek()                      # builds the table
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            obs, reward, done, status = env.step(a)
            env.seek(out=out)
    torch.cuda.current_stream(dev).wait_stream(s)
    for k in range(1, 4):
        a.copy_(moves[k])
        g.replay()
        t_obs, t_reward, t_done, t_status = twin.step(moves[k])
        t_out = twin.seek()
        torch.cuda.synchronize(dev)
        assert torch.equal(obs, t_obs) and torch.equal(status, t_status), k
        assert torch.equal(reward, t_reward) and torch.equal(done, t_done), k
        for x, y in zip(out, t_out):
            assert torch.equal(x, y), k
        assert int((out[0][:, 0] > 0).sum()) > 0
