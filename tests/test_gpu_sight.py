"""GPU: orx_sight (BatchedEngine.sight / seen_view / sees_other) against the
host reference ``sight.visible(eng.snapshot(), ...)``, bit for bit, on the
five configurations of sight_cases.GPU_CASES driven to the tick at which
tests/test_sight.py shows the oracle's states hide and show players, NPCs and
walls.

Batch sizes 1, 63, 65 and 200: a lone game, a partial workgroup, a workgroup
plus one game (64 games per workgroup), several workgroups, and with an odd
window side a byte count that is no multiple of 16 -- the byte tail
of the 16-bytes-per-lane masking.  Every output is a view into a poisoned
buffer (tests/guarded.py): the row words at a 16-byte boundary and 4 bytes past
one, the planes at one and 1 byte past it (the byte path).  The planes hold
orx_view's output first; a cell orx_sight skipped keeps its view code, which
is non-zero without bit 6 in the grid, where the reference is 0 or has bit 6.
"""
import numpy as np
import pytest

import sight_cases as sc
import view_cases as vc
from guarded import POISONS, Guarded

pytestmark = pytest.mark.gpu

CASES = sc.cases()
BATCHES = (1, 63, 65, 200)
# the outputs asked for: (rows, cells, health)
MODES = ((True, False, False), (False, True, False), (False, True, True), (True, True, True))


def make_engine(case, n_games, **kw):
    from optimax_rogue_amd.engine import BatchedEngine
    return BatchedEngine(case["cfg"], n_games, seed=case["seed"], **kw)


def driven(name, n_games):
    eng = make_engine(CASES[name], n_games)
    vc.drive_engine(eng, CASES[name])
    return eng


def check_sight(eng, cfg, radius, player, what, skews=((0, 0), (4, 1))):
    """orx_sight of one engine state, radius and player in every output mode,
    under both poisons and both placements, against the reference."""
    import torch
    from optimax_rogue_amd import sight, view
    from optimax_rogue_amd.engine import _ptr
    snap, B, V = eng.snapshot(), eng.B, 2 * radius + 1
    cells, hp = view.render_view(snap, cfg, player, radius, bank=eng.bank, health=True)
    vis = sight.visible(snap, cfg, player, radius, bank=eng.bank)
    want_rows = sight.pack_rows(vis)
    want_cells, want_hp = sight.apply(cells, vis, hp)
    in_grid = (cells & 3) != 0
    assert (cells[in_grid] != 0).all() and not (cells & sight.SIGHT_SEEN).any()
    for poison in POISONS:
        for row_skew, cell_skew in skews:
            for with_rows, with_cells, with_hp in MODES:
                msg = f"{what} R={radius} player {player} poison {poison:#x} skew {cell_skew}"
                gr = Guarded(eng.device, torch.uint32, (B, V), poison, row_skew)
                gc = Guarded(eng.device, torch.uint8, (B, V, V), poison, cell_skew)
                gh = Guarded(eng.device, torch.uint8, (B, V, V), poison, cell_skew)
                eng.view(radius, player=player, health=True, out=(gc.out, gh.out))
                eng._call("orx_sight", player, radius, _ptr(gr.out) if with_rows else None,
                          _ptr(gc.out) if with_cells else None, _ptr(gh.out) if with_hp else None,
                          B, eng._stream())
                # what was not asked for is what it was: poison, or the view
                gr.check(want_rows if with_rows else np.full((B, V), poison * 0x01010101, np.uint32),
                         msg + " rows")
                gc.check(want_cells if with_cells else cells, msg + " cells")
                gh.check(want_hp if with_hp else hp, msg + " health")
    return vis, cells


@pytest.mark.parametrize("n_games", BATCHES)
@pytest.mark.parametrize("name", sc.GPU_CASES)
def test_sight_matches_visible(name, n_games):
    case = CASES[name]
    eng = driven(name, n_games)
    hidden = lit = 0
    for radius in sc.RADII:
        for player in (0, 1):
            vis, cells = check_sight(eng, case["cfg"], radius, player, f"case {name} B={n_games}")
            hidden += int((~vis & ((cells & 3) != 0)).sum())
            lit += int(vis.sum())
    assert lit > 0
    if n_games == sc.N_GAMES and case["cfg"].layouts is not None:
        assert hidden > 0            # (a bank's walls hide cells of the grid)
    if case["cfg"].layouts is None:
        assert hidden == 0           # (the closed form: everything in the grid is seen)


def test_engine_states_are_the_oracles(oracle_lib):
    """The states the GPU test looks at in the new case are the ones
    test_sight.py's coverage conditions were asserted on."""
    case = CASES["wg"]
    got, want = driven("wg", sc.N_GAMES).snapshot(), vc.oracle_states(case)[1]
    for k in ("p_x", "p_y", "p_depth", "p_health", "p_layout", "npc_alive", "episode"):
        assert np.array_equal(np.asarray(got[k], np.int64), np.asarray(want[k], np.int64)), k


def test_wrappers_out_reuse_and_checks():
    import torch
    from optimax_rogue_amd import sight, view
    case = CASES["wg"]
    eng = driven("wg", 65)
    snap, cfg = eng.snapshot(), case["cfg"]
    for radius, player in ((5, 0), (15, 1), (1, 1)):
        V = 2 * radius + 1
        cells, hp = view.render_view(snap, cfg, player, radius, bank=eng.bank, health=True)
        vis = sight.visible(snap, cfg, player, radius, bank=eng.bank)
        want_c, want_h = sight.apply(cells, vis, hp)
        rows = eng.sight(radius, player=player)
        assert rows.dtype == torch.uint32 and tuple(rows.shape) == (65, V)
        assert np.array_equal(rows.cpu().numpy(), sight.pack_rows(vis))
        got = eng.seen_view(radius, player=player)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want_c)
        c, h = eng.seen_view(radius, player=player, health=True)
        assert np.array_equal(c.cpu().numpy(), want_c) and np.array_equal(h.cpu().numpy(), want_h)
    # out= is written and returned
    out = torch.full((65, 11), -1, dtype=torch.int32, device=eng.device).view(torch.uint32)
    assert eng.sight(5, out=out) is out
    assert torch.equal(out.view(torch.int32), eng.sight(5).view(torch.int32))
    pair = (torch.full((65, 11, 11), 255, dtype=torch.uint8, device=eng.device),
            torch.full((65, 11, 11), 255, dtype=torch.uint8, device=eng.device))
    c, h = eng.seen_view(5, health=True, out=pair)
    assert c is pair[0] and h is pair[1]
    want = eng.seen_view(5, health=True)
    assert torch.equal(c, want[0]) and torch.equal(h, want[1])
    one = torch.full((65, 11, 11), 255, dtype=torch.uint8, device=eng.device)
    assert eng.seen_view(5, out=one) is one and torch.equal(one, want[0])
    # every bad argument is refused on the host, before any launch
    u8, u32 = torch.uint8, torch.uint32
    for kw in (dict(radius=0), dict(radius=16), dict(radius=5, player=2),
               dict(radius=5, out=torch.empty((65, 12), dtype=u32, device=eng.device)),
               dict(radius=5, out=torch.empty((64, 11), dtype=u32, device=eng.device)),
               dict(radius=5, out=torch.empty((65, 11), dtype=torch.int32, device=eng.device)),
               dict(radius=5, out=torch.empty((65, 11), dtype=u32)),
               dict(radius=5, out=torch.empty((65, 22), dtype=u32, device=eng.device)[:, ::2])):
        with pytest.raises(ValueError):
            eng.sight(**kw)
    for kw in (dict(radius=0), dict(radius=16), dict(radius=5, player=2),
               dict(radius=5, out=torch.empty((65, 11, 12), dtype=u8, device=eng.device)),
               dict(radius=5, out=torch.empty((65, 11, 11), dtype=u8)),
               dict(radius=5, health=True, out=one),
               dict(radius=5, health=True, out=(one, one))):
        with pytest.raises(ValueError):
            eng.seen_view(**kw)
    for radius, player in ((0, 0), (16, 0), (5, 2)):
        with pytest.raises(ValueError):
            eng.sees_other(radius, player)
    assert torch.equal(one, want[0])      # (no refused call wrote)


def test_sight_leaves_the_state_untouched():
    case = CASES["wg"]
    eng = driven("wg", 63)
    before = eng.snapshot()
    actions = eng.actions.clone()
    for radius in (1, 15):
        for player in (0, 1):
            eng.sight(radius, player=player)
            eng.seen_view(radius, player=player, health=True)
            eng.sees_other(radius, player=player)
    after = eng.snapshot()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert bool((eng.actions == actions).all())
    # no random words either: the next ticks equal an engine's that never looked
    twin = driven("wg", 63)
    for e in (eng, twin):
        e.step(e.policy(1, 1))
    a, b = eng.snapshot(), twin.snapshot()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ("c", "wg"))
def test_the_players_see_each_other_or_neither_does(name):
    from optimax_rogue_amd import sight
    case = CASES[name]
    eng = driven(name, sc.N_GAMES)
    a, b = eng.sees_other(15, 0), eng.sees_other(15, 1)
    assert str(a.dtype) == "torch.bool" and tuple(a.shape) == (sc.N_GAMES,)
    assert bool((a == b).all()) and bool(a.any()) and not bool(a.all())
    snap = eng.snapshot()
    for p, got in ((0, a), (1, b)):
        vis = sight.visible(snap, case["cfg"], p, 15, bank=eng.bank)
        assert np.array_equal(got.cpu().numpy(), sc.sees_other(snap, vis, p, 15))
    # a smaller window: the other player may be outside it
    vis = sight.visible(snap, case["cfg"], 0, 1, bank=eng.bank)
    assert np.array_equal(eng.sees_other(1, 0).cpu().numpy(), sc.sees_other(snap, vis, 0, 1))


def test_step_then_seen_view_in_one_graph():
    """env.step(a) followed by env.seen_view(5) captured in one graph (a linear
    chain on the capture stream): three replays against an eager twin."""
    import torch
    from optimax_rogue_amd import VecEnv
    from optimax_rogue_amd.sight import SIGHT_SEEN
    case = CASES["wg"]
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
    cells = torch.zeros((B, 11, 11), dtype=torch.uint8, device=dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            obs, reward, done, status = env.step(a)
            env.seen_view(5, out=cells)
    torch.cuda.current_stream(dev).wait_stream(s)
    for k in range(1, 4):
        a.copy_(moves[k])
        g.replay()
        t_obs, t_reward, t_done, t_status = twin.step(moves[k])
        t_cells = twin.seen_view(5)
        torch.cuda.synchronize(dev)
        assert torch.equal(obs, t_obs) and torch.equal(status, t_status), k
        assert torch.equal(reward, t_reward) and torch.equal(done, t_done), k
        assert torch.equal(cells, t_cells), k
        assert int((cells == 0).sum()) > 0 and int((cells & SIGHT_SEEN != 0).sum()) > 0
