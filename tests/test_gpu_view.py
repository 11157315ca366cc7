"""GPU: orx_view (BatchedEngine.view / VecEnv.view) against the host reference
``render_view(eng.snapshot(), ...)``: exact equality over every game and
cell, on the five configurations of view_cases driven to the tick at which
tests/test_view.py shows the oracle's states cover every kind of cell.

Batch sizes 1, 63, 65 and 200: a lone game, a partial wave, a wave plus one
game, and (with an odd window side) a total byte count that is no multiple
of 16 -- the byte tail of the 16-byte-per-lane stream-out.  At radius 15 a
workgroup takes 32 games (16 with the health plane), at radius 1 and 5 it
takes 64, so 65 and 200 games are several workgroups of every shape.
"""
import numpy as np
import pytest

import view_cases as vc

pytestmark = pytest.mark.gpu

CASES = vc.cases()
BATCHES = (1, 63, 65, 200)


def make_engine(case, n_games, **kw):
    from optimax_rogue_amd.engine import BatchedEngine
    return BatchedEngine(case["cfg"], n_games, seed=case["seed"], **kw)


def check_views(eng, case, radii=None):
    """Every radius, player and health setting of one engine state; returns
    the OR of all cell codes seen."""
    from optimax_rogue_amd.view import render_view
    snap = eng.snapshot()
    seen = 0
    for radius in radii or case["radii"]:
        for player in (0, 1):
            want_c, want_h = render_view(snap, case["cfg"], player, radius, bank=eng.bank,
                                         health=True)
            cells = eng.view(radius, player=player)
            cells2, health = eng.view(radius, player=player, health=True)
            V = 2 * radius + 1
            for t in (cells, cells2, health):
                assert str(t.dtype) == "torch.uint8"
                assert tuple(t.shape) == (eng.B, V, V) and t.is_contiguous()
            assert np.array_equal(cells.cpu().numpy(), want_c), (radius, player)
            assert np.array_equal(cells2.cpu().numpy(), want_c), (radius, player)
            assert np.array_equal(health.cpu().numpy(), want_h), (radius, player)
            seen |= int(np.bitwise_or.reduce(want_c, axis=None))
    return seen


@pytest.mark.parametrize("n_games", BATCHES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_view_matches_render_view(name, n_games):
    case = CASES[name]
    eng = make_engine(case, n_games)
    check_views(eng, case, radii=case["radii"][:1])      # the start state
    vc.drive_engine(eng, case)
    seen = check_views(eng, case)
    if n_games == vc.N_GAMES and case["cfg"].n_npcs:
        assert seen & 8 and seen & 4                        # NPCs and the other player in sight


def test_engine_states_are_the_oracles(oracle_lib):
    """The states the GPU test views are the ones test_view.py's coverage
    conditions were asserted on."""
    case = CASES["a"]
    eng = make_engine(case, vc.N_GAMES)
    vc.drive_engine(eng, case)
    got, want = eng.snapshot(), vc.oracle_states(case)[1]
    for k in ("p_x", "p_y", "p_depth", "p_health", "st_x", "st_y", "npc_alive", "episode"):
        assert np.array_equal(np.asarray(got[k], np.int64), np.asarray(want[k], np.int64)), k


def test_view_items():
    """The item bits with the character mechanics: every dying NPC drops."""
    from optimax_rogue_amd import EnvConfig
    from optimax_rogue_amd.enums import EXT_RPG
    from optimax_rogue_amd.view import VIEW_ITEM, VIEW_ITEM_KIND
    case = dict(cfg=EnvConfig(width=10, height=8, n_npcs=4, flags=EXT_RPG, item_drop_pct=100),
                seed=21, ticks=20, policies=(1, 1), radii=(1, 5))
    eng = make_engine(case, vc.N_GAMES)
    vc.drive_engine(eng, case)
    assert int(eng.item_mask[0].ne(0).sum()) > 0
    seen = check_views(eng, case)
    assert seen & VIEW_ITEM and seen & VIEW_ITEM_KIND


def test_view_out_reuse_and_checks():
    import torch
    case = CASES["a"]
    eng = make_engine(case, 65)
    vc.drive_engine(eng, case)
    want_c, want_h = eng.view(5, health=True)
    out = torch.full((65, 11, 11), 255, dtype=torch.uint8, device=eng.device)
    got = eng.view(5, out=out)
    assert got is out and got.data_ptr() == out.data_ptr()
    assert torch.equal(out, want_c)
    pair = (torch.full_like(out, 255), torch.full_like(out, 255))
    c, h = eng.view(5, health=True, out=pair)
    assert c is pair[0] and h is pair[1]
    assert torch.equal(c, want_c) and torch.equal(h, want_h)
    # every bad argument is refused on the host, before any launch
    for kw in (dict(radius=0), dict(radius=16), dict(radius=5, player=2),
               dict(radius=5, out=torch.empty((65, 11, 12), dtype=torch.uint8, device=eng.device)),
               dict(radius=5, out=torch.empty((64, 11, 11), dtype=torch.uint8, device=eng.device)),
               dict(radius=5, out=torch.empty((65, 11, 11), dtype=torch.int8, device=eng.device)),
               dict(radius=5, out=torch.empty((65, 11, 11), dtype=torch.uint8)),
               dict(radius=5, health=True, out=out)):
        with pytest.raises(ValueError):
            eng.view(**kw)


def test_view_leaves_the_state_untouched():
    case = CASES["d"]
    eng = make_engine(case, 63)
    vc.drive_engine(eng, case)
    before = eng.snapshot()
    grid = eng.npc_grid.clone()
    actions = eng.actions.clone()
    for radius in (1, 15):
        for player in (0, 1):
            eng.view(radius, player=player, health=True)
    after = eng.snapshot()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert bool((eng.npc_grid == grid).all()) and bool((eng.actions == actions).all())
    # no random words either: the next ticks equal an engine's that never looked
    twin = make_engine(case, 63)
    vc.drive_engine(twin, case)
    for e in (eng, twin):
        e.step(e.policy(1, 1))
    a, b = eng.snapshot(), twin.snapshot()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_view_on_a_side_stream():
    import torch
    from optimax_rogue_amd.view import render_view
    case = CASES["c"]
    eng = make_engine(case, 200)
    vc.drive_engine(eng, case)
    want = render_view(eng.snapshot(), case["cfg"], 1, 5, bank=eng.bank)
    s = torch.cuda.Stream(device=eng.device)
    s.wait_stream(torch.cuda.current_stream(eng.device))
    with torch.cuda.stream(s):
        cells = eng.view(5, player=1)
        done = torch.cuda.Event()
        done.record(s)
    done.synchronize()
    assert np.array_equal(cells.cpu().numpy(), want)


def test_step_then_view_in_one_graph():
    """env.step(a) followed by env.view(5) captured in one graph (a linear
    chain on the capture stream): three replays against an eager twin."""
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
    cells = torch.zeros((B, 11, 11), dtype=torch.uint8, device=dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            obs, reward, done, status = env.step(a)
            env.view(5, out=cells)
    torch.cuda.current_stream(dev).wait_stream(s)
    for k in range(1, 4):
        a.copy_(moves[k])
        g.replay()
        t_obs, t_reward, t_done, t_status = twin.step(moves[k])
        t_cells = twin.view(5)
        torch.cuda.synchronize(dev)
        assert torch.equal(obs, t_obs) and torch.equal(status, t_status), k
        assert torch.equal(reward, t_reward) and torch.equal(done, t_done), k
        assert torch.equal(cells, t_cells), k
        assert int((cells & 12 != 0).sum()) > 0
