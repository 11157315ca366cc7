"""GPU: orx_path_ticks (BatchedEngine.path_ticks / rush_moves and VecEnv's
pass-throughs) against the host statement ``path.ticks(eng.snapshot(), ...)``,
bit for bit, into poisoned buffers (tests/guarded.py).

The shapes are the smallest at which the kernel can go wrong: widths 4, 31, 32,
33, 64 and 65 (the row word's boundary and its carry) at heights 4 and 7, 0, 1,
16, 17, 40 and 255 NPCs on 20 x 20 (a lane owns up to four slots), batches of
1, 5 and 257 (partial workgroups), and one 256 x 256 serpentine with two NPCs
in its corridor (a game per workgroup, a search of 32,000 steps, a jump of 127).
Then the call's variants, the hand-built states of ticks_cases through
``load_snapshot``, and the play-out through ``VecEnv.step``: eagerly, and once
more with the step and the query captured in one graph.
"""
import itertools

import numpy as np
import pytest

import ticks_cases as tc
from guarded import POISONS, Guarded

pytestmark = pytest.mark.gpu

STAY = tc.STAY


def make_engine(cfg, n_games, seed=1, **kw):
    from optimax_rogue_amd.engine import BatchedEngine
    return BatchedEngine(cfg, n_games, seed=seed, **kw)


def specs(B, radius):
    import torch
    V = 2 * (radius or 0) + 1
    return ((torch.int32, (B,)), (torch.int8, (B,)), (torch.uint16, (B, V, V)))


def raw_call(eng, player, radius, outs):
    from optimax_rogue_amd.engine import _ptr
    eng._call("orx_path_ticks", _ptr(eng.route_planes), player, radius or 0,
              *(None if g is None else _ptr(g.out) for g in outs), eng.B, eng._stream())


def check_ticks(eng, cfg, radii=(None, 5), players=(0, 1), poisons=POISONS[:1], what=""):
    """The kernel's three outputs equal the reference on the engine's state."""
    from optimax_rogue_amd.path import query, ticks
    snap = eng.snapshot()
    for player, radius in itertools.product(players, radii):
        want = ticks(snap, cfg, player, radius, bank=eng.bank)
        for poison in poisons:
            outs = [Guarded(eng.device, dt, shape, poison, 2 if j == 2 else 0)
                    for j, (dt, shape) in enumerate(specs(eng.B, radius)[:len(want)])]
            raw_call(eng, player, radius, outs + [None] * (3 - len(outs)))
            for g, w, name in zip(outs, want, ("ticks", "move", "window")):
                g.check(w, f"{what} player {player} radius {radius} {name} poison {poison:#x}")
        dist = query(snap, cfg, player, bank=eng.bank)[0]
        assert ((want[0] >= dist) | (want[0] == -1)).all()
    return snap


def room_or_bank(W, H, K, bank_seed=None, **kw):
    from optimax_rogue_amd import DungeonBank, EnvConfig
    layouts = None
    if bank_seed is not None:
        layouts = DungeonBank.random(W, H, 3, seed=bank_seed, wall_p=0.25).layouts
    return EnvConfig(width=W, height=H, n_npcs=K, layouts=layouts, max_ticks=0, **kw)


@pytest.mark.parametrize("H", (4, 7))
@pytest.mark.parametrize("W", (4, 31, 32, 33, 64, 65))
def test_widths_round_the_word_boundary(W, H):
    K = 1 if W * H < 40 else 3
    cfgs = [room_or_bank(W, H, K)]
    if W >= 31 and H == 7:
        cfgs.append(room_or_bank(W, H, K, bank_seed=W))
    for cfg in cfgs:
        eng = make_engine(cfg, 65, seed=W + H)
        check_ticks(eng, cfg, (None, 1, 15), what=f"{W}x{H} start")
        eng.rollout(4, 1, 1)
        check_ticks(eng, cfg, (None, 5), what=f"{W}x{H}")


@pytest.mark.parametrize("K", (0, 1, 16, 17, 40, 255))
def test_npc_counts(K):
    cfg = room_or_bank(20, 20, K, player_damage=3)
    eng = make_engine(cfg, 65, seed=K)
    eng.rollout(3, 1, 1)
    check_ticks(eng, cfg, (None, 5, 15), what=f"K={K}")


@pytest.mark.parametrize("B", (1, 5, 257))
def test_partial_workgroups(B):
    case = tc.cases()["bank"]
    eng = make_engine(case["cfg"], B, seed=case["seed"])
    eng.rollout(tc.WARMUP, 1, 1)
    check_ticks(eng, case["cfg"], (None, 1, 5), poisons=POISONS, what=f"B={B}")


def variants():
    from optimax_rogue_amd import EnvConfig
    out = dict(tc.cases())
    wg = out["bank"]["cfg"].layouts
    out["p1_below"] = dict(cfg=EnvConfig(width=12, height=10, n_npcs=6, layouts=wg, start_mode=2,
                                         p1_depth=1, p2_depth=0, max_ticks=0), seed=9)
    out["stock"] = dict(cfg=EnvConfig(width=8, height=8, n_npcs=4, rng=1, max_ticks=0), seed=1000)
    return out


@pytest.mark.parametrize("name", sorted(variants()))
def test_ticks_matches_the_host(name):
    """ticks_cases' configurations (the rooms and banks of the table, Together,
    a weak and a strong player), both Separated orders and stock seeding: both
    players, with a window at radii 1, 5 and 15 and without one."""
    case = variants()[name]
    eng = make_engine(case["cfg"], 301, seed=case["seed"])
    eng.rollout(tc.WARMUP, 1, 1)
    check_ticks(eng, case["cfg"], (None, 1, 5, 15), what=name)


def test_every_null_output_form_in_poisoned_buffers():
    from optimax_rogue_amd.path import ticks
    case = tc.cases()["room"]
    eng = make_engine(case["cfg"], 65, seed=case["seed"])
    eng.rollout(tc.WARMUP, 1, 1)
    radius, player = 3, 0
    want = ticks(eng.snapshot(), case["cfg"], player, radius)
    for mask in range(1, 8):
        for poison in POISONS:
            outs = [Guarded(eng.device, dt, shape, poison, 2 * (mask & 1) if j == 2 else 0)
                    if mask >> j & 1 else None for j, (dt, shape) in enumerate(specs(65, radius))]
            raw_call(eng, player, radius, outs)
            for g, w, what in zip(outs, want, ("ticks", "move", "window")):
                if g is not None:
                    g.check(w, f"outputs {mask:#x} {what} poison {poison:#x}")


def test_out_reuse_passthroughs_and_refusals():
    import ctypes
    import torch
    from optimax_rogue_amd import VecEnv
    case = tc.cases()["bank"]
    env = VecEnv(case["cfg"], 65, seed=case["seed"], opponent=1, check_actions=False)
    eng = env.engine
    eng.rollout(tc.WARMUP, 1, 1)
    dev = eng.device
    u16 = lambda t: t.view(torch.int16) if t.dtype == torch.uint16 else t
    same = lambda xs, ys: all(torch.equal(u16(x), u16(y)) for x, y in zip(xs, ys))
    want = eng.path_ticks(radius=2)
    fresh = lambda R=2: tuple(torch.full(shape, 7, dtype=torch.int16, device=dev).to(dt)
                              if dt != torch.uint16 else
                              torch.full(shape, 7, dtype=torch.int16, device=dev).view(dt)
                              for dt, shape in specs(65, R))
    out = fresh()
    got = eng.path_ticks(radius=2, out=out)
    assert all(g is o for g, o in zip(got, out)) and same(got, want)
    got = eng.path_ticks(player=1, out=out[:2])
    assert same(got, eng.path_ticks(player=1))
    assert same(env.path_ticks(radius=2), want)
    moves = env.rush_moves()
    assert moves.dtype == torch.int8 and tuple(moves.shape) == (65,)
    assert torch.equal(moves, want[1])
    assert torch.equal(env.rush_moves(1), eng.path_ticks(player=1)[1])
    t, m, w = fresh()
    for kw in (dict(player=2), dict(player=-1), dict(radius=0), dict(radius=16), dict(out=t),
               dict(out=(t, m, w)), dict(radius=2, out=(t, m)), dict(radius=1, out=(t, m, w)),
               dict(out=(t[:64], m)), dict(out=(t.to(torch.int64), m)), dict(out=(m, t)),
               dict(out=(t, m.cpu()))):
        with pytest.raises(ValueError):
            eng.path_ticks(**kw)
    with pytest.raises(ValueError):
        env.rush_moves(2)
    # the C codes: ORX_EINVAL from the host side of the entry point
    lib, vp = eng.lib, ctypes.c_void_p
    p = lambda x: vp(x.data_ptr())
    planes, st = p(eng.route_planes), eng._stream()
    q = lambda *args: lib.orx_path_ticks(eng._pcfg, eng._pst, *args)
    assert q(planes, 2, 2, p(t), p(m), p(w), 65, st) == -22
    assert b"player" in lib.orx_last_error()
    assert q(planes, 0, 2, None, None, None, 65, st) == -22
    assert q(planes, 0, 0, p(t), p(m), p(w), 65, st) == -22
    assert b"radius" in lib.orx_last_error()
    assert q(planes, 0, 2, p(t), p(m), p(w), 0, st) == -22
    assert q(None, 0, 2, p(t), p(m), p(w), 65, st) == -22
    assert b"planes" in lib.orx_last_error()
    assert q(planes, 0, 2, vp(t.data_ptr() + 2), p(m), p(w), 65, st) == -22
    assert q(planes, 0, 2, p(t), p(m), vp(w.data_ptr() + 1), 65, st) == -22
    assert b"aligned" in lib.orx_last_error()
    # a bad radius without a window is ignored
    assert q(planes, 0, 99, p(t), p(m), None, 65, st) == 0
    assert same((t, m), want)


@pytest.mark.parametrize("rows, damage", [(tc.HAND, 2), (tc.HAND_WEAK, 1)])
def test_hand_built_states(rows, damage):
    """One game per sentence of the definition, through ``load_snapshot``: the
    kernel gives the values written out in ticks_cases, and the reference's
    window."""
    cfg = tc.hand_cfg(2, player_damage=damage)
    eng = make_engine(cfg, len(rows))
    eng.load_snapshot(tc.hand_snap([dict(me=me, npcs=npcs) for _, me, npcs, _, _ in rows], 2))
    got, move = eng.path_ticks()
    assert got.cpu().tolist() == [r[3] for r in rows]
    assert move.cpu().tolist() == [r[4] for r in rows]
    check_ticks(eng, cfg, (None, 1, 5), players=(0,), poisons=POISONS, what="hand-built")


def test_the_largest_grid_a_long_search_and_a_long_jump():
    """B = 3 on the 256 x 256 serpentine (route_cases.serpentine, the corridor
    of route_serpentine.py): the asker at its start, an NPC of 127 health and
    one of 3 in the corridor against a = 1.  The corridor forces both fights:
    the construction's moves plus the blows.  A window is refused there."""
    import route_cases as rc
    from optimax_rogue_amd import DungeonBank, EnvConfig
    lay, start, end, moves = rc.serpentine(256, 256)
    bank = DungeonBank(lay[None])
    cfg = EnvConfig(width=256, height=256, n_npcs=2, layouts=bank.layouts, max_ticks=0)
    B = 3
    eng = make_engine(cfg, B)
    snap = dict(p_x=np.ones((2, B), np.int32), p_y=np.ones((2, B), np.int32),
                p_depth=np.zeros((2, B), np.int32), p_layout=np.zeros((2, B), np.int16),
                npc_pos=np.zeros((2, B), np.uint16), npc_health=np.zeros((2, B), np.int8),
                npc_alive=np.array([3, 1, 0], np.uint32))
    snap["npc_pos"][0], snap["npc_pos"][1] = 100 | 1 << 8, 50 | 3 << 8
    snap["npc_health"][0], snap["npc_health"][1] = 127, 3
    eng.load_snapshot(snap)
    got, move = eng.path_ticks()
    assert got.cpu().tolist() == [moves + 127 + 3, moves + 127, moves]
    assert move.cpu().tolist() == [tc.RIGHT] * 3
    check_ticks(eng, cfg, (None,), players=(0,), what="serpentine")
    with pytest.raises(ValueError):
        eng.path_ticks(radius=1)


def test_ticks_leaves_the_state_and_the_generators_untouched():
    case = variants()["stock"]
    eng, twin = (make_engine(case["cfg"], 65, seed=case["seed"]) for _ in range(2))
    for e in (eng, twin):
        e.rollout(tc.WARMUP, 1, 1)
    before = eng.snapshot()
    assert "mt_py" in before and "mt_np" in before
    for player in (0, 1):
        eng.path_ticks(player=player, radius=4)
        eng.rush_moves(player)
    after = eng.snapshot()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    for _ in range(3):
        eng.path_ticks()
        for e in (eng, twin):
            e.step(e.policy(1, 1))
    a, b = eng.snapshot(), twin.snapshot()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def played_env(name, **kw):
    from optimax_rogue_amd import Policy, VecEnv
    case = tc.cases()[name]
    env = VecEnv(case["cfg"], tc.N_GAMES, seed=case["seed"], opponent=Policy.Stay,
                 check_actions=False, **kw)
    env.engine.rollout(tc.WARMUP, 1, 1)
    return env


@pytest.mark.parametrize("name", ("bank", "room"))
def test_rushing_on_the_device_descends_on_schedule(name):
    """env.step(env.rush_moves()) for player 1, Stay for player 2 and the NPCs,
    in every game whose players are on different depths: ticks drops by exactly
    one per tick and the depth changes exactly in the tick where it was 1."""
    import torch
    env = played_env(name)
    eng = env.engine
    ticks, move = env.path_ticks()
    d0 = eng.p_depth[0].clone()
    playing = d0 != eng.p_depth[1]
    assert bool((ticks[playing] > 0).all())
    played, descended = int(playing.sum()), 0
    for _ in range(400):
        if not bool(playing.any()):
            break
        assert torch.equal(env.rush_moves(), move)
        env.step(torch.where(playing, move, STAY).to(torch.int8))
        now, nmove = env.path_ticks()
        n0 = eng.p_depth[0].clone()
        last, rest = playing & (ticks == 1), playing & (ticks > 1)
        assert bool((n0[last] == d0[last] + 1).all()), "did not descend where ticks was 1"
        assert bool((n0[rest] == d0[rest]).all()), "the depth changed before ticks was 1"
        assert bool((now[rest] == ticks[rest] - 1).all()), "ticks did not drop by exactly one"
        descended += int(last.sum())
        playing, ticks, move, d0 = rest, now, nmove, n0
    assert not bool(playing.any())
    assert played >= 280 and descended == played, (played, descended)


def test_rush_step_ticks_in_one_graph():
    """The closed loop -- rush_moves, step, path_ticks -- captured in one graph:
    its replays equal an eager twin, and ticks drops by one per replay in the
    games that walk on their depth.  The planes' first use inside a capture is
    refused."""
    import torch
    env, twin = (played_env("bank", out_buffers=1) for _ in range(2))
    dev, B = env.device, tc.N_GAMES
    a = torch.full((B,), STAY, dtype=torch.int8, device=dev)
    for e in (env, twin):          # (the first step settles the host-side launch blocks)
        e.step(a)
    out = (torch.zeros((B,), dtype=torch.int32, device=dev),
           torch.zeros((B,), dtype=torch.int8, device=dev),
           torch.zeros((B, 7, 7), dtype=torch.int16, device=dev).view(torch.uint16))
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    refused = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(refused, stream=s):
            out[0].zero_()
            with pytest.raises(RuntimeError, match="before capturing"):
                env.path_ticks(radius=3, out=out)
    env.path_ticks()                # packs the planes
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            obs, reward, done, status = env.step(env.rush_moves())
            env.path_ticks(radius=3, out=out)
    torch.cuda.current_stream(dev).wait_stream(s)
    eng = env.engine
    walked = 0
    for k in range(3):
        before, _ = twin.path_ticks()
        d0, d1 = twin.engine.p_depth[0].clone(), twin.engine.p_depth[1].clone()
        g.replay()
        t_obs, t_reward, t_done, t_status = twin.step(twin.rush_moves())
        t_out = twin.path_ticks(radius=3)
        torch.cuda.synchronize(dev)
        assert torch.equal(obs, t_obs) and torch.equal(status, t_status), k
        assert torch.equal(reward, t_reward) and torch.equal(done, t_done), k
        for x, y in zip(out, t_out):
            assert torch.equal(x.view(torch.int16) if x.dtype == torch.uint16 else x,
                               y.view(torch.int16) if y.dtype == torch.uint16 else y), k
        rest = (d0 != d1) & (before > 1)
        assert bool((out[0][rest] == before[rest] - 1).all()), k
        assert bool((eng.p_depth[0][rest] == d0[rest]).all()), k
        last = (d0 != d1) & (before == 1)
        assert bool((eng.p_depth[0][last] == d0[last] + 1).all()), k
        walked += int(rest.sum())
    assert walked >= 100
