"""GPU: orx_path_threat (BatchedEngine.threat / flee_moves / threat_view and
VecEnv's pass-throughs) against the host statement ``path.threat(eng.snapshot(),
...)``, with exact equality over every game, column and window cell.

The engine states are threat_cases.gpu_cases(): seek_cases' configurations (the
room and banks, a Separated start where the NPC column is absent, K = 0, 4, 6,
24 and 40, moving NPCs, items) plus K = 1, 16, 17, a bank without NPCs and
stock seeding, at the start and after their ticks, at batch sizes 1, 65 and 301
(a lone game, a wave plus one, a workgroup plus a tail at every window's games
per workgroup) and radii 1, 5, 15 and none.
"""
import itertools

import numpy as np
import pytest

import seek_cases as sc
import threat_cases as tc
from guarded import POISONS, Guarded

pytestmark = pytest.mark.gpu

CASES = tc.gpu_cases()
BATCHES = (1, 65, 301)
NAMES = ("dist", "move", "target", "after", "window")


def make_engine(case, n_games, **kw):
    from optimax_rogue_amd.engine import BatchedEngine
    return BatchedEngine(case["cfg"], n_games, seed=case["seed"], **kw)


def dtypes():
    import torch
    return (torch.int32, torch.int8, torch.int16, torch.int32, torch.uint16)


def shapes(B, radius):
    V = 2 * (radius or 0) + 1
    return ((B, 4), (B, 4), (B, 4), (B, 8), (B, V, V))


def check_threat(eng, case, radii):
    from optimax_rogue_amd.path import threat
    snap = eng.snapshot()
    for player, radius in itertools.product((0, 1), radii):
        want = threat(snap, case["cfg"], player, radius, bank=eng.bank)
        got = eng.threat(player=player, radius=radius)
        assert len(got) == (4 if radius is None else 5) and (want[4] is None) == (radius is None)
        for g, w, dt, shape, what in zip(got, want, dtypes(), shapes(eng.B, radius), NAMES):
            assert g.dtype == dt and tuple(g.shape) == shape and g.is_contiguous(), what
            bad = np.argwhere(g.cpu().numpy() != w)
            assert len(bad) == 0, (what, player, radius, len(bad), bad[:5].tolist())


@pytest.mark.parametrize("n_games", BATCHES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_threat_matches_the_host(name, n_games):
    case = CASES[name]
    eng = make_engine(case, n_games)
    check_threat(eng, case, (None, 5))                     # the start state
    sc.vc.drive_engine(eng, case)
    check_threat(eng, case, (None, 1, 5, 15))


def raw_call(eng, player, radius, outs):
    from optimax_rogue_amd.engine import _ptr
    eng._call("orx_path_threat", _ptr(eng.pair_field), player, radius,
              *(None if g is None else _ptr(g.out) for g in outs), eng.B, eng._stream())


@pytest.mark.parametrize("name", ["a", "pockets"])
def test_every_null_output_form_in_poisoned_buffers(name):
    """All 31 sets of outputs, each output a view into a buffer filled with a
    poison byte: what is asked for equals the reference under both poisons (no
    cell skipped), the bytes around it stay poison, and on odd sets the window
    starts at an offset that is no multiple of 16."""
    from optimax_rogue_amd.path import threat
    case = CASES[name]
    eng = make_engine(case, 65)
    sc.vc.drive_engine(eng, case)
    radius, player = 3, 1
    want = threat(eng.snapshot(), case["cfg"], player, radius, bank=eng.bank)
    for mask in range(1, 32):
        for poison in POISONS:
            outs = [Guarded(eng.device, dt, shape, poison, 2 * (mask & 1) if j == 4 else 0)
                    if mask >> j & 1 else None
                    for j, (dt, shape) in enumerate(zip(dtypes(), shapes(65, radius)))]
            raw_call(eng, player, radius, outs)
            for g, w, what in zip(outs, want, NAMES):
                if g is not None:
                    g.check(w, f"{name} outputs {mask:#x} {what} poison {poison:#x}")


def test_out_reuse_passthroughs_and_refusals():
    import ctypes
    import torch
    from optimax_rogue_amd import VecEnv, _lib
    case = CASES["c"]
    env = VecEnv(case["cfg"], 65, seed=case["seed"], opponent=1, check_actions=False)
    eng = env.engine
    sc.vc.drive_engine(eng, case)
    dev = eng.device
    want = eng.threat(radius=2)
    fresh = lambda R=2: tuple(torch.full(shape, -7, dtype=torch.int16, device=dev).to(dt)
                              if dt != torch.uint16 else
                              torch.full(shape, 7, dtype=torch.int16, device=dev).view(dt)
                              for dt, shape in zip(dtypes(), shapes(65, R)))
    out = fresh()
    got = eng.threat(radius=2, out=out)
    assert all(g is o for g, o in zip(got, out))
    assert all(torch.equal(g.view(torch.int16) if g.dtype == torch.uint16 else g,
                           w.view(torch.int16) if w.dtype == torch.uint16 else w)
               for g, w in zip(got, want))
    got = eng.threat(player=1, out=out[:4])
    assert all(torch.equal(g, w) for g, w in zip(got, eng.threat(player=1)))
    # VecEnv's pass-throughs are the engine's answers
    assert all(torch.equal(g.view(torch.int16) if g.dtype == torch.uint16 else g,
                           w.view(torch.int16) if w.dtype == torch.uint16 else w)
               for g, w in zip(env.threat(radius=2), want))
    assert torch.equal(env.threat_view(2).view(torch.int16), want[4].view(torch.int16))
    moves = env.flee_moves()
    assert moves.dtype == torch.int8 and tuple(moves.shape) == (65,)
    assert torch.equal(moves, want[1][:, 2])
    assert torch.equal(env.flee_moves(1), eng.threat(player=1)[1][:, 2])
    # every bad argument is refused on the host, before any launch
    d, m, t, a, w = fresh()
    big = torch.zeros((65 * 4 + 8,), dtype=torch.int32, device=dev)
    for kw in (dict(player=2), dict(player=-1), dict(radius=0), dict(radius=16),
               dict(out=(d, m, t)), dict(out=d), dict(out=(d, m, t, a, w)),
               dict(radius=2, out=(d, m, t, a)), dict(radius=1, out=(d, m, t, a, w)),
               dict(out=(d[:64], m, t, a)), dict(out=(d, m, t, a[:, :4])),
               dict(out=(d.to(torch.int64), m, t, a)), dict(out=(d, t, m, a)),
               dict(out=(d, m.cpu(), t, a)), dict(out=(d, m, t, d)),
               dict(out=(big[1:65 * 4 + 1].view(65, 4), m, t, a))):     # misaligned rows
        with pytest.raises(ValueError):
            eng.threat(**kw)
    with pytest.raises(ValueError):
        env.threat_view(0)
    with pytest.raises(ValueError):
        env.flee_moves(2)
    # the C codes: ORX_EINVAL from the host side of the entry point
    lib, vp = eng.lib, ctypes.c_void_p
    p = lambda x: vp(x.data_ptr())
    pairs, st = p(eng.pair_field), eng._stream()
    q = lambda *args: lib.orx_path_threat(eng._pcfg, eng._pst, *args)
    assert q(pairs, 2, 2, p(d), p(m), p(t), p(a), p(w), 65, st) == -22
    assert b"player" in lib.orx_last_error()
    assert q(pairs, 0, 2, None, None, None, None, None, 65, st) == -22
    assert q(pairs, 0, 0, p(d), p(m), p(t), p(a), p(w), 65, st) == -22
    assert b"radius" in lib.orx_last_error()
    assert q(pairs, 0, 16, p(d), p(m), p(t), p(a), p(w), 65, st) == -22
    assert q(pairs, 0, 2, p(d), p(m), p(t), p(a), p(w), 0, st) == -22
    assert q(None, 0, 2, p(d), p(m), p(t), p(a), p(w), 65, st) == -22
    assert b"pairs" in lib.orx_last_error()
    for j, (x, off) in enumerate(((d, 4), (m, 1), (t, 2), (a, 8), (w, 1))):
        args = [p(d), p(m), p(t), p(a), p(w)]
        args[j] = vp(x.data_ptr() + off)
        assert q(pairs, 0, 2, *args, 65, st) == -22, j
        assert b"aligned" in lib.orx_last_error()
    assert lib.orx_path_threat(eng._pcfg, None, pairs, 0, 2, p(d), p(m), p(t), p(a), p(w), 65,
                               st) == -22
    with pytest.raises(_lib.OrxError):
        eng._call("orx_path_threat", pairs, 3, 2, p(d), p(m), p(t), p(a), p(w), 65, st)
    # a bad radius without a window is ignored
    assert q(pairs, 0, 99, p(d), p(m), p(t), p(a), None, 65, st) == 0
    assert all(torch.equal(g, x) for g, x in zip((d, m, t, a), want))


def test_threat_leaves_the_state_and_the_generators_untouched():
    """It reads the state and draws no random words: in stock-seed mode, where
    every game owns its generators, their states stay, and the next ticks equal
    an engine's that never asked."""
    case = CASES["stock"]
    eng, twin = make_engine(case, 65), make_engine(case, 65)
    for e in (eng, twin):
        sc.vc.drive_engine(e, case)
    before = eng.snapshot()
    assert "mt_py" in before and "mt_np" in before
    for player in (0, 1):
        eng.threat(player=player, radius=4)
        eng.flee_moves(player)
    after = eng.snapshot()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    for _ in range(3):
        eng.threat()
        for e in (eng, twin):
            e.step(e.policy(1, 1))
    a, b = eng.snapshot(), twin.snapshot()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["a", "c", "pockets"])
def test_fleeing_on_the_device_gets_what_after_promised(name):
    """env.step(env.flee_moves()) with player 2 and every NPC standing still
    (an all-Stay ``npc_moves`` table): in the games still in progress on the
    same depth and episode, the next ``dist`` of column THREAT_ANY is what
    ``after`` said of the move played."""
    import torch
    from optimax_rogue_amd import Policy, VecEnv
    case = CASES[name]
    cfg, B = case["cfg"], 301
    env = VecEnv(cfg, B, seed=case["seed"], opponent=Policy.Stay, check_actions=False)
    eng = env.engine
    sc.vc.drive_engine(eng, case)
    stay = torch.full((eng.K, B), 5, dtype=torch.int8, device=env.device)
    held = moved = 0
    for tick in range(6):
        dist, move, _, after = env.threat()
        m = env.flee_moves()
        assert torch.equal(m, move[:, 2])
        promised = after.gather(1, m.to(torch.int64)[:, None])[:, 0]
        assert torch.equal(after[:, 5], dist[:, 2])
        depth, episode = eng.p_depth[0].clone(), eng.episode.clone()
        live = eng.status == 1
        obs, reward, done, status = env.step(m, npc_moves=stay)
        same = live & ~done & (status == 1) & (eng.p_depth[0] == depth) & (eng.episode == episode)
        now = env.threat()[0][:, 2]
        bad = same & (now != promised)
        assert not bool(bad.any()), (tick, torch.nonzero(bad).flatten().tolist()[:5])
        held += int(same.sum())
        moved += int((same & (m != 5)).sum())
    assert held >= B and moved >= 10         # (the comparison was made, and on games that moved)


def test_flee_step_threat_in_one_graph():
    """The closed loop -- flee_moves, step, threat -- captured in one graph (a
    linear chain on the capture stream): three replays equal an eager twin.
    The table's first use inside a capture is refused."""
    import torch
    from optimax_rogue_amd import VecEnv
    case = CASES["pockets"]
    B = 200
    mk = lambda: VecEnv(case["cfg"], B, seed=case["seed"], opponent=1, check_actions=False,
                        out_buffers=1)
    env, twin = mk(), mk()
    dev = env.device
    a = torch.full((B,), 5, dtype=torch.int8, device=dev)
    for e in (env, twin):          # (the first step settles the host-side launch blocks)
        e.step(a)
    out = tuple(torch.zeros(shape, dtype=torch.int16, device=dev).to(dt) if dt != torch.uint16
                else torch.zeros(shape, dtype=torch.int16, device=dev).view(dt)
                for dt, shape in zip(dtypes(), shapes(B, 3)))
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    refused = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(refused, stream=s):
            out[0].zero_()
            with pytest.raises(RuntimeError, match="before capturing"):
                env.threat(radius=3, out=out)
    env.threat()                    # builds the table
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            obs, reward, done, status = env.step(env.flee_moves())
            env.threat(radius=3, out=out)
    torch.cuda.current_stream(dev).wait_stream(s)
    moved = 0
    for k in range(3):
        g.replay()
        m = twin.flee_moves()
        moved += int((m != 5).sum())
        t_obs, t_reward, t_done, t_status = twin.step(m)
        t_out = twin.threat(radius=3)
        torch.cuda.synchronize(dev)
        assert torch.equal(obs, t_obs) and torch.equal(status, t_status), k
        assert torch.equal(reward, t_reward) and torch.equal(done, t_done), k
        for x, y in zip(out, t_out):
            assert torch.equal(x.view(torch.int16) if x.dtype == torch.uint16 else x,
                               y.view(torch.int16) if y.dtype == torch.uint16 else y), k
    assert moved > 0 and int((out[0][:, 2] >= 0).sum()) > 0
