"""GPU: orx_explore_update / orx_explore_seek (BatchedEngine.explore,
explore_seek, explore_map, explore_forget; VecEnv.explore_moves) against the
host reference ``optimax_rogue_amd.explore``, bit for bit, on the four
configurations of explore_cases driven through runs of ticks, so that the maps
are cleared (descents, new episodes) and filled again.

Every launch stands alone: the reference's map and key BEFORE the call are
uploaded, the kernel's map, key, ``gained`` and planes AFTER it are compared.
Batch sizes 1, 63, 65 and 200: a lone game, a partial workgroup, a workgroup
plus one game (64 games per workgroup of the update, 4 of the seek), several
workgroups.  Every buffer the kernels write -- and the map, which they update
in place -- is a view into a poisoned buffer (tests/guarded.py), under both
poisons, at a 16-byte boundary and past one (the planes by 1 byte: the byte
path; the words by 4; the key and the seek's rows by 16).  The planes hold
orx_view's output first; a cell the update skipped keeps its view code, which
has neither bit 6 nor bit 7.  The outputs not asked for keep their poison.
"""
import numpy as np
import pytest

import explore_cases as ec
from guarded import POISONS, Guarded

pytestmark = pytest.mark.gpu

CASES = ec.cases()
BATCHES = (1, 63, 65, 200)
# case -> (updates, engine ticks between two of them, radii)
RUNS = {"m": (10, 6, (1, 5, 15)), "x": (8, 4, (1, 5, 15)), "a": (8, 5, (1, 5, 15)), "e": (5, 2, (5,))}
# the update's outputs asked for, (gained, cells, health), and the seek's (dist, move, target)
UPDATE_MODES = ((True, True, True), (False, True, False), (True, False, False), (False, True, True))
SEEK_MODES = ((True, True, True), (True, False, False), (False, True, False), (False, False, True),
              (True, True, False), (False, True, True), (True, False, True))
# (poison, the words' skew, the planes' skew, the 16-byte rows' skew)
PLACEMENTS = tuple((poison, 4 * k, k, 16 * k) for poison in POISONS for k in (0, 1))


def make_engine(case, n_games, **kw):
    from optimax_rogue_amd.engine import BatchedEngine
    return BatchedEngine(case["cfg"], n_games, seed=case["seed"], **kw)


def upload(g, a):
    """numpy ``a`` into the guarded tensor, bit for bit."""
    import torch
    as_int = {np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype)
    t = torch.from_numpy(np.ascontiguousarray(a).view(as_int)).to(g.out.device)
    (g.out.view(torch.int32) if a.dtype == np.uint32 else g.out).copy_(t)


def poisoned(shape, dtype, poison):
    """What an output nobody wrote holds."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.full(n, poison, np.uint8).view(dtype).reshape(shape)


def check_update(eng, cfg, snap, radius, player, memory, key, rows, what, turn):
    """orx_explore_update of one engine state from the map (memory, key): every
    placement, the output modes in turn, against ``explore.update``.  Returns
    the reference's (memory, key) after the call, and one kernel-written pair
    of guarded buffers for the seek."""
    import torch
    from optimax_rogue_amd import explore, view
    from optimax_rogue_amd.engine import _ptr
    B, V = eng.B, 2 * radius + 1
    H, WW = int(cfg.height), explore.words(cfg.width)
    cells, hp = view.render_view(snap, cfg, player, radius, bank=eng.bank, health=True)
    after_m, after_k, want_c, want_h = memory.copy(), key.copy(), cells.copy(), hp.copy()
    want_g = explore.update(after_m, after_k, snap, cfg, player, radius, rows, want_c, want_h)
    assert not (cells & 0xC0).any()
    for n, (poison, word_skew, cell_skew, row_skew) in enumerate(PLACEMENTS):
        with_g, with_c, with_h = UPDATE_MODES[(n + turn) % len(UPDATE_MODES)]
        msg = f"{what} R={radius} player {player} poison {poison:#x} skew {cell_skew}"
        gr = Guarded(eng.device, torch.uint32, (B, V), poison, word_skew)
        gm = Guarded(eng.device, torch.uint32, (B, H, WW), poison, word_skew)
        gk = Guarded(eng.device, torch.int32, (B, 4), poison, row_skew)
        gg = Guarded(eng.device, torch.int32, (B,), poison, word_skew)
        gc = Guarded(eng.device, torch.uint8, (B, V, V), poison, cell_skew)
        gh = Guarded(eng.device, torch.uint8, (B, V, V), poison, cell_skew)
        upload(gr, rows), upload(gm, memory), upload(gk, key)
        eng.view(radius, player=player, health=True, out=(gc.out, gh.out))
        eng._call("orx_explore_update", player, radius, _ptr(gr.out), _ptr(gm.out), _ptr(gk.out),
                  _ptr(gg.out) if with_g else None, _ptr(gc.out) if with_c else None,
                  _ptr(gh.out) if with_h else None, B, eng._stream())
        gr.check(rows, msg + " rows (an input)")
        gm.check(after_m, msg + " memory")
        gk.check(after_k, msg + " key")
        gg.check(want_g if with_g else poisoned((B,), np.int32, poison), msg + " gained")
        gc.check(want_c if with_c else cells, msg + " cells")
        gh.check(want_h if with_h else hp, msg + " health")
    return after_m, after_k, (gm, gk)


def check_seek(eng, cfg, snap, player, memory, key, what, turn, on_device=None):
    """orx_explore_seek of one engine state and map: every placement, the NULL
    forms in turn, against ``explore.seek``."""
    import torch
    from optimax_rogue_amd import explore
    from optimax_rogue_amd.engine import _ptr
    B = eng.B
    want = explore.seek(memory, key, snap, cfg, player, bank=eng.bank)
    pairs = eng.pair_field
    for n, (poison, word_skew, _, row_skew) in enumerate(PLACEMENTS):
        mode = SEEK_MODES[(n + turn) % len(SEEK_MODES)]
        msg = f"{what} seek player {player} poison {poison:#x} skew {row_skew} outputs {mode}"
        if on_device is not None and n == 0:
            gm, gk = on_device                       # (what the update kernel itself wrote)
        else:
            gm = Guarded(eng.device, torch.uint32, memory.shape, poison, word_skew)
            gk = Guarded(eng.device, torch.int32, (B, 4), poison, row_skew)
            upload(gm, memory), upload(gk, key)
        outs = [Guarded(eng.device, dt, (B, 4), poison, skew) for dt, skew in
                ((torch.int32, row_skew), (torch.int8, word_skew), (torch.int32, row_skew))]
        eng._call("orx_explore_seek", _ptr(pairs), player, _ptr(gm.out), _ptr(gk.out),
                  *(_ptr(g.out) if on else None for g, on in zip(outs, mode)), B, eng._stream())
        gm.check(memory, msg + " memory (an input)")
        gk.check(key, msg + " key (an input)")
        for g, w, on, nm in zip(outs, want, mode, ("dist", "move", "target")):
            g.check(w if on else poisoned((B, 4), w.dtype, poison), f"{msg} {nm}")
    return want


@pytest.mark.parametrize("n_games", BATCHES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_update_and_seek_match_the_reference(name, n_games):
    from optimax_rogue_amd import explore, sight, view
    case = CASES[name]
    cfg = case["cfg"]
    updates, stride, radii = RUNS[name]
    eng = make_engine(case, n_games)
    W, H = int(cfg.width), int(cfg.height)
    maps = {(R, p): explore.empty(n_games, W, H) for R in radii for p in (0, 1)}
    cleared = gained = absent = found = turn = 0
    for u in range(updates):
        for _ in range(stride if u else 0):
            eng.step(eng.policy(*case["policies"]))
        snap = eng.snapshot()
        for R in radii:
            for p in (0, 1):
                what = f"case {name} B={n_games} update {u}"
                memory, key = maps[R, p]
                stale = ~explore.valid(key, snap, p)
                cleared += int((stale & (key[:, 3] >= 0)).sum())
                if R == radii[0]:
                    # the map of an earlier state: stale keys give ABSENT
                    check_seek(eng, cfg, snap, p, memory, key, what + " (before)", turn)
                rows = sight.pack_rows(sight.visible_of(
                    view.render_view(snap, cfg, p, R, bank=eng.bank)))
                memory, key, dev = check_update(eng, cfg, snap, R, p, memory, key, rows, what, turn)
                maps[R, p] = (memory, key)
                dist = check_seek(eng, cfg, snap, p, memory, key, what, turn, on_device=dev)[0]
                gained += int(key[:, 3].sum())
                absent += int((dist[:, :2] == -2).sum())
                found += int((dist[:, :2] > 0).sum())
                turn += 1
    assert gained > 0 and found > 0
    if n_games == ec.N_GAMES:
        assert absent > 0
        if name != "x":
            assert cleared > 0        # (maps crossed a descent or a new episode)


def test_rows_outside_the_grid_and_the_window_change_nothing():
    """Row words of all ones: the bits >= V and those of cells outside the grid
    are ignored -- the maps equal the reference's, so no game wrote into its
    neighbour's, and the guards round the buffer are intact."""
    from optimax_rogue_amd import explore
    for name, n_games in (("e", 65), ("x", 63)):
        case = CASES[name]
        cfg = case["cfg"]
        eng = make_engine(case, n_games)
        for _ in range(3):
            eng.step(eng.policy(*case["policies"]))
        snap = eng.snapshot()
        for R in (1, 15):
            rows = np.full((n_games, 2 * R + 1), 0xFFFFFFFF, np.uint32)
            memory, key = explore.empty(n_games, cfg.width, cfg.height)
            memory, key, _ = check_update(eng, cfg, snap, R, 0, memory, key, rows,
                                          f"case {name} all-ones rows", 0)
            known = explore.unpack(memory, cfg.width)
            x, y = snap["p_x"][0], snap["p_y"][0]
            for b in range(n_games):
                box = np.zeros_like(known[b])
                box[max(0, x[b] - R):x[b] + R + 1, max(0, y[b] - R):y[b] + R + 1] = True
                assert np.array_equal(known[b], box), (name, R, b)


def test_the_engines_own_map_through_a_run():
    """BatchedEngine.explore / explore_seek / explore_map chained over ticks
    (the kernel's own map each time) against the reference chained the same
    way; ``out=`` reuse; explore_forget; load_snapshot forgets."""
    import torch
    from optimax_rogue_amd import explore, sight, view
    case = CASES["m"]
    cfg, B, R = case["cfg"], 65, case["radius"]
    eng = make_engine(case, B)
    maps = [explore.empty(B, cfg.width, cfg.height) for _ in (0, 1)]
    V = 2 * R + 1
    outs = (torch.empty(B, dtype=torch.int32, device=eng.device),
            torch.full((B, V, V), 255, dtype=torch.uint8, device=eng.device),
            torch.full((B, V, V), 255, dtype=torch.uint8, device=eng.device))
    seek_outs = tuple(torch.empty((B, 4), dtype=dt, device=eng.device)
                      for dt in (torch.int32, torch.int8, torch.int32))
    for tick in range(30):
        if tick:
            eng.step(eng.policy(*case["policies"]))
        snap = eng.snapshot()
        for p in (0, 1):
            cells, hp = view.render_view(snap, cfg, p, R, bank=eng.bank, health=True)
            rows = sight.pack_rows(sight.visible_of(cells))
            memory, key = maps[p]
            want_g = explore.update(memory, key, snap, cfg, p, R, rows, cells, hp)
            if tick % 3 == 0:
                got = eng.explore(R, player=p, view=True, health=True, out=outs)
                assert all(a is b for a, b in zip(got, outs))
            elif tick % 3 == 1:
                got = eng.explore(R, player=p, view=True, health=True)
            else:
                got = (eng.explore(R, player=p),) + eng.explore(R, player=p, view=True)[1:] + (None,)
                assert got[0].dtype == torch.int32 and tuple(got[0].shape) == (B,)
            assert np.array_equal(got[0].cpu().numpy(), want_g), (tick, p)
            assert np.array_equal(got[1].cpu().numpy(), cells), (tick, p)
            if got[2] is not None:
                assert np.array_equal(got[2].cpu().numpy(), hp), (tick, p)
            mem_t, key_t = eng.explore_map(p)
            assert mem_t.dtype == torch.uint32 and tuple(mem_t.shape) == memory.shape
            assert np.array_equal(mem_t.view(torch.int32).cpu().numpy().view(np.uint32), memory)
            assert np.array_equal(key_t.cpu().numpy(), key), (tick, p)
            want = explore.seek(memory, key, snap, cfg, p, bank=eng.bank)
            got = eng.explore_seek(p, out=seek_outs) if tick % 2 else eng.explore_seek(p)
            for g, w in zip(got, want):
                assert np.array_equal(g.cpu().numpy(), w), (tick, p)
    # forgetting one player's map, then both
    assert int(eng.explore_map(0)[1][:, 3].min()) >= 0
    eng.explore_forget(0)
    assert bool((eng.explore_map(0)[1] == -1).all()) and not bool(eng.explore_map(0)[0].view(torch.int32).any())
    assert int(eng.explore_map(1)[1][:, 3].min()) >= 0
    d = eng.explore_seek(0)[0]
    assert bool((d == -2).all())
    eng.explore(R, player=0)
    eng.load_snapshot(eng.snapshot())
    for p in (0, 1):
        assert bool((eng.explore_map(p)[1] == -1).all())
        assert not bool(eng.explore_map(p)[0].view(torch.int32).any())
    # every bad argument is refused on the host, before any launch
    before = [t.clone() for t in outs]
    for kw in (dict(radius=0), dict(radius=16), dict(radius=R, player=2), dict(radius=R, health=True),
               dict(radius=R, out=outs), dict(radius=R, view=True, out=outs[:1]),
               dict(radius=R, view=True, out=(outs[0], outs[1][:, :, :4])),
               dict(radius=R, view=True, health=True, out=(outs[0], outs[1], outs[1])),
               dict(radius=R, out=torch.empty(B, dtype=torch.int32))):
        with pytest.raises(ValueError):
            eng.explore(**kw)
    for kw in (dict(player=2), dict(out=seek_outs[:2]),
               dict(out=(seek_outs[0], seek_outs[1], seek_outs[0])),
               dict(out=(seek_outs[0], seek_outs[1], seek_outs[2].to(torch.int16)))):
        with pytest.raises(ValueError):
            eng.explore_seek(**kw)
    assert all(torch.equal(a, b) for a, b in zip(before, outs))


def test_explore_leaves_the_state_untouched():
    case = CASES["m"]
    eng, twin = make_engine(case, 63), make_engine(case, 63)
    for e in (eng, twin):
        for _ in range(5):
            e.step(e.policy(*case["policies"]))
    before = eng.snapshot()
    for p in (0, 1):
        eng.explore(2, player=p, view=True, health=True)
        eng.explore_seek(p)
    after = eng.snapshot()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    # no random words either: the next ticks equal an engine's that never looked
    for e in (eng, twin):
        e.step(e.policy(*case["policies"]))
    a, b = eng.snapshot(), twin.snapshot()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_the_first_map_is_not_allocated_under_capture():
    import torch
    case = CASES["m"]
    eng = make_engine(case, 8)
    eng.step(eng.policy(1, 1))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=eng.device)
    s.wait_stream(torch.cuda.current_stream(eng.device))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            with pytest.raises(RuntimeError, match="before capturing"):
                eng.explore_map(0)
            eng.step(eng.policy(1, 1))
    torch.cuda.current_stream(eng.device).wait_stream(s)
    assert not eng._explore_maps


def test_the_closed_loop_in_one_graph():
    """env.step(a), env.explore(2), env.explore_seek() and the next actions out
    of its moves, captured in one graph (a linear chain on the capture
    stream): replays against an eager twin."""
    import torch
    from optimax_rogue_amd import VecEnv
    case = CASES["m"]
    B = 200
    mk = lambda: VecEnv(case["cfg"], B, seed=case["seed"], opponent=1, check_actions=False,
                        out_buffers=1)
    env, twin = mk(), mk()
    dev = env.device
    a = torch.full((B,), 5, dtype=torch.int64, device=dev)
    b = a.clone()
    for e in (env, twin):          # (the first calls settle the launch blocks, the map, the table)
        e.step(a)
        e.explore(2)
        e.explore_seek()
    gained = torch.zeros(B, dtype=torch.int32, device=dev)
    rows = tuple(torch.zeros((B, 4), dtype=dt, device=dev)
                 for dt in (torch.int32, torch.int8, torch.int32))

    def choose(dist, move):
        stairs = torch.where(dist[:, 1] > 0, move[:, 1], 5)
        return torch.where(dist[:, 0] > 0, move[:, 0], stairs).to(torch.int64)

    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            obs, reward, done, status = env.step(a)
            env.explore(2, out=gained)
            env.explore_seek(out=rows)
            a.copy_(choose(rows[0], rows[1]))
    torch.cuda.current_stream(dev).wait_stream(s)
    total = descents = 0
    for k in range(40):
        g.replay()
        t_obs, t_reward, t_done, t_status = twin.step(b)
        t_gained = twin.explore(2)
        t_rows = twin.explore_seek()
        b = choose(t_rows[0], t_rows[1])
        torch.cuda.synchronize(dev)
        assert torch.equal(obs, t_obs) and torch.equal(status, t_status), k
        assert torch.equal(reward, t_reward) and torch.equal(done, t_done), k
        assert torch.equal(gained, t_gained), k
        assert all(torch.equal(x, y) for x, y in zip(rows, t_rows)), k
        assert torch.equal(a, b) and torch.equal(b.to(torch.int8), twin.explore_moves()), k
        total += int(gained.sum())
        descents += int((obs[:, 2] > 0).sum())
    for p_env, p_twin in zip(env.engine.explore_map(0), twin.engine.explore_map(0)):
        assert torch.equal(p_env.view(torch.int32), p_twin.view(torch.int32))
    assert total > 0 and descents > 0      # (the explorer explores, then takes the staircase)


def test_the_explorer_on_the_device():
    """Player 1 alone on its depth of the 12 x 10 bank (Separated start, no
    NPCs, no tick limit; player 2 Stays): following explore_moves' frontier
    move for at most 4 * W * H ticks leaves no frontier in any game, and what
    it knows covers every cell at finite pair distance from its start."""
    import torch
    from optimax_rogue_amd import EnvConfig, VecEnv, explore
    from optimax_rogue_amd.path import PATH_UNREACHABLE, SEEK_ABSENT
    layouts = CASES["m"]["cfg"].layouts
    cfg = EnvConfig(width=12, height=10, n_npcs=0, max_ticks=0, start_mode=2, p1_depth=1,
                    p2_depth=0, layouts=layouts)
    B, W, H = 200, 12, 10
    env = VecEnv(cfg, B, seed=77, opponent=None, check_actions=False)
    eng = env.engine
    first = eng.snapshot()
    start = first["p_x"][0].astype(np.int64) * H + first["p_y"][0]
    actions = torch.full((B, 2), 5, dtype=torch.int8, device=env.device)
    for ticks in range(4 * W * H + 1):
        env.explore(2)
        dist, move, _ = env.explore_seek()
        go = dist[:, 0] > 0
        if not bool(go.any()):
            break
        # explore_moves is the frontier's move wherever one is left
        assert torch.equal(env.explore_moves()[go], move[:, 0][go])
        actions[:, 0] = torch.where(go, move[:, 0], 5)
        env.step(actions)
    else:
        raise AssertionError(f"the explorer did not end within {4 * W * H} ticks")
    snap = eng.snapshot()
    assert (snap["p_depth"][0] == 1).all() and (snap["episode"] == 0).all()
    assert (snap["p_layout"][0] == first["p_layout"][0]).all()
    assert bool((dist[:, 0] == SEEK_ABSENT).all())
    memory, key = eng.explore_map(0)
    known = explore.unpack(memory.view(torch.int32).cpu().numpy().view(np.uint32), W)
    assert np.array_equal(key[:, 3].cpu().numpy(), known.sum(axis=(1, 2)))
    pairs = eng.bank.pair_field()
    reachable = (pairs[first["p_layout"][0].astype(np.int64), start] < PATH_UNREACHABLE)
    assert reachable.any(axis=1).all() and not (reachable.reshape(B, W, H) & ~known).any()
    print(f"explorer on the device: {ticks} ticks of {W * H} cells")
