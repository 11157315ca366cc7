"""GPU: orx_route_planes / orx_route (BatchedEngine.route_planes, explore_route,
explore_route_moves; VecEnv's pass-throughs) against the host reference
``optimax_rogue_amd.route``, bit for bit, on engine states with the engine's
own maps, through runs of explore_cases' four configurations.

Batches of 1, 65 and 301 games: a lone game, workgroups of four games plus
one, many workgroups.  Both players; goals of four classes (a known Ground
cell, an unknown cell, a Wall, none).  Every output is a view into a poisoned
buffer (tests/guarded.py), under both poisons, at a 16-byte boundary and past
one, each NULL-output form in turn; ``memory`` and ``key`` are unchanged after
the call and the state is untouched.  Then the shapes at which the kernel takes
another path: two map words per row (40 x 8), H > 64 with three words (96 x
80), a map whose planes do not fit LDS (8 x 4096 and 4 x 16384: the reached
planes alone are staged), and the largest bank grid, a 256 x 256 serpentine
whose length comes from its construction, in a process with a time limit of
its own.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import explore_cases as ec
import route_cases as rc
from guarded import POISONS, Guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ec.cases()
BATCHES = (1, 65, 301)
RUNS = {"m": (6, 6), "x": (5, 5), "a": (5, 6), "e": (4, 3)}     # case -> (updates, ticks between)
MODES = ((True, True, True), (True, False, False), (False, True, False), (False, False, True),
         (True, True, False), (False, True, True), (True, False, True))
# (poison, the words' skew, the 16-byte rows' skew)
PLACEMENTS = tuple((poison, 4 * k, 16 * k) for poison in POISONS for k in (0, 1))


def upload(g, a):
    """numpy ``a`` into the guarded tensor, bit for bit."""
    import torch
    as_int = {np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype)
    t = torch.from_numpy(np.ascontiguousarray(a).view(as_int)).to(g.out.device)
    (g.out.view(torch.int32) if a.dtype == np.uint32 else g.out).copy_(t)


def poisoned(shape, dtype, poison):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.full(n, poison, np.uint8).view(dtype).reshape(shape)


def host(t):
    import torch
    if t.dtype == torch.uint32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    return t.cpu().numpy()


def check_route(eng, cfg, snap, player, memory, key, goal, what, turn):
    """orx_route of one engine state and map: every placement, the NULL forms
    in turn, against ``route.route``.  Returns the reference's rows."""
    import torch
    from optimax_rogue_amd import route
    from optimax_rogue_amd.engine import _ptr
    B = eng.B
    want = route.route(memory, key, snap, cfg, player, goal=goal, bank=eng.bank)
    for n, (poison, word_skew, row_skew) in enumerate(PLACEMENTS):
        mode = MODES[(n + turn) % len(MODES)]
        msg = f"{what} route player {player} poison {poison:#x} skew {row_skew} outputs {mode}"
        gm = Guarded(eng.device, torch.uint32, memory.shape, poison, word_skew)
        gk = Guarded(eng.device, torch.int32, (B, 4), poison, row_skew)
        upload(gm, memory), upload(gk, key)
        gg = None
        if goal is not None:
            gg = Guarded(eng.device, torch.int32, (B,), poison, word_skew)
            upload(gg, goal)
        outs = [Guarded(eng.device, dt, (B, 4), poison, skew) for dt, skew in
                ((torch.int32, row_skew), (torch.int8, word_skew), (torch.int32, row_skew))]
        eng._call("orx_route", _ptr(eng.route_planes), player, _ptr(gm.out), _ptr(gk.out),
                  None if gg is None else _ptr(gg.out),
                  *(_ptr(g.out) if on else None for g, on in zip(outs, mode)), B, eng._stream())
        gm.check(memory, msg + " memory (an input)")
        gk.check(key, msg + " key (an input)")
        if gg is not None:
            gg.check(goal, msg + " goal (an input)")
        for g, w, on, nm in zip(outs, want, mode, ("dist", "move", "target")):
            g.check(w if on else poisoned((B, 4), w.dtype, poison), f"{msg} {nm}")
    return want


@pytest.mark.parametrize("n_games", BATCHES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_route_matches_the_reference(name, n_games):
    import torch
    from optimax_rogue_amd import explore, route
    from optimax_rogue_amd.engine import BatchedEngine
    case = CASES[name]
    cfg, R = case["cfg"], case["radius"]
    updates, stride = RUNS[name]
    eng = BatchedEngine(cfg, n_games, seed=case["seed"])
    W, H = int(cfg.width), int(cfg.height)
    rs = np.random.RandomState(n_games + W)
    seen = {}
    turn = 0
    outs = tuple(torch.empty((n_games, 4), dtype=dt, device=eng.device)
                 for dt in (torch.int32, torch.int8, torch.int32))
    for u in range(updates):
        for _ in range(stride if u else 0):
            eng.step(eng.policy(*case["policies"]))
        for p in (0, 1):
            what = f"case {name} B={n_games} update {u}"
            if u:
                # the map of an earlier state: stale keys give ABSENT
                snap = eng.snapshot()
                memory, key = (host(t) for t in eng.explore_map(p))
                check_route(eng, cfg, snap, p, memory, key, None, what + " (before)", turn)
            eng.explore(R, player=p)
            snap = eng.snapshot()
            memory, key = (host(t) for t in eng.explore_map(p))
            tiles = ec.tiles_of(cfg, snap, p, eng.bank)
            goal, classes = rc.draw_goals(rs, tiles, explore.unpack(memory, W), H)
            want = check_route(eng, cfg, snap, p, memory, key, goal, what, turn)
            for c in classes:
                seen[c] = seen.get(c, 0) + 1
            for col in range(3):
                seen[col, "reached"] = seen.get((col, "reached"), 0) + int((want[0][:, col] > 0).sum())
            # the engine's own map, through the engine's methods; ``out=`` reuse
            goal_t = torch.from_numpy(goal.astype(np.int64)).to(eng.device)
            got = eng.explore_route(p, goal=goal_t, out=outs) if u % 2 else eng.explore_route(p, goal=goal_t)
            assert not u % 2 or all(a is b for a, b in zip(got, outs))
            for g, w in zip(got, want):
                assert np.array_equal(host(g), w), what
            no_goal = eng.explore_route(p)
            assert np.array_equal(host(no_goal[0])[:, :2], want[0][:, :2]), what
            assert bool((no_goal[0][:, 2] == -2).all()) and bool((no_goal[2][:, 2] == -1).all())
            assert np.array_equal(host(eng.explore_route_moves(p)), route.router_moves(want[0], want[1]))
            for k, v in eng.snapshot().items():
                assert np.array_equal(v, snap[k]), (what, "state changed", k)
            for t, a in zip(eng.explore_map(p), (memory, key)):
                assert np.array_equal(host(t), a), (what, "map changed")
            turn += 1
    if n_games >= 65 and name != "e":       # (4 x 4 is known at a glance: nothing to walk to)
        assert seen[0, "reached"] > 0 and seen[1, "reached"] > 0
        assert all(seen.get(c, 0) > 0 for c in rc.GOAL_CLASSES) and seen[2, "reached"] > 0, seen
    assert eng._pair_field is None


@pytest.mark.parametrize("W,H,L", ((40, 8, 3), (96, 80, 2)))
def test_planes_and_routes_on_wider_and_taller_grids(W, H, L):
    """orx_route_planes equals ``route.planes`` (two words per row; three, and
    more rows than a wave has lanes), and the router's run on the same bank
    equals the reference in every state."""
    import torch
    from optimax_rogue_amd import DungeonBank, EnvConfig, VecEnv, explore, route
    bank = DungeonBank.random(W, H, L, seed=W + H, wall_p=0.2, connected=True)
    cfg = EnvConfig(width=W, height=H, n_npcs=0, max_ticks=0, start_mode=2, p1_depth=1, p2_depth=0,
                    layouts=bank.layouts)
    env = VecEnv(cfg, 9, seed=5, opponent=None, check_actions=False)
    eng = env.engine
    planes = eng.route_planes
    assert planes.dtype == torch.uint32 and tuple(planes.shape) == (L, 2, H, (W + 31) // 32)
    assert np.array_equal(host(planes), route.planes(bank.layouts))
    assert eng.route_planes is planes
    actions = torch.full((9, 2), 5, dtype=torch.int8, device=env.device)
    rs = np.random.RandomState(W)
    reached = 0
    for tick in range(40):
        env.explore(5)
        snap = eng.snapshot()
        memory, key = (host(t) for t in eng.explore_map(0))
        goal, _ = rc.draw_goals(rs, ec.tiles_of(cfg, snap, 0, eng.bank), explore.unpack(memory, W), H)
        want = route.route(memory, key, snap, cfg, 0, goal=goal, bank=eng.bank)
        got = env.explore_route(goal=torch.from_numpy(goal).to(env.device))
        for g, w in zip(got, want):
            assert np.array_equal(host(g), w), (W, H, tick)
        reached += int((want[0][:, :3] > 0).sum())
        actions[:, 0] = torch.where(got[0][:, 0] > 0, got[1][:, 0], 5)
        env.step(actions)
    assert reached > 0 and eng._pair_field is None


@pytest.mark.parametrize("W,H", ((8, 4096), (4, 16384)))
def test_a_map_whose_planes_do_not_fit_lds(W, H):
    """No bank, a narrow room thousands of rows tall: five planes of H words do
    not fit 64 KiB, so the kernel stages the reached planes alone (at 4 x 16384
    they take 128 KiB).  The player knows 400 rows of it."""
    import torch
    from optimax_rogue_amd import EnvConfig, explore, route
    from optimax_rogue_amd.engine import BatchedEngine
    cfg = EnvConfig(width=W, height=H, n_npcs=0)
    B = 3
    eng = BatchedEngine(cfg, B, seed=3)
    mid = H // 2
    eng.p_x[0, :] = torch.tensor([1, W - 2, 1], dtype=torch.int32)
    eng.p_y[0, :] = torch.tensor([mid, mid + 150, 1], dtype=torch.int32)
    eng.st_x[0, :], eng.st_y[0, :] = W - 2, mid - 120
    snap = eng.snapshot()
    known = np.zeros((B, W, H), bool)
    known[:2, :, mid - 200:mid + 200] = True
    known[2, :, :60] = True                  # (the third game: by the top wall, no staircase seen)
    memory = explore.pack(known)
    key = np.stack([snap["episode"], snap["p_depth"][0], snap["tick"], known.sum(axis=(1, 2))],
                   axis=1).astype(np.int32)
    goal = np.array([(W - 2) * H + mid + 190, 1 * H + mid - 199, 2 * H + 500], np.int32)
    want = check_route(eng, cfg, snap, 0, memory, key, goal, f"{W} x {H}", 0)
    assert want[0][0].tolist()[:3] == [199, 120 + W - 3, 190 + W - 3]
    assert want[0][2].tolist()[:3] == [58, -2, -1]


def test_the_largest_grid_in_a_process_of_its_own():
    """B = 2 on a fully known 256 x 256 serpentine, the player at one end and
    the goal (the staircase) at the other; the second game's map is empty.  A
    wrong LDS size or an unbounded loop shows here: the run has a time limit of
    its own."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "route_serpentine.py")],
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "serpentine 256 x 256: ok" in r.stdout, r.stdout


def test_the_pair_table_is_not_needed():
    from optimax_rogue_amd import route
    from optimax_rogue_amd.engine import BatchedEngine
    case = CASES["m"]
    eng = BatchedEngine(case["cfg"], 65, seed=case["seed"])
    eng.PAIR_FIELD_MAX_BYTES = 0
    for _ in range(6):
        eng.step(eng.policy(*case["policies"]))
        eng.explore(2)
    with pytest.raises(ValueError, match="PAIR_FIELD_MAX_BYTES"):
        eng.explore_seek()
    got = eng.explore_route()
    memory, key = (host(t) for t in eng.explore_map(0))
    want = route.route(memory, key, eng.snapshot(), case["cfg"], 0, bank=eng.bank)
    for g, w in zip(got, want):
        assert np.array_equal(host(g), w)
    assert eng._pair_field is None


def router_env(B):
    from optimax_rogue_amd import DungeonBank, EnvConfig, VecEnv
    bank = DungeonBank.random(24, 20, 4, seed=2420, wall_p=0.3, connected=True)
    cfg = EnvConfig(width=24, height=20, n_npcs=0, max_ticks=0, start_mode=2, p1_depth=1, p2_depth=0,
                    layouts=bank.layouts)
    return VecEnv(cfg, B, seed=11, opponent=3, check_actions=False, out_buffers=1)    # (Policy.Stay)


def test_the_router_on_the_device():
    """``step(explore_route_moves())`` then ``explore(radius)``: within 4 * W *
    H ticks every game has been left without a frontier cell to walk to (it
    then takes the staircase it knows a way to, and starts on the next depth)."""
    import torch
    B, W, H, R = 64, 24, 20, 3
    env = router_env(B)
    env.explore(R)
    finished = torch.zeros(B, dtype=torch.bool, device=env.device)
    descended = torch.zeros(B, dtype=torch.bool, device=env.device)
    for ticks in range(4 * W * H + 1):
        dist = env.explore_route()[0]
        finished |= dist[:, 0] < 0
        if bool(finished.all()):
            break
        env.step(env.explore_route_moves().to(torch.int64))
        env.explore(R)
        descended |= env.engine.p_depth[0] > 1
    else:
        raise AssertionError(f"the router did not end within {4 * W * H} ticks")
    assert env.engine._pair_field is None
    print(f"router on the device: {ticks} ticks of {W * H} cells; {int(descended.sum())} games "
          "had descended meanwhile")


def test_the_router_loop_in_one_graph():
    """The same loop captured in one HIP graph after a warm call gives the
    eager loop's states; the first ``route_planes`` under capture raises."""
    import torch
    B, R = 64, 3
    env, twin, cold = router_env(B), router_env(B), router_env(8)
    dev = env.device
    for e in (env, twin):
        e.step(torch.full((B,), 5, dtype=torch.int64, device=dev))
        e.explore(R)
        e.explore_route_moves()
    a = torch.full((B,), 5, dtype=torch.int64, device=dev)
    cold.step(torch.full((8,), 5, dtype=torch.int64, device=dev))
    cold.explore(R)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            with pytest.raises(RuntimeError, match="before capturing"):
                cold.engine.route_planes
            a.copy_(env.explore_route_moves())
            env.step(a)
            env.explore(R)
    torch.cuda.current_stream(dev).wait_stream(s)
    assert cold.engine._route_planes is None
    for k in range(60):
        g.replay()
        twin.step(twin.explore_route_moves().to(torch.int64))
        twin.explore(R)
    torch.cuda.synchronize(dev)
    x, y = env.engine.snapshot(), twin.engine.snapshot()
    for k in x:
        assert np.array_equal(x[k], y[k]), k
    for p_env, p_twin in zip(env.engine.explore_map(0), twin.engine.explore_map(0)):
        assert torch.equal(p_env.view(torch.int32), p_twin.view(torch.int32))
    assert (x["tick"] > 0).all()
