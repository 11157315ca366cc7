"""GPU: orx_moves (BatchedEngine.moves / VecEnv.moves / VecEnv.action_mask)
against the host reference ``moves.outcomes(cfg, eng.snapshot(), player)``:
exact equality over every game and column, on the seven configurations of
moves_cases after 12 fused RandomBot ticks, and against the engine's own tick
move by move.

Batch sizes 1, 63, 64, 65 and 1000: a lone game, the tails of a wave (one lane
short, full, one over) and of the 256-thread workgroup (1000 = 3 * 256 + 232),
the smallest shapes at which a one-lane-per-game kernel can go wrong; plus one
run at 4,096 games.  The kernel has two NPC paths (slot scan up to 16 NPCs,
the occupancy grid above: case "dense") and two tile paths (closed form, bank:
case "bank"); every case runs at every size.
"""
import numpy as np
import pytest

import moves_cases as mc

pytestmark = pytest.mark.gpu

CASES = mc.cases()
BATCHES = (1, 63, 64, 65, 1000)
TICKS = 12


def make_engine(case, n_games):
    from optimax_rogue_amd.engine import BatchedEngine
    eng = BatchedEngine(case["cfg"], n_games, seed=case["seed"])
    eng.rollout(TICKS, 1, 1)
    return eng


def check_moves(eng, cfg):
    """Both players, with and without the optional outputs; returns the
    reference's kind arrays."""
    import torch
    from optimax_rogue_amd import moves as mv
    snap = eng.snapshot()
    kinds = []
    for player in (0, 1):
        want = mv.outcomes(cfg, snap, player)
        got = eng.moves(player)
        only = eng.moves_kind(player)
        for t, dt in zip(got + (only,), (torch.uint8, torch.int16, torch.int16, torch.uint8)):
            assert t.dtype == dt and tuple(t.shape) == (eng.B, mv.MOVES_COLS) and t.is_contiguous()
        for name, g, w in zip(("kind", "target", "amount"), got, want):
            assert np.array_equal(g.cpu().numpy(), w), (name, player)
        assert np.array_equal(only.cpu().numpy(), want[0]), ("kind alone", player)
        kinds.append(want[0])
    return kinds


@pytest.mark.parametrize("n_games", BATCHES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_moves_match_outcomes(name, n_games):
    case = CASES[name]
    eng = make_engine(case, n_games)
    kinds = check_moves(eng, case["cfg"])
    if n_games == 1000:
        seen = set(np.unique(np.concatenate(kinds) & 7).tolist())
        assert {1, 2, 3, 5} <= seen, seen            # REST, BLOCKED, STEP, ATTACK_NPC


@pytest.mark.parametrize("name", sorted(CASES))
def test_moves_match_outcomes_at_4096(name):
    from optimax_rogue_amd import moves as mv
    case = CASES[name]
    eng = make_engine(case, 4096)
    kinds = np.concatenate(check_moves(eng, case["cfg"]))
    seen = set(np.unique(kinds & mv.OUT_MASK).tolist())
    assert set(range(1, 7)) <= seen, seen
    assert (kinds & mv.OUT_LETHAL).any()
    if name in mc.EXTENSIONS:
        assert mv.OUT_HEAL in seen


def test_extension_flags_reach_the_kernel():
    """ITEM and COOLDOWN need longer games than 12 ticks: the cases' own tick
    counts, on the engine."""
    from optimax_rogue_amd import moves as mv
    from optimax_rogue_amd.engine import BatchedEngine
    flags = 0
    for name in mc.EXTENSIONS:
        case = CASES[name]
        eng = BatchedEngine(case["cfg"], mc.N_GAMES, seed=case["seed"])
        eng.rollout(case["ticks"], 1, 1)
        for kind in check_moves(eng, case["cfg"]):
            flags |= int(np.bitwise_or.reduce(kind, axis=None))
    assert flags & mv.OUT_ITEM and flags & mv.OUT_COOLDOWN and flags & mv.OUT_LETHAL


def test_moves_out_reuse_and_checks():
    import torch
    case = CASES["base8"]
    eng = make_engine(case, 65)
    want = eng.moves(1)
    dev = eng.device
    mk = lambda dt, shape=(65, 8): torch.full(shape, 77, dtype=dt, device=dev)
    out = (mk(torch.uint8), mk(torch.int16), mk(torch.int16))
    got = eng.moves(1, out=out)
    for g, o, w in zip(got, out, want):
        assert g is o and torch.equal(o, w)
    # every bad argument is refused on the host, before any launch
    k, t, a = out
    for kw in (dict(player=2), dict(player=-1),
               dict(out=(k, t)), dict(out=k),
               dict(out=(mk(torch.int8), t, a)),
               dict(out=(k, mk(torch.int32), a)),
               dict(out=(k, t, mk(torch.uint8))),
               dict(out=(mk(torch.uint8, (64, 8)), t, a)),
               dict(out=(k, mk(torch.int16, (65, 6)), a)),
               dict(out=(k, t, mk(torch.int16, (8, 65)).t())),
               dict(out=(k, t, mk(torch.int16, (528,))[1:521].view(65, 8))),   # misaligned rows
               dict(out=(k.cpu(), t, a)),
               dict(out=(k, t, t))):
        with pytest.raises(ValueError):
            eng.moves(**kw)
    with pytest.raises(ValueError):
        eng.moves_kind(2)


def test_moves_leave_the_state_untouched():
    case = CASES["dense"]
    eng = make_engine(case, 63)
    before = eng.snapshot()
    grid = eng.npc_grid.clone()
    for player in (0, 1):
        eng.moves(player)
        eng.moves_kind(player)
    after = eng.snapshot()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert bool((eng.npc_grid == grid).all())
    # no random words either: the next tick equals an engine's that never asked
    twin = make_engine(case, 63)
    for e in (eng, twin):
        e.step(e.policy(1, 1))
    a, b = eng.snapshot(), twin.snapshot()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_moves_in_stock_seed_mode():
    """It draws no random words, so it works where every game owns its
    generators: the same answers, and the generators' states untouched."""
    from optimax_rogue_amd import EnvConfig
    case = dict(cfg=EnvConfig(width=8, height=8, n_npcs=4, rng=1), seed=1000)
    eng, twin = make_engine(case, 65), make_engine(case, 65)
    before = eng.snapshot()
    kinds = check_moves(eng, case["cfg"])
    assert {2, 3, 5} <= set(np.unique(np.concatenate(kinds) & 7).tolist())
    after = eng.snapshot()
    for k in ("mt_py", "mt_np", "dstore"):
        assert np.array_equal(before[k], after[k]), k
    for e in (eng, twin):
        e.step(e.policy(1, 1))
    a, b = eng.snapshot(), twin.snapshot()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["bank", "character"])
def test_action_mask_and_a_masked_policy(name):
    """VecEnv.action_mask is the reference's mask, and a policy drawing
    uniformly among the allowed moves for 32 ticks never plays a move the
    updater turns into a Stay."""
    import torch
    from optimax_rogue_amd import VecEnv
    from optimax_rogue_amd import moves as mv
    case = CASES[name]
    cfg, B = case["cfg"], 512
    M = mc.n_moves(cfg)
    env = VecEnv(cfg, B, seed=case["seed"], opponent=1, check_actions=True)
    gen = torch.Generator(device=env.device).manual_seed(7)
    refused = played = 0
    for tick in range(32):
        snap = env.engine.snapshot()
        want = mv.outcomes(cfg, snap, 0)
        mask = env.action_mask(0)
        assert mask.dtype == torch.bool and tuple(mask.shape) == (B, M)
        assert np.array_equal(mask.cpu().numpy(), mv.action_mask(want[0], M)), tick
        got = env.moves(0)
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), w), tick
        assert bool(mask[:, 4].all())                                   # Stay is always allowed
        action = torch.multinomial(mask.float(), 1, generator=gen)[:, 0] + 1
        chosen = want[0][np.arange(B), action.cpu().numpy()]
        assert ((chosen & mv.OUT_MASK) != mv.OUT_BLOCKED).all()
        assert not (chosen & mv.OUT_COOLDOWN).any()
        refused += int((~mask).sum())
        env.step(action)
        # the tick agrees where the other player cannot interfere: a STEP moved
        post = env.engine.snapshot()
        a = action.cpu().numpy()
        # (not within two cells, and not one depth above: a descent could land
        # it on the target cell before the learner moves)
        gap = snap["p_depth"][0] - snap["p_depth"][1]
        far = ((gap != 0) & (gap != 1)) | ((gap == 0) & (
            np.abs(snap["p_x"][0] - snap["p_x"][1]) + np.abs(snap["p_y"][0] - snap["p_y"][1]) > 2))
        stepped = ((chosen & mv.OUT_MASK) == mv.OUT_STEP) & far & (snap["status"] == 1)
        dx = np.array([0, 0, 1, 0, -1, 0, 0])[a]
        dy = np.array([0, -1, 0, 1, 0, 0, 0])[a]
        assert (post["p_x"][0][stepped] == (snap["p_x"][0] + dx)[stepped]).all(), tick
        assert (post["p_y"][0][stepped] == (snap["p_y"][0] + dy)[stepped]).all(), tick
        played += int(stepped.sum())
    assert refused > 0 and played > 100
    assert env.bad_actions() == 0


def test_moves_are_what_the_engine_tick_does():
    """The kernel against the engine's own tick (not only numpy): from one
    snapshot, every move of both players played as (m, Stay)."""
    import torch
    case = CASES["base8"]
    cfg = case["cfg"]
    eng = make_engine(case, mc.N_GAMES)
    snap = eng.snapshot()
    total = {}
    for p in (0, 1):
        pred = tuple(t.cpu().numpy() for t in eng.moves(p))
        for m in range(1, mc.n_moves(cfg) + 1):
            eng.load_snapshot(snap)
            actions = torch.from_numpy(mc.actions_for(eng.B, p, m)).to(eng.device)
            _, ev, nev = eng.step(actions, events=True)
            c = mc.compare_move(cfg, snap, pred, p, m, eng.snapshot(), ev.cpu().numpy(),
                                nev.cpu().numpy())
            for k, v in c.items():
                total[k] = min(total.get(k, v), v) if k == "games" else total.get(k, 0) + v
    assert total["games"] >= 0.95 * mc.N_GAMES
    for outcome in ("REST", "BLOCKED", "STEP", "DESCEND", "ATTACK_NPC", "ATTACK_PLAYER"):
        assert total[outcome] >= 100, total
    assert total["LETHAL"] >= 50, total


def test_step_then_moves_in_one_graph():
    """env.step(a) followed by env.moves(out=...) captured in one graph (a
    linear chain on the capture stream): each of three replays equals the
    reference on the state that replay left."""
    import torch
    from optimax_rogue_amd import VecEnv
    from optimax_rogue_amd import moves as mv
    case = CASES["base6"]
    cfg, B = case["cfg"], 200
    env = VecEnv(cfg, B, seed=case["seed"], opponent=1, check_actions=False, out_buffers=1)
    dev = env.device
    gen = torch.Generator().manual_seed(5)
    plays = torch.randint(1, 6, (12, B), generator=gen, dtype=torch.int64).to(dev)
    a = plays[0].clone()
    for k in range(8):             # (the first step settles the host-side launch blocks)
        env.step(plays[k])
    out = tuple(torch.zeros((B, 8), dtype=dt, device=dev)
                for dt in (torch.uint8, torch.int16, torch.int16))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            env.step(a)
            env.moves(0, out=out)
    torch.cuda.current_stream(dev).wait_stream(s)
    seen = 0
    for k in range(8, 11):
        a.copy_(plays[k])
        g.replay()
        torch.cuda.synchronize(dev)
        want = mv.outcomes(cfg, env.engine.snapshot(), 0)
        for t, w in zip(out, want):
            assert np.array_equal(t.cpu().numpy(), w), k
        seen |= int(np.bitwise_or.reduce(want[0] & mv.OUT_MASK == mv.OUT_ATTACK_NPC, axis=None))
    assert seen
