"""GPU: the tick with the NPCs' moves supplied by the caller (include/orx_npc.h:
orx_npc_step, orx_npc_step_events, orx_npc_step_n, orx_npc_env_step and the
Python layers above them) -- against the reference's fixtures
(tests/golden/given/), the C oracle, oracle/pyref.py and itself.  All state is
integer: every comparison is exact."""
import numpy as np
import pytest

from golden_util import compare_state
from npc_given_cases import (BASE_CFG, GIVEN_CASES, KEYED_CASES, GivenGame, RecordingGame, bank,
                             given_fixture, random_table)

pytestmark = pytest.mark.gpu

B301 = 301   # two workgroups, a partial wave, an odd table stride
CFGS = {
    "k6": dict(BASE_CFG),
    "k12": dict(BASE_CFG, width=9, height=9, n_npcs=12),            # NCAP 16
    "k30": dict(BASE_CFG, width=12, height=12, n_npcs=30, npc_health=2),   # dense
    "bank": dict(BASE_CFG, width=9, height=8),
    "sep": dict(BASE_CFG, flags=3, sep_period=3, start_mode=2, p1_depth=0, p2_depth=1),
    "stock": dict(BASE_CFG, rng=1),
}


def _layouts(name):
    return bank(9, 8, 4, 207) if name == "bank" else None


def _engine(cfg, n_games, seed, offset=0, layouts=None):
    import torch
    from optimax_rogue_amd import EnvConfig
    from optimax_rogue_amd.engine import BatchedEngine
    return BatchedEngine(EnvConfig.from_dict(cfg, layouts=layouts), n_games, seed=seed,
                         game_offset=offset, device=torch.device("cuda", 0))


def _dev(a, eng):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _rows(s):
    """The 14 observation fields [14, B] of an engine-layout state."""
    return np.stack([s["p_x"][0], s["p_y"][0], s["p_depth"][0], s["p_health"][0],
                     s["p_x"][1], s["p_y"][1], s["p_depth"][1], s["p_health"][1],
                     s["tick"], s["status"], s["st_x"][0], s["st_y"][0], s["st_x"][1],
                     s["st_y"][1]]).astype(np.int32)


def _same(a, b, K, where):
    compare_state(a, b, K, where)
    compare_state(b, a, K, where)   # (live slots by either side's alive bits)


def _env_slot(eng):
    """(launch, obs, reward, done, status, bad): orx_npc_env_step over the
    engine's argument block, both players' actions given."""
    import torch
    from optimax_rogue_amd.enums import OBS_FIELDS, Policy
    d = eng.device
    obs = torch.zeros((eng.B, len(OBS_FIELDS)), dtype=torch.int32, device=d)
    rew = torch.zeros(eng.B, dtype=torch.float32, device=d)
    done = torch.zeros(eng.B, dtype=torch.bool, device=d)
    status = torch.zeros(eng.B, dtype=torch.int32, device=d)
    bad = torch.zeros(1, dtype=torch.int32, device=d)
    go = eng.env_step_slot(Policy.NONE, obs, rew, done, status, bad)
    go.outputs = (obs, rew, done, status, bad)   # (the block holds their addresses only)
    return go, obs, rew, done, status, bad


# -- 1. the reference's fixtures ------------------------------------------------
@pytest.mark.parametrize("name", GIVEN_CASES)
def test_fixture_step_and_events(name):
    """orx_npc_step_events equals the reference run with the table behind its
    decide_npc_move hook: every state field after every step, every event
    record in order."""
    fx = given_fixture(name)
    eng = _engine(fx.cfg, fx.G, fx.seed, fx.game_offset, layouts=fx.layouts)
    assert eng.max_events(given=True) == max(8, 6 + 2 * fx.K)
    compare_state(eng.snapshot(), fx.state(0), fx.K, f"{name} reset")
    acts, table = _dev(fx.actions, eng), _dev(fx.z["npc_moves"], eng)
    for t in range(fx.T):
        if fx.stock:   # the bots' draws share each game's random stream
            assert np.array_equal(eng.policy(*fx.policy).cpu().numpy(), fx.actions[t])
        _, ev, n = eng.step(acts[t], events=True, npc_moves=table[t])
        ev, n = ev.cpu().numpy(), n.cpu().numpy()
        for g in range(fx.G):
            got = [tuple(int(v) for v in r) for r in ev[g, : n[g]]]
            assert got == fx.events(t, g), (name, t, g, got, fx.events(t, g))
        compare_state(eng.snapshot(), fx.state(t + 1), fx.K, f"{name} t={t + 1}")


@pytest.mark.parametrize("name", KEYED_CASES)
def test_fixture_step_n_and_env_step(name):
    """The keyed fixtures through orx_npc_step_n in one launch (every tick's
    row, the final state) and through orx_npc_env_step (obs, reward, done,
    status of every step)."""
    import torch
    from optimax_rogue_amd import VecEnv
    from optimax_rogue_amd.enums import OBS_FIELDS
    fx = given_fixture(name)
    want = np.stack([_rows(fx.state(t + 1)) for t in range(fx.T)])
    eng = _engine(fx.cfg, fx.G, fx.seed, fx.game_offset, layouts=fx.layouts)
    acts, table = _dev(fx.actions, eng), _dev(fx.z["npc_moves"], eng)
    obs = torch.zeros((fx.T, len(OBS_FIELDS), fx.G), dtype=torch.int32, device=eng.device)
    eng.step_n(acts, obs=obs, npc_moves=table)
    assert np.array_equal(obs.cpu().numpy(), want), name
    compare_state(eng.snapshot(), fx.state(fx.T), fx.K, f"{name} step_n final")

    eng = _engine(fx.cfg, fx.G, fx.seed, fx.game_offset, layouts=fx.layouts)
    go, o, rew, done, status, _ = _env_slot(eng)
    for t in range(fx.T):
        go(acts[t].data_ptr(), 1, 2, None, table[t].data_ptr())
        before, after = (torch.from_numpy(fx.state(t + k)["status"].astype(np.int32))
                         for k in (0, 1))
        w_rew, w_done = VecEnv.outcome(before, after)
        assert np.array_equal(o.cpu().numpy().T, want[t]), (name, t)
        assert torch.equal(rew.cpu(), w_rew) and torch.equal(done.cpu(), w_done), (name, t)
        assert torch.equal(status.cpu(), after), (name, t)
    compare_state(eng.snapshot(), fx.state(fx.T), fx.K, f"{name} env_step final")


# -- 2. an all-Stay table plays the ORX_NPC_STAY game -----------------------------
@pytest.mark.parametrize("name", ["k6", "k12", "k30", "bank", "sep", "stock"])
def test_all_stay_table_equals_the_stay_oracle(name, oracle_lib):
    import torch
    cfg, lay, seed, T = CFGS[name], _layouts(name), 4100, 120
    eng = _engine(cfg, B301, seed, layouts=lay)
    ora = oracle_lib.Oracle(dict(cfg, npc_policy=0), B301, seed, record_events=True, layouts=lay)
    ora.reset()
    K = cfg["n_npcs"]
    stay = torch.full((K, B301), 5, dtype=torch.int8, device=eng.device)
    _same(eng.snapshot(), ora.export(), K, f"{name} reset")
    for t in range(T):
        a = ora.policy(2, 1)
        assert np.array_equal(eng.policy(2, 1).cpu().numpy(), a), (name, t)
        ora.step(a)
        _, ev, n = eng.step(events=True, npc_moves=stay)
        compare_state(eng.snapshot(), ora.export(), K, f"{name} t={t + 1}")
        ev, n = ev.cpu().numpy(), n.cpu().numpy()
        for g in range(32):
            got = [tuple(int(v) for v in r) for r in ev[g, : n[g]]]
            assert got == ora.events(g), (name, t, g)


# -- 3. a table of a built-in AI's decisions plays that AI's game ------------------
@pytest.mark.parametrize("npc_policy", [1, 2])
def test_ai_table_equals_the_ai(npc_policy):
    from oracle.pyref import batch_state
    G, T, seed = 64, 100, 4200
    cfg = dict(BASE_CFG, npc_policy=npc_policy, policy=(1, 1))
    K = cfg["n_npcs"]
    table = np.full((T, K, G), 5, np.int8)
    games = [RecordingGame(cfg, seed, g, table, g) for g in range(G)]
    actions = np.zeros((T, G, 2), np.int8)
    states = []
    for t in range(T):
        for g, game in enumerate(games):
            actions[t, g] = game.policy()
            game.step(*actions[t, g])
        states.append(batch_state(games))
    assert (table != 5).any()
    eng = _engine(dict(cfg, npc_policy=0), G, seed)       # (npc_policy is not read)
    ai = _engine(cfg, G, seed) if npc_policy == 2 else None   # the engine's own CHASE run
    acts, tab = _dev(actions, eng), _dev(table, eng)
    for t in range(T):
        eng.step(acts[t], npc_moves=tab[t])
        snap = eng.snapshot()
        compare_state(snap, states[t], K, f"policy {npc_policy} t={t + 1}")
        if ai is not None:
            ai.step(acts[t])
            _same(ai.snapshot(), snap, K, f"orx_step CHASE t={t + 1}")


# -- 4. random tables against the pinned CPU restatement ---------------------------
@pytest.mark.parametrize("name", ["k6", "k12", "k30", "bank"])
def test_random_table_vs_given_game(name):
    from oracle.pyref import batch_state
    G, T, seed = 64, 100, 4300
    cfg, lay = dict(CFGS[name], policy=(1, 1)), _layouts(name)
    K = cfg["n_npcs"]
    table = random_table(T, K, G, 4301)
    games = [GivenGame(cfg, seed, 7 + g, table, g, layouts=lay) for g in range(G)]
    eng = _engine(cfg, G, seed, offset=7, layouts=lay)
    compare_state(eng.snapshot(), batch_state(games), K, f"{name} reset")
    tab = _dev(table, eng)
    episodes = 0
    for t in range(T):
        a = np.array([game.policy() for game in games], np.int8)
        want_ev = [game.step(*a[g]) for g, game in enumerate(games)]
        _, ev, n = eng.step(_dev(a, eng), events=True, npc_moves=tab[t])
        snap = eng.snapshot()
        compare_state(snap, batch_state(games), K, f"{name} t={t + 1}")
        ev, n = ev.cpu().numpy(), n.cpu().numpy()
        for g in range(0, G, 8):
            assert [tuple(int(v) for v in r) for r in ev[g, : n[g]]] == want_ev[g], (name, t, g)
        episodes = int(snap["episode"].max())
    assert episodes >= 2   # (autoreset: the table is indexed by step across episodes)


# -- 5. the entry points agree ------------------------------------------------------
@pytest.mark.parametrize("name", ["k6", "k12", "k30", "bank"])
def test_entry_points_agree(name):
    """orx_npc_step_n == 40 x orx_npc_step (int32 and compact rows);
    orx_npc_env_step == orx_npc_step plus VecEnv.outcome; events on / off
    give one state (the commute shortcut against the ordered path)."""
    import torch
    from optimax_rogue_amd import VecEnv
    from optimax_rogue_amd.engine import decode_compact
    from optimax_rogue_amd.enums import OBS_COMPACT, OBS_COMPACT_FIELDS, OBS_FIELDS
    T, seed = 40, 4400
    cfg, lay = CFGS[name], _layouts(name)
    K = cfg["n_npcs"]
    mk = lambda: _engine(cfg, B301, seed, offset=11, layouts=lay)
    step, evs, many, compact, env = mk(), mk(), mk(), mk(), mk()
    rng = np.random.default_rng(4401)
    acts = _dev(rng.integers(1, 6, size=(T, B301, 2), dtype=np.int8), step)
    tab = _dev(random_table(T, K, B301, 4402), step)
    go, o, rew, done, status, _ = _env_slot(env)
    rows = []
    for t in range(T):
        before = step.status.clone()
        after = step.step(acts[t], npc_moves=tab[t]).clone()
        evs.step(acts[t], events=True, npc_moves=tab[t])
        go(acts[t].data_ptr(), 1, 2, None, tab[t].data_ptr())
        snap = step.snapshot()
        rows.append(_rows(snap))
        _same(evs.snapshot(), snap, K, f"{name} events t={t + 1}")
        _same(env.snapshot(), snap, K, f"{name} env_step t={t + 1}")
        w_rew, w_done = VecEnv.outcome(before, after)
        assert np.array_equal(o.cpu().numpy().T, rows[-1]), (name, t)
        assert torch.equal(rew, w_rew) and torch.equal(done, w_done), (name, t)
        assert torch.equal(status, after), (name, t)
    rows = np.stack(rows)
    obs = torch.zeros((T, len(OBS_FIELDS), B301), dtype=torch.int32, device=step.device)
    many.step_n(acts, obs=obs, npc_moves=tab)
    assert np.array_equal(obs.cpu().numpy(), rows), name
    _same(many.snapshot(), step.snapshot(), K, f"{name} step_n")
    cobs = torch.zeros((T, len(OBS_COMPACT_FIELDS), B301), dtype=torch.int32, device=step.device)
    compact.step_n(acts, obs=cobs, obs_format=OBS_COMPACT, npc_moves=tab)
    assert np.array_equal(decode_compact(cobs).cpu().numpy(), rows), name
    _same(compact.snapshot(), step.snapshot(), K, f"{name} step_n compact")
    assert int(step.counters[3].sum()) > 0 and int(step.counters[0].sum()) > 0


# -- 6. refusals ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k6", "k30"])
def test_bad_bytes_stop_exactly_their_games(name):
    """A 0 and a 6 in an alive NPC's slot stop exactly those games with status
    16: nothing of them changes, they restart on the next step, bad_actions
    rises by their count.  The same bytes in dead slots change nothing."""
    import torch
    cfg, seed = CFGS[name], 4500
    K = cfg["n_npcs"]
    eng, twin = _engine(cfg, B301, seed), _engine(cfg, B301, seed)
    slot = _env_slot(eng)
    go, status, bad = slot[0], slot[4], slot[5]
    go2 = _env_slot(twin)[0]
    rng = np.random.default_rng(4501)
    acts = _dev(rng.integers(1, 6, size=(40, B301, 2), dtype=np.int8), eng)
    tab = _dev(random_table(40, K, B301, 4502), eng)
    for t in range(12):   # NPCs die (on staircases, in combat): dead slots appear
        go(acts[t].data_ptr(), 1, 2, None, tab[t].data_ptr())
        go2(acts[t].data_ptr(), 1, 2, None, tab[t].data_ptr())
    alive = eng.npc_state()[3].cpu().numpy().astype(bool)
    live = eng.status.cpu().numpy() == 1
    assert (~alive).any() and alive.any()
    first_alive = alive.argmax(0)
    has_dead, first_dead = (~alive).any(0), (~alive).argmax(0)
    t12 = tab[12].cpu().numpy().copy()
    clean = t12.copy()
    games = np.flatnonzero(live & alive.any(0))
    zero, six = games[::7], games[3::7]
    assert len(zero) > 5 and len(six) > 5 and not set(zero) & set(six)
    t12[first_alive[zero], zero] = 0
    t12[first_alive[six], six] = 6
    others = np.setdiff1d(np.flatnonzero(has_dead), np.concatenate([zero, six]))
    assert len(others) > 5
    t12[first_dead[others], others] = rng.choice(np.array([0, 6, -1, 77], np.int8), len(others))
    before = eng.snapshot()
    assert int(bad.item()) == 0
    dirty = _dev(t12, eng)
    go(acts[12].data_ptr(), 1, 2, None, dirty.data_ptr())
    go2(acts[12].data_ptr(), 1, 2, None, _dev(clean, twin).data_ptr())
    after, want = eng.snapshot(), twin.snapshot()
    stopped = np.concatenate([zero, six])
    assert (after["status"][stopped] == 16).all() and (status.cpu().numpy()[stopped] == 16).all()
    assert int(bad.item()) == len(stopped)
    assert set(np.flatnonzero(after["status"] == 16)) == set(stopped.tolist())
    keep = np.ones(B301, bool)
    keep[stopped] = False
    for k, v in after.items():   # the stopped games: only their status moved ...
        if k != "status":
            assert np.array_equal(v[..., stopped], before[k][..., stopped]), k
        # ... and every other game played the clean table's tick
        assert np.array_equal(v[..., keep], want[k][..., keep]), k
    go(acts[13].data_ptr(), 1, 2, None, tab[13].data_ptr())
    s = eng.snapshot()
    assert (s["status"][stopped] == 1).all()
    assert np.array_equal(s["episode"][stopped], before["episode"][stopped] + 1)
    assert (s["tick"][stopped] == 1).all()
    assert int(bad.item()) == len(stopped)


def test_table_is_ignored_on_reset_steps():
    """A step that resets a game (autoreset) does not look at its column of
    the table, as it does not look at its actions: garbage there changes
    nothing and stops nothing."""
    import torch
    cfg, seed, T = dict(CFGS["k6"], max_ticks=8), 4600, 24
    eng, twin = _engine(cfg, B301, seed), _engine(cfg, B301, seed)
    rng = np.random.default_rng(4601)
    acts = _dev(rng.integers(1, 6, size=(T, B301, 2), dtype=np.int8), eng)
    tab = _dev(random_table(T, 6, B301, 4602), eng)
    resets = 0
    for t in range(T):
        finished = eng.status != 1
        resets += int(finished.sum())
        dirty = torch.where(finished[None], torch.full_like(tab[t], 77), tab[t])
        eng.step(acts[t], npc_moves=dirty)
        twin.step(acts[t], npc_moves=tab[t])
        _same(eng.snapshot(), twin.snapshot(), 6, f"t={t + 1}")
    assert resets >= 2 * B301 and int((eng.status >= 16).sum()) == 0


def test_python_layers_refuse_bad_tables():
    import torch
    from optimax_rogue_amd import EnvConfig, VecEnv
    eng = _engine(CFGS["k6"], 8, 1)
    good = torch.full((6, 8), 5, dtype=torch.int8, device=eng.device)
    for bad in (good[:5], good.to(torch.int32), good.t().contiguous().t(), good.cpu()):
        with pytest.raises(ValueError):
            eng.step(npc_moves=bad)
    with pytest.raises(ValueError):
        eng.step_n(torch.full((2, 8, 2), 5, dtype=torch.int8, device=eng.device), npc_moves=good)
    with pytest.raises(ValueError):
        _engine(dict(CFGS["k6"], n_npcs=0), 8, 1).step(npc_moves=good)
    env = VecEnv(EnvConfig.from_dict(CFGS["k6"]), 8, seed=1, opponent=1, check_actions=False)
    a = torch.full((8,), 5, dtype=torch.int64, device=env.device)
    for bad in (good[:5], good.t(), good.float()):
        with pytest.raises(ValueError):
            env.step(a, npc_moves=bad)
    # other integer dtypes: 257 does not wrap to 1 -- it stops the game
    t = good.to(torch.int64)
    t[0, 3] = 257
    assert env.step(a, npc_moves=t)[3].tolist() == [1, 1, 1, 16, 1, 1, 1, 1]
    x, y, hp, alive = env.engine.npc_state()
    snap = env.engine.snapshot()
    assert x.dtype == torch.int32 and tuple(alive.shape) == (6, 8)
    assert np.array_equal(x.cpu().numpy(), snap["npc_pos"] & 0xFF)
    assert np.array_equal(y.cpu().numpy(), snap["npc_pos"] >> 8)
    assert np.array_equal(hp.cpu().numpy(), snap["npc_health"])
    assert np.array_equal(alive.cpu().numpy(), (snap["npc_alive"][None] >> np.arange(6)[:, None]) & 1)


def test_npc_state_dense_rows():
    """npc_state() over the dense form's alive rows (K > 32: [words][games])."""
    from optimax_rogue_amd.enums import npc_alive_bits
    cfg = dict(BASE_CFG, width=14, height=14, n_npcs=40)
    eng = _engine(cfg, 37, 5)
    tab = _dev(random_table(10, 40, 37, 6), eng)
    for t in range(10):
        eng.step(npc_moves=tab[t])
    alive = eng.npc_state()[3].cpu().numpy()
    snap = eng.snapshot()
    assert np.array_equal(alive.astype(bool), npc_alive_bits(snap["npc_alive"], 40))
    assert 0 < alive.sum() < alive.size


# -- 7. VecEnv -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k6", "stock"])
def test_vecenv_ring_graph_and_shards(name):
    """VecEnv.step(actions, npc_moves): the output ring, a captured HIP graph
    (the static table tensor rewritten between replays) and two game_offset
    shards all equal eager stepping of the whole batch."""
    import torch
    from optimax_rogue_amd import EnvConfig, VecEnv
    cfg = EnvConfig.from_dict(CFGS[name])
    K, T, seed = 6, 12, 4700
    half = B301 // 2
    mk = lambda n=B301, off=0, **kw: VecEnv(cfg, n, seed=seed, game_offset=off, opponent=1,
                                            check_actions=False, **kw)
    eager, ring = mk(), mk(out_buffers=2)
    lo, hi = mk(half), mk(B301 - half, half)
    dev = eager.device
    gen = torch.Generator().manual_seed(4701)
    a = torch.randint(1, 6, (T, B301), generator=gen, dtype=torch.int64).to(dev)
    tab = torch.randint(1, 6, (T, K, B301), generator=gen, dtype=torch.int64).to(dev)
    tab8 = tab.to(torch.int8)
    outs = []
    for t in range(T):
        want = [v.clone() for v in eager.step(a[t], npc_moves=tab8[t])]
        outs.append(want)
        got = ring.step(a[t], npc_moves=tab[t])       # (an int64 table: cast on the device)
        parts = [lo.step(a[t, :half], npc_moves=tab8[t, :, :half]),
                 hi.step(a[t, half:], npc_moves=tab8[t, :, half:])]
        for j in range(4):
            assert torch.equal(got[j], want[j]), (name, t, j)
            assert torch.equal(torch.cat([parts[0][j], parts[1][j]]), want[j]), (name, t, j)
    assert int(eager.engine.counters[3].sum()) > 0
    if name == "stock":
        return   # (stock-seed mode steps through orx_policy + orx_npc_step: not captured here)
    graphed = mk(out_buffers=1)
    sa, st = a[0].clone(), tab8[0].clone()
    graphed.step(sa, npc_moves=st)   # (the first step settles the host-side launch blocks)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            obs, reward, done, status = graphed.step(sa, npc_moves=st)
    torch.cuda.current_stream(dev).wait_stream(s)
    for t in range(1, T):
        sa.copy_(a[t])
        st.copy_(tab8[t])
        g.replay()
        torch.cuda.synchronize(dev)
        for got, want in zip((obs, reward, done, status), outs[t]):
            assert torch.equal(got, want), t


# -- 8. the reference's hook on GameUpdater ---------------------------------------------
def _as_record(u):
    from optimax_rogue_amd import updates as U
    if isinstance(u, U.EntityCombatUpdate):
        (flag,) = tuple(u.tags)
        return (1, u.attacker_iden, u.defender_iden, int(flag))
    if isinstance(u, U.EntityDeathUpdate):
        return (2, u.entity_iden, 0, 0)
    if isinstance(u, U.EntityPositionUpdate):
        return (3, u.entity_iden, u.depth, (u.posx & 0xFFFF) | (u.posy << 16))
    return (4, 0, u.depth, 0)


@pytest.mark.parametrize("g", [0, 5, 11])
def test_game_updater_hook(g):
    """A GameUpdater subclass overriding decide_npc_move with the fixture's
    table: the update lists and the mutated GameStateView equal the
    reference's, the hook is asked once per NPC in entities order."""
    import torch
    from optimax_rogue_amd import DungeonDespawningStrategy
    from optimax_rogue_amd.enums import Move
    from optimax_rogue_amd.updater import GameUpdater
    fx = given_fixture("given_regs_8x8")
    c, table = fx.cfg, fx.z["npc_moves"]
    asked = []

    class TableUpdater(GameUpdater):
        t = 0

        def decide_npc_move(self, game_state, ent, result):
            assert result == [] and ent.iden >= 3
            asked.append(ent.iden)
            return Move(int(table[self.t, ent.iden - 3, g]))

    upd = TableUpdater((c["width"], c["height"]), DungeonDespawningStrategy(c["despawn"]),
                       c["max_ticks"] or None, seed=fx.seed, game_id=fx.game_offset + g,
                       n_npcs=c["n_npcs"], device=torch.device("cuda", 0))
    gs = upd.setup_game()
    order = played = 0
    for t in range(fx.T):
        if fx.state(t)["status"][g] != 1:
            break   # the reference game is over (the fixture autoresets; GameUpdater does not)
        upd.t = t
        del asked[:]
        want_asked = [e.iden for e in gs.entities if e.iden >= 3]
        res, ups = upd.update(gs, fx.actions[t, g, 0], fx.actions[t, g, 1])
        assert asked == want_asked, t
        assert [_as_record(u) for u in ups] == fx.events(t, g), t
        assert [u.order for u in ups] == list(range(order, order + len(ups)))
        order += len(ups)
        assert int(res) == fx.state(t + 1)["status"][g]
        assert gs == upd.engine.game_states([0])[0], t
        ents = [(e.iden, e.depth, e.x, e.y, e.health) for e in gs.entities]
        assert ents == fx.entities(t + 1, g), t
        played += 1
    assert played >= 10 and any(r[1] >= 3 for t in range(played) for r in fx.events(t, g))


def test_game_updater_without_override_plays_npc_policy():
    """No override: behaviour is unchanged, npc_policy still selects the AI."""
    import torch
    from optimax_rogue_amd import DungeonDespawningStrategy
    from optimax_rogue_amd.enums import NpcPolicy
    from optimax_rogue_amd.updater import BatchedUpdater, GameUpdater
    dev = torch.device("cuda", 0)
    upd = GameUpdater((8, 8), DungeonDespawningStrategy.Unreachable, 40, seed=9, game_id=3,
                      n_npcs=6, device=dev, npc_policy=NpcPolicy.Chase)
    ref = _engine(dict(BASE_CFG, max_ticks=40, npc_policy=2, autoreset=0), 1, 9, offset=3)
    gs = upd.setup_game()
    rng = np.random.default_rng(10)
    moved = False
    for t in range(30):
        m = rng.integers(1, 6, size=2)
        _, ups = upd.update(gs, int(m[0]), int(m[1]))
        ref.actions[0, 0], ref.actions[0, 1] = int(m[0]), int(m[1])
        ref.step()
        _same(upd.engine.snapshot(), ref.snapshot(), 6, f"t={t}")
        moved = moved or any(_as_record(u)[0] == 3 and _as_record(u)[1] >= 3 for u in ups)
    assert moved
    # BatchedUpdater.update(p1, p2, npc_moves) == engine.step(npc_moves=...)
    bu = BatchedUpdater((8, 8), DungeonDespawningStrategy.Unreachable, 30, n_games=16, seed=4,
                        n_npcs=6, device=dev, autoreset=True)
    eng = _engine(dict(BASE_CFG), 16, 4)
    tab = random_table(20, 6, 16, 12)
    for t in range(20):
        m = rng.integers(1, 6, size=(16, 2)).astype(np.int8)
        bu.update(m[:, 0], m[:, 1], npc_moves=tab[t].astype(np.int64))
        eng.step(_dev(m, eng), npc_moves=_dev(tab[t], eng))
        _same(bu.engine.snapshot(), eng.snapshot(), 6, f"batched t={t}")
    with pytest.raises(ValueError):
        bu.update(m[:, 0], m[:, 1], npc_moves=tab[0][:5])
