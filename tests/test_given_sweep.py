"""CPU: the C oracle's given tick (oracle_step_given, ``Oracle.step(actions,
npc_moves=)``: include/orx_npc.h restated) pinned before
tests/test_gpu_given_sweep.py compares the engine with it, then the sweep's
draws and their coverage on the oracle alone:

  * the four reference fixtures of tests/golden/given/ replay through it with
    every state field after every tick, every event, World.dungeons and the
    entity order equal;
  * on the sweep's flag-free cases it equals oracle/pyref.py's Game with the
    guards and the table behind decide_npc_move (npc_given_cases.GivenGame);
  * an all-Stay table plays the oracle's npc_policy 0 run on every case, the
    two flags included;
  * a table recorded from either built-in AI replays to that AI's own oracle
    run (keyed cases);
  * ``given_sweep.guard_sample`` (what the GPU side counts on the engine's
    states) counts what the oracle counted;
  * ``check_draw`` on every case and ``check_coverage`` on the whole sweep.

Integers compared exactly; nothing here needs a GPU.
"""
import numpy as np
import pytest

import given_sweep as gs
from golden_util import compare_state
from npc_given_cases import GIVEN_CASES, GivenGame, RecordingGame, given_fixture

CASES = [gs.draw(c) for c in range(gs.N_CASES)]
PLAIN = [d.case for d in CASES if not d.cfg["flags"]]              # pyref restates flags 0 only
KEYED_PLAIN = [d.case for d in CASES if not d.cfg["flags"] and d.keyed]
N_PYREF = 16      # games of the Python restatement per case
N_SMALL = 64      # games of the oracle-against-oracle checks per case


def same(a, b, K, where):
    compare_state(a, b, K, where)
    compare_state(b, a, K, where)   # (live slots by either side's alive bits)


# -- 1. the reference's fixtures ---------------------------------------------------
@pytest.mark.parametrize("name", GIVEN_CASES)
def test_oracle_given_tick_vs_reference_fixture(oracle_lib, name):
    fx = given_fixture(name)
    table = fx.z["npc_moves"]
    ora = oracle_lib.Oracle(fx.cfg, fx.G, fx.seed, fx.game_offset, record_events=True,
                            layouts=fx.layouts)
    ora.reset()
    same(ora.export(), fx.state(0), fx.K, f"{name} reset")
    for t in range(fx.T):
        if fx.stock:   # the bots' draws share each game's random stream
            assert np.array_equal(ora.policy(*fx.policy), fx.actions[t]), (name, t)
        ora.step(fx.actions[t], npc_moves=table[t])
        same(ora.export(), fx.state(t + 1), fx.K, f"{name} t={t + 1}")
        for g in range(fx.G):
            assert ora.events(g) == fx.events(t, g), (name, t, g)
            assert ora.world(g) == fx.world(t + 1, g), (name, t, g)
            assert [e[:5] for e in ora.entities(g)] == fx.entities(t + 1, g), (name, t, g)
    tally = ora.given_tally()
    assert tally["refused"].sum() == 0 and tally["dead_bad"].sum() == 0
    # (make_given.py applied the guards to what it recorded: the fixtures meet them)
    assert tally["guard2"].sum() > 0 and tally["guard3"].sum() > 0


def test_oracle_refuses_a_cfg_outside_the_given_ticks_domain(oracle_lib):
    base = dict(width=8, height=8, n_npcs=3)
    a = np.full((4, 2), 5, np.int8)
    for cfg, K in ((dict(base, n_npcs=0), 1), (dict(base, flags=4), 3), (dict(base, flags=67), 3)):
        ora = oracle_lib.Oracle(cfg, 4, 1)
        ora.reset()
        with pytest.raises(ValueError):
            ora.step(a, npc_moves=np.full((K, 4), 5, np.int8))
    ora = oracle_lib.Oracle(dict(base, flags=3, sep_period=2), 4, 1)
    ora.reset()
    for bad in (np.full((4, 3), 5, np.int8), np.full((3, 4), 5, np.int32)):
        with pytest.raises(ValueError):
            ora.step(a, npc_moves=bad)
    ora.step(a, npc_moves=np.full((3, 4), 5, np.int8))


# -- 2. the Python restatement -------------------------------------------------------
class _SweepRules:
    """pyref.Game plays the reference's fixed players (health 10, damage 2,
    armor 1) and valid moves only; the sweep draws the players' attributes and
    puts bytes outside the Move codes into both logs.  This gives the players
    the cfg's attributes and stops a game on such a byte as include/orx.h and
    include/orx_npc.h say: status 16, nothing played, restart on the next
    step."""

    def setup(self):
        super().setup()
        c = self.cfg
        for e in self.gs.entities[:2]:
            e.health = e.base_max_health = int(c["player_health"])
            e.base_damage, e.base_armor = int(c["player_damage"]), int(c["player_armor"])

    def bad_table(self):
        return False

    def step(self, m1, m2):
        if self.status == gs.IN_PROGRESS and (not 1 <= m1 <= 5 or not 1 <= m2 <= 5
                                              or self.bad_table()):
            self.status = gs.BAD_ACTION_STATUS
            self.t += 1
            return []
        return super().step(m1, m2)


class SweepGivenGame(_SweepRules, GivenGame):
    def bad_table(self):
        return any(not 1 <= int(self.table[self.t, e.iden - 3, self.g]) <= 5
                   for e in self.gs.entities if e.iden >= 3)


class SweepRecordingGame(_SweepRules, RecordingGame):
    pass


def pyref_cfg(d, **kw):
    cfg = dict(start_mode=1, p1_depth=0, p2_depth=0, autoreset=1, rng=0, npc_policy=0)
    cfg.update(d.cfg)
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("case", PLAIN)
def test_oracle_given_tick_vs_pyref(oracle_lib, case):
    from oracle.pyref import batch_state
    d = CASES[case]
    n = min(d.B, N_PYREF)
    table, actions = (np.ascontiguousarray(a) for a in
                      (gs.tables(d)[0][:, :, :n], gs.tables(d)[1][:, :n]))
    games = [SweepGivenGame(pyref_cfg(d), d.seed, d.off + g, table, g, layouts=d.layouts)
             for g in range(n)]
    ora = oracle_lib.Oracle(d.cfg, n, d.seed, d.off, record_events=True, layouts=d.layouts)
    ora.reset(episode=np.zeros(n, np.int32))
    same(ora.export(), batch_state(games), d.K, f"{gs.where(d)} reset")
    for t in range(d.T):
        want = [game.step(int(actions[t, g, 0]), int(actions[t, g, 1]))
                for g, game in enumerate(games)]
        ora.step(actions[t], npc_moves=table[t])
        same(ora.export(), batch_state(games), d.K, f"{gs.where(d)} t={t + 1}")
        for g in range(n):
            assert ora.events(g) == want[g], (gs.where(d), t, g)
            assert ora.world(g) == games[g].world_list(), (gs.where(d), t, g)


# -- 3. an all-Stay table plays the npc_policy 0 game ----------------------------------
def equal_runs(a, b, msg):
    sa, sb = a.export(), b.export()
    assert sa.keys() == sb.keys(), msg
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), (msg, k)
    assert [a.events(g) for g in range(a.B)] == [b.events(g) for g in range(a.B)], msg


@pytest.mark.parametrize("case", range(gs.N_CASES))
def test_all_stay_table_is_the_stay_game(oracle_lib, case):
    d = CASES[case]
    n = min(d.B, N_SMALL)
    actions = gs.tables(d)[1][:, :n]
    mk = lambda cfg: oracle_lib.Oracle(cfg, n, d.seed, d.off, record_events=True, layouts=d.layouts)
    given, stay = mk(d.cfg), mk(dict(d.cfg, npc_policy=0))
    table = np.full((d.K, n), 5, np.int8)
    for o in (given, stay):
        o.reset(episode=np.zeros(n, np.int32))
    for t in range(d.T):
        if not d.keyed:   # (stock seeding: the bots' draws are part of each game's stream)
            assert np.array_equal(given.policy(1, 2), stay.policy(1, 2))
        given.step(actions[t], npc_moves=table)
        stay.step(actions[t])
        equal_runs(given, stay, (gs.where(d), t))
    tally = given.given_tally()
    assert not any(tally[k].sum() for k in ("guard1", "guard2", "guard3", "refused", "dead_bad"))


# -- 4. a recorded AI replays to that AI's oracle run ------------------------------------
@pytest.mark.parametrize("npc_policy", [1, 2])
@pytest.mark.parametrize("case", KEYED_PLAIN)
def test_recorded_ai_table_replays_the_ai(oracle_lib, case, npc_policy):
    d = CASES[case]
    n = min(d.B, N_PYREF)
    actions = np.ascontiguousarray(gs.tables(d)[1][:, :n])
    table = np.full((d.T, d.K, n), 5, np.int8)
    games = [SweepRecordingGame(pyref_cfg(d, npc_policy=npc_policy), d.seed, d.off + g, table, g,
                                layouts=d.layouts) for g in range(n)]
    for t in range(d.T):
        for g, game in enumerate(games):
            game.step(int(actions[t, g, 0]), int(actions[t, g, 1]))
    mk = lambda cfg: oracle_lib.Oracle(cfg, n, d.seed, d.off, record_events=True, layouts=d.layouts)
    given, ai = mk(d.cfg), mk(dict(d.cfg, npc_policy=npc_policy))
    for o in (given, ai):
        o.reset(episode=np.zeros(n, np.int32))
    for t in range(d.T):
        given.step(actions[t], npc_moves=table[t])
        ai.step(actions[t])
        equal_runs(given, ai, (gs.where(d), npc_policy, t))
    from oracle.pyref import batch_state
    same(ai.export(), batch_state(games), d.K, f"{gs.where(d)} pyref's AI run")
    # (the AIs hold the guards themselves: what they decided passes unchanged)
    tally = given.given_tally()
    assert not any(tally[k].sum() for k in ("guard1", "guard2", "guard3", "refused"))


# -- 5. the numpy counts of the GPU side against the oracle's own ---------------------------
@pytest.mark.parametrize("case", range(gs.N_CASES))
def test_guard_sample_counts_what_the_oracle_counted(oracle_lib, case):
    """Over the first 64 games, on the sampled ticks: refused and dead-slot
    ticks of every game, the three guards' counts of every game whose NPC
    depth the snapshot holds."""
    d = CASES[case]
    n = min(d.B, gs.SAMPLE_GAMES)
    table, actions = gs.tables(d)
    cfg, bank = gs.env_config(d), gs.bank_of(d)
    ora = oracle_lib.Oracle(d.cfg, n, d.seed, d.off, layouts=d.layouts)
    ora.reset(episode=np.zeros(n, np.int32))
    for t in range(d.T):
        tab = np.ascontiguousarray(table[t][:, :n])
        if gs.sampled(t):
            s = gs.guard_sample(cfg, bank, ora.export(), tab, actions[t, :n])
            before = ora.given_tally()
        ora.step(actions[t, :n], npc_moves=tab)
        if gs.sampled(t):
            delta = {k: v - before[k] for k, v in ora.given_tally().items()}
            msg = (gs.where(d), t)
            assert np.array_equal(delta["refused"], s["live_bad"]), msg
            assert np.array_equal(delta["dead_bad"], s["dead_bad"]), msg
            seen = s["unwatched"] == 0
            for k in ("guard1", "guard2", "guard3"):
                assert np.array_equal(delta[k][seen], s[k][seen]), (msg, k)
            assert not delta["guard1"][~seen].any() and not delta["guard2"][~seen].any(), msg


# -- 6. the draws and what they cover ------------------------------------------------------
def test_draws_are_valid_and_varied():
    seen = set()
    for d in CASES:
        gs.check_draw(d)
        again = gs.draw(d.case)
        assert again.cfg == d.cfg and again.T == d.T and again.data_seed == d.data_seed
        seen |= {"act " + d.act_dtype, "table " + d.table_dtype, f"opponent {d.opponent}",
                 f"ring {d.out_buffers}", "rows " + d.rows, f"B{d.B}"}
        seen |= {"compact refused"} if d.rows != d.rows_drawn else set()
        seen |= {"edge K"} if d.K != d.drawn_K else set()
        seen |= {"offset > 11"} if d.off > 11 else set()
    want = {"act " + t for t in gs.DTYPES} | {"table " + t for t in gs.DTYPES}
    want |= {f"opponent {o}" for o in (None, 1, 2)} | {"ring 0", "ring 2", "edge K", "offset > 11"}
    want |= {"rows " + r for r in gs.ROWS} | {f"B{b}" for b in (1, 63, 257, 1000, 1531)}
    if gs.N_CASES >= 96:
        assert want <= seen, want - seen
    stock = sum(not d.keyed for d in CASES)
    assert stock <= gs.MAX_STOCK * len(CASES), stock
    # the fuzz's own draws are what they were: the sweep only reads _draw
    from test_gpu_fuzz import _draw
    assert _draw(3)[0] == _draw(3, base=1000)[0]
    table, actions = gs.tables(CASES[0])
    assert table.dtype == np.int8 and actions.dtype == np.int8
    assert gs.as_dtype(np.array([-1, 5], np.int8), "uint8").tolist() == [255, 5]
    assert gs.as_dtype(np.array([-1, 5], np.int8), "int64").tolist() == [-1, 5]


def test_coverage(oracle_lib):
    """Conditions, not measurements: the oracle's runs of the whole sweep, at
    every case's own batch, reach every instance class, edge K, mode, guard,
    refusal and event the sweep is for."""
    if gs.N_CASES < 96:
        pytest.skip("the coverage conditions are those of the whole sweep")
    tallies, own = [], []
    for d in CASES:
        table, actions = gs.tables(d)
        r = gs.play(d, table, actions, events=False)
        tallies.append(gs.tally(d, r.status, r.final, r.samples, r.c_tally["npc_kill"]))
        own.append(r.c_tally)
    total, oracle_total = gs.add_up(tallies), gs.add_up(own)
    print("oracle coverage:", total, oracle_total)
    gs.check_coverage(total, oracle_total)
