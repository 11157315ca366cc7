"""GPU: the tick with the NPCs' moves supplied by the caller -- orx_npc_step,
orx_npc_step_events, orx_npc_step_n, orx_npc_env_step (include/orx_npc.h) and
``VecEnv.step(actions, npc_moves=)`` above them -- over the given sweep's draws
(tests/given_sweep.py): the fuzz's configuration space inside the given tick's
domain, K at every edge of the kernels' instance space (NCAP 8 / 16 / dense,
one and several alive words, bank or not), batches of 1, 63, 257, 1000 and 1531
games, tables and action logs with bytes outside the Move codes.

Per case every leg starts from the same reset and is compared exactly with the
C oracle's given tick (pinned to the reference's fixtures and to pyref by
tests/test_given_sweep.py), state comparisons in both directions:
  A  orx_npc_step_events every tick: status every tick, the events of three
     drawn games every tick, the state every 20 ticks and at the end (the
     ordered path of the register NPCs);
  B  orx_npc_step without events: status every tick, the final state (the
     commute shortcut);
  C  orx_npc_step_n in two launches over the same table (keyed cases): no,
     int32 or compact rows by the draw, into poison-guarded buffers, once per
     poison; the final state;
  D  VecEnv.step(actions, npc_moves=table[t]) with the drawn dtypes, opponent
     and output ring (keyed cases): obs, reward, done, status and the actions
     played every tick, bad_actions() and the episode returns at the end;
  E  on odd cases, orx_npc_env_step over the argument block directly, its four
     outputs in poison-guarded buffers (the poison alternating by tick), obs
     off 16-byte alignment.
The table and the action log are unchanged after every leg.  A last test holds
the engine's own tallies to ``check_coverage`` and to the oracle's counts.
All values are integers (reward: -1, 0, 1): every comparison is exact.
"""
import numpy as np
import pytest

import given_sweep as gs
from golden_util import compare_state
from guarded import POISONS, Guarded, same

pytestmark = pytest.mark.gpu

CASES = [gs.draw(c) for c in range(gs.N_CASES)]
TALLIES = {}               # case -> (given_sweep.tally of the engine's run, of the oracle's)


def both_ways(a, b, K, msg):
    compare_state(a, b, K, msg)
    compare_state(b, a, K, msg)   # (live slots by either side's alive bits)


def new_engine(d):
    import torch
    from optimax_rogue_amd.engine import BatchedEngine
    return BatchedEngine(gs.env_config(d), d.B, seed=d.seed, game_offset=d.off,
                         device=torch.device("cuda", 0))


def npc_kills(eng, d, ev, nev):
    """Ticks that left a player at health <= 0 after an NPC's blow took health
    from it, over the batch: from this tick's event records and p_health, on
    the device."""
    import torch
    if d.cfg["npc_damage"] - d.cfg["npc_armor"] <= 0:
        return 0
    valid = torch.arange(ev.shape[1], device=ev.device)[None, :] < nev[:, None]
    blow = valid & (ev[:, :, 0] == 1) & (ev[:, :, 1] >= 3)
    n = 0
    for p in (0, 1):
        n += int(((blow & (ev[:, :, 2] == p + 1)).any(dim=1) & (eng.p_health[p] <= 0)).sum())
    return n


def leg_events(d, run, table, actions, acts, tab, cfg, bank, msg):
    """Leg A; returns the engine's tally of the run."""
    import torch
    eng = new_engine(d)
    assert eng.max_events(given=True) == max(8, 6 + 2 * d.K), msg
    both_ways(eng.snapshot(), run.reset, d.K, f"{msg} reset")
    status = np.zeros((d.T + 1, d.B), np.int32)
    status[0] = eng.status.cpu().numpy()
    games = torch.tensor(d.event_games, device=eng.device)
    samples, kills = {}, 0
    for t in range(d.T):
        if gs.sampled(t):
            samples[t] = gs.guard_sample(cfg, bank, eng.snapshot(), table[t], actions[t])
        st, ev, nev = eng.step(acts[t], events=True, npc_moves=tab[t])
        status[t + 1] = st.cpu().numpy()
        assert np.array_equal(status[t + 1], run.status[t + 1]), f"{msg} events status t={t + 1}"
        kills += npc_kills(eng, d, ev, nev)
        ev3, n3 = ev[games].cpu().numpy(), nev[games].cpu().numpy()
        for j, g in enumerate(d.event_games):
            got = [tuple(int(v) for v in r) for r in ev3[j, : n3[j]]]
            assert got == run.events[t][g], f"{msg} events t={t + 1} game {g}"
        if t in run.states:
            both_ways(eng.snapshot(), run.states[t], d.K, f"{msg} events t={t + 1}")
    return gs.tally(d, status, eng.snapshot(), samples, kills)


def leg_plain(d, run, acts, tab, msg):
    """Leg B."""
    eng = new_engine(d)
    for t in range(d.T):
        st = eng.step(acts[t], npc_moves=tab[t])
        assert np.array_equal(st.cpu().numpy(), run.status[t + 1]), f"{msg} step status t={t + 1}"
    both_ways(eng.snapshot(), run.final, d.K, f"{msg} step final")


def leg_step_n(d, run, acts, tab, poison, msg):
    """Leg C with one poison."""
    import torch
    from optimax_rogue_amd.engine import decode_compact
    from optimax_rogue_amd.enums import OBS_COMPACT, OBS_COMPACT_FIELDS, OBS_FIELDS, OBS_INT32
    eng = new_engine(d)
    fmt, R = ((OBS_COMPACT, len(OBS_COMPACT_FIELDS)) if d.rows == "compact"
              else (OBS_INT32, len(OBS_FIELDS)))
    t0 = 0
    for n in (d.T // 2, d.T - d.T // 2):
        what = f"{msg} step_n rows {d.rows} ticks {t0}..{t0 + n} poison {poison:#x}"
        want = run.rows[t0:t0 + n]
        if d.rows == "none":
            eng.step_n(acts[t0:t0 + n], npc_moves=tab[t0:t0 + n])
        else:
            g = Guarded(eng.device, torch.int32, (n, R, d.B), poison)
            eng.step_n(acts[t0:t0 + n], obs=g.out, obs_format=fmt, npc_moves=tab[t0:t0 + n])
            if d.rows == "compact":
                g.check(g.out.cpu().numpy(), what)      # (the guard bytes)
                same(decode_compact(g.out), want, what)
            else:
                g.check(want, what)
        t0 += n
        assert np.array_equal(eng.status.cpu().numpy(), run.status[t0]), what
    both_ways(eng.snapshot(), run.final, d.K, f"{msg} step_n final")


def played(run, t):
    """What the engine writes into ``engine.actions`` on step t: the pair
    played, a value outside the Move codes as 0; only the games in progress
    play one."""
    a = run.played[t]
    return np.where((a >= 1) & (a <= 5), a, 0).astype(np.int8), run.status[t] == gs.IN_PROGRESS


def learner_actions(d, actions, t, dev):
    import torch
    a = actions[t] if d.opponent is None else np.ascontiguousarray(actions[t, :, 0])
    return torch.from_numpy(gs.as_dtype(a, d.act_dtype).copy()).to(dev)


def leg_vecenv(d, run, table, actions, msg):
    """Leg D."""
    import torch
    from optimax_rogue_amd import VecEnv
    dev = torch.device("cuda", 0)
    env = VecEnv(gs.env_config(d), d.B, seed=d.seed, game_offset=d.off, device=dev,
                 opponent=d.opponent, out_buffers=d.out_buffers, check_every=1 << 30)
    rew_sum, done_sum = np.zeros(d.B, np.float64), np.zeros(d.B, np.int64)
    for t in range(d.T):
        what = f"{msg} VecEnv.step t={t + 1}"
        tab = torch.from_numpy(gs.as_dtype(table[t], d.table_dtype).copy()).to(dev)
        obs, reward, done, status = env.step(learner_actions(d, actions, t, dev), npc_moves=tab)
        w_rew, w_done = gs.outcome(run.status[t], run.status[t + 1])
        same(obs, np.ascontiguousarray(run.rows[t].T), what + " obs")
        same(reward, w_rew, what + " reward")
        same(done, w_done, what + " done")
        same(status, run.status[t + 1], what + " status")
        want, live = played(run, t)
        got = env.engine.actions.cpu().numpy()
        assert np.array_equal(got[live], want[live]), what + " actions played"
        rew_sum += w_rew
        done_sum += w_done
    refused = int(((run.status[:-1] == gs.IN_PROGRESS)
                   & (run.status[1:] == gs.BAD_ACTION_STATUS)).sum())
    assert env.bad_actions() == refused, (msg, env.bad_actions(), refused)
    both_ways(env.engine.snapshot(), run.final, d.K, f"{msg} VecEnv final")
    # the rewards are the episode returns; every done is a result or a refusal
    ret = env.engine.episode_returns().cpu().numpy()
    assert np.array_equal(ret[0], run.final["ret_sum"]), msg
    assert np.array_equal(ret[1], run.final["ep_count"]), msg
    assert np.array_equal(rew_sum.astype(np.int64), run.final["ret_sum"].astype(np.int64)), msg
    stops = ((run.status[:-1] == gs.IN_PROGRESS) & (run.status[1:] >= 16)).sum(axis=0)
    assert np.array_equal(done_sum, run.final["ep_count"].astype(np.int64) + stops), msg


def leg_env_slot(d, run, table, actions, msg):
    """Leg E."""
    import torch
    from optimax_rogue_amd.enums import OBS_FIELDS, Policy
    eng = new_engine(d)
    dev, B = eng.device, d.B
    tab = torch.from_numpy(table).to(dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    outs = {p: (Guarded(dev, torch.int32, (B, len(OBS_FIELDS)), p, skew=4),
                Guarded(dev, torch.float32, (B,), p), Guarded(dev, torch.uint8, (B,), p),
                Guarded(dev, torch.int32, (B,), p)) for p in POISONS}
    go = {p: eng.env_step_slot(Policy.NONE if d.opponent is None else d.opponent,
                               *(g.out for g in outs[p]), bad) for p in POISONS}
    nb = torch.empty((), dtype=getattr(torch, d.act_dtype)).element_size()
    for t in range(d.T):
        p = POISONS[t % 2]
        what = f"{msg} env_step_slot t={t + 1} poison {p:#x}"
        for g in outs[p]:
            g.buf.fill_(p)
        a = learner_actions(d, actions, t, dev)
        go[p](a.data_ptr(), nb, a.dim(), None, tab[t].data_ptr())
        w_rew, w_done = gs.outcome(run.status[t], run.status[t + 1])
        for g, want, name in zip(outs[p], (np.ascontiguousarray(run.rows[t].T), w_rew,
                                           w_done.astype(np.uint8), run.status[t + 1]),
                                 ("obs", "reward", "done", "status")):
            g.check(want, f"{what} {name}")
    assert torch.equal(tab.cpu(), torch.from_numpy(table)), f"{msg} env_step_slot: table changed"
    both_ways(eng.snapshot(), run.final, d.K, f"{msg} env_step_slot final")


@pytest.mark.parametrize("case", range(gs.N_CASES))
def test_given_tick_equals_the_oracle(case, oracle_lib):
    import torch
    d = CASES[case]
    msg = gs.where(d)
    table, actions = gs.tables(d)
    cfg, bank = gs.env_config(d), gs.bank_of(d)
    run = gs.play(d, table, actions)
    dev = torch.device("cuda", 0)
    acts, tab = torch.from_numpy(actions).to(dev), torch.from_numpy(table).to(dev)

    def logs_unchanged(leg):
        assert torch.equal(acts.cpu(), torch.from_numpy(actions)), f"{msg} {leg}: actions changed"
        assert torch.equal(tab.cpu(), torch.from_numpy(table)), f"{msg} {leg}: table changed"

    engine_tally = leg_events(d, run, table, actions, acts, tab, cfg, bank, msg)
    logs_unchanged("events")
    TALLIES[case] = (engine_tally, gs.tally(d, run.status, run.final, run.samples,
                                            run.c_tally["npc_kill"]))
    leg_plain(d, run, acts, tab, msg)
    logs_unchanged("step")
    if not d.keyed:
        return   # (orx_npc_step_n and orx_npc_env_step refuse stock-seed mode)
    for poison in POISONS if d.rows != "none" else POISONS[:1]:
        leg_step_n(d, run, acts, tab, poison, msg)
    logs_unchanged("step_n")
    env_run = run if d.opponent is None else gs.play(d, table, actions, opponent=d.opponent,
                                                     events=False)
    leg_vecenv(d, env_run, table, actions, msg)
    if case % 2:
        leg_env_slot(d, env_run, table, actions, msg)
    torch.cuda.synchronize()


def test_engine_runs_cover_the_given_tick():
    """given_sweep.check_coverage on what the ENGINE's runs gave (leg A's
    status, final counters, event records and sampled states of the cases
    above), equal count for count to the oracle's."""
    if gs.N_CASES < 96:
        pytest.skip("the coverage conditions are those of the whole sweep")
    import torch
    for d in CASES:
        if d.case not in TALLIES:   # (a case that did not run in this process: leg A here)
            table, actions = gs.tables(d)
            run = gs.play(d, table, actions)
            dev = torch.device("cuda", 0)
            got = leg_events(d, run, table, actions, torch.from_numpy(actions).to(dev),
                             torch.from_numpy(table).to(dev), gs.env_config(d), gs.bank_of(d),
                             gs.where(d))
            TALLIES[d.case] = (got, gs.tally(d, run.status, run.final, run.samples,
                                             run.c_tally["npc_kill"]))
    for d in CASES:
        engine, oracle = TALLIES[d.case]
        assert engine == oracle, (gs.where(d), engine, oracle)
    total = gs.add_up(TALLIES[d.case][0] for d in CASES)
    print("engine coverage:", total)
    gs.check_coverage(total)
    stock = sum(not d.keyed for d in CASES)
    assert stock <= gs.MAX_STOCK * len(CASES), stock
