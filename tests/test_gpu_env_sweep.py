"""GPU: the learner's tick, ``VecEnv.step`` (orx_env_step_args in one launch;
orx_policy + orx_step in stock-seed mode), over the fuzz's UNMODIFIED draws
(test_gpu_fuzz._draw at a base of its own): every extension flag, no NPCs,
register and dense NPCs, Stay and moving NPCs, items, heals (action 6 valid),
banks, stock seeding, batches of 1 to 1531 -- against the C oracle, which
shares no code with the kernels.

Per case, for the case's ticks (at most 80, fewer where the oracle's run of
the batch would take more than a few seconds):
  * ``VecEnv.step`` with the drawn action dtype, opponent (None: self-play,
    RandomBot, StaircaseBot) and output ring; player 2's move on the oracle's
    side is ``ora.policy(0, opponent, given)``;
  * obs, reward, done, status and the actions played are compared every tick
    (reward and done against a numpy restatement from the oracle's two status
    vectors), the whole state at the end, ``episode_returns()`` with the
    oracle's sums;
  * about 0.3% of the learner's actions are outside the Move codes, and
    ``bad_actions()`` must count exactly the game-ticks they stopped;
  * on keyed cases the action log the oracle recorded is then replayed through
    orx_step_n in two launches, with int32 rows on even cases and compact rows
    on odd ones (int32 where check_compact refuses the cfg), and the rows are
    the oracle's.
All values are integers (reward: -1, 0, 1): every comparison is exact.
"""
import types

import numpy as np
import pytest

import given_sweep as gs
from golden_util import compare_state
from guarded import same
from test_gpu_fuzz import HEAL, ITEMS, MANA, _draw

N_CASES = 96
EBASE = 13000
STREAM = 0xE57E9                      # the sweep's own draws: (EBASE + case) ^ STREAM
BAD_ACTION = 0.003
T_MAX = 80


def compact_ok(cfg: dict) -> bool:
    """What the engine's check_compact accepts (include/orx.h), every flag."""
    m = gs.COMPACT_MAX_STAT
    ok = gs.compact_ok(dict(cfg, flags=cfg["flags"] & 1))
    if cfg["flags"] & MANA:
        ok = ok and cfg["mana_max"] <= m
    if cfg["flags"] & ITEMS:
        ok = ok and cfg["item_bonus"] * cfg["item_slots"] <= m
    return bool(ok)


def draw(case: int):
    cfg, layouts, B, T, seed, off, pol, _ = _draw(case, base=EBASE)
    rs = np.random.RandomState((EBASE + case) ^ STREAM)
    d = types.SimpleNamespace(case=case, cfg=cfg, layouts=layouts, B=B, seed=seed, off=off,
                              K=cfg["n_npcs"], keyed=not cfg.get("rng"))
    d.T = min(T, T_MAX, max(gs.T_MIN, gs.NPC_TICKS_MAX // max(1, gs.tick_cost(cfg, B))))
    d.data_seed = int(rs.randint(0, 2 ** 31))
    d.act_dtype = str(rs.choice(gs.DTYPES))
    d.opponent = [None, 1, 2][int(rs.randint(0, 3))]
    d.out_buffers = int(rs.choice([0, 2]))
    d.hi = 6 if cfg["flags"] & HEAL else 5
    d.rows = "compact" if case % 2 and compact_ok(cfg) else "int32"
    return d


CASES = [draw(c) for c in range(N_CASES)]


def where(d) -> str:
    return (f"env sweep case {d.case} (base {EBASE}) {d.cfg} B={d.B} T={d.T} seed={d.seed} "
            f"off={d.off} bank={d.layouts is not None} dtype={d.act_dtype} opponent={d.opponent} "
            f"ring={d.out_buffers} rows={d.rows}")


def action_log(d) -> np.ndarray:
    """int8 [T][B][2]: uniform over the Move codes (the heal where it is one),
    about 0.3% of the bytes outside them."""
    rs = np.random.RandomState(d.data_seed)
    a = rs.randint(1, d.hi + 1, size=(d.T, d.B, 2)).astype(np.int8)
    bad = rs.rand(d.T, d.B, 2) < BAD_ACTION
    a[bad] = rs.choice(np.array([0, -1, d.hi + 1, 99], np.int8), size=int(bad.sum()))
    return a


def classes(d) -> set:
    K = d.K
    ncap = "ncap0" if K == 0 else gs.ncap_class(K)
    out = {f"{ncap}_{'bank' if d.layouts is not None else 'plain'}",
           "flags on" if d.cfg["flags"] else "flags off", f"opponent {d.opponent}",
           "rows " + d.rows, "act " + d.act_dtype, f"ring {d.out_buffers}"}
    out |= {"moving"} if d.cfg.get("npc_policy") else set()
    out |= {"stock"} if not d.keyed else set()
    out |= {"heal"} if d.cfg["flags"] & HEAL else set()
    out |= {"items"} if d.cfg["flags"] & ITEMS and K else set()
    return out


WANT = ({f"{n}_{b}" for n in ("ncap0", "ncap8", "ncap16", "dense") for b in ("bank", "plain")}
        | {"flags on", "flags off", "moving", "stock", "heal", "items", "rows int32",
           "rows compact", "ring 0", "ring 2"} | {f"opponent {o}" for o in (None, 1, 2)}
        | {"act " + t for t in gs.DTYPES})


def test_draws_cover_every_class():
    """All eight (NCAP 0 / 8 / 16 / dense) x bank classes, flags on and off,
    moving NPCs, stock seeding, heals, items and every drawn form occur among
    the cases the GPU test below is parametrised over."""
    seen = set()
    for d in CASES:
        seen |= classes(d)
        assert 8 <= d.T <= T_MAX and d.B <= 1531, where(d)
    assert WANT <= seen, WANT - seen
    assert _draw(3)[0] == _draw(3, base=1000)[0]   # (the fuzz's own draws are what they were)


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(N_CASES))
def test_vecenv_step_equals_the_oracle(case, oracle_lib):
    import torch
    from optimax_rogue_amd import VecEnv
    from optimax_rogue_amd.engine import BatchedEngine, decode_compact
    from optimax_rogue_amd.enums import OBS_COMPACT, OBS_COMPACT_FIELDS, OBS_FIELDS, OBS_INT32
    d = CASES[case]
    msg = where(d)
    cfg = gs.env_config(d)
    dev = torch.device("cuda", 0)
    log = action_log(d)
    ora = oracle_lib.Oracle(d.cfg, d.B, d.seed, d.off, layouts=d.layouts)
    ora.reset(episode=np.zeros(d.B, np.int32))
    env = VecEnv(cfg, d.B, seed=d.seed, game_offset=d.off, device=dev, opponent=d.opponent,
                 out_buffers=d.out_buffers, check_every=1 << 30)
    for a, b in ((env.engine.snapshot(), ora.export()), (ora.export(), env.engine.snapshot())):
        compare_state(a, b, d.K, f"{msg} reset")
    before = ora.export()["status"]
    rows, played, refused = [], [], 0
    for t in range(d.T):
        what = f"{msg} t={t + 1}"
        given = log[t]
        a = given if d.opponent is None else ora.policy(0, d.opponent, given)
        ora.step(a)
        s = ora.export()
        learner = given if d.opponent is None else np.ascontiguousarray(given[:, 0])
        obs, reward, done, status = env.step(
            torch.from_numpy(gs.as_dtype(learner, d.act_dtype).copy()).to(dev))
        w_rew, w_done = gs.outcome(before, s["status"])
        rows.append(gs.obs_rows(s))
        same(obs, np.ascontiguousarray(rows[-1].T), what + " obs")
        same(reward, w_rew, what + " reward")
        same(done, w_done, what + " done")
        same(status, s["status"], what + " status")
        live = before == gs.IN_PROGRESS
        want = np.where((a >= 1) & (a <= d.hi), a, 0).astype(np.int8)
        got = env.engine.actions.cpu().numpy()
        assert np.array_equal(got[live], want[live]), what + " actions played"
        refused += int((live & (s["status"] == gs.BAD_ACTION_STATUS)).sum())
        played.append(np.array(a, np.int8))
        before = s["status"]
    final = ora.export()
    compare_state(env.engine.snapshot(), final, d.K, f"{msg} final")
    compare_state(final, env.engine.snapshot(), d.K, f"{msg} final")
    ret = env.engine.episode_returns().cpu().numpy()
    assert np.array_equal(ret[0], final["ret_sum"]) and np.array_equal(ret[1], final["ep_count"]), msg
    assert env.bad_actions() == refused, (msg, env.bad_actions(), refused)
    if not d.keyed:
        return   # (orx_step_n refuses stock-seed mode)
    # the recorded log through orx_step_n, in two launches
    eng = BatchedEngine(cfg, d.B, seed=d.seed, game_offset=d.off, device=dev)
    acts = torch.from_numpy(np.stack(played)).to(dev)
    rows = np.stack(rows)
    fmt, R = ((OBS_COMPACT, len(OBS_COMPACT_FIELDS)) if d.rows == "compact"
              else (OBS_INT32, len(OBS_FIELDS)))
    t0 = 0
    for n in (d.T // 2, d.T - d.T // 2):
        out = torch.zeros((n, R, d.B), dtype=torch.int32, device=dev)
        eng.step_n(acts[t0:t0 + n], obs=out, obs_format=fmt)
        got = decode_compact(out) if d.rows == "compact" else out
        same(got, rows[t0:t0 + n], f"{msg} step_n rows {d.rows} ticks {t0}..{t0 + n}")
        t0 += n
    compare_state(eng.snapshot(), final, d.K, f"{msg} step_n final")
    compare_state(final, eng.snapshot(), d.K, f"{msg} step_n final")
    torch.cuda.synchronize()
