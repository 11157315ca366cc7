"""The given-tick sweep's draw and the checks tests/test_given_sweep.py (CPU,
the oracle alone) and tests/test_gpu_given_sweep.py (the engine) share.

``draw(case)`` is ``test_gpu_fuzz._draw(case, base=GBASE)`` brought into the
domain of the tick with the NPCs' moves supplied by the caller
(include/orx_npc.h: n_npcs > 0, flags within 1 | 2) by a stream of its own,
``(GBASE + case) ^ STREAM``, as ``query_sweep.draw`` does: the flags are
masked, K = 0 becomes a K from the edges of the kernels' instance space (and
about a third of the other cases get one too), ``npc_policy`` stays where it
was drawn (the entry points must not read it).  The same stream fixes T, the
table [T][K][B] and the action log [T][B][2] (both with about 0.3% of their
bytes outside the Move codes, wherever they fall), the dtypes ``VecEnv.step``
is handed, the opponent, the output ring and the row form ``step_n`` is asked
for.  GBASE and the two rates were set on the CPU so that the ORACLE's runs
alone meet ``check_coverage`` (the first base tried did; the table's rate is
capped per game-tick, ``tables``).

``play`` is the oracle's run of a case (what every GPU leg is compared with),
``guard_sample`` what one tick's state and table add to the coverage counts
(numpy, on a ``snapshot()``-shaped dict of either side), ``tally`` a run's
counts and ``check_coverage`` the conditions.
"""
import os
import types

import numpy as np

from test_gpu_fuzz import _draw

# ORX_GSWEEP_CASES / ORX_GSWEEP_BASE widen or move the sweep for ad-hoc runs
N_CASES = int(os.environ.get("ORX_GSWEEP_CASES", "96"))
GBASE = int(os.environ.get("ORX_GSWEEP_BASE", "9000"))
STREAM = 0x61FE7                      # the sweep's own draws: (GBASE + case) ^ STREAM
EDGE_K = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255)
EDGE_SHARE = 0.33                     # of the cases that drew K > 0
BAD_BYTE = 0.003                      # share of the table's bytes outside 1..5 ...
BAD_TICK = 0.05                       # ... but at most this share of a game's ticks holds one
BAD_ACTION = 0.003                    # share of the action log's bytes outside 1..5
BAD_BYTES = (0, 6, -1, 127, -128)
BAD_ACTIONS = (0, 6, -1, 99)
T_RANGE = (40, 80)
T_MIN, NPC_TICKS_MAX = 8, 2_500_000   # the cut of T: T * tick_cost stays under NPC_TICKS_MAX
DTYPES = ("int8", "uint8", "int16", "int32", "int64")
ROWS = ("none", "int32", "compact")
MAX_STOCK = 0.30                      # share of the cases whose step_n / env_step legs skip
STATE_EVERY = 20                      # ticks between the full-state comparisons of a leg
SAMPLE_EVERY, SAMPLE_GAMES = 8, 64    # guard_sample: every 8th tick, the first 64 games
IN_PROGRESS, BAD_ACTION_STATUS = 1, 16
COMPACT_MAX_STAT = 8000               # include/orx.h ORX_COMPACT_MAX_STAT


def compact_ok(cfg: dict) -> bool:
    """What the engine's check_compact accepts (include/orx.h, the compact
    rows' bounds) for a cfg of this sweep (flags within 1 | 2)."""
    m = COMPACT_MAX_STAT
    ok = cfg["width"] <= 256 and cfg["height"] <= 256 and 1 <= cfg["max_ticks"] < (1 << 27)
    ok = ok and cfg["player_health"] <= m and cfg["player_damage"] <= m
    ok = ok and cfg["player_armor"] >= -m and cfg["npc_damage"] <= m
    if cfg["flags"] & 1:
        ok = ok and cfg["max_ticks"] // max(cfg["sep_period"], 1) <= m
    return bool(ok)


def tick_cost(cfg: dict, B: int) -> int:
    """What one tick of the batch costs the oracle, in NPC moves: every NPC's
    move, and the literal scans of the W x H tiles that its resets make."""
    return B * (cfg["n_npcs"] + cfg["width"] * cfg["height"] // 256)


def draw(case: int, base: int = None):
    """The case as a namespace: ``cfg`` (dict), ``layouts``, ``B``, ``pol``,
    ``seed``, ``off`` of the fuzz's draw (K and flags brought into the given
    tick's domain), and ``T`` (``T_drawn`` in 40..80, cut where the batch is
    costly), ``data_seed`` (of ``tables``), ``act_dtype``,
    ``table_dtype``, ``opponent``, ``out_buffers``, ``rows`` (the form step_n
    is asked for), ``rows_drawn``, ``event_games`` [3], ``keyed``."""
    base = GBASE if base is None else base
    cfg, layouts, B, _, seed, off, pol, _ = _draw(case, base=base)
    rs = np.random.RandomState((base + case) ^ STREAM)
    d = types.SimpleNamespace(case=case, layouts=layouts, B=B, pol=pol, seed=seed, off=off)
    cfg["flags"] &= 3
    W, H = cfg["width"], cfg["height"]
    room = ((W - 2) * (H - 2) - 3 if layouts is None
            else int((layouts == 1).sum(axis=(1, 2)).min()) - 3)
    edges = [k for k in EDGE_K if k <= room]
    # both draws are taken whether or not they apply (the later ones stay put)
    lean, pick = rs.rand(), rs.rand()
    d.drawn_K = cfg["n_npcs"]
    if cfg["n_npcs"] == 0 or lean < EDGE_SHARE:
        cfg["n_npcs"] = edges[int(pick * len(edges))]
    # T: 40..80, cut where the oracle's run of the batch would take more than a
    # few seconds -- the ticks, not the space
    d.T_drawn = int(rs.randint(T_RANGE[0], T_RANGE[1] + 1))
    d.T = min(d.T_drawn, max(T_MIN, NPC_TICKS_MAX // tick_cost(cfg, B)))
    d.data_seed = int(rs.randint(0, 2 ** 31))
    d.act_dtype = str(rs.choice(DTYPES))
    d.table_dtype = str(rs.choice(DTYPES))
    d.opponent = [None, 1, 2][int(rs.randint(0, 3))]
    d.out_buffers = int(rs.choice([0, 2]))
    d.rows_drawn = str(rs.choice(ROWS))
    d.rows = "int32" if d.rows_drawn == "compact" and not compact_ok(cfg) else d.rows_drawn
    d.event_games = [int(g) for g in rs.randint(0, B, size=3)]
    d.cfg = cfg
    d.K = cfg["n_npcs"]
    d.keyed = not cfg.get("rng")
    return d


def tables(d):
    """``(table, actions)``: int8 [T][K][B] and [T][B][2], uniform 1..5 with the
    two rates of bytes outside the Move codes (the table's capped at BAD_TICK
    / K: at 0.3% of the bytes a game of 255 NPCs would be stopped every other
    tick and never get anywhere)."""
    rs = np.random.RandomState(d.data_seed)
    table = rs.randint(1, 6, size=(d.T, d.K, d.B)).astype(np.int8)
    bad = rs.rand(d.T, d.K, d.B) < min(BAD_BYTE, BAD_TICK / d.K)
    table[bad] = rs.choice(np.array(BAD_BYTES, np.int8), size=int(bad.sum()))
    actions = rs.randint(1, 6, size=(d.T, d.B, 2)).astype(np.int8)
    bad = rs.rand(d.T, d.B, 2) < BAD_ACTION
    actions[bad] = rs.choice(np.array(BAD_ACTIONS, np.int8), size=int(bad.sum()))
    return table, actions


def as_dtype(a: np.ndarray, name: str) -> np.ndarray:
    """The int8 log in the dtype a learner hands over: sign-extended, and for
    uint8 the same bytes (-1 is 255: still outside the Move codes)."""
    return a.view(np.uint8) if name == "uint8" else a.astype(name)


def where(d) -> str:
    """What a failure message needs to run the case again alone."""
    return (f"given sweep case {d.case} (base {GBASE}) {d.cfg} B={d.B} T={d.T} seed={d.seed} "
            f"off={d.off} bank={d.layouts is not None} dtypes={d.act_dtype}/{d.table_dtype} "
            f"opponent={d.opponent} ring={d.out_buffers} rows={d.rows}")


def check_draw(d) -> None:
    """orx_validate_cfg's rules, the given tick's domain, the engine's room for
    the NPCs and the cap on the compact rows' skips."""
    cfg = d.cfg
    assert cfg["width"] >= 4 and cfg["height"] >= 4, where(d)
    assert 1 <= d.K <= 255 and not cfg["flags"] & ~3, where(d)
    assert d.K == d.drawn_K or d.K in EDGE_K, where(d)
    if d.layouts is not None:
        assert (d.layouts == 1).sum(axis=(1, 2)).min() >= d.K + 2, where(d)
    else:
        assert (cfg["width"] - 2) * (cfg["height"] - 2) - 1 >= d.K + 2, where(d)
    assert T_RANGE[0] <= d.T_drawn <= T_RANGE[1] and T_MIN <= d.T <= d.T_drawn, where(d)
    assert d.T == d.T_drawn or d.T == T_MIN or (d.T + 1) * tick_cost(cfg, d.B) > NPC_TICKS_MAX, \
        where(d)
    assert d.B <= 1531, where(d)
    assert all(0 <= g < d.B for g in d.event_games), where(d)
    # compact rows are given up only where check_compact would refuse the cfg
    assert (d.rows != d.rows_drawn) == (d.rows_drawn == "compact" and not compact_ok(cfg)), where(d)
    assert d.rows == "int32" or d.rows == d.rows_drawn, where(d)


def env_config(d):
    from optimax_rogue_amd import EnvConfig
    return EnvConfig.from_dict(d.cfg, layouts=d.layouts)


def bank_of(d):
    if d.layouts is None:
        return None
    from optimax_rogue_amd import DungeonBank
    return DungeonBank(np.array(d.layouts))


def obs_rows(s: dict) -> np.ndarray:
    """The 14 observation fields [14, B] of an engine-layout state."""
    return np.stack([s["p_x"][0], s["p_y"][0], s["p_depth"][0], s["p_health"][0],
                     s["p_x"][1], s["p_y"][1], s["p_depth"][1], s["p_health"][1],
                     s["tick"], s["status"], s["st_x"][0], s["st_y"][0], s["st_x"][1],
                     s["st_y"][1]]).astype(np.int32)


def outcome(before: np.ndarray, after: np.ndarray):
    """(reward float32, done bool) of one step from its two status vectors: a
    game that was in progress and is no longer is done -- by a result (1 for
    Player1Win = 2, -1 for Player2Win = 3, 0 for Tie = 4) or by an engine stop
    code (>= 16, reward 0).  A step that restarts a game is not done."""
    done = (before == IN_PROGRESS) & (after != IN_PROGRESS)
    reward = np.where(done & (after == 2), 1.0, np.where(done & (after == 3), -1.0, 0.0))
    return reward.astype(np.float32), done


def _first(snap: dict, n: int) -> dict:
    """The first ``n`` games of the fields npc_query.options reads."""
    keys = ("p_x", "p_y", "p_depth", "p_health", "st_x", "st_y", "p_layout", "npc_pos",
            "npc_health", "npc_alive", "status")
    return {k: np.asarray(snap[k])[..., :n] for k in keys if k in snap}


def guard_sample(cfg, bank, snap: dict, table_t: np.ndarray, actions_t: np.ndarray,
                 n_games: int = SAMPLE_GAMES) -> dict:
    """What the tick that plays ``table_t`` [K][B] and ``actions_t`` [B][2] on
    the state ``snap`` does with the table, over the first ``n_games`` games,
    per game (int64 [n] each): ``live_bad`` (a byte outside 1..5 in a live
    slot of a game in progress: the tick is refused), ``live_bad_high`` (...
    and every such slot is 32 or above: dense NPCs' second alive word on), ``dead_bad`` (a tick
    that is played although a dead slot holds such a byte), ``guard1`` /
    ``guard2`` / ``guard3`` (non-Stay bytes of live slots that the guard
    replaces in a played tick) and ``unwatched`` (games whose NPC depth exists
    with no player on it: the snapshot does not hold that dungeon, so their
    guard counts are left at 0).  From npc_query.options, the numpy reference
    of orx_npc_options (held to the guards by tests/test_npc_query.py)."""
    from optimax_rogue_amd import npc_query
    from optimax_rogue_amd.enums import (NPC_DEPTH_GONE, NPC_DEPTH_UNWATCHED, NPC_DEPTH_WATCHED,
                                         NPC_OUT_BLOCKED, NPC_OUT_FROZEN, NPC_OUT_MASK,
                                         NPC_OUT_REST)
    s = _first(snap, n_games)
    n = len(s["status"])
    kind, _, _, depth = npc_query.options(s, cfg, bank)            # [K, n, 8], [n]
    kind = kind.astype(np.int64) & NPC_OUT_MASK
    alive = kind[:, :, 5] == NPC_OUT_REST
    tb = table_t[:, :n].astype(np.int64)
    bad = (tb < 1) | (tb > 5)
    a = actions_t[:n].astype(np.int64)
    in_progress = s["status"] == IN_PROGRESS
    live_bad = in_progress & (bad & alive).any(axis=0)
    high = np.arange(len(tb))[:, None] >= 32          # the second and later alive words
    live_bad_high = in_progress & (bad & alive & high).any(axis=0) \
        & ~(bad & alive & ~high).any(axis=0)
    played = in_progress & ~live_bad & ((a >= 1) & (a <= 5)).all(axis=1)
    dead_bad = played & (bad & ~alive).any(axis=0)
    does = np.take_along_axis(kind, np.clip(tb, 1, 5)[:, :, None], axis=2)[:, :, 0]
    moves = alive & played[None] & ~bad & (tb != 5)
    frozen = moves & (does == NPC_OUT_FROZEN)
    out = dict(live_bad=live_bad, dead_bad=dead_bad, live_bad_high=live_bad_high,
               guard1=(frozen & (depth == NPC_DEPTH_GONE)[None]).sum(axis=0),
               guard2=(frozen & (depth == NPC_DEPTH_WATCHED)[None]).sum(axis=0),
               guard3=(moves & (does == NPC_OUT_BLOCKED)).sum(axis=0),
               unwatched=depth == NPC_DEPTH_UNWATCHED)
    return {k: np.asarray(v).astype(np.int64) for k, v in out.items()}


def sampled(t: int) -> bool:
    return t % SAMPLE_EVERY == 0


def play(d, table, actions, opponent=None, events=True, n_games=None):
    """The oracle's run of the case over ``table`` and ``actions`` (player 2's
    move from ``ora.policy(0, opponent, given)`` where there is an opponent).
    A namespace: ``status`` [T + 1][B] (row 0: after the reset), ``rows``
    [T][14][B], ``played`` [T][B][2], ``states`` {t: export after step t} for
    every STATE_EVERY-th step and the last, ``events`` [T] -> {game: records}
    of ``d.event_games``, ``samples`` {t: guard_sample before step t},
    ``final`` (the last export), ``c_tally`` (Oracle.given_tally summed)."""
    from oracle.oracle import Oracle
    n = d.B if n_games is None else int(n_games)
    cfg, bank = env_config(d), bank_of(d)
    ora = Oracle(d.cfg, n, d.seed, d.off, record_events=events, layouts=d.layouts)
    ora.reset(episode=np.zeros(n, np.int32))
    r = types.SimpleNamespace(ora=ora, states={}, events=[], samples={}, reset=ora.export())
    r.status = np.zeros((d.T + 1, n), np.int32)
    r.rows = np.zeros((d.T, 14, n), np.int32)
    r.played = np.zeros((d.T, n, 2), np.int8)
    r.status[0] = r.reset["status"]
    snap = r.reset
    for t in range(d.T):
        a = actions[t, :n]
        if opponent is not None:
            a = ora.policy(0, opponent, a)
        if sampled(t):
            r.samples[t] = guard_sample(cfg, bank, snap, table[t][:, :n], a)
        ora.step(a, npc_moves=np.ascontiguousarray(table[t][:, :n]))
        snap = ora.export()
        r.played[t], r.status[t + 1], r.rows[t] = a, snap["status"], obs_rows(snap)
        if events:
            r.events.append({g: ora.events(g) for g in d.event_games if g < n})
        if t % STATE_EVERY == STATE_EVERY - 1 or t == d.T - 1:
            r.states[t] = snap
    r.final = snap
    r.c_tally = {k: int(v.sum()) for k, v in ora.given_tally().items()}
    return r


def ncap_class(K: int) -> str:
    return "ncap8" if K <= 8 else "ncap16" if K <= 16 else "dense"


def tally(d, status, final, samples, npc_kill) -> dict:
    """A run's coverage counts, from what either side gives: the draw's kind,
    ``status`` [T + 1][B] of every step, the ``final`` state's counters, the
    ``samples`` of guard_sample and the count of ticks that left a player at
    health <= 0 after an NPC's blow took health from it."""
    c = {}

    def add(name, n):
        c[name] = c.get(name, 0) + int(n)

    cfg, K = d.cfg, d.K
    add(f"{ncap_class(K)}_{'bank' if d.layouts is not None else 'plain'}", 1)
    add("dense_gt32", K > 32)
    add("dense_gt64", K > 64)
    for k in (1, 8, 9, 16, 17):
        add(f"K{k}", K == k)
    add("stock", bool(cfg.get("rng")))
    add("flag1", bool(cfg["flags"] & 1))
    add("flag2", bool(cfg["flags"] & 2))
    add("start_mode2", cfg.get("start_mode") == 2)
    add("despawn1", cfg["despawn"] == 1)
    add("despawn2", cfg["despawn"] == 2)
    add("max_ticks0", cfg["max_ticks"] == 0)
    add("B1", d.B == 1)
    add("B1531", d.B == 1531)
    add("npc_policy_kept", bool(cfg.get("npc_policy")))
    add("cases", 1)
    add("stock_cases", not d.keyed)
    status = np.asarray(status)
    add("refused", ((status[:-1] == IN_PROGRESS) & (status[1:] == BAD_ACTION_STATUS)).sum())
    add("finished", ((status[:-1] == IN_PROGRESS) & (status[1:] >= 2) & (status[1:] <= 4)).sum())
    counters = np.asarray(final["counters"]).astype(np.int64)
    add("combat", counters[0].sum())
    add("descend", counters[1].sum())
    add("dungeon", counters[2].sum())
    add("npc_death", counters[3].sum())
    add("autoreset", np.asarray(final["episode"]).astype(np.int64).sum())
    add("npc_kill", npc_kill)
    for s in samples.values():
        watched = s["unwatched"] == 0
        for k in ("live_bad", "live_bad_high", "dead_bad"):
            add("sample_" + k, s[k].sum())
        for k in ("guard1", "guard2", "guard3"):
            add("sample_" + k, s[k][watched].sum())
    return c


def add_up(tallies) -> dict:
    total = {}
    for c in tallies:
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    return total


# every count must be positive over the whole sweep (conditions, not measurements)
COVERAGE = tuple(
    [f"{n}_{b}" for n in ("ncap8", "ncap16", "dense") for b in ("bank", "plain")]
    + ["dense_gt32", "dense_gt64", "K1", "K8", "K9", "K16", "K17", "stock", "flag1", "flag2",
       "start_mode2", "despawn1", "despawn2", "max_ticks0", "B1", "B1531", "npc_policy_kept",
       "refused", "finished", "combat", "descend", "dungeon", "npc_death", "autoreset", "npc_kill",
       "sample_live_bad", "sample_live_bad_high", "sample_dead_bad", "sample_guard1", "sample_guard2", "sample_guard3"])
# ... and, on the CPU, the oracle's own counts over every game and tick
ORACLE_COVERAGE = ("guard1", "guard2", "guard3", "refused", "dead_bad", "npc_kill")


def check_coverage(total: dict, oracle_total: dict = None) -> None:
    """Every count of COVERAGE is positive (and of ORACLE_COVERAGE where the
    oracle's own tallies are given), and at most MAX_STOCK of the cases skip
    the legs the engine refuses in stock-seed mode; names what is short."""
    short = [k for k in COVERAGE if total.get(k, 0) <= 0]
    if oracle_total is not None:
        short += ["oracle " + k for k in ORACLE_COVERAGE if oracle_total.get(k, 0) <= 0]
    assert not short, f"coverage short: {short}; all: {total} {oracle_total}"
    assert total["stock_cases"] <= MAX_STOCK * total["cases"], total
