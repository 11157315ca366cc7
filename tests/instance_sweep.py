"""The ledger of rollout and replay kernel instances, and one small request
per instance (shared by test_instance_sweep.py on the CPU and
test_gpu_instance_sweep.py on the GPU; numpy only, no torch, no GPU).

orx_rollout and orx_step_n dispatch to explicit template instantiations named
by X-macro lists in optimax_rogue_amd/csrc/orx_engine.hip.  The five lists are
restated here by hand, in the template-argument order the macros use;
``instance_of`` restates the dispatch of orx_rollout_ex and launch_step_n over
a plan of tests/plan_main.cpp; ``REQUESTS`` is a written-down table with at
least one request per instance: a configuration, a bank or none, the bots, the
row format, which outputs are given and the ORX_* overrides that pin the plan
whatever the device.  ``run_oracle`` plays a request's three launches on the C
oracle and says what the run contained (the witnesses).

Shapes: 257 games (whole workgroups plus a last wave of one game at 8, 16, 32
and 64 games per wave alike), a non-zero game offset, a 12 x 10 grid, 0 / 5 /
12 / 30 NPCs for NCAP 0 / 8 / 16 / dense, max_ticks 24 and three launches of 20
ticks, so episodes end and restart inside a launch and the state crosses
launches twice.
"""
from collections import namedtuple

import numpy as np

S, P = True, False        # AUX: kStreamAux (nontemporal rows) / kPartialAux
T, F = True, False
DENSE = 256               # kDense
B, N_LAUNCHES, N_TICKS = 257, 3, 20
W, H, MAX_TICKS = 12, 10, 24
K_OF = {0: 0, 8: 5, 16: 12, DENSE: 30}
MANA, HEAL, LEVEL, ITEMS, README = 4, 8, 16, 32, 64

# ---------------------------------------------------------------------------
# The instance lists of orx_engine.hip, by hand.
# ---------------------------------------------------------------------------
# ORX_PAIR_LIST: pair_rollout_kernel<NCAP, PM, AUX, SEP, CF, GRID>
PAIR_LIST = (
    # ORX_PAIR_LIST_A(0), ORX_PAIR_LIST_B(0)
    (0, 1, S, F, F, F), (0, 1, P, F, F, F), (0, 2, S, F, F, F), (0, 2, P, F, F, F),
    (0, 2, S, T, F, F), (0, 2, P, T, F, F),
    (0, 1, S, F, T, F), (0, 1, P, F, T, F), (0, 2, S, F, T, F), (0, 2, P, F, T, F),
    (0, 2, S, T, T, F), (0, 2, P, T, T, F),
    (0, 3, S, F, F, F), (0, 3, P, F, F, F), (0, 3, S, F, F, T), (0, 3, P, F, F, T),
    (0, 1, S, F, F, T), (0, 1, P, F, F, T), (0, 2, S, F, F, T), (0, 2, P, F, F, T),
    # ORX_PAIR_LIST_A(8), ORX_PAIR_LIST_B(8)
    (8, 1, S, F, F, F), (8, 1, P, F, F, F), (8, 2, S, F, F, F), (8, 2, P, F, F, F),
    (8, 2, S, T, F, F), (8, 2, P, T, F, F),
    (8, 1, S, F, T, F), (8, 1, P, F, T, F), (8, 2, S, F, T, F), (8, 2, P, F, T, F),
    (8, 2, S, T, T, F), (8, 2, P, T, T, F),
    (8, 3, S, F, F, F), (8, 3, P, F, F, F), (8, 3, S, F, F, T), (8, 3, P, F, F, T),
    (8, 1, S, F, F, T), (8, 1, P, F, F, T), (8, 2, S, F, F, T), (8, 2, P, F, F, T),
    # ORX_PAIR_LIST_A(16), ORX_PAIR_LIST_B(16)
    (16, 1, S, F, F, F), (16, 1, P, F, F, F), (16, 2, S, F, F, F), (16, 2, P, F, F, F),
    (16, 2, S, T, F, F), (16, 2, P, T, F, F),
    (16, 1, S, F, T, F), (16, 1, P, F, T, F), (16, 2, S, F, T, F), (16, 2, P, F, T, F),
    (16, 2, S, T, T, F), (16, 2, P, T, T, F),
    (16, 3, S, F, F, F), (16, 3, P, F, F, F), (16, 3, S, F, F, T), (16, 3, P, F, F, T),
    (16, 1, S, F, F, T), (16, 1, P, F, F, T), (16, 2, S, F, F, T), (16, 2, P, F, F, T),
    # ORX_PAIR_LIST_M(0 / 8 / 16)
    (0, 4, S, F, F, F), (0, 4, P, F, F, F), (0, 5, S, F, F, F), (0, 5, P, F, F, F),
    (8, 4, S, F, F, F), (8, 4, P, F, F, F), (8, 5, S, F, F, F), (8, 5, P, F, F, F),
    (16, 4, S, F, F, F), (16, 4, P, F, F, F), (16, 5, S, F, F, F), (16, 5, P, F, F, F),
)
# ORX_PAIR_LIST_L(0 / 8 / 16): pair_rollout_kernel, PM 6 (orx_step_n's paired replay)
PAIR_LIST_L = (
    (0, 6, S, F, F, F), (0, 6, P, F, F, F), (0, 6, S, F, T, F), (0, 6, P, F, T, F),
    (8, 6, S, F, F, F), (8, 6, P, F, F, F), (8, 6, S, F, T, F), (8, 6, P, F, T, F),
    (16, 6, S, F, F, F), (16, 6, P, F, F, F), (16, 6, S, F, T, F), (16, 6, P, F, T, F),
)
# ORX_ROLLOUT_LIST: rollout_kernel<NCAP, PM, GRID, AUX, CF>
ROLLOUT_LIST = (
    # ORX_ROLLOUT_LIST_N(0)
    (0, 0, F, S, F), (0, 1, F, S, F), (0, 1, F, P, F), (0, 2, F, S, F), (0, 2, F, P, F),
    (0, 3, F, S, F), (0, 3, F, P, F),
    (0, 0, T, S, F), (0, 1, T, S, F), (0, 1, T, P, F), (0, 2, T, S, F), (0, 2, T, P, F),
    (0, 3, T, S, F), (0, 3, T, P, F),
    (0, 1, F, S, T), (0, 1, F, P, T), (0, 2, F, S, T), (0, 2, F, P, T),
    # ORX_ROLLOUT_LIST_N(8)
    (8, 0, F, S, F), (8, 1, F, S, F), (8, 1, F, P, F), (8, 2, F, S, F), (8, 2, F, P, F),
    (8, 3, F, S, F), (8, 3, F, P, F),
    (8, 0, T, S, F), (8, 1, T, S, F), (8, 1, T, P, F), (8, 2, T, S, F), (8, 2, T, P, F),
    (8, 3, T, S, F), (8, 3, T, P, F),
    (8, 1, F, S, T), (8, 1, F, P, T), (8, 2, F, S, T), (8, 2, F, P, T),
    # ORX_ROLLOUT_LIST_N(16)
    (16, 0, F, S, F), (16, 1, F, S, F), (16, 1, F, P, F), (16, 2, F, S, F), (16, 2, F, P, F),
    (16, 3, F, S, F), (16, 3, F, P, F),
    (16, 0, T, S, F), (16, 1, T, S, F), (16, 1, T, P, F), (16, 2, T, S, F), (16, 2, T, P, F),
    (16, 3, T, S, F), (16, 3, T, P, F),
    (16, 1, F, S, T), (16, 1, F, P, T), (16, 2, F, S, T), (16, 2, F, P, T),
    # ORX_ROLLOUT_LIST_DENSE
    (DENSE, 0, F, S, F), (DENSE, 0, T, S, F),
    (DENSE, 1, F, S, F), (DENSE, 1, F, P, F), (DENSE, 2, F, S, F), (DENSE, 2, F, P, F),
    (DENSE, 1, T, S, F), (DENSE, 1, T, P, F), (DENSE, 2, T, S, F), (DENSE, 2, T, P, F),
)
# ORX_NG_LIST: (NCAP, GRID) of lane_rollout_kernel<N, G, true, false> (stock seeding)
NG_LIST = ((0, F), (8, F), (16, F), (DENSE, F), (0, T), (8, T), (16, T), (DENSE, T))
# ORX_MOV_ROLLOUT_LIST: (NCAP, GRID, MT) of lane_rollout_kernel<N, G, MT, true>
MOV_ROLLOUT_LIST = (
    (8, F, F), (16, F, F), (DENSE, F, F), (8, T, F), (16, T, F), (DENSE, T, F),
    (8, F, T), (16, F, T), (DENSE, F, T), (8, T, T), (16, T, T), (DENSE, T, T),
)
# ORX_REPLAY_LIST: replay_kernel<NCAP, ROWS, EXT>
REPLAY_LIST = (
    (0, 0, F), (0, 1, F), (0, 2, F), (8, 0, F), (8, 1, F), (8, 2, F),
    (16, 0, F), (16, 1, F), (16, 2, F),
    (0, 0, T), (0, 1, T), (0, 2, T), (8, 0, T), (8, 1, T), (8, 2, T),
    (16, 0, T), (16, 1, T), (16, 2, T),
)

PAIR, ROLLOUT, LANE, REPLAY = ("pair_rollout_kernel", "rollout_kernel", "lane_rollout_kernel",
                               "replay_kernel")


def ledger():
    """Every instance as (kernel, template arguments)."""
    out = [(PAIR, a) for a in PAIR_LIST + PAIR_LIST_L]
    out += [(ROLLOUT, a) for a in ROLLOUT_LIST]
    out += [(LANE, (n, g, True, False)) for n, g in NG_LIST]
    out += [(LANE, (n, g, mt, True)) for n, g, mt in MOV_ROLLOUT_LIST]
    out += [(REPLAY, a) for a in REPLAY_LIST]
    return out


def instance_name(inst):
    """``kernel<args>`` as the source spells it (kDense, kStreamAux, false ...)."""
    kernel, args = inst
    aux_at = {PAIR: 2, ROLLOUT: 3}.get(kernel, -1)
    words = []
    for i, a in enumerate(args):
        if i == aux_at:
            words.append("kStreamAux" if a else "kPartialAux")
        elif isinstance(a, bool):
            words.append("true" if a else "false")
        else:
            words.append("kDense" if i == 0 and a == DENSE else str(a))
    return "%s<%s>" % (kernel, ", ".join(words))


def ncap_for(K):
    return 0 if K == 0 else 8 if K <= 8 else 16 if K <= 16 else DENSE


# ---------------------------------------------------------------------------
# Requests
# ---------------------------------------------------------------------------
# want: the instance the request exists for; kind: "rollout" / "step_n"; cfg:
# the orx_cfg_t fields that differ from the oracle's defaults; bank: the
# layouts' count or 0; fmt: "int32" / "compact" / None (no rows); act: the
# action buffer is given (rollouts); env: the ORX_* overrides
Request = namedtuple("Request", "want kind cfg bank bots fmt act env seed offset")

_BASE = dict(width=W, height=H, max_ticks=MAX_TICKS, player_health=4, player_damage=2,
             player_armor=0, npc_health=2, npc_damage=1, npc_armor=0)
_RPG = MANA | LEVEL | ITEMS


def _cfg(variant, N, **kw):
    """The configuration of a variant, so that the switch an instance compiles
    in is exercised: "sep" starts the players on different depths with
    separation damage every 2-3 ticks; "rpg" is mana, levelling and items with
    weak NPCs that nearly always drop; the others are named by their flags."""
    c = dict(_BASE, n_npcs=K_OF[N], despawn=1 + (N == 8))
    if variant == "sep":
        c.update(flags=1, start_mode=2, p1_depth=(N == 16), p2_depth=1 + (N != 0),
                 sep_period=2 + (N == 8), player_health=9)
    elif variant == "rpg":
        c.update(flags=_RPG | (HEAL if N == 8 else 0), npc_health=1 + (N == 16),
                 item_drop_pct=90, item_bonus=1, item_slots=2, xp_per_kill=2, xp_per_level=2,
                 mana_max=6, mana_regen=1, mana_per_point=1, player_health=6)
    elif variant == "dd":
        c.update(flags=2)
    elif variant == "readme":
        c.update(flags=README | MANA, combat_cooldown=2)
    elif variant == "sepdd":
        c.update(flags=3, start_mode=2, p1_depth=0, p2_depth=1, sep_period=3, player_health=9)
    else:
        assert variant == "plain", variant
    c.update(kw)
    return c


def bank_layouts(n):
    """n explicit-grid layouts [n, W, H] of Tile codes: a wall ring (layout 1's
    left edge open), inner walls on a diagonal lattice that shifts with the
    layout, and two or three staircases."""
    out = np.ones((n, W, H), np.uint8)
    for li in range(n):
        t = out[li]
        t[[0, -1], :] = 2
        t[:, [0, -1]] = 2
        if li == 1:
            t[0, 1:H - 1] = 1
        for x in range(2, W - 2):
            for y in range(2, H - 2):
                if (3 * x + 5 * y + 2 * li) % 13 == 0:
                    t[x, y] = 2
        for sx, sy in ((1 + li, 1), (W - 2, H - 2 - li), (5, 4 + li % 3))[:2 + li % 2]:
            t[sx, sy] = 3
    return out


def _lanes(n, paired=None, replay=False):
    env = {"ORX_ROLLOUT_LANES": str(n)}
    if paired is not None:
        env["ORX_REPLAY_PAIRED" if replay else "ORX_ROLLOUT_PAIRED"] = str(int(paired))
    return env


_RR, _SS, _RS, _SR = (1, 1), (2, 2), (1, 2), (2, 1)


def _pair_rows(N):
    """(want, variant, bank layouts, bots, games per wave, rows) per instance of
    ORX_PAIR_LIST_A / _B / _M (N): 32 games per wave store whole lines
    (kStreamAux), 8 and 16 partial ones."""
    return [
        ((N, 1, S, F, F, F), "plain", 0, _RR, 32, "int32"),
        ((N, 1, P, F, F, F), "plain", 0, _RR, 8, "int32"),
        ((N, 2, S, F, F, F), "plain", 0, _SS, 32, "int32"),
        ((N, 2, P, F, F, F), "plain", 0, _SS, 16, "int32"),
        ((N, 2, S, T, F, F), "sep", 0, _SS, 32, "int32"),
        ((N, 2, P, T, F, F), "sep", 0, _SS, 8, "int32"),
        ((N, 1, S, F, T, F), "plain", 0, _RR, 32, "compact"),
        ((N, 1, P, F, T, F), "plain", 0, _RR, 16, "compact"),
        ((N, 2, S, F, T, F), "plain", 0, _SS, 32, "compact"),
        ((N, 2, P, F, T, F), "plain", 0, _SS, 8, "compact"),
        ((N, 2, S, T, T, F), "sep", 0, _SS, 32, "compact"),
        ((N, 2, P, T, T, F), "sep", 0, _SS, 16, "compact"),
        ((N, 3, S, F, F, F), "rpg", 0, _RR, 32, "int32"),
        ((N, 3, P, F, F, F), "rpg", 0, _RR, 8, "int32"),
        ((N, 3, S, F, F, T), "rpg", 4, _RR, 32, "int32"),
        ((N, 3, P, F, F, T), "rpg", 5, _RR, 16, "int32"),
        ((N, 1, S, F, F, T), "plain", 3, _RR, 32, "int32"),
        ((N, 1, P, F, F, T), "plain", 6, _RR, 8, "int32"),
        ((N, 2, S, F, F, T), "plain", 5, _SS, 32, "int32"),
        ((N, 2, P, F, F, T), "plain", 4, _SS, 16, "int32"),
        ((N, 4, S, F, F, F), "plain", 0, _RS, 32, "int32"),
        ((N, 4, P, F, F, F), "plain", 0, _RS, 8, "int32"),
        ((N, 5, S, F, F, F), "plain", 0, _SR, 32, "int32"),
        ((N, 5, P, F, F, F), "plain", 0, _SR, 16, "int32"),
    ]


def _rollout_rows(N):
    """(want, variant, bank, bots, games per wave, rows, act given) per instance
    of ORX_ROLLOUT_LIST_N(N), ORX_ROLLOUT_PAIRED=0 on each; the generic form
    (PM 0) three times: no rows, int32 rows without the actions, compact rows
    (where PM 1 / 2 have a compact instance, with bots or a flag they do not
    serve).  64 and 32 games per wave store whole lines, 16 and 8 partial."""
    return [
        ((N, 0, F, S, F), "plain", 0, _RR, 64, None, False),
        ((N, 0, F, S, F), "sep", 0, _SS, 16, "int32", False),
        ((N, 0, F, S, F), "dd" if N != 8 else "readme", 0, _RR if N != 16 else (2, 3), 32,
         "compact", True),
        ((N, 1, F, S, F), "plain", 0, _RR, 64, "int32", True),
        ((N, 1, F, P, F), "plain", 0, _RR, 16, "int32", True),
        ((N, 2, F, S, F), "sep", 0, _SS, 32, "int32", True),
        ((N, 2, F, P, F), "plain", 0, _SS, 8, "int32", True),
        ((N, 3, F, S, F), "rpg", 0, _RR, 64, "int32", True),
        ((N, 3, F, P, F), "rpg", 0, _RR, 16, "int32", True),
        ((N, 0, T, S, F), "rpg", 4, _RR, 32, None, False),
        ((N, 0, T, S, F), "plain", 5, _SR, 8, "int32", False),
        ((N, 0, T, S, F), "plain", 3, _SS, 64, "compact", True),
        ((N, 1, T, S, F), "plain", 6, _RR, 32, "int32", True),
        ((N, 1, T, P, F), "plain", 3, _RR, 8, "int32", True),
        ((N, 2, T, S, F), "plain", 4, _SS, 64, "int32", True),
        ((N, 2, T, P, F), "sep", 5, _SS, 16, "int32", True),
        ((N, 3, T, S, F), "rpg", 5, _RR, 64, "int32", True),
        ((N, 3, T, P, F), "rpg", 3, _RR, 16, "int32", True),
        ((N, 1, F, S, T), "plain", 0, _RR, 32, "compact", True),
        ((N, 1, F, P, T), "plain", 0, _RR, 16, "compact", True),
        ((N, 2, F, S, T), "plain", 0, _SS, 64, "compact", True),
        ((N, 2, F, P, T), "sep", 0, _SS, 8, "compact", True),
    ]


# ORX_ROLLOUT_LIST_DENSE (30 NPCs never pair: no ORX_ROLLOUT_PAIRED here)
_DENSE_ROWS = [
    ((DENSE, 0, F, S, F), "plain", 0, _RS, 16, None, False),
    ((DENSE, 0, F, S, F), "dd", 0, _RR, 64, "int32", False),
    ((DENSE, 0, F, S, F), "plain", 0, _RR, 32, "compact", True),
    ((DENSE, 0, T, S, F), "plain", 3, _RR, 64, None, False),
    ((DENSE, 0, T, S, F), "sep", 4, _SS, 32, "int32", False),
    ((DENSE, 0, T, S, F), "plain", 5, _SS, 16, "compact", True),
    ((DENSE, 1, F, S, F), "plain", 0, _RR, 32, "int32", True),
    ((DENSE, 1, F, P, F), "plain", 0, _RR, 16, "int32", True),
    ((DENSE, 2, F, S, F), "plain", 0, _SS, 64, "int32", True),
    ((DENSE, 2, F, P, F), "sep", 0, _SS, 8, "int32", True),
    ((DENSE, 1, T, S, F), "plain", 4, _RR, 64, "int32", True),
    ((DENSE, 1, T, P, F), "plain", 6, _RR, 8, "int32", True),
    ((DENSE, 2, T, S, F), "sep", 3, _SS, 32, "int32", True),
    ((DENSE, 2, T, P, F), "plain", 5, _SS, 16, "int32", True),
]

# lane_rollout_kernel<N, G, MT, MOV>: (want, variant, extra fields, bank, bots,
# rows, act given); the moving instances take both npc_policy values
_LANE_ROWS = [
    # ORX_NG_LIST: stock seeding, NPCs that stay
    ((0, F, T, F), "plain", dict(rng=1), 0, _RR, "int32", True),
    ((8, F, T, F), "plain", dict(rng=1), 0, _SS, "compact", True),
    ((16, F, T, F), "plain", dict(rng=1), 0, _RS, None, False),
    ((DENSE, F, T, F), "plain", dict(rng=1), 0, _RR, "int32", True),
    ((0, T, T, F), "plain", dict(rng=1), 4, _SS, "int32", True),
    ((8, T, T, F), "plain", dict(rng=1), 3, _RR, "int32", False),
    ((16, T, T, F), "plain", dict(rng=1), 5, _SR, "compact", True),
    ((DENSE, T, T, F), "plain", dict(rng=1), 6, _RR, "int32", True),
    # ORX_MOV_ROLLOUT_LIST
    ((8, F, F, T), "plain", dict(npc_policy=1), 0, _RR, "int32", True),
    ((16, F, F, T), "plain", dict(npc_policy=2), 0, _SS, "compact", True),
    ((DENSE, F, F, T), "dd", dict(npc_policy=1), 0, _RS, "int32", True),
    ((8, T, F, T), "plain", dict(npc_policy=2), 4, _RR, "int32", True),
    ((16, T, F, T), "sepdd", dict(npc_policy=1), 3, _SS, "int32", False),
    ((DENSE, T, F, T), "plain", dict(npc_policy=2), 5, _RR, "compact", True),
    ((8, F, T, T), "plain", dict(npc_policy=2, rng=1), 0, _SR, "int32", True),
    ((16, F, T, T), "plain", dict(npc_policy=1, rng=1), 0, _RR, None, False),
    ((DENSE, F, T, T), "plain", dict(npc_policy=2, rng=1), 0, _SS, "int32", True),
    ((8, T, T, T), "plain", dict(npc_policy=1, rng=1), 6, _SS, "compact", True),
    ((16, T, T, T), "plain", dict(npc_policy=2, rng=1), 4, _RR, "int32", True),
    ((DENSE, T, T, T), "dd", dict(npc_policy=1, rng=1), 3, _RR, "int32", True),
]


def _pair_log_rows(N):
    """ORX_PAIR_LIST_L(N): (want, bots whose moves are logged, games per wave, rows)."""
    return [
        ((N, 6, S, F, F, F), _RR, 32, "int32"),
        ((N, 6, P, F, F, F), _SS, 8, "int32"),
        ((N, 6, S, F, T, F), _RS, 32, "compact"),
        ((N, 6, P, F, T, F), _SR, 16, "compact"),
    ]


def _replay_rows(N):
    """ORX_REPLAY_LIST (N): (want, variant, bots, games per wave, rows,
    ORX_REPLAY_PAIRED=0 -- where the plan would pair).  EXT: any flag."""
    return [
        ((N, 0, F), "plain", _RS, 64, None, False),
        ((N, 1, F), "plain", _RR, 16, "int32", True),
        ((N, 2, F), "plain", _SS, 32, "compact", True),
        ((N, 0, T), "sep", _SS, 16, None, False),
        ((N, 1, T), "rpg", _RR, 64, "int32", False),
        ((N, 2, T), "readme" if N != 16 else "dd", _SR, 8, "compact", False),
    ]


def _requests():
    out = []

    def add(kernel, want, kind, cfg, bank, bots, fmt, act, env):
        i = len(out)
        out.append(Request((kernel, want), kind, cfg, bank, bots, fmt, act, env,
                           seed=1009 + 17 * i, offset=4096 + 29 * i))

    for N in (0, 8, 16):
        for want, variant, bank, bots, lanes, fmt in _pair_rows(N):
            add(PAIR, want, "rollout", _cfg(variant, N), bank, bots, fmt, True, _lanes(lanes))
    for N in (0, 8, 16):
        for want, variant, bank, bots, lanes, fmt, act in _rollout_rows(N):
            add(ROLLOUT, want, "rollout", _cfg(variant, N), bank, bots, fmt, act,
                _lanes(lanes, paired=False))
    for want, variant, bank, bots, lanes, fmt, act in _DENSE_ROWS:
        add(ROLLOUT, want, "rollout", _cfg(variant, DENSE), bank, bots, fmt, act, _lanes(lanes))
    for want, variant, extra, bank, bots, fmt, act in _LANE_ROWS:
        add(LANE, want, "rollout", _cfg(variant, want[0], **extra), bank, bots, fmt, act, {})
    for N in (0, 8, 16):
        for want, bots, lanes, fmt in _pair_log_rows(N):
            add(PAIR, want, "step_n", _cfg("plain", N), 0, bots, fmt, False, _lanes(lanes))
    for N in (0, 8, 16):
        for want, variant, bots, lanes, fmt, unpair in _replay_rows(N):
            add(REPLAY, want, "step_n", _cfg(variant, N), 0, bots, fmt, False,
                _lanes(lanes, paired=False if unpair else None, replay=True))
    return out


REQUESTS = _requests()


def request_id(i):
    r = REQUESTS[i]
    rows = {None: "norows", "int32": "int32", "compact": "compact"}[r.fmt]
    return "%03d-%s-%s%s" % (i, instance_name(r.want).replace(" ", ""), rows,
                            "" if r.act or r.kind == "step_n" else "-noact")


# ---------------------------------------------------------------------------
# The dispatch, restated
# ---------------------------------------------------------------------------
def plan_line(r, concurrency=1):
    """The request as a line of tests/plan_main.cpp's input (without a device)."""
    d = dict(flags=0, rng=0, npc_policy=0)
    d.update(r.cfg)
    head = [r.kind, d["width"], d["height"], d["n_npcs"], d["flags"], r.bank, d["rng"],
            d["npc_policy"]]
    if r.kind == "rollout":
        args = [r.bots[0], r.bots[1], B, int(r.fmt is not None and r.act),
                int(r.fmt == "compact"), concurrency]
    else:
        args = [B, {None: 0, "int32": 1, "compact": 2}[r.fmt], concurrency]
    return " ".join(str(w) for w in head + args + ["%s=%s" % kv for kv in sorted(r.env.items())])


PLAN_KEYS = ("form", "pm", "lanes", "nt", "threads", "blocks", "lds_bytes", "lds_n", "lds_bits",
             "lds_rows")
# every override orx_plan.h reads for these launches (a request sets its own, no other)
PLAN_OVERRIDES = ("ORX_ROLLOUT_LANES", "ORX_ROLLOUT_PAIRED", "ORX_ROLLOUT_THREADS",
                  "ORX_MOV_LANES", "ORX_REPLAY_PAIRED", "ORX_STEP_N_GENERIC", "ORX_NO_LDS_TILES",
                  "ORX_NO_LDS_BITS", "ORX_REFUSE_LDS_RAISE")


def build_plan_main(directory):
    """tests/plan_main.cpp built with g++ as test_plan.py builds it; its path."""
    import os
    import subprocess
    exe = os.path.join(str(directory), "plan_main")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_main.cpp")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", src, "-o", exe], check=True)
    return exe


def plans_of(exe, requests, device=None):
    """One plan (a dict of PLAN_KEYS) per request, on ``device`` (SIMDs, LDS
    bytes) or on plan_main's own."""
    import os
    import subprocess
    lines = [("" if device is None else "%d %d " % device) + plan_line(r) for r in requests]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True,
                       env={k: v for k, v in os.environ.items() if not k.startswith("ORX_")})
    assert r.returncode == 0, r.stderr
    out = [dict(zip(PLAN_KEYS, (w if i == 0 else int(w) for i, w in enumerate(l.split()))))
           for l in r.stdout.splitlines()]
    assert len(out) == len(requests)
    return out


def instance_of(plan, cfg, request):
    """The instance orx_rollout_ex (ORX_LANE_ROLLOUT, ORX_PAIR, ORX_ROLLOUT_AC)
    or launch_step_n (ORX_PAIR_LOG, ORX_REPLAY) launches for ``plan`` (a dict of
    plan_main's output), or None for a form outside the ledger."""
    nc = ncap_for(cfg.get("n_npcs", 0))
    flags = cfg.get("flags", 0)
    grid = request.bank > 0
    mt = cfg.get("rng", 0) == 1
    sep = bool(flags & 1)
    form, pm, nt = plan["form"], plan["pm"], bool(plan["nt"])
    if request.kind == "rollout":
        cf = request.fmt == "compact"
        if form == "moving":
            return (LANE, (nc, grid, mt, True))
        if form == "mt":
            return (LANE, (nc, grid, True, False))
        if form == "paired":
            return (PAIR, (nc, pm, nt, pm == 2 and sep, cf, grid))
        if form == "one-lane":   # (the generic form has one instance for both formats)
            return (ROLLOUT, (nc, pm, grid, nt, cf and pm != 0))
        return None
    rows = {None: 0, "int32": 1, "compact": 2}[request.fmt]
    if form == "paired":
        return (PAIR, (nc, 6, nt, False, rows == 2, False))
    if form == "replay":
        return (REPLAY, (nc, rows, flags != 0))
    return None


# ---------------------------------------------------------------------------
# The oracle's side of a request
# ---------------------------------------------------------------------------
BAD_BYTES = (0, -1, 7, 99)   # outside the Move codes (6 is a heal under EXT_HEAL)


def obs_rows(ex):
    """The 14 OBS_FIELDS rows of an oracle export: int32 [14, games]."""
    return np.stack([ex["p_x"][0], ex["p_y"][0], ex["p_depth"][0], ex["p_health"][0],
                     ex["p_x"][1], ex["p_y"][1], ex["p_depth"][1], ex["p_health"][1],
                     ex["tick"], ex["status"], ex["st_x"][0], ex["st_y"][0],
                     ex["st_x"][1], ex["st_y"][1]]).astype(np.int32)


def layouts_of(r):
    return bank_layouts(r.bank) if r.bank else None


def new_oracle(oracle_mod, r, record_events=False):
    o = oracle_mod.Oracle(r.cfg, B, r.seed, r.offset, layouts=layouts_of(r),
                          record_events=record_events)
    o.reset(episode=np.zeros(B, np.int32))
    return o


def run_oracle(oracle_mod, r, witness=False, ticks=N_TICKS):
    """Plays the request's launches on the oracle: per launch the actions
    [ticks, B, 2] (for a replay: the log, the bots' moves with about 1% of the
    bytes outside the Move codes), the rows [ticks, 14, B] and the state after
    it.  With ``witness`` also the set of things the run contained:
    "max_ticks" / "win" (an episode so ended), "restart" (an episode ended and
    the next began inside one launch), "descend", "npc_hit" (a combat between a
    player and an NPC), "sep_damage", "item" / "level" (picked up / gained) and
    "layouts" (two or more of a bank's layouts in use)."""
    K, flags = r.cfg["n_npcs"], r.cfg.get("flags", 0)
    o = new_oracle(oracle_mod, r, record_events=witness and K > 0)
    rs = np.random.RandomState(r.seed)
    seen, launches = set(), []
    prev = o.export()
    for _ in range(N_LAUNCHES):
        acts, rows = [], []
        for t in range(ticks):
            a = o.policy(*r.bots)
            if r.kind == "step_n":
                bad = rs.rand(B, 2) < 0.01
                a[bad] = rs.choice(BAD_BYTES, size=int(bad.sum())).astype(np.int8)
            o.step(a)
            s = o.export()
            acts.append(a)
            rows.append(obs_rows(s))
            if witness:
                _witness(o, r, prev, s, t, seen)
            prev = s
        launches.append((np.stack(acts), np.stack(rows), prev))
    return (launches, seen) if witness else launches


def _witness(o, r, prev, s, t, seen):
    K, flags = r.cfg["n_npcs"], r.cfg.get("flags", 0)
    same = s["episode"] == prev["episode"]          # (a played tick, not a restart)
    alive = (s["p_health"] > 0).all(axis=0)
    if (same & (s["status"] == 4) & (s["tick"] >= MAX_TICKS) & alive).any():
        seen.add("max_ticks")
    if (same & ((s["status"] == 2) | (s["status"] == 3))).any():
        seen.add("win")
    if t > 0 and (~same & (prev["status"] != 1)).any():   # ended at tick t - 1 of this launch
        seen.add("restart")
    cnt, was = s["counters"], prev["counters"]
    if (same & (cnt[1] > was[1])).any():
        seen.add("descend")
    if K > 0 and "npc_hit" not in seen:
        for g in np.flatnonzero(same & (cnt[0] > was[0])):
            if any(e[0] == 1 and (e[1] >= 3) != (e[2] >= 3) for e in o.events(int(g))):
                seen.add("npc_hit")
                break
    if flags & 1 and (same & (s["sep_start"] >= 0) &
                      ((s["p_health"] < prev["p_health"]).any(axis=0))).any():
        seen.add("sep_damage")
    if "p_rpg" in s:
        rpg, old = s["p_rpg"], prev["p_rpg"]
        if (same & (rpg[4] > old[4]).any(axis=0)).any():
            seen.add("item")
        per = max(1, r.cfg.get("xp_per_level", 3))
        if (same & (rpg[1] // per > old[1] // per).any(axis=0)).any():
            seen.add("level")
    if r.bank and len(np.unique(s["p_layout"])) >= 2:
        seen.add("layouts")


def wanted_witnesses(r):
    """What the run of a request must contain for its instance to be exercised."""
    K, flags = r.cfg["n_npcs"], r.cfg.get("flags", 0)
    want = {"max_ticks", "win", "restart", "descend"}
    if K > 0:
        want.add("npc_hit")
    if flags & 1:
        want.add("sep_damage")
    if r.want[0] in (PAIR, ROLLOUT) and r.want[1][1] == 3 and K > 0:
        want |= {"item", "level"}    # (PM 3 without NPCs has nothing to kill: mana only)
    if r.bank:
        want.add("layouts")
    return want
