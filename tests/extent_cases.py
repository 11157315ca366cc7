"""The ledger of buffers that pass 2^31 and 2^32 bytes (or 2^31 elements), and
the windows of games that are compared there (shared by test_extent.py on the
CPU and test_gpu_extent.py on the GPU; numpy only, no torch, no GPU).

A game depends on its global id only, so the games on either side of a
boundary are checked against an oracle of 64 games (``window_oracle``) or a
numpy reference on a slice of the state (``slice_snapshot``), while the GPU
does the launch over the whole batch.

One ``Row`` per buffer family: its configuration, the buffer's dtype and shape
(``"B"`` and ``"T"`` stand for the batch and the tick count), and the batches
at which it is run.  A ``Case`` is a row at one batch; it names the boundaries
the buffer crosses there, the 64-game windows and, for buffers whose batch is
not the first axis, the rows ([..] indices before the batch axis) that
straddle each boundary.  No test may allocate more than ``LIMIT`` bytes on the
device, so a boundary whose smallest crossing needs more is recorded in the
row's ``omitted`` and not built.
"""
from collections import namedtuple

import numpy as np

GiB = 1 << 30
LIMIT = 9 * GiB
WIN = 64
BYTE, ELEM = "byte", "elem"
BOUNDARIES = ((BYTE, 1 << 31), (BYTE, 1 << 32), (ELEM, 1 << 31))
SIZES = {"u8": 1, "i8": 1, "u16": 2, "i16": 2, "u32": 4, "i32": 4}

# name; cfg (the orx_cfg_t fields that differ from the oracle's defaults); bank
# (layouts or 0); bots; seed; offset; T (ticks of the launch that fills the
# buffer, or None); dtype, shape of the buffer; batches; other (name -> bytes
# per game of everything else the test allocates: state, inputs, outputs);
# entry (the entry points held to the oracle or reference); omitted;
# in_state: the buffer is one of the engine's own tensors (counted in state_bytes)
Row = namedtuple("Row", "name cfg bank bots seed offset T dtype shape batches other entry omitted "
                 "in_state", defaults=(False,))


def dstore_depths(max_ticks):
    """orx_dstore_depths: the slots of a player's ring of remembered dungeons."""
    if max_ticks <= 0:
        return 4096
    n = 256
    while n < max_ticks and n < 65536:
        n <<= 1
    return n


def state_bytes(cfg, bank=0):
    """Bytes per game of a BatchedEngine's resident state (engine.py)."""
    K = cfg.get("n_npcs", 0)
    n = 4 * (6 * 2 + 5 + 4) + 2                      # players, stairs, scalars, counters, actions
    n += 3 * max(K, 1) + 4 * (1 if K <= 32 else (K + 31) // 32)
    if K > 16:
        n += cfg["width"] * cfg["height"]            # npc_grid
    if bank:
        n += 4                                       # p_layout
    if cfg.get("flags", 0) & 1:
        n += 4
    if cfg.get("rng", 0) == 1:
        n += 2 * 625 * 4 + 16 * dstore_depths(cfg.get("max_ticks", 1000))
    return n


_DENSE = dict(n_npcs=255, npc_health=1, npc_damage=1, player_health=3, player_damage=2,
              player_armor=0, max_ticks=12)
_GRID_ENTRY = ("orx_reset", "orx_policy", "orx_step", "orx_step_events", "orx_rollout",
               "orx_rollout (ORX_ROLLOUT_LANES=64)", "orx_step_n", "VecEnv.step", "orx_npc_step",
               "orx_moves", "orx_npc_options", "npc_grid rule")
# ticks of the grid rows' run, per entry point in the order they are played
GRID_TICKS = dict(step=3, events=3, rollout=14, rollout64=14, step_n=8, env=2, given=3)
_GRID_OTHER = dict(events=8 * 16 + 4, log=GRID_TICKS["step_n"] * 2, env_out=14 * 4 + 4 + 1 + 4 + 2,
                   rows=GRID_TICKS["rollout"] * (14 * 4 + 2), npc_moves=255, moves=2 * 8 * 5,
                   options=255 * 8 + 1)
_STOCK = dict(width=6, height=6, rng=1, start_mode=2, p1_depth=0, p2_depth=1, despawn=1)
# T * 14 * B and T * 6 * B just past 2^31 elements (stock seeding keeps 9 KiB
# of generators and store per game, so its row takes fewer games and more ticks)
TRAJ_B, TRAJ_T, COMPACT_T = (1 << 18) + WIN, 586, 1366
STOCK_B, STOCK_T = (1 << 16) + WIN, 2340


def _form(name, N, bank, bots, fmt, env, replay_env=None, **extra):
    """A trajectory form: the configuration of instance_sweep's "plain"
    variant at NCAP ``N`` (12 x 10, max_ticks 24), the bank's layout count,
    the bots, the row format, the ORX_* overrides that pin the launch as
    instance_sweep pins it, and those of the orx_step_n replay of the recorded
    actions (None: the form is not replayed)."""
    import instance_sweep as sw
    return dict(name=name, cfg=sw._cfg("plain", N, **extra), bank=bank, bots=bots, fmt=fmt,
                env=env, replay_env=replay_env)


def traj_forms(row_name):
    import instance_sweep as sw
    if row_name == "traj_stock":
        return [_form("stock", 0, 0, (1, 2), "int32", {}, rng=1)]
    fmt = "compact" if row_name == "traj_compact" else "int32"
    forms = [_form("paired", 0, 0, (1, 1), fmt, sw._lanes(32),
                   sw._lanes(32, paired=True, replay=True)),
             _form("one-lane", 8, 0, (2, 2), fmt, sw._lanes(64, paired=False),
                   sw._lanes(64, paired=False, replay=True))]
    if fmt == "int32":
        forms += [_form("bank", 8, 3, (1, 2), fmt, sw._lanes(32)),
                  _form("moving", 8, 0, (1, 1), fmt, {}, npc_policy=1)]
    return forms


_VIEW = dict(width=12, height=10, n_npcs=5, npc_health=2, max_ticks=24, player_health=6,
             player_armor=0)
_VIEW_ENTRY = ("orx_view", "orx_sight", "orx_explore_update")
_PATH_ENTRY = ("orx_path_query", "orx_path_threat", "orx_path_ticks")
RADIUS = 15

_TRAJ_STATE = dict(width=12, height=10, n_npcs=5, max_ticks=24)
_TRAJ_ENTRY = ("orx_rollout", "orx_step_n")

ROWS = (
    Row("grid_wide", dict(_DENSE, width=256, height=256, n_npcs=32, max_ticks=16), 0, (1, 1), 31, 1000, None,
        "u8", ("B", 65536), (32768 + WIN, 65536 + WIN), _GRID_OTHER, _GRID_ENTRY,
        "2^31 elements are 2^31 bytes here; nothing omitted", in_state=True),
    Row("grid_dense", dict(_DENSE, width=64, height=64), 0, (1, 1), 32, 1000, None,
        "u8", ("B", 4096), ((1 << 19) + WIN, (1 << 20) + WIN), _GRID_OTHER, _GRID_ENTRY,
        "nothing omitted", in_state=True),
    Row("traj_int32", _TRAJ_STATE, 3, None, 33, 1000, TRAJ_T, "i32", ("T", 14, "B"), (TRAJ_B,),
        dict(act=TRAJ_T * 2), _TRAJ_ENTRY, "2^32 elements (16 GiB) omitted"),
    Row("traj_stock", dict(_TRAJ_STATE, n_npcs=0, rng=1), 0, None, 37, 1000, STOCK_T, "i32",
        ("T", 14, "B"), (STOCK_B,), dict(act=STOCK_T * 2), ("orx_rollout",),
        "2^32 elements (16 GiB) omitted"),
    Row("traj_compact", _TRAJ_STATE, 0, None, 34, 1000, COMPACT_T, "u32", ("T", 6, "B"),
        (TRAJ_B,), dict(act=COMPACT_T * 2), _TRAJ_ENTRY, "2^32 elements (16 GiB) omitted"),
    Row("dstore", dict(_STOCK, max_ticks=1000), 0, (2, 2), 35, 1000, 40, "i32",
        (2, 1024, 2, "B"), ((1 << 17) + WIN, (1 << 18) + WIN), {},
        ("orx_seed_mt", "orx_reset", "orx_rollout", "snapshot()['dstore']"),
        "2^31 elements: 8 GiB of store beside 2.5 GiB of generators at 2^19 games; omitted",
        in_state=True),
    Row("mt", dict(_STOCK, max_ticks=16), 0, (2, 2), 36, 1000, 40, "u32", (625, "B"),
        (858994 + WIN,), {}, ("orx_seed_mt", "orx_reset", "orx_rollout"),
        "2^32 bytes needs 1,717,987 games: two generators of 4 GiB each beside 7 GiB of "
        "store; omitted with 2^31 elements", in_state=True),
    Row("window_u8", _VIEW, 3, (1, 1), 38, 1000, 6, "u8", ("B", 31, 31), (2234638 + WIN,),
        dict(health=961, sight=124, memory=4 * 10 + 16, gained=4), _VIEW_ENTRY,
        "2^32 bytes with both planes (8 GiB) and the sight rows do not fit: omitted here, "
        "crossed by window_u8_cells with the cells plane alone"),
    Row("window_u8_cells", _VIEW, 3, (1, 1), 38, 1000, 6, "u8", ("B", 31, 31), (4469276 + WIN,),
        dict(sight=124, memory=4 * 10 + 16, gained=4), _VIEW_ENTRY,
        "2^31 elements are 2^31 bytes here; nothing omitted"),
    Row("window_u16", _VIEW, 0, (1, 1), 41, 1000, 6, "u16", ("B", 31, 31), (2234638 + WIN,),
        dict(rows=5 + 60 + 5), _PATH_ENTRY, "2^32 elements (8 GiB) omitted"),
    Row("window_u16_bank", _VIEW, 2, (1, 1), 42, 1000, 6, "u16", ("B", 31, 31), (2234638 + WIN,),
        dict(rows=5 + 60 + 5), _PATH_ENTRY, "2^32 elements (8 GiB) omitted"),
    Row("memory", dict(width=256, height=256, max_ticks=50), 0, (1, 1), 39, 1000, 3, "u32",
        ("B", 256, 8), ((1 << 18) + WIN, (1 << 19) + WIN, (1 << 20) + WIN),
        dict(key=16, sight=124, gained=4, seek=2 * (16 + 4 + 16)),
        ("orx_explore_update", "orx_explore_seek", "orx_route"), "2^32 elements (16 GiB) omitted"),
    Row("options", dict(width=18, height=19, n_npcs=255, npc_health=2, max_ticks=24), 0, (1, 1),
        40, 1000, 4, "u8", (255, "B", 8), (1052688 + WIN,),
        dict(target_or_amount=255 * 8 * 2, where=1, moves=8),
        ("orx_npc_options", "orx_moves"),
        "2^32 bytes of kind needs 2,105,377 games and 2.6 GiB of state beside it: omitted; "
        "target and amount (int16) cross 2^32 bytes at this batch"),
)
ROW = {r.name: r for r in ROWS}



class Case:
    """A row at one batch."""

    def __init__(self, row, B):
        self.row, self.B = row, int(B)
        self.name = "%s-%d" % (row.name, B)
        self.T = row.T
        self.shape = tuple(self.B if d == "B" else row.T if d == "T" else d for d in row.shape)
        self.axis = row.shape.index("B")
        self.itemsize = SIZES[row.dtype]
        self.elems = int(np.prod([int(d) for d in self.shape], dtype=object))
        self.nbytes = self.elems * self.itemsize

    def boundaries(self):
        """(kind, value, element index of the first element past it) of every
        boundary strictly inside the buffer."""
        out = []
        for kind, v in BOUNDARIES:
            e = v // self.itemsize if kind == BYTE else v
            if 0 < e < self.elems and e not in [x for _, _, x in out]:
                out.append((kind, v, e))
        return out

    def locate(self, elem):
        """``(lead, game, trail)``: the indices before the batch axis, the game
        and the indices after it of flat element ``elem``."""
        idx = np.unravel_index(int(elem), self.shape)
        idx = tuple(int(i) for i in idx)
        return idx[:self.axis], idx[self.axis], idx[self.axis + 1:]

    def window_at(self, elem):
        """First game of the 64-game window around the boundary before flat
        element ``elem``: the games of elements ``elem - 1`` and ``elem`` lie
        inside it, with a game on either side where one game straddles it."""
        g = self.locate(elem)[1]
        return min(max(g - WIN // 2, 0), self.B - WIN)

    def windows(self):
        """First games of the compared windows, ascending: [0, 64), one per
        boundary, the last 64 games."""
        return sorted({0, self.B - WIN} | {self.window_at(e) for _, _, e in self.boundaries()})

    def games(self):
        return np.concatenate([np.arange(g0, g0 + WIN) for g0 in self.windows()])

    def leads(self):
        """The rows (indices before the batch axis) that straddle a boundary."""
        return [self.locate(e)[0] for _, _, e in self.boundaries()]

    def allocation(self):
        """Bytes the case's GPU test allocates: state, the buffer itself when
        it is not part of the state, and the row's other buffers."""
        per_game = state_bytes(self.row.cfg, self.row.bank) + sum(self.row.other.values())
        own = 0 if self.row.in_state else self.nbytes
        return per_game * self.B + own


CASES = [Case(r, B) for r in ROWS for B in r.batches]
CASE = {c.name: c for c in CASES}


def slice_snapshot(snap, idx):
    """The games ``idx`` of a snapshot-shaped dict: every array has the batch
    as its last axis."""
    return {k: np.ascontiguousarray(np.asarray(v)[..., idx]) for k, v in snap.items()}


def window_oracle(oracle_mod, case, g0, n=WIN, cfg=None, layouts=None, record_events=False):
    """The oracle of games [g0, g0 + n) of the case's batch, reset into episode 0."""
    o = oracle_mod.Oracle(case.row.cfg if cfg is None else cfg, n, case.row.seed,
                          case.row.offset + g0, layouts=layouts, record_events=record_events)
    o.reset(episode=np.zeros(n, np.int32))
    return o


class Windows:
    """The window oracles of a case as one oracle over ``case.games()``."""

    def __init__(self, oracle_mod, case, cfg=None, layouts=None, record_events=False):
        self.case = case
        self.parts = [window_oracle(oracle_mod, case, g0, WIN, cfg, layouts, record_events)
                      for g0 in case.windows()]
        self.K = self.parts[0].K
        self.n = WIN * len(self.parts)

    def policy(self, p1, p2):
        return np.concatenate([o.policy(p1, p2) for o in self.parts])

    def step(self, actions, npc_moves=None):
        for j, o in enumerate(self.parts):
            s = slice(j * WIN, (j + 1) * WIN)
            o.step(actions[s], None if npc_moves is None else npc_moves[:, s])

    def export(self):
        parts = [o.export() for o in self.parts]
        return {k: np.concatenate([p[k] for p in parts], axis=-1) for k in parts[0]}

    def events(self, j):
        return self.parts[j // WIN].events(j % WIN)


def obs_rows(ex):
    """The 14 OBS_FIELDS rows of an oracle export: int32 [14, games]."""
    from instance_sweep import obs_rows as rows
    return rows(ex)


def play(win, bots, ticks, witness=None, actions=None, npc_moves=None, events=False):
    """``ticks`` ticks of the window oracles with the bots' moves (or
    ``actions[t]`` / ``npc_moves[t]``): the actions [ticks, n, 2], the rows
    [ticks, 14, n], with ``events`` every tick's event lists per game (else
    None) and the state after them.  ``witness`` (a Witness) looks at every
    tick."""
    acts, rows, evs = [], [], []
    prev = win.export()
    for t in range(ticks):
        a = win.policy(*bots) if actions is None else actions[t]
        win.step(a, None if npc_moves is None else npc_moves[t])
        s = win.export()
        acts.append(a)
        rows.append(obs_rows(s))
        if events:
            evs.append([win.events(g) for g in range(win.n)])
        if witness is not None:
            witness.see(win, prev, s, t)
        prev = s
    return np.stack(acts), np.stack(rows), evs if events else None, prev


def popcount(a):
    a = np.asarray(a).astype(np.uint32).reshape(-1, np.asarray(a).shape[-1])
    return np.unpackbits(a.view(np.uint8).reshape(a.shape[0], a.shape[1], 4), axis=2).sum(
        axis=(0, 2))


class Witness:
    """What a run of the window oracles contained, per game: sets of window
    game indices under "npc_hit", "npc_death", "restart" (an episode ended and
    the next began inside one ``play``), "end_ticks" / "end_win" (how an episode
    ended), "descend", "descend_p2" and "recall" (player 1 entered a depth that
    player 2 had made: p2's start depth <= depth < p2's depth)."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.seen = {}

    def add(self, what, games):
        self.seen.setdefault(what, set()).update(int(g) for g in np.flatnonzero(games))

    def see(self, win, prev, s, t):
        same = s["episode"] == prev["episode"]
        cnt, was = s["counters"], prev["counters"]
        self.add("npc_hit", same & (cnt[0] > was[0]) & self._npc_fight(win, same & (cnt[0] > was[0])))
        if win.K:
            self.add("npc_death", same & (popcount(s["npc_alive"]) < popcount(prev["npc_alive"])))
        self.add("restart", ~same & (prev["status"] != 1) & (t > 0))
        alive = (s["p_health"] > 0).all(axis=0)
        self.add("end_ticks", same & (s["status"] == 4) & alive)
        self.add("end_win", same & ((s["status"] == 2) | (s["status"] == 3)))
        down = same[None] & (s["p_depth"] > prev["p_depth"])
        self.add("descend", down.any(axis=0))
        self.add("descend_p2", down[1])
        p2_start = self.cfg.get("p2_depth", 0) if self.cfg.get("start_mode", 1) == 2 else 0
        nd = s["p_depth"][0]
        self.add("recall", down[0] & (p2_start <= nd) & (nd < prev["p_depth"][1]))

    @staticmethod
    def _npc_fight(win, games):
        out = np.zeros(len(games), bool)
        for g in np.flatnonzero(games):
            out[g] = any(e[0] == 1 and (e[1] >= 3) != (e[2] >= 3) for e in win.events(int(g)))
        return out

    def sides(self, what, case):
        """Per boundary of ``case``: (games before it, games after it) among the
        window games that saw ``what`` (indices into ``case.games()``)."""
        games = case.games()
        hit = np.zeros(len(games), bool)
        hit[list(self.seen.get(what, ()))] = True
        out = []
        for _, _, e in case.boundaries():
            g0 = case.window_at(e)
            cut = case.locate(e)[1]
            inside = (games >= g0) & (games < g0 + WIN)
            out.append((int((hit & inside & (games < cut)).sum()),
                        int((hit & inside & (games >= cut)).sum())))
        return out


# ---------------------------------------------------------------------------
# The runs, on the window oracles
# ---------------------------------------------------------------------------
GRID_STAGES = ("step", "events", "rollout", "rollout64", "step_n", "env", "given")
GRID_BAD = 0.01    # share of the step_n log's bytes outside the Move codes


def grid_run(oracle_mod, case, witness=None):
    """The grid rows' run on the window oracles: per stage of GRID_STAGES a
    dict of the actions [ticks, n, 2], the NPCs' moves [ticks, K, n] (the
    "given" stage, else None), each tick's event lists per game, the rows and
    the state after the stage; first the state after the reset."""
    win = Windows(oracle_mod, case, record_events=True)
    rs = np.random.RandomState(case.row.seed)
    out = {"reset": win.export()}
    uniq, inv = np.unique(case.games(), return_inverse=True)
    for name in GRID_STAGES:
        n = GRID_TICKS[name]
        acts = npc = None
        # (windows may overlap: a game gets the same bytes in each of them)
        if name == "step_n":    # a log: moves with a few bytes that are no Move
            acts = rs.randint(1, 6, size=(n, len(uniq), 2)).astype(np.int8)
            bad = rs.rand(n, len(uniq), 2) < GRID_BAD
            acts[bad] = rs.choice((0, -1, 7, 99), size=int(bad.sum())).astype(np.int8)
            acts = np.ascontiguousarray(acts[:, inv])
        if name == "given":
            npc = rs.randint(1, 6, size=(n, win.K, len(uniq))).astype(np.int8)
            npc = np.ascontiguousarray(npc[:, :, inv])
        a, rows, events, state = play(win, case.row.bots, n, witness, acts, npc, events=True)
        out[name] = dict(act=a, npc=npc, events=events, rows=rows, state=state)
    return out


def traj_run(oracle_mod, case, form, witness=None):
    """A trajectory form's launch on the window oracles: the actions [T, n, 2],
    the rows [T, 14, n] and the state after it."""
    import instance_sweep as sw
    layouts = sw.bank_layouts(form["bank"]) if form["bank"] else None
    win = Windows(oracle_mod, case, cfg=form["cfg"], layouts=layouts)
    a, rows, _, state = play(win, form["bots"], case.T, witness)
    return a, rows, state


def stock_run(oracle_mod, case, witness=None):
    """The dstore and mt rows' stock-seed rollout on the window oracles: the
    actions, the rows and the state after it."""
    win = Windows(oracle_mod, case)
    a, rows, _, state = play(win, case.row.bots, case.T, witness)
    return a, rows, state


def query_layouts(case):
    import instance_sweep as sw
    return sw.bank_layouts(case.row.bank) if case.row.bank else None


def query_bank(case):
    from optimax_rogue_amd.dungeons import DungeonBank
    return DungeonBank(query_layouts(case)) if case.row.bank else None


def query_cfg(case):
    from optimax_rogue_amd import EnvConfig
    return EnvConfig.from_dict(case.row.cfg, layouts=query_layouts(case))


def query_run(oracle_mod, case):
    """The query rows' state on the window oracles: ``case.T`` ticks of the
    bots from the reset; the oracles and the actions played."""
    win = Windows(oracle_mod, case, layouts=query_layouts(case))
    acts, _, _, _ = play(win, case.row.bots, case.T)
    return win, acts


def view_refs(case, snap, health):
    """The window_u8 rows' references on a snapshot slice: view, the sight
    rows, seen_view and explore(view=True) from an empty map, as dicts of
    name -> array."""
    from optimax_rogue_amd import explore, sight, view
    cfg, bank = query_cfg(case), query_bank(case)
    n = snap["tick"].shape[-1]
    cells, hp = view.render_view(snap, cfg, 0, RADIUS, bank=bank, health=True)
    vis = sight.visible(snap, cfg, 0, RADIUS, bank=bank)
    out = {"view_cells": cells, "sight": sight.pack_rows(vis)}
    seen_c, seen_h = sight.apply(cells, vis, hp)
    out["seen_cells"] = seen_c
    memory, key = explore.empty(n, cfg.width, cfg.height)
    ex_c, ex_h = cells.copy(), hp.copy()
    out["gained"] = explore.update(memory, key, snap, cfg, 0, RADIUS, out["sight"], ex_c, ex_h)
    out["explore_cells"], out["memory"], out["key"] = ex_c, memory, key
    if health:
        out.update(view_health=hp, seen_health=seen_h, explore_health=ex_h)
    return out


def path_refs(case, snap):
    """The window_u16 rows' references on a snapshot slice: path.query,
    path.threat and path.ticks of player 1 at radius 15, as name -> array."""
    from optimax_rogue_amd import path
    cfg, bank = query_cfg(case), query_bank(case)
    out = {}
    for name, fn, fields in (("query", path.query, ("dist", "move", "window")),
                             ("threat", path.threat, ("dist", "move", "target", "after", "window")),
                             ("ticks", path.ticks, ("ticks", "move", "window"))):
        for f, a in zip(fields, fn(snap, cfg, 0, RADIUS, bank=bank)):
            out[f"{name}_{f}"] = a
    return out


MEMORY_RADIUS = 4   # (explore.seek and route.route search whole 256 x 256 arrays per
#                      game; route's search grows with the known area)


def memory_refs(case, snaps):
    """The memory row's references on all the window games: explore.update
    over the states ``snaps`` (gained per state), then explore.seek and
    route.route on the last.  Windows may overlap: each distinct game is
    computed once."""
    from optimax_rogue_amd import explore, route, sight
    cfg = query_cfg(case)
    uniq, first, inv = np.unique(case.games(), return_index=True, return_inverse=True)
    snaps = [slice_snapshot(s, first) for s in snaps]
    memory, key = explore.empty(len(uniq), cfg.width, cfg.height)
    gained = [explore.update(memory, key, s, cfg, 0, MEMORY_RADIUS,
                             sight.pack_rows(sight.visible(s, cfg, 0, MEMORY_RADIUS)))[inv]
              for s in snaps]
    return dict(gained=gained, memory=memory[inv], key=key[inv],
                seek=tuple(a[inv] for a in explore.seek(memory, key, snaps[-1], cfg, 0)),
                route=tuple(a[inv] for a in route.route(memory, key, snaps[-1], cfg, 0)))


def memory_run(oracle_mod, case):
    """The memory row on the window oracles: the state before each of the
    ``case.T`` explore calls and the actions played between them."""
    win = Windows(oracle_mod, case)
    snaps, acts = [win.export()], []
    for _ in range(case.T - 1):
        a = win.policy(*case.row.bots)
        win.step(a)
        acts.append(a)
        snaps.append(win.export())
    return snaps, acts


def options_refs(case, snap):
    from optimax_rogue_amd import moves, npc_query
    cfg = query_cfg(case)
    kind, target, amount, where = npc_query.options(snap, cfg)
    return dict(kind=kind, target=target, amount=amount, where=where,
                moves_kind=moves.outcomes(cfg, snap, 0)[0])
