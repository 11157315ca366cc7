"""GPU: every kernel where a buffer passes 2^31 and 2^32 bytes (or 2^31
elements), one test per case of extent_cases.py: one engine at the case's
batch and one launch per entry point, then the windows of 64 games around every
boundary (and the first and last 64 games) against window oracles or the numpy
references, bit-exact.  The windows are selected on the device; no whole buffer
is copied to the host.  test_extent.py shows on the CPU that each boundary lies
inside its buffer and its window, and that the compared games contain NPC
fights, restarts, descents and recalls.

A case is skipped only where the device has less free memory than its
allocation plus 1 GiB (never on an MI355X)."""
import gc
import time

import numpy as np
import pytest

import extent_cases as xc
from golden_util import compare_state
from guarded import POISONS

pytestmark = pytest.mark.gpu


def _poison(t, poison):
    """Fills a contiguous tensor's bytes with one of guarded.py's poisons."""
    import torch
    t.view(-1).view(torch.uint8).fill_(poison)
    return t


def _start(case):
    """Frees what earlier tests left cached, then skips where the case does
    not fit; the device and the window games' indices on it."""
    import torch
    gc.collect()
    torch.cuda.empty_cache()
    dev = torch.device("cuda", 0)
    free, _ = torch.cuda.mem_get_info(dev)
    need = case.allocation() + xc.GiB
    if free < need:
        pytest.skip(f"{case.name}: {need / xc.GiB:.1f} GiB needed, {free / xc.GiB:.1f} GiB free")
    return dev, torch.from_numpy(case.games()).to(dev)


def _done(name, t0, dev):
    """Ends a case: its wall time and peak allocation, which stays in the limit."""
    import torch
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev)
    print(f"\n{name}: {time.time() - t0:.1f} s, {peak / xc.GiB:.2f} GiB at its peak")
    assert peak <= xc.LIMIT, (name, peak)


def _engine(cfg, B, case, dev, layouts=None, offset=0, **kw):
    from optimax_rogue_amd import EnvConfig
    from optimax_rogue_amd.engine import BatchedEngine
    return BatchedEngine(EnvConfig.from_dict(cfg, layouts=layouts), B, seed=case.row.seed,
                         game_offset=case.row.offset + offset, device=dev, **kw)


def _window_state(eng, idx):
    """snapshot() of the games ``idx`` alone, selected on the device."""
    from optimax_rogue_amd.engine import STATE_FIELDS
    pick = lambda f: getattr(eng, f).index_select(-1, idx).cpu().numpy()
    out = {}
    for f in STATE_FIELDS:
        a = pick(f)
        if f == "npc_pos":
            a = a.view(np.uint16)[: eng.K]
        elif f == "npc_health":
            a = a[: eng.K]
        elif f == "npc_alive":
            a = a.view(np.uint32)
        out[f] = a
    if eng.bank is not None:
        out["p_layout"] = pick("p_layout")
    if eng.sep_start is not None:
        out["sep_start"] = pick("sep_start")
    return out


def _same_state(eng, idx, want, where):
    got = _window_state(eng, idx)
    compare_state(got, want, eng.K, where)
    compare_state(want, got, eng.K, where + " (oracle against engine)")


def _same(got, want, where, axes):
    got = got.cpu().numpy()
    want = np.asarray(want)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    bad = np.argwhere(got.astype(np.int64) != want.astype(np.int64))
    assert not len(bad), f"{where}: differs at {axes} {bad[:5].tolist()} (window game indices)"


def _check_grid(eng, idx, snap, where):
    """_check_npc_grid's rule (test_gpu_parity.py) on the windows' rows of the
    grid: slot + 1 exactly on the live NPCs' cells and 0 elsewhere."""
    from optimax_rogue_amd.enums import npc_alive_bits
    K, H = eng.K, int(eng.cfg.height)
    grid = eng.npc_grid.index_select(0, idx).cpu().numpy()
    want = np.zeros_like(grid)
    live = npc_alive_bits(snap["npc_alive"], K)
    pos = np.asarray(snap["npc_pos"]).astype(np.int64)
    k, g = np.nonzero(live)
    want[g, (pos[k, g] & 0xFF) * H + (pos[k, g] >> 8)] = k + 1
    bad = np.argwhere(grid != want)
    assert not len(bad), f"{where}: npc_grid differs at [window game, cell] {bad[:5].tolist()}"


def _spread(window, idx, B, fill, dev, axis):
    """A whole-batch int8 tensor holding ``fill`` with the window games'
    entries of ``window`` (numpy, games along ``axis``) in place."""
    import torch
    shape = list(window.shape)
    shape[axis] = B
    full = torch.full(shape, fill, dtype=torch.int8, device=dev)
    full.index_copy_(axis, idx, torch.from_numpy(np.ascontiguousarray(window)).to(dev))
    return full


GRID = [c for c in xc.CASES if c.row.name.startswith("grid_")]


@pytest.mark.parametrize("case", GRID, ids=lambda c: c.name)
def test_grid_rows(case, oracle_lib, monkeypatch):
    """npc_grid [B][W * H] past 2^31 and 2^32 bytes: reset, policy, step, step
    with events, both rollout forms, step_n, VecEnv.step, the given-NPC tick,
    then orx_moves and orx_npc_options, on one engine."""
    import torch
    import instance_sweep as sw
    from optimax_rogue_amd import EnvConfig, moves, npc_query
    from optimax_rogue_amd.vecenv import VecEnv
    t0 = time.time()
    dev, idx = _start(case)
    torch.cuda.reset_peak_memory_stats(dev)
    for k in sw.PLAN_OVERRIDES:
        monkeypatch.delenv(k, raising=False)
    row, B, n = case.row, case.B, len(idx)
    want = xc.grid_run(oracle_lib, case)
    cfg = EnvConfig.from_dict(row.cfg)
    env = VecEnv(cfg, B, seed=row.seed, game_offset=row.offset, device=dev, opponent=None,
                 check_actions=False)
    eng = env.engine
    assert eng.npc_grid.numel() * eng.npc_grid.element_size() == case.nbytes

    def after(stage):
        state = want[stage] if stage == "reset" else want[stage]["state"]
        _same_state(eng, idx, state, f"{case.name} {stage}")
        _check_grid(eng, idx, state, f"{case.name} {stage}")

    after("reset")
    w = want["step"]
    for t in range(len(w["act"])):
        a = eng.policy(*row.bots)
        _same(a.index_select(0, idx), w["act"][t], f"{case.name} policy tick {t}", "[game, player]")
        eng.step(a)
    after("step")

    w = want["events"]
    for t in range(len(w["act"])):
        _, ev, nev = eng.step(_spread(w["act"][t], idx, B, 5, dev, 0), events=True)
        ev, nev = ev.index_select(0, idx).cpu().numpy(), nev.index_select(0, idx).cpu().numpy()
        for g in range(n):
            got = [tuple(int(v) for v in r) for r in ev[g, : nev[g]]]
            assert got == w["events"][t][g], (case.name, "events", t, g)
    after("events")

    T = xc.GRID_TICKS["rollout"]
    obs = torch.empty((T, 14, B), dtype=torch.int32, device=dev)
    act = torch.empty((T, B, 2), dtype=torch.int8, device=dev)
    for stage, lanes, poison in (("rollout", None, POISONS[0]), ("rollout64", 64, POISONS[1])):
        if lanes is not None:
            monkeypatch.setenv("ORX_ROLLOUT_LANES", str(lanes))
            assert eng.rollout_lanes() == lanes
        w = want[stage]
        _poison(obs, poison), _poison(act, poison)
        eng.rollout(T, *row.bots, obs=obs, act=act)
        _same(obs.index_select(2, idx), w["rows"], f"{case.name} {stage} rows", "[tick, field, game]")
        _same(act.index_select(1, idx), w["act"], f"{case.name} {stage} act", "[tick, game, player]")
        after(stage)
    monkeypatch.delenv("ORX_ROLLOUT_LANES")
    del act

    w = want["step_n"]
    T = len(w["act"])
    _poison(obs, POISONS[0])
    eng.step_n(_spread(w["act"], idx, B, 5, dev, 1), obs=obs[:T])
    _same(obs[:T].index_select(2, idx), w["rows"], f"{case.name} step_n rows", "[tick, field, game]")
    after("step_n")
    del obs

    w = want["env"]
    status = want["step_n"]["state"]["status"]
    for t in range(len(w["act"])):
        o, reward, done, st = env.step(_spread(w["act"][t], idx, B, 5, dev, 0))
        _same(o.index_select(0, idx), w["rows"][t].T, f"{case.name} env obs tick {t}", "[game, field]")
        new = w["rows"][t][9]
        r, d = VecEnv.outcome(torch.from_numpy(status), torch.from_numpy(new))
        _same(st.index_select(0, idx), new, f"{case.name} env status tick {t}", "[game]")
        _same(reward.index_select(0, idx), r.numpy(), f"{case.name} env reward tick {t}", "[game]")
        _same(done.index_select(0, idx), d.numpy(), f"{case.name} env done tick {t}", "[game]")
        status = new
    after("env")

    w = want["given"]
    for t in range(len(w["act"])):
        eng.step(_spread(w["act"][t], idx, B, 5, dev, 0),
                 npc_moves=_spread(w["npc"][t], idx, B, 5, dev, 1))
    after("given")

    snap = w["state"]
    for p in (0, 1):
        shape = (B, moves.MOVES_COLS)
        outs = tuple(_poison(torch.empty(shape, dtype=dt, device=dev), POISONS[p])
                     for dt in (torch.uint8, torch.int16, torch.int16))
        got = eng.moves(p, out=outs)
        for name, g, r in zip(("kind", "target", "amount"), got, moves.outcomes(cfg, snap, p)):
            _same(g.index_select(0, idx), r, f"{case.name} moves({p}) {name}", "[game, move]")
    del outs, got
    # kind and where (target and amount NULL, as npc_options_kind() calls it:
    # all four outputs at 255 NPCs are the "options" extent, 10 KB per game)
    kind = _poison(torch.empty((eng.K, B, moves.MOVES_COLS), dtype=torch.uint8, device=dev),
                   POISONS[0])
    where = _poison(torch.empty(B, dtype=torch.uint8, device=dev), POISONS[0])
    eng._call("orx_npc_options", kind.data_ptr(), None, None, where.data_ptr(), B, eng._stream())
    ref = npc_query.options(snap, cfg)
    _same(kind.index_select(1, idx), ref[0], f"{case.name} npc_options kind", "[slot, game, move]")
    _same(where.index_select(0, idx), ref[3], f"{case.name} npc_options where", "[game]")
    _done(case.name, t0, dev)


TRAJ = [(c, f) for c in xc.CASES if c.row.name.startswith("traj_")
        for f in xc.traj_forms(c.row.name)]


@pytest.mark.parametrize("case,form", TRAJ,
                         ids=lambda v: v.name if hasattr(v, "name") else v["name"])
def test_traj_rows(case, form, oracle_lib, monkeypatch):
    """Trajectory rows [T][rows][B] past 2^31 and 2^32 bytes and 2^31
    elements: orx_rollout in the form's pinned launch, then (forms with
    replay_env) orx_step_n replaying the recorded actions into the same
    buffer: every tick's rows and actions of the window games -- the rows that
    straddle the boundaries among them -- and the state after."""
    import torch
    import instance_sweep as sw
    from optimax_rogue_amd.engine import decode_compact, obs_rows
    from optimax_rogue_amd.enums import OBS_COMPACT, OBS_INT32
    t0 = time.time()
    dev, idx = _start(case)
    torch.cuda.reset_peak_memory_stats(dev)
    where = f"{case.name} {form['name']}"
    want_act, want_rows, want_state = xc.traj_run(oracle_lib, case, form)
    fmt = OBS_COMPACT if form["fmt"] == "compact" else OBS_INT32
    layouts = sw.bank_layouts(form["bank"]) if form["bank"] else None
    T, B = case.T, case.B
    assert (T, obs_rows(fmt), B) == case.shape
    obs = torch.empty(case.shape, dtype=torch.int32, device=dev)
    act = torch.empty((T, B, 2), dtype=torch.int8, device=dev)
    assert obs.numel() * 4 == case.nbytes
    # the compared rows hold the ones that straddle the boundaries
    games = case.games()
    for _, _, e in case.boundaries():
        (t, f), g, _ = case.locate(e)
        assert g - 1 in games and g in games and 0 <= t < T

    def rows_of(buf):
        sel = buf.index_select(2, idx)
        return decode_compact(sel) if form["fmt"] == "compact" else sel

    def launch(kind, env, poison):
        for k in sw.PLAN_OVERRIDES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = _engine(form["cfg"], B, case, dev, layouts)
        _poison(obs, poison)
        if kind == "rollout":
            if form["fmt"] == "int32" and form["name"] in ("paired", "one-lane"):
                shape = eng.rollout_shape(*form["bots"], trajectory=True)
                assert shape["lanes_per_game"] == 1 + (form["name"] == "paired"), (where, shape)
            _poison(act, poison)
            eng.rollout(T, *form["bots"], obs=obs, act=act, obs_format=fmt)
            _same(act.index_select(1, idx), want_act, f"{where} {kind} act", "[tick, game, player]")
        else:
            eng.step_n(act, obs=obs, obs_format=fmt)
        _same(rows_of(obs), want_rows, f"{where} {kind} rows", "[tick, field, game]")
        _same_state(eng, idx, want_state, f"{where} after {kind}")

    launch("rollout", form["env"], POISONS[0])
    if form["replay_env"] is not None:
        launch("step_n", form["replay_env"], POISONS[1])
    _done(where, t0, dev)


STOCK = [c for c in xc.CASES if c.row.name in ("dstore", "mt")]


@pytest.mark.parametrize("case", STOCK, ids=lambda c: c.name)
def test_stock_rows(case, oracle_lib):
    """The stock-seed generators [625][B] and dungeon store [2][N][2][B] past
    2^31 and 2^32 bytes: orx_seed_mt, orx_reset and a rollout of two
    StaircaseBots from separated starts.  The state of the window games
    against the window oracles.  Their generators and their whole store (every
    slot of both players' rings) against engines of the 64 games alone: the
    same kernels at a small batch, so that part is a check that the answer
    does not depend on the extent, not an independent reference (the oracle
    exports neither; it holds the state, whose recalls read the store)."""
    import torch
    t0 = time.time()
    dev, idx = _start(case)
    torch.cuda.reset_peak_memory_stats(dev)
    row, B = case.row, case.B
    _, _, want_state = xc.stock_run(oracle_lib, case)
    win = xc.Windows(oracle_lib, case)
    eng = _engine(row.cfg, B, case, dev, reset=False)
    which = "dstore" if row.name == "dstore" else "mt_py"
    buf = getattr(eng, which)
    assert tuple(buf.shape) == case.shape and buf.numel() * 4 == case.nbytes
    for f in ("mt_py", "mt_np", "dstore"):   # orx_seed_mt fills or clears every word
        _poison(getattr(eng, f), POISONS[0])
    eng.seed_rng()
    eng.reset()
    small = [_engine(row.cfg, xc.WIN, case, dev, offset=g0) for g0 in case.windows()]

    def same(what):
        for f in ("mt_py", "mt_np", "dstore"):
            got = getattr(eng, f).index_select(-1, idx)
            ref = torch.cat([getattr(s, f) for s in small], dim=-1)
            if f == "dstore":
                # a slot is (depth, payload).  orx_seed_mt writes -1 into every
                # depth word and no payload (its loop stores dstore[2 * k * B + i]
                # only), and MtSrc::recall reads a payload only after it found
                # its depth in the depth word: an emptied slot's payload is
                # whatever the buffer held
                payload = torch.tensor([False, True], device=dev)[:, None]
                empty = (ref[:, :, 0] == -1)[:, :, None] & payload
                got, ref = got.masked_fill(empty, 0), ref.masked_fill(empty, 0)
            _same(got, ref.cpu().numpy(), f"{case.name} {what} {f}", "[.., game]")

    _same_state(eng, idx, win.export(), f"{case.name} reset")
    same("reset")
    eng.rollout(case.T, *row.bots)
    for s in small:
        s.rollout(case.T, *row.bots)
    _same_state(eng, idx, want_state, f"{case.name} rollout")
    same("rollout")
    # the store's compared slots are in use on both players' halves
    ds = eng.dstore.index_select(-1, idx).cpu().numpy()
    assert (ds[0, :, 1] != 0).any() and (ds[1, :, 1] != 0).any(), case.name
    _done(case.name, t0, dev)


def _query_engine(case, dev):
    return _engine(case.row.cfg, case.B, case, dev, xc.query_layouts(case))


def _play(eng, idx, acts, bots, where):
    """Plays the window oracles' ticks on the engine: the bots' moves for the
    whole batch from orx_policy, the window games' checked against ``acts``."""
    for t, want in enumerate(acts):
        a = eng.policy(*bots)
        _same(a.index_select(0, idx), want, f"{where} policy tick {t}", "[game, player]")
        eng.step(a)


VIEW = [c for c in xc.CASES if c.row.name in ("window_u8", "window_u8_cells")]


@pytest.mark.parametrize("case", VIEW, ids=lambda c: c.name)
def test_window_u8_rows(case, oracle_lib):
    """The radius-15 window planes uint8 [B][31][31] past 2^31 (cells and
    health) and 2^32 bytes (cells): orx_view, orx_sight's row words and its
    masking in place, and orx_explore_update's remembered view, against
    render_view, sight and explore on the window oracles' state."""
    import torch
    t0 = time.time()
    dev, idx = _start(case)
    torch.cuda.reset_peak_memory_stats(dev)
    health = case.row.name == "window_u8"
    win, acts = xc.query_run(oracle_lib, case)
    snap = win.export()
    want = xc.view_refs(case, snap, health)
    eng = _query_engine(case, dev)
    _play(eng, idx, acts, case.row.bots, case.name)
    _same_state(eng, idx, snap, f"{case.name} state")
    R, B = xc.RADIUS, case.B
    planes = [torch.empty(case.shape, dtype=torch.uint8, device=dev) for _ in range(1 + health)]
    assert planes[0].numel() == case.nbytes
    out = tuple(planes) if health else planes[0]

    def same(what):
        for name, p in zip(("cells", "health"), planes):
            _same(p.index_select(0, idx), want[f"{what}_{name}"], f"{case.name} {what} {name}",
                  "[game, row, column]")

    for p in planes:
        _poison(p, POISONS[0])
    eng.view(R, player=0, health=health, out=out)
    same("view")
    rows = _poison(torch.empty((B, 2 * R + 1), dtype=torch.int32, device=dev), POISONS[1])
    eng.sight(R, player=0, out=rows.view(torch.uint32))
    _same(rows.index_select(0, idx), want["sight"].view(np.int32), f"{case.name} sight", "[game, row]")
    del rows
    eng.seen_view(R, player=0, health=health, out=out)   # (view again, masked in place)
    same("seen")
    for p in planes:
        _poison(p, POISONS[1])
    gained = _poison(torch.empty(B, dtype=torch.int32, device=dev), POISONS[1])
    eng.explore(R, player=0, view=True, health=health, out=(gained,) + tuple(planes))
    same("explore")
    _same(gained.index_select(0, idx), want["gained"], f"{case.name} gained", "[game]")
    memory, key = eng.explore_map(0)
    _same(memory.view(torch.int32).index_select(0, idx), want["memory"].view(np.int32),
          f"{case.name} memory", "[game, y, word]")
    _same(key.index_select(0, idx), want["key"], f"{case.name} key", "[game, field]")
    _done(case.name, t0, dev)


@pytest.mark.parametrize("case", [c for c in xc.CASES if c.row.name == "memory"],
                         ids=lambda c: c.name)
def test_memory_rows(case, oracle_lib):
    """The remembered map uint32 [B][256][8] past 2^31 and 2^32 bytes and 2^31
    elements: orx_explore_update over three states, then orx_explore_seek and
    orx_route -- the windows' maps, keys and gained against explore.update,
    their (dist, move, target) against explore.seek and route.route."""
    import torch
    t0 = time.time()
    dev, idx = _start(case)
    torch.cuda.reset_peak_memory_stats(dev)
    snaps, acts = xc.memory_run(oracle_lib, case)
    want = xc.memory_refs(case, snaps)
    eng = _query_engine(case, dev)
    memory, key = eng.explore_map(0)
    assert tuple(memory.shape) == case.shape and memory.numel() * 4 == case.nbytes
    for t in range(case.T):
        if t:
            _play(eng, idx, acts[t - 1:t], case.row.bots, f"{case.name} state {t}")
        gained = _poison(torch.empty(case.B, dtype=torch.int32, device=dev), POISONS[t % 2])
        eng.explore(xc.MEMORY_RADIUS, player=0, out=gained)
        _same(gained.index_select(0, idx), want["gained"][t], f"{case.name} gained {t}", "[game]")
    _same(memory.view(torch.int32).index_select(0, idx), want["memory"].view(np.int32),
          f"{case.name} memory", "[game, y, word]")
    _same(key.index_select(0, idx), want["key"], f"{case.name} key", "[game, field]")
    shape = (case.B, 4)
    for name, call in (("seek", eng.explore_seek), ("route", eng.explore_route)):
        outs = tuple(_poison(torch.empty(shape, dtype=dt, device=dev), POISONS[0])
                     for dt in (torch.int32, torch.int8, torch.int32))
        got = call(player=0, out=outs)
        for what, g, r in zip(("dist", "move", "target"), got, want[name]):
            _same(g.index_select(0, idx), r, f"{case.name} {name} {what}", "[game, column]")
    _done(case.name, t0, dev)


@pytest.mark.parametrize("case", [c for c in xc.CASES if c.row.name == "options"],
                         ids=lambda c: c.name)
def test_options_rows(case, oracle_lib):
    """orx_npc_options' kind uint8 [255][B][8] past 2^31 bytes, target and
    amount int16 past 2^32 (one of the two beside kind per launch: all three
    exceed the allocation limit), and orx_moves, against npc_query.options and
    moves.outcomes on the window oracles' state."""
    import torch
    t0 = time.time()
    dev, idx = _start(case)
    torch.cuda.reset_peak_memory_stats(dev)
    win, acts = xc.query_run(oracle_lib, case)
    snap = win.export()
    want = xc.options_refs(case, snap)
    eng = _query_engine(case, dev)
    _play(eng, idx, acts, case.row.bots, case.name)
    _same_state(eng, idx, snap, f"{case.name} state")
    B = case.B
    kind = torch.empty(case.shape, dtype=torch.uint8, device=dev)
    where = torch.empty(B, dtype=torch.uint8, device=dev)
    assert kind.numel() == case.nbytes
    for j, name in enumerate(("target", "amount")):
        wide = _poison(torch.empty(case.shape, dtype=torch.int16, device=dev), POISONS[j])
        _poison(kind, POISONS[j]), _poison(where, POISONS[j])
        args = [kind.data_ptr(), None, None, where.data_ptr()]
        args[1 + j] = wide.data_ptr()
        eng._call("orx_npc_options", *args, B, eng._stream())
        _same(kind.index_select(1, idx), want["kind"], f"{case.name} kind", "[slot, game, move]")
        _same(wide.index_select(1, idx), want[name], f"{case.name} {name}", "[slot, game, move]")
        _same(where.index_select(0, idx), want["where"], f"{case.name} where", "[game]")
        del wide   # (before the other one is made: both beside kind pass the limit)
    mk = _poison(torch.empty((B, 8), dtype=torch.uint8, device=dev), POISONS[0])
    eng._call("orx_moves", 0, mk.data_ptr(), None, None, B, eng._stream())
    _same(mk.index_select(0, idx), want["moves_kind"], f"{case.name} moves kind", "[game, move]")
    _done(case.name, t0, dev)


U16 = [c for c in xc.CASES if c.row.name.startswith("window_u16")]


@pytest.mark.parametrize("case", U16, ids=lambda c: c.name)
def test_window_u16_rows(case, oracle_lib):
    """The radius-15 distance windows uint16 [B][31][31] past 2^31 and 2^32
    bytes (2^31 elements), without a bank and with one of two layouts:
    orx_path_query, orx_path_threat and orx_path_ticks, every output, against
    path.query, path.threat and path.ticks on the window oracles' state."""
    import torch
    t0 = time.time()
    dev, idx = _start(case)
    torch.cuda.reset_peak_memory_stats(dev)
    win, acts = xc.query_run(oracle_lib, case)
    snap = win.export()
    want = xc.path_refs(case, snap)
    eng = _query_engine(case, dev)
    assert (eng.bank is not None) == bool(case.row.bank)
    _play(eng, idx, acts, case.row.bots, case.name)
    _same_state(eng, idx, snap, f"{case.name} state")
    R, B = xc.RADIUS, case.B
    # (uint16 storage as int16: the window games are selected from that view)
    window = torch.empty(case.shape, dtype=torch.int16, device=dev)
    assert window.numel() * 2 == case.nbytes
    new = lambda dt, *shape: _poison(torch.empty(shape, dtype=dt, device=dev), POISONS[1])
    calls = (
        ("query", eng.path, ("dist", "move"), (new(torch.int32, B), new(torch.int8, B))),
        ("threat", eng.threat, ("dist", "move", "target", "after"),
         (new(torch.int32, B, 4), new(torch.int8, B, 4), new(torch.int16, B, 4),
          new(torch.int32, B, 8))),
        ("ticks", eng.path_ticks, ("ticks", "move"), (new(torch.int32, B), new(torch.int8, B))))
    for j, (name, call, fields, outs) in enumerate(calls):
        _poison(window, POISONS[j % 2])
        call(player=0, radius=R, out=outs + (window.view(torch.uint16),))
        for f, g in zip(fields, outs):
            _same(g.index_select(0, idx), want[f"{name}_{f}"], f"{case.name} {name} {f}", "[game, ..]")
        _same(window.index_select(0, idx), want[f"{name}_window"].view(np.int16),
              f"{case.name} {name} window", "[game, row, column]")
    _done(case.name, t0, dev)
