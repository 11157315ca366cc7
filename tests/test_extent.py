"""CPU: the extent ledger's arithmetic, the window oracle, and that the runs
test_gpu_extent.py compares contain what makes a passing comparison mean
something -- all from the oracle alone (extent_cases.py)."""
import numpy as np
import pytest

import extent_cases as xc

IDS = [c.name for c in xc.CASES]


@pytest.mark.parametrize("case", xc.CASES, ids=IDS)
def test_ledger_arithmetic(case):
    """Extents recomputed from dtype and shape: every named boundary lies
    strictly inside the buffer, its window holds a game on both sides of it
    (for a batch-strided buffer: on the row that straddles it), and the
    allocation fits."""
    size = {"u8": 1, "u16": 2, "i32": 4, "u32": 4}[case.row.dtype]
    shape = [case.B if d == "B" else case.T if d == "T" else d for d in case.row.shape]
    elems = 1
    for d in shape:
        elems *= int(d)
    assert (case.elems, case.nbytes) == (elems, elems * size)
    assert case.allocation() <= xc.LIMIT
    bounds = case.boundaries()
    assert any(k == xc.BYTE and v == 1 << 31 for k, v, _ in bounds), "2^31 bytes not crossed"
    # a boundary the row's largest batch does not cross is named in its omissions
    if case.B == max(case.row.batches) and len(bounds) < len(xc.BOUNDARIES) \
            and case.nbytes != case.elems:
        assert "omitted" in case.row.omitted, case.name
    windows, games = case.windows(), set(case.games().tolist())
    assert windows[0] == 0 and windows[-1] == case.B - xc.WIN
    assert all(0 <= g0 <= case.B - xc.WIN for g0 in windows)
    strides = [int(np.prod(shape[i + 1:], dtype=object)) for i in range(len(shape))]
    for kind, v, e in bounds:
        assert 0 < e < elems and 0 < e * size < elems * size
        assert e * size == v if kind == xc.BYTE else e == v
        g0 = case.window_at(e)
        assert g0 in windows
        before, after = case.locate(e - 1), case.locate(e)
        for lead, g, trail in (before, after):   # (locate() against the strides)
            assert sum(i * s for i, s in zip(lead + (g,) + trail, strides)) in (e - 1, e)
        if case.axis == 0:
            # [B][..]: the last game before the boundary and the first after it
            lo, hi = before[1], after[1] if after[1] != before[1] else after[1] + 1
            if after[1] == before[1]:
                lo = before[1] - 1   # (one game straddles it: a whole game on either side)
            assert g0 <= lo < hi < g0 + xc.WIN and {lo, hi} <= games
        else:
            # [..][B]: both elements on one compared row, its games g - 1 and g
            assert before[0] == after[0] and after[0] in case.leads()
            assert before[1] + 1 == after[1]
            assert g0 <= before[1] < after[1] < g0 + xc.WIN and {before[1], after[1]} <= games


def test_ledger_rows_and_sizes():
    """The rows' sizes are the engine's: the dungeon store's slots, the
    state's bytes per game against the tensors BatchedEngine makes."""
    assert xc.dstore_depths(1000) == 1024 and xc.dstore_depths(16) == 256
    assert xc.ROW["dstore"].shape[1] == xc.dstore_depths(xc.ROW["dstore"].cfg["max_ticks"])
    for r in ("grid_wide", "grid_dense"):
        cfg = xc.ROW[r].cfg
        assert xc.ROW[r].shape[1] == cfg["width"] * cfg["height"] and cfg["n_npcs"] >= 17
    assert len({r.name for r in xc.ROWS}) == len(xc.ROWS)
    for r in xc.ROWS:
        assert r.offset != 0 and r.omitted


def test_window_oracle_is_the_batch(oracle_lib):
    """window_oracle of games [g0, g0 + n) equals games g0.. of one larger
    oracle, through resets, NPC fights and descents."""
    case = xc.Case(xc.Row("probe", dict(width=9, height=8, n_npcs=20, npc_health=1, max_ticks=15),
                          0, (1, 2), 5, 777, None, "u8", ("B", 72), (3000,), {}, (), ""), 3000)
    whole = oracle_lib.Oracle(case.row.cfg, case.B, case.row.seed, case.row.offset)
    whole.reset(episode=np.zeros(case.B, np.int32))
    parts = {g0: xc.window_oracle(oracle_lib, case, g0) for g0 in (0, 1499, case.B - xc.WIN)}
    for t in range(40):
        a = whole.policy(*case.row.bots)
        whole.step(a)
        want = whole.export()
        for g0, o in parts.items():
            idx = np.arange(g0, g0 + xc.WIN)
            ap = o.policy(*case.row.bots)
            assert np.array_equal(ap, a[idx]), (t, g0)
            o.step(ap)
            got = o.export()
            for k, w in xc.slice_snapshot(want, idx).items():
                assert np.array_equal(got[k], w), (t, g0, k)
    assert want["ep_count"].sum() > 0 and want["counters"][1].sum() > 0


@pytest.fixture(scope="module")
def grid_witness(oracle_lib):
    out = {}
    for case in xc.CASES:
        if case.row.name.startswith("grid_"):
            w = xc.Witness(case.row.cfg)
            xc.grid_run(oracle_lib, case, w)
            out[case.name] = w
    return out


@pytest.mark.parametrize("case", [c for c in xc.CASES if c.row.name.startswith("grid_")],
                         ids=lambda c: c.name)
def test_grid_coverage(case, grid_witness):
    """NPC hits, NPC deaths and a restart inside the run among the compared
    games; in grid_dense at least one of each on both sides of every boundary."""
    w = grid_witness[case.name]
    for what in ("npc_hit", "npc_death", "restart"):
        assert w.seen.get(what), (case.name, what)
        if case.row.name == "grid_dense":
            for before, after in w.sides(what, case):
                assert before > 0 and after > 0, (case.name, what, before, after)


TRAJ = [(c, f) for c in xc.CASES if c.row.name.startswith("traj_")
        for f in xc.traj_forms(c.row.name)]


@pytest.mark.parametrize("case,form", TRAJ, ids=lambda v: v.name if hasattr(v, "name") else v["name"])
def test_traj_coverage(case, form, oracle_lib):
    """Both episode ends and a descent among the compared games."""
    w = xc.Witness(form["cfg"])
    xc.traj_run(oracle_lib, case, form, w)
    for what in ("end_ticks", "end_win", "descend", "restart"):
        assert w.seen.get(what), (case.name, form["name"], what)


@pytest.mark.parametrize("case", [c for c in xc.CASES if c.row.name in ("dstore", "mt")],
                         ids=lambda c: c.name)
def test_stock_coverage(case, oracle_lib):
    """A descent by player 2 and, in the dstore row, a recall by player 1 of a
    dungeon player 2 made -- on both sides of every boundary's window."""
    w = xc.Witness(case.row.cfg)
    xc.stock_run(oracle_lib, case, w)
    assert w.seen.get("descend_p2"), case.name
    if case.row.name == "dstore":
        assert w.seen.get("recall"), case.name
        for what in ("descend_p2", "recall"):
            for before, after in w.sides(what, case):
                assert before > 0 and after > 0, (case.name, what, before, after)


QUERY = [c for c in xc.CASES if c.row.name in ("window_u8", "window_u8_cells", "options",
                                               "window_u16", "window_u16_bank")]


@pytest.mark.parametrize("case", QUERY, ids=lambda c: c.name)
def test_window_coverage(case, oracle_lib):
    """The compared windows are not all one value, on either side of a boundary."""
    win, _ = xc.query_run(oracle_lib, case)
    snap = win.export()
    if case.row.name.startswith("window_u16"):   # (the three windows; the rest is a row per game)
        refs = {k: v for k, v in xc.path_refs(case, snap).items() if k.endswith("window")}
        assert len(refs) == 3
    elif case.row.name == "options":
        refs = xc.options_refs(case, snap)
    else:
        refs = xc.view_refs(case, snap, health=case.row.name == "window_u8")
    games = case.games()
    for name, a in refs.items():
        if name in ("where", "key"):   # (a byte and a key row per game: no window buffer)
            continue
        axis = 1 if name in ("kind", "target", "amount") else 0
        for _, _, e in case.boundaries():
            cut, g0 = case.locate(e)[1], case.window_at(e)
            for side in ((games >= g0) & (games < cut), (games >= cut) & (games < g0 + xc.WIN)):
                assert len(np.unique(np.compress(side, a, axis=axis))) > 1, (case.name, name)


@pytest.mark.parametrize("case", [c for c in xc.CASES if c.row.name == "memory"][-1:],
                         ids=lambda c: c.name)
def test_memory_coverage(case, oracle_lib):
    """gained > 0 and a frontier target on both sides of every boundary (the
    largest batch: its windows hold every boundary of the smaller ones, at the
    same games)."""
    from optimax_rogue_amd.explore import EXPLORE_FRONTIER
    small = {e for c in xc.CASES if c.row.name == "memory" for _, _, e in c.boundaries()}
    assert small == {e for _, _, e in case.boundaries()}
    snaps, _ = xc.memory_run(oracle_lib, case)
    refs = xc.memory_refs(case, snaps)
    games = case.games()
    for _, _, e in case.boundaries():
        cut, g0 = case.locate(e)[1], case.window_at(e)
        for side in ((games >= g0) & (games < cut), (games >= cut) & (games < g0 + xc.WIN)):
            assert side.sum() >= xc.WIN // 2
            assert all((g[side] > 0).any() for g in refs["gained"]), case.name
            for dist, move, target in (refs["seek"], refs["route"]):
                assert (target[side, EXPLORE_FRONTIER] >= 0).any(), case.name
                assert (dist[side, EXPLORE_FRONTIER] > 0).any(), case.name
