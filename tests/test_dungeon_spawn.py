"""CPU: the oracle's side of test_gpu_dungeon_spawn.py.  Every dungeon of the
oracle's world is the one spawn_dungeon draws from the (game, episode, depth,
generation) stream (oracle/pyref.py's words), with the generation that
dungeon_cases.Tracker derives from the players' depths alone; and every Unused
case holds a generation-1 descent whose staircase differs from generation
0's, so the GPU test can tell the two apart."""
import numpy as np
import pytest

import dungeon_cases as dc


@pytest.fixture(scope="module")
def runs(oracle_lib):
    return {c.name: dc.run(oracle_lib, c) for c in dc.CASES}


def test_cases_span_the_issue():
    cfgs = [c.cfg for c in dc.CASES]
    assert {c["despawn"] for c in cfgs} == {dc.UNREACHABLE, dc.UNUSED}
    assert {c.get("start_mode", dc.TOGETHER) for c in cfgs} == {dc.TOGETHER, dc.SEPARATED}
    assert {c.bank for c in dc.CASES} >= {0, 1, 6}
    sides = [s for c in cfgs for s in (c["width"], c["height"])]
    assert min(sides) == 4 and max(sides) == 40
    assert {b for c in dc.CASES for b in c.bots} == {1, 2}


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_world_is_the_keyed_spawn(case, runs):
    ticks, tr = runs[case.name]
    seen = 0
    for t, _, s, rows in ticks:
        want = dc.ref_rows(case, rows[:, 0] + dc.OFFSET, rows[:, 1], rows[:, 2], rows[:, 3])
        bad = np.flatnonzero((want != rows[:, 4:7]).any(axis=1))
        assert not len(bad), (case.name, t, rows[bad[:3]], want[bad[:3]])
        seen += len(rows)
        if case.cfg["despawn"] == dc.UNUSED:   # World == {p1.d, p2.d}
            for g in np.unique(rows[:, 0]):
                assert set(rows[rows[:, 0] == g, 2]) == {int(s["p_depth"][0][g]),
                                                         int(s["p_depth"][1][g])}
    assert seen > dc.B * dc.TICKS // 2 and tr.descents > dc.B // 4, (case.name, seen, tr.descents)
    assert tr.unknown.sum() < dc.B // 2


@pytest.mark.parametrize("case", [c for c in dc.CASES if c.cfg["despawn"] == dc.UNUSED],
                         ids=lambda c: c.name)
def test_generation_one_descents(case, runs):
    ticks, tr = runs[case.name]
    assert tr.gen1, case.name
    differ = 0
    for t, g, p, nd, od in tr.gen1:
        assert nd != od
        s = ticks[t][2]
        ep = int(s["episode"][g])
        landed = (int(s["st_x"][p][g]), int(s["st_y"][p][g]))
        one, zero = (dc.ref_spawn(case, g + dc.OFFSET, ep, nd, gen) for gen in (1, 0))
        assert landed == one[:2], (case.name, t, g, p, nd)
        if case.bank:
            assert int(s["p_layout"][p][g]) == one[2]
        differ += one != zero
    assert differ > 0, case.name
