"""CPU: the numpy references of the six query kernels over the query sweep's
draws (tests/query_sweep.py: the fuzz's configuration space plus radii,
optional outputs, tick counts and the item and cooldown leans), on ORACLE
states alone -- what tests/test_gpu_query_sweep.py then holds the kernels to:

  * ``moves.outcomes`` against the oracle's tick, move by move, on every case
    without moving NPCs (moves_cases.compare_move, as test_moves.run_case);
  * ``render_view``, ``path.seek`` and ``npc_query.seek`` against per-game
    restatements in the reference's schema, on a subset of the cases;
  * ``path.query``'s distance on every bank case against scipy's Dijkstra;
  * the coverage conditions: the sweep's states reach every outcome, flag,
    seek answer, NPC form and depth state (a sweep of absent targets would
    prove nothing).

Integers compared exactly; nothing here needs a GPU.
"""
import functools
import os

import numpy as np
import pytest

import moves_cases as mc
import path_cases as pc
import query_sweep as qs
import seek_cases as sc
import view_cases as vc

CASES = [qs.draw(c) for c in range(qs.N_CASES)]
STILL = [d.case for d in CASES if not d.moving]         # (m, Stay) is exact with Stay NPCs
BANKS = [d.case for d in CASES if d.layouts is not None]
N_GAMES = 256
# the per-game restatements are Python loops: "<cases>x<games>", spread over the
# sweep; scipy's all-pairs tables keep them to grids of at most 1,600 cells
N_RESTATE, RESTATE_GAMES = (int(v) for v in
                            os.environ.get("ORX_QSWEEP_RESTATE", "24x24").split("x"))
SMALL = [d.case for d in CASES if d.cfg["width"] * d.cfg["height"] <= 1600]
RESTATE = SMALL[::max(1, len(SMALL) // N_RESTATE)][:N_RESTATE]


def test_draws_are_valid_and_varied():
    """Every draw satisfies orx_validate_cfg's rules, both leans and every
    optional-output form occur, and at most a tenth of the cases skip the
    seeks."""
    seen = set()
    for d in CASES:
        qs.check_draw(d)
        again = qs.draw(d.case)
        assert again.cfg == d.cfg and again.ticks == d.ticks and again.radius == d.radius
        seen |= {d.lean, f"ticks{d.ticks}", f"B{d.B}"}
        seen |= {f"health{int(v)}" for v in d.health} | {f"window{int(v)}" for v in d.window}
        seen |= {f"moves{v}" for v in d.moves_mask} | {f"seek{v}" for v in d.seek_mask}
        seen |= {f"npc{d.npc_mask}"} | {f"R{r}" for r in d.radius}
        seen |= {"npc_health127"} if d.cfg["npc_health"] == 127 and d.cfg["n_npcs"] else set()
        seen |= {"big bank"} if d.layouts is not None and d.cfg["width"] != d.cfg["height"] \
            and d.cfg["width"] * d.cfg["height"] > 144 else set()
    want = {None, "items", "cooldown", "health0", "health1", "window0", "window1", "npc_health127",
            "big bank", "R1", "R15"}
    want |= {f"ticks{t}" for t in qs.TICKS + qs.LEAN_TICKS}
    want |= {f"B{b}" for b in (1, 63, 257, 1000, 1531)}
    want |= {f"moves{v}" for v in range(4)} | {f"seek{v}" for v in range(1, 8)}
    want |= {f"npc{v}" for v in range(8)}
    if qs.N_CASES >= 96:
        assert want <= seen, want - seen
    unseekable = sum(not d.seekable for d in CASES)
    assert unseekable <= qs.MAX_UNSEEKABLE * len(CASES), unseekable
    # the fuzz's own draws are what they were: the sweep only reads _draw
    from test_gpu_fuzz import _draw
    assert _draw(3)[0] == _draw(3, base=1000)[0]


@functools.lru_cache(maxsize=None)
def run_moves(case):
    """Plays every (player, move) of a case against the oracle at N_GAMES
    games; returns compare_move's summed counts."""
    from optimax_rogue_amd import moves as mv
    d = CASES[case]
    cfg = qs.env_config(d)
    total = {}
    rolled = qs.rolled_oracle(d, N_GAMES, record_events=True)
    pre = rolled.export()
    for p in (0, 1):
        pred = mv.outcomes(cfg, pre, p)
        for a, dt in zip(pred, (np.uint8, np.int16, np.int16)):
            assert a.dtype == dt and a.shape == (N_GAMES, mv.MOVES_COLS), qs.where(d)
        for m in range(1, mc.n_moves(cfg) + 1):
            ora = rolled.clone()      # (the same state for every move, rolled once)
            ora.step(mc.actions_for(ora.B, p, m))
            ev, nev = mc.oracle_events(ora)
            try:
                c = mc.compare_move(cfg, pre, pred, p, m, ora.export(), ev, nev)
            except AssertionError as e:
                raise AssertionError(f"{qs.where(d)}: {e}") from e
            for k, v in c.items():
                total[k] = total.get(k, 0) + v
    return total


@pytest.mark.parametrize("case", STILL)
def test_outcomes_are_what_the_oracle_does(oracle_lib, case):
    total = run_moves(case)
    # not vacuous: a finished game shows its result for one tick and restarts,
    # so at any tick most games are InProgress and were compared
    moves = 2 * mc.n_moves(qs.env_config(CASES[case]))
    assert total["games"] >= 0.5 * N_GAMES * moves, (qs.where(CASES[case]), total)


# the first case of each kind of state a copy has to carry (a narrowed sweep may lack some)
CLONED = sorted({next((d.case for d in CASES if kind(d)), 0) for kind in (
    lambda d: True, lambda d: d.layouts is not None, lambda d: d.cfg.get("rng"),
    lambda d: d.moving, lambda d: d.lean == "items")})


@pytest.mark.parametrize("case", CLONED)
def test_a_cloned_oracle_continues_like_a_rolled_one(oracle_lib, case):
    """``Oracle.clone`` (what run_moves plays every move in): the copy's next
    ticks, events included, are those of a second oracle rolled to the state."""
    d = CASES[case]
    a = qs.rolled_oracle(d, 64, record_events=True)
    b = qs.rolled_oracle(d, 64, record_events=True).clone()
    for t in range(4):
        act = a.policy(1, 1)
        assert np.array_equal(act, b.policy(1, 1)), (qs.where(d), t)
        a.step(act)
        b.step(act)
        sa, sb = a.export(), b.export()
        assert sa.keys() == sb.keys()
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), (qs.where(d), t, k)
        assert [a.events(g) for g in range(64)] == [b.events(g) for g in range(64)]
    # and the original is left as it was by what its copy played
    c = qs.rolled_oracle(d, 64, record_events=True)
    twin = c.clone()
    before = c.export()
    twin.step(twin.policy(1, 1))
    after = c.export()
    for k in before:
        assert np.array_equal(before[k], after[k]), (qs.where(d), k)


def expected_npc_seek(gs, snap, i, cfg, dists):
    """``(dist, move, target)`` lists [K][4] of game ``i``: every NPC's walk to
    each player -- seek_cases.Distances from the other end (the walking
    distance is symmetric) -- and the nearer of the two, in plain loops over
    the game in the reference's schema."""
    W, H, K = int(cfg.width), int(cfg.height), int(cfg.n_npcs)
    nd = int(cfg.p1_depth) if int(cfg.start_mode) == 2 else 0
    cell = lambda x, y: int(x) * H + int(y)
    dist = [[sc.ABSENT] * 4 for _ in range(K)]
    move = [[sc.STAY] * 4 for _ in range(K)]
    target = [[-1] * 4 for _ in range(K)]
    players = [gs.iden_lookup[1], gs.iden_lookup[2]]
    if not any(pl.depth == nd for pl in players):
        return dist, move, target
    for k in range(K):
        npc = gs.iden_lookup.get(3 + k)
        if npc is None:
            continue
        for p, pl in enumerate(players):
            if pl.depth != nd:
                continue
            table, _, layout = dists.table(p, i)
            row = table[cell(pl.x, pl.y)]
            far = int(row[cell(npc.x, npc.y)]) >= sc.FAR_V
            reach = -1 if far else int(row[cell(npc.x, npc.y)])
            dist[k][p], target[k][p] = reach, p + 1
            if reach <= 0:
                continue
            for code, (dx, dy) in enumerate(((0, -1), (1, 0), (0, 1), (-1, 0)), start=1):
                x, y = npc.x + dx, npc.y + dy
                if not (0 <= x < W and 0 <= y < H):
                    continue
                if layout[x, y] == pc.STAIR and (x, y) != (pl.x, pl.y):
                    continue
                if int(row[cell(x, y)]) == reach - 1:
                    move[k][p] = code
                    break
        # the nearer: a distance beats unreachable beats absent, player 1 a tie
        rank = lambda v: v if v >= 0 else (1 << 30) - v
        q = 1 if rank(dist[k][1]) < rank(dist[k][0]) else 0
        dist[k][2], move[k][2], target[k][2] = dist[k][q], move[k][q], target[k][q]
    return dist, move, target


@pytest.mark.parametrize("case", RESTATE)
def test_references_match_the_reference_schema(oracle_lib, case):
    """``render_view`` (item bits masked: the schema has no items),
    ``path.seek`` and ``npc_query.seek`` against the per-game restatements."""
    from optimax_rogue_amd import compat, npc_query, path
    from optimax_rogue_amd.view import VIEW_ITEM, VIEW_ITEM_KIND, render_view
    d = CASES[case]
    cfg, bank, n = qs.env_config(d), qs.bank_of(d), RESTATE_GAMES
    snap = qs.rolled_oracle(d, n).export()
    games = [compat.game_state(snap, i, cfg, None, bank=bank) for i in range(n)]
    dists = sc.Distances(cfg, snap)
    plain = np.uint8(0xFF & ~(VIEW_ITEM | VIEW_ITEM_KIND))
    for player in (0, 1):
        cells, health = render_view(snap, cfg, player, d.radius[player], bank=bank, health=True)
        assert not (cells & 0xC0).any() and not health[(cells & 12) == 0].any(), qs.where(d)
        got = path.seek(snap, cfg, player, bank=bank)
        for i, gs in enumerate(games):
            want_c, want_h = vc.expected_window(gs, player, d.radius[player])
            assert np.array_equal(cells[i] & plain, want_c), (qs.where(d), "cells", player, i)
            assert np.array_equal(health[i], want_h), (qs.where(d), "health", player, i)
            want = sc.expected_seek(gs, snap, i, cfg, player, dists)[:3]
            for g, w, what in zip(got, want, ("dist", "move", "target")):
                assert g[i].tolist() == list(w), (qs.where(d), "seek", what, player, i)
    if int(cfg.n_npcs):
        got = npc_query.seek(snap, cfg, bank)
        for i, gs in enumerate(games):
            want = expected_npc_seek(gs, snap, i, cfg, dists)
            for g, w, what in zip(got, want, ("dist", "move", "target")):
                assert g[:, i].tolist() == w, (qs.where(d), "npc_seek", what, i)


@pytest.fixture(scope="module")
def sweep(oracle_lib):
    """case -> (state of the oracle at the draw's own batch after its ticks,
    that state's tally): what the engine's states are, bit for bit."""
    out = {}
    for d in CASES:
        cfg, bank = qs.env_config(d), qs.bank_of(d)
        snap = qs.rolled_oracle(d).export()
        out[d.case] = (snap, qs.tally(d, cfg, snap, qs.references(d, cfg, snap, bank)))
    return out


@pytest.mark.parametrize("case", BANKS)
def test_bank_distance_is_dijkstras(sweep, case):
    """``path.query``'s ``dist`` of both players on a bank: scipy's Dijkstra
    from all staircases of the player's layout, at the player's cell."""
    from optimax_rogue_amd import path
    d = CASES[case]
    cfg, snap = qs.env_config(d), sweep[case][0]
    fields = {}
    for p in (0, 1):
        dist = path.query(snap, cfg, p, bank=qs.bank_of(d))[0]
        assert dist.dtype == np.int32 and dist.shape == (d.B,)
        for i in range(d.B):
            lay = int(snap["p_layout"][p][i])
            if lay not in fields:
                fields[lay] = pc.dijkstra_field(d.layouts[lay]).astype(np.int64)
            want = int(fields[lay][int(snap["p_x"][p][i]), int(snap["p_y"][p][i])])
            assert int(dist[i]) == (-1 if want == 0xFFFE else want), (qs.where(d), p, i)


def test_coverage(sweep):
    """Conditions, not measurements, on the oracle's states and the references
    alone, summed over the sweep and both players (query_sweep.COVERAGE)."""
    if qs.N_CASES < 96:
        pytest.skip("the coverage conditions are those of the whole sweep")
    qs.check_coverage(qs.add_up(t for _, t in sweep.values()))
