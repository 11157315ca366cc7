"""CPU: the enemies' queries (include/orx_npc_query.h) without a GPU -- the
numpy reference (optimax_rogue_amd/npc_query.py) against the guards the
reference fixtures pin, against the CPU restatement of the tick move by move,
against ``path.seek`` from the players' side and against hand-built states;
the header against the export table and the library, the build id, and the
host-side refusals from a plain C consumer."""
import os
import re
import subprocess

import numpy as np
import pytest

from npc_given_cases import guarded
from npc_query_cases import (check_outcome, env_config, given_runs, hand_seek, hand_states,
                             play_one, start_run)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = ("regs", "dense", "bank")


@pytest.fixture(scope="module")
def played():
    """name -> (cfg, bank, [(tick, games deep-copied, snapshot)]): every run
    of given_runs() played once with RandomBot players and a random table."""
    import copy
    from optimax_rogue_amd import DungeonBank
    from oracle.pyref import batch_state
    out = {}
    for name, run in given_runs().items():
        cfg = env_config(run["cfg"], run["layouts"])
        bank = None if run["layouts"] is None else DungeonBank(run["layouts"])
        games, _ = start_run(run)
        ticks = []
        for t in range(run["T"]):
            ticks.append((t, copy.deepcopy(games), batch_state(games)))
            for g in games:
                g.step(*g.policy())
        out[name] = (cfg, bank, ticks)
    return out


@pytest.mark.parametrize("name", RUNS)
def test_mask_is_the_guards(played, name):
    """At every tick, for every live NPC and every move: the guards of
    tests/npc_given_cases.guarded (pinned to the reference fixtures by
    test_npc_given.py) replace the move exactly where ``options`` says FROZEN
    or BLOCKED, and ``action_mask`` is False exactly there."""
    from optimax_rogue_amd import enums as E, npc_query
    cfg, bank, ticks = played[name]
    n = {"live": 0, "replaced": 0, "dead": 0}
    for t, games, snap in ticks:
        kind, _, _, where = npc_query.options(snap, cfg, bank)
        mask = npc_query.action_mask(kind, where)
        assert mask.shape == (cfg.n_npcs, len(games), 5) and mask[:, :, 4].all()
        assert (where != E.NPC_DEPTH_UNWATCHED).all()   # (Together: never)
        for b, game in enumerate(games):
            gs = game.gs
            for k in range(cfg.n_npcs):
                e = gs.iden_lookup.get(3 + k)
                if e is None:
                    assert not kind[k, b].any() and list(mask[k, b]) == [False] * 4 + [True]
                    n["dead"] += 1
                    continue
                for m in range(1, 6):
                    out = int(kind[k, b, m]) & E.NPC_OUT_MASK
                    replaced = guarded(gs, e, m) != m
                    assert replaced == (out in (E.NPC_OUT_FROZEN, E.NPC_OUT_BLOCKED)), \
                        (name, t, b, k, m, out)
                    assert bool(mask[k, b, m - 1]) == (not replaced)
                    n["live"] += 1
                    n["replaced"] += replaced
    assert n["live"] > 1000 and n["replaced"] > 100 and n["dead"] > 10, n


@pytest.mark.parametrize("name", RUNS)
def test_outcome_is_what_the_tick_does(played, name):
    """At sampled ticks, every move of every live NPC of every game in
    progress is played alone (everyone else on Stay) in a deep copy of the
    game: the NPC's new cell or removal and the health the predicted target
    loses are what kind / target / amount / LETHAL said.  The runs reach every
    kind (counted on the CPU before the test was relied on)."""
    from optimax_rogue_amd import npc_query
    from oracle.pyref import IN_PROGRESS
    cfg, bank, ticks = played[name]
    seen = {}
    for t, games, snap in ticks[::3]:
        kind, target, amount, _ = npc_query.options(snap, cfg, bank)
        for b, game in enumerate(games):
            if game.status != IN_PROGRESS:
                continue
            for k in range(cfg.n_npcs):
                if 3 + k not in game.gs.iden_lookup:
                    continue
                for m in range(1, 6):
                    after = play_one(game, k, m)
                    for nm in check_outcome(game, after, k, m, kind[k, b, m], target[k, b, m],
                                            amount[k, b, m]):
                        seen[nm] = seen.get(nm, 0) + 1
    want = {"REST", "STEP", "STAIRS", "ATTACK_PLAYER", "ATTACK_NPC", "LETHAL", "FROZEN", "BLOCKED"}
    if name == "dense":
        want -= {"LETHAL"}   # (12 x 12 with 8 games: the other two runs reach it)
    assert want <= set(seen), (name, seen)


@pytest.mark.parametrize("name", ("regs", "bank"))
def test_seek_is_the_players_seek_from_the_other_end(played, name):
    """Column p of NPC k's row is ``path.seek``'s distance from player p to the
    nearest NPC of a state in which slot k alone is alive (the walking distance
    is symmetric), in the closed form and on a bank; the NEAREST column is the
    lesser of the two, player 1 on a tie; the move leads to a cell one closer."""
    from optimax_rogue_amd import npc_query, path
    from optimax_rogue_amd.enums import NPC_SEEK_NEAREST
    cfg, bank, ticks = played[name]
    K = cfg.n_npcs
    n = {"finite": 0, "absent": 0, "p2 nearer": 0}
    for t, games, snap in ticks[::4]:
        dist, move, target = npc_query.seek(snap, cfg, bank)
        assert dist.shape == (K, len(games), 4) and dist.dtype == np.int32
        assert move.dtype == np.int8 and target.dtype == np.int16
        assert (dist[:, :, 3] == path.SEEK_ABSENT).all() and (move[:, :, 3] == 5).all()
        assert (target[:, :, 3] == -1).all()
        alive = np.asarray(snap["npc_alive"]).astype(np.int64)
        for k in range(K):
            only = dict(snap, npc_alive=alive & (1 << k))
            for p in (0, 1):
                d, _, tg = path.seek(only, cfg, p, bank)
                assert (dist[k, :, p] == d[:, path.SEEK_NPC]).all(), (name, t, k, p)
                assert (target[k, :, p] == np.where(tg[:, path.SEEK_NPC] < 0, -1, p + 1)).all()
        # the nearer: finite < unreachable (-1) < absent (-2)
        rank = lambda d: np.where(d >= 0, d, np.where(d == -1, 1 << 20, 1 << 21))
        second = rank(dist[:, :, 1]) < rank(dist[:, :, 0])
        for a in (dist, move, target):
            assert (a[:, :, NPC_SEEK_NEAREST] == np.where(second, a[:, :, 1], a[:, :, 0])).all()
        assert ((move != 5) == (dist > 0)).all()
        n["finite"] += int((dist[:, :, :2] > 0).sum())
        n["absent"] += int((dist[:, :, :2] == path.SEEK_ABSENT).sum())
        n["p2 nearer"] += int(second.sum())
    assert n["finite"] > 100 and n["absent"] > 10 and n["p2 nearer"] > 10, n


def test_hunt_moves_take_the_step_or_the_attack(played):
    """``hunt_moves``: NEAREST's move where ``options`` calls it STEP or
    ATTACK_PLAYER, else Stay."""
    from optimax_rogue_amd import enums as E, npc_query
    cfg, bank, ticks = played["bank"]
    n = {"moves": 0, "held": 0}
    for t, games, snap in ticks[::5]:
        kind, _, _, _ = npc_query.options(snap, cfg, bank)
        _, move, target = npc_query.seek(snap, cfg, bank)
        hunt = npc_query.hunt_moves(kind, move, target)
        assert hunt.shape == (cfg.n_npcs, len(games)) and hunt.dtype == np.int8
        for k in range(cfg.n_npcs):
            for b in range(len(games)):
                m = int(move[k, b, E.NPC_SEEK_NEAREST])
                out = int(kind[k, b, m]) & E.NPC_OUT_MASK
                ok = out in (E.NPC_OUT_STEP, E.NPC_OUT_ATTACK_PLAYER)
                assert int(hunt[k, b]) == (m if ok else 5)
                n["moves"] += ok
                n["held"] += m != 5 and not ok
    assert n["moves"] > 50 and n["held"] > 0, n


@pytest.mark.parametrize("name", ("room", "unwatched", "gone"))
def test_hand_built_states(name):
    """One hand-built state per row of the header's rule table (a dead slot's
    stale cell, amount == health and health - 1, an occupant on a staircase, a
    player next to a staircase on the NPCs' depth and on another, UNWATCHED
    and GONE): the expectations are written from the header."""
    from optimax_rogue_amd import enums as E, npc_query
    case = hand_states()[name]
    cfg = env_config(case["cfg"])
    kind, target, amount, where = npc_query.options(case["snap"], cfg)
    assert list(where) == case["where"] and where.dtype == np.uint8
    for (b, k, m), want in case["expect"].items():
        got = (int(kind[k, b, m]), int(target[k, b, m]), int(amount[k, b, m]))
        assert got == want, (name, b, k, m, got, want)
    for a, pad in ((kind, 0), (target, -1), (amount, 0)):
        assert (a[:, :, [0, 6, 7]] == pad).all()
    dist, move, target = npc_query.seek(case["snap"], cfg)
    for (nm, b, k), want in hand_seek().items():
        if nm == name:
            got = tuple((int(dist[k, b, c]), int(move[k, b, c]), int(target[k, b, c]))
                        for c in range(3))
            assert got == want, (name, b, k, got, want)
    mask = npc_query.action_mask(kind, where)
    unw = where == E.NPC_DEPTH_UNWATCHED
    live = kind[:, :, 5] == E.NPC_OUT_REST
    assert mask[:, :, 4].all() and not mask[~live][:, :4].any()
    assert mask[live & unw[None, :]].all()


def test_queries_need_npcs():
    from optimax_rogue_amd import EnvConfig, npc_query
    snap = {"p_depth": np.zeros((2, 1), np.int32)}
    for fn in (npc_query.options, npc_query.seek):
        with pytest.raises(ValueError):
            fn(snap, EnvConfig(width=8, height=8, n_npcs=0))


def test_header_is_the_export_table():
    from optimax_rogue_amd import _lib, enums
    with open(os.path.join(ROOT, "include", "orx_npc_query.h")) as f:
        text = f.read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+ORX_(NPC_(?:OUT|DEPTH|SEEK)_\w+)\s+(\d+)",
                                             text)}
    want = {n: getattr(enums, n) for n in dir(enums)
            if re.match(r"NPC_(OUT|DEPTH|SEEK)_", n) and isinstance(getattr(enums, n), int)}
    want.pop("NPC_OUT_MASK")   # (the header uses ORX_OUT_MASK)
    assert defs == want and len(defs) == 15
    assert [defs["NPC_OUT_" + n] for n in enums.NPC_OUT_NAMES] == list(range(8))
    decl = sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(orx_\w+)\s*\(", text, re.M)))
    assert decl == sorted(_lib.NPC_QUERY_EXPORTS) and len(decl) == 3
    # orx.h and orx_npc.h are what they were, and the ABI version with them
    for hdr in ("orx.h", "orx_npc.h"):
        with open(os.path.join(ROOT, "include", hdr)) as f:
            assert "orx_npc_options" not in f.read()
    assert _lib.ABI_VERSION == 7


def test_npc_query_header_in_a_plain_c_consumer(engine_lib, tmp_path):
    """include/orx_npc_query.h compiles as C99 and every refusal of
    orx_npc_options and orx_npc_seek comes back from the host, before any
    launch (no GPU calls)."""
    exe = tmp_path / "npc_query_abi_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "npc_query_abi_check.c"), "-o", str(exe),
                    "-L", os.path.join(ROOT, "optimax_rogue_amd"), "-lorx",
                    "-Wl,-rpath," + os.path.join(ROOT, "optimax_rogue_amd")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orx_npc_query refusals: 42 of 42" in r.stdout
