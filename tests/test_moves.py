"""CPU: the per-move outcomes' host statement (optimax_rogue_amd.moves) against
the C oracle, move by move -- every move of both players is played as (m, Stay)
in a fresh oracle rolled to the same state, and what the tick did is compared
with what ``outcomes`` said -- plus the coverage those states give, the
header's constants, the library's exports and ids, and the entry point's
refusals from a plain-C consumer.  Integers compared exactly; nothing here
needs a GPU (the last tests load the built library, no GPU calls).
"""
import functools
import os
import re

import numpy as np
import pytest

import moves_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mc.cases()


@functools.lru_cache(maxsize=None)
def run_case(name):
    """Plays every (player, move) of a case against the oracle; returns the
    summed counts of moves_cases.compare_move (and the fewest games compared
    in one step as 'games')."""
    from optimax_rogue_amd import moves as mv
    case = CASES[name]
    cfg = case["cfg"]
    total = {}
    for p in (0, 1):
        for m in range(1, mc.n_moves(cfg) + 1):
            ora = mc.rolled_oracle(case)
            pre = ora.export()
            pred = mv.outcomes(cfg, pre, p)
            for a, dt in zip(pred, (np.uint8, np.int16, np.int16)):
                assert a.dtype == dt and a.shape == (mc.N_GAMES, mv.MOVES_COLS)
            ora.step(mc.actions_for(ora.B, p, m))
            ev, nev = mc.oracle_events(ora)
            c = mc.compare_move(cfg, pre, pred, p, m, ora.export(), ev, nev)
            for k, v in c.items():
                total[k] = min(total.get(k, v), v) if k == "games" else total.get(k, 0) + v
    return total


@pytest.mark.parametrize("name", sorted(CASES))
def test_outcomes_are_what_the_oracle_does(oracle_lib, name):
    total = run_case(name)
    # no game is left out but those not InProgress before the step
    assert total["games"] >= 0.95 * mc.N_GAMES, total


def test_unused_columns_and_mask(oracle_lib):
    from optimax_rogue_amd import moves as mv
    for name in ("base8", "character"):
        case = CASES[name]
        cfg = case["cfg"]
        M = mc.n_moves(cfg)
        assert M == (6 if name == "character" else 5)
        pre = mc.rolled_oracle(case, 256).export()
        kind, target, amount = mv.outcomes(cfg, pre, 1)
        for col in [0] + list(range(M + 1, mv.MOVES_COLS)):
            assert (kind[:, col] == mv.OUT_NONE).all() and (target[:, col] == -1).all()
            assert (amount[:, col] == 0).all()
        assert (kind[:, 1:M + 1] & mv.OUT_MASK != mv.OUT_NONE).all()
        mask = mv.action_mask(kind, M)
        assert mask.dtype == bool and mask.shape == (256, M)
        want = ((kind[:, 1:M + 1] & 7) != 2) & ((kind[:, 1:M + 1] & 32) == 0)
        assert np.array_equal(mask, want) and mask[:, 4].all() and not mask.all()
    for bad in (2, -1, 0.5):
        with pytest.raises(ValueError):
            mv.outcomes(cfg, pre, bad)


def test_coverage(oracle_lib):
    """A condition, not a measurement: the oracle's states alone exercise every
    outcome and every flag."""
    for name in mc.BASE:
        total = run_case(name)
        for outcome in ("REST", "BLOCKED", "STEP", "DESCEND", "ATTACK_NPC", "ATTACK_PLAYER"):
            assert total[outcome] >= 100, (name, outcome, total)
        assert total["LETHAL"] >= 50, (name, total)
    ext = [run_case(name) for name in mc.EXTENSIONS]
    for flag in ("ITEM", "HEAL>0", "COOLDOWN"):
        assert sum(t[flag] for t in ext) >= 10, (flag, ext)
    # the other paths: player 2 off the NPCs' depth, a bank, dense NPCs
    for name in ("sep", "bank", "dense"):
        total = run_case(name)
        assert min(total[o] for o in ("BLOCKED", "STEP", "DESCEND", "ATTACK_NPC",
                                      "ATTACK_PLAYER")) >= 10, (name, total)


def test_header_constants_are_the_modules():
    from optimax_rogue_amd import _lib, moves
    with open(os.path.join(ROOT, "include", "orx_moves.h")) as f:
        text = f.read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(ORX_(?:OUT|MOVES)_\w+)\s+(\d+)", text)}
    want = {"ORX_MOVES_COLS": moves.MOVES_COLS}
    want.update({"ORX_" + n: getattr(moves, n) for n in dir(moves) if n.startswith("OUT_")
                 and isinstance(getattr(moves, n), int)})
    assert defs == want and len(defs) == 13
    assert [defs["ORX_OUT_" + n] for n in moves.OUT_NAMES] == list(range(8))
    assert (defs["ORX_OUT_LETHAL"], defs["ORX_OUT_ITEM"], defs["ORX_OUT_COOLDOWN"]) == (8, 16, 32)
    decl = sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(orx_\w+)\s*\(", text, re.M)))
    assert decl == sorted(_lib.MOVES_EXPORTS)
    # orx.h is what it was: the new entry points are not declared there
    with open(os.path.join(ROOT, "include", "orx.h")) as f:
        assert "orx_moves" not in f.read()


def test_moves_header_in_a_plain_c_consumer(engine_lib, tmp_path):
    """include/orx_moves.h compiles as C99 and every refusal of orx_moves comes
    back from the host, before any launch (no GPU calls)."""
    import subprocess
    exe = tmp_path / "moves_abi_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "moves_abi_check.c"), "-o", str(exe),
                    "-L", os.path.join(ROOT, "optimax_rogue_amd"), "-lorx",
                    "-Wl,-rpath," + os.path.join(ROOT, "optimax_rogue_amd")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orx_moves refusals: 26 of 26" in r.stdout
