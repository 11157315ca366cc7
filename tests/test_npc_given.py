"""CPU: the given-NPC-move tick (include/orx_npc.h) without a GPU -- the CPU
restatement against the reference's fixtures, the header against the export
table and the library, the build id, and the host-side refusals from a plain
C consumer."""
import os
import re
import subprocess

import numpy as np
import pytest

from golden_util import compare_state
from npc_given_cases import GIVEN_CASES, GivenGame, given_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", GIVEN_CASES)
def test_given_game_vs_reference_fixture(name):
    """GivenGame (oracle/pyref.py's Game with decide_npc_move = the guards plus
    a table) equals the reference run of tests/golden/make_given.py tick by
    tick: states, events, World.dungeons and GameState.entities order.  It is
    what the GPU tests compare larger sweeps against."""
    from oracle.pyref import batch_state
    fx = given_fixture(name)
    table = fx.z["npc_moves"]
    assert table.dtype == np.int8 and table.shape == (fx.T, fx.K, fx.G)
    assert table.min() >= 1 and table.max() <= 5
    assert int(fx.cfg["npc_policy"]) == 0   # (the entry points do not read it)
    cfg = dict(fx.cfg, policy=fx.policy)
    games = [GivenGame(cfg, fx.seed, fx.game_offset + g, table, g, layouts=fx.layouts)
             for g in range(fx.G)]
    compare_state(batch_state(games), fx.state(0), fx.K, f"{name} t=0")
    for t in range(fx.T):
        for g, game in enumerate(games):
            a = game.policy()
            assert list(fx.actions[t, g]) == a, f"{name} policy t={t} g={g}"
            ev = game.step(*a)
            assert ev == fx.events(t, g), (name, t, g)
            assert game.world_list() == fx.world(t + 1, g), (name, t, g)
            assert game.entity_list() == fx.entities(t + 1, g), (name, t, g)
        compare_state(batch_state(games), fx.state(t + 1), fx.K, f"{name} t={t + 1}")


@pytest.mark.parametrize("name", GIVEN_CASES)
def test_fixture_holds_every_kind_of_npc_event(name):
    """The condition make_given.py puts on its seeds, on the committed data: an
    NPC move, an NPC staircase death (a death that no sweep explains: the NPC
    was not hit to 0), NPC->player combat, NPC->NPC Block / Ambush / Flee and
    player->NPC combat; and every file stays under 256 KB."""
    fx = given_fixture(name)
    ev = fx.z["events"]
    combat = ev[ev[:, 0] == 1]
    npc_att, npc_def = combat[:, 1] >= 3, combat[:, 2] >= 3
    assert ((ev[:, 0] == 3) & (ev[:, 1] >= 3)).any()
    assert (npc_att & ~npc_def).any() and (~npc_att & npc_def).any()
    for flag in (1, 2, 3):   # Block, Ambush, Flee
        assert (npc_att & npc_def & (combat[:, 3] == flag)).any(), flag
    # staircase deaths: an NPC that died with health left (every hit takes 1:
    # the players' 2 - 1, the NPCs' 1 - 0) was not swept, it stepped onto stairs
    assert int(fx.cfg["player_damage"]) - int(fx.cfg["player_armor"]) == 1
    assert int(fx.cfg["npc_damage"]) - int(fx.cfg["npc_armor"]) == 1
    stair_deaths = 0
    for t in range(fx.T):
        hp = fx.z["npc_health"][t]
        for g in range(fx.G):
            rows = fx.events(t, g)
            for ty, iden, _, _ in rows:
                if ty == 2 and iden >= 3:
                    hits = sum(1 for r in rows if r[0] == 1 and r[2] == iden)
                    stair_deaths += int(hp[iden - 3, g]) - hits > 0
    assert stair_deaths > 0
    path = os.path.join(ROOT, "tests", "golden", "given", name + ".npz")
    assert os.path.getsize(path) <= 256 * 1024


def test_header_is_the_export_table():
    from optimax_rogue_amd import _lib
    with open(os.path.join(ROOT, "include", "orx_npc.h")) as f:
        text = f.read()
    decl = sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(orx_\w+)\s*\(", text, re.M)))
    assert decl == sorted(_lib.NPC_EXPORTS) and len(decl) == 6
    # orx.h is what it was: the new entry points are not declared there
    with open(os.path.join(ROOT, "include", "orx.h")) as f:
        assert "orx_npc_" not in f.read()


def test_npc_header_in_a_plain_c_consumer(engine_lib, tmp_path):
    """include/orx_npc.h compiles as C99; orx_npc_max_events answers 22 / 516
    / ORX_MAX_EVENTS; n_npcs = 0, flags outside the limit, a NULL table, an
    invalid cfg and (orx_npc_step_n, orx_npc_env_step) a stock-seed cfg are
    refused on the host, before any device call."""
    exe = tmp_path / "npc_abi_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "npc_abi_check.c"), "-o", str(exe),
                    "-L", os.path.join(ROOT, "optimax_rogue_amd"), "-lorx",
                    "-Wl,-rpath," + os.path.join(ROOT, "optimax_rogue_amd")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orx_npc refusals: 30 of 30" in r.stdout


def test_plan_takes_the_moving_form_for_given_moves(tmp_path):
    """orx_plan.h: a call that brings the NPCs' moves is planned as
    Form::kMoving whatever cfg.npc_policy says; without them the plan is what
    it was (a host compiler builds the header alone)."""
    src = tmp_path / "plan_given.cpp"
    src.write_text('''
#include <cstdio>
#include "optimax_rogue_amd/csrc/orx_plan.h"
using namespace orx_dev;
int main() {
  orx_cfg_t c{};
  c.width = 8; c.height = 8; c.n_npcs = 6; c.npc_policy = ORX_NPC_STAY;
  const Env env{};
  const Device dev{1024, kMaxLdsBlock};
  int bad = 0;
  bad += plan_step_n(&c, 301, 1, 1, env, dev).form == Form::kMoving;
  bad += plan_step_n(&c, 301, 1, 1, env, dev, true).form != Form::kMoving;
  bad += plan_env_step(&c, 301, true, env).form == Form::kMoving;
  bad += plan_env_step(&c, 301, true, env, true).form != Form::kMoving;
  c.npc_policy = ORX_NPC_CHASE;
  bad += plan_step_n(&c, 301, 1, 1, env, dev, true).form != Form::kMoving;
  bad += plan_step_n(&c, 301, 1, 1, env, dev).form != Form::kMoving;
  c.n_npcs = 0;   // (the entry points refuse it; the plan has no NPCs to move)
  bad += plan_env_step(&c, 301, true, env, true).form == Form::kMoving;
  std::printf("bad %d\\n", bad);
  return bad;
}
''')
    exe = tmp_path / "plan_given"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(src), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
