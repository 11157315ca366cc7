"""The configurations tests/test_view.py (CPU, oracle states) and
tests/test_gpu_view.py (engine states) check the egocentric view on, and an
independent restatement of the view for one game in the reference's schema.

Seeds and tick counts were picked on the CPU so that the ORACLE's states alone
meet every coverage condition test_view.py asserts (NPC and other-player bits,
cells outside the grid on all four sides, staircases, a dead NPC's empty last
cell, players on different depths, a bank's second staircase and interior
walls).  The engine is bit-exact with the oracle, so the GPU test sees the
same states.
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_GAMES = 200
RADII = (1, 5, 15)


def make_layouts(*args, **kw):
    """tests/golden/make_golden.make_layouts (the fixtures' bank generator;
    importing that module needs nothing of the reference)."""
    spec = importlib.util.spec_from_file_location(
        "make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.make_layouts(*args, **kw)


def cases():
    """name -> dict(cfg=EnvConfig, seed, ticks, policies=(p1, p2), radii)."""
    from optimax_rogue_amd import EnvConfig
    return {
        # a: Together, RandomBots, episodes end at 30 ticks
        "a": dict(cfg=EnvConfig(width=10, height=8, n_npcs=4, max_ticks=30), seed=11, ticks=24,
                  policies=(1, 1), radii=RADII),
        # b: Separated (NPCs on depth 1 with player 1), StaircaseBot vs RandomBot
        "b": dict(cfg=EnvConfig(width=10, height=8, n_npcs=4, start_mode=2, p1_depth=1,
                                p2_depth=0), seed=12, ticks=12, policies=(2, 1), radii=RADII),
        # c: a dungeon bank with open borders, interior walls, one or two staircases
        "c": dict(cfg=EnvConfig(width=9, height=8, n_npcs=6,
                                layouts=make_layouts(9, 8, 4, 13, n_stairs=(1, 2),
                                                     open_border=True)),
                  seed=13, ticks=20, policies=(1, 1), radii=RADII),
        # d: dense NPCs (K > 16: the occupancy-grid engine forms)
        "d": dict(cfg=EnvConfig(width=20, height=20, n_npcs=40), seed=14, ticks=30,
                  policies=(1, 1), radii=RADII),
        # e: the smallest board, no NPCs: the window is mostly outside the grid
        "e": dict(cfg=EnvConfig(width=4, height=4, n_npcs=0), seed=15, ticks=10,
                  policies=(1, 1), radii=(5,)),
    }


def bank_of(cfg):
    if cfg.layouts is None:
        return None
    from optimax_rogue_amd import DungeonBank
    return DungeonBank(cfg.layouts)


def oracle_states(case, n_games=N_GAMES):
    """(state after reset, state after case['ticks'] ticks) of the C oracle,
    both snapshot()-shaped (Oracle.export)."""
    from oracle.oracle import Oracle
    cfg = case["cfg"]
    ora = Oracle(cfg.to_dict(), n_games, case["seed"], layouts=cfg.layouts)
    ora.reset(episode=np.zeros(n_games, np.int32))
    first = ora.export()
    for _ in range(case["ticks"]):
        ora.step(ora.policy(*case["policies"]))
    return first, ora.export()


def drive_engine(eng, case):
    """The same ticks on a BatchedEngine (made with the case's cfg and seed)."""
    for _ in range(case["ticks"]):
        eng.step(eng.policy(*case["policies"]))


def expected_window(gs, player, radius):
    """(cells, health) uint8 [V, V] of ``player`` (0 / 1) of one game in the
    reference's schema (compat.GameStateView), by map.py's rule
    (optimax_rogue_cmdspec/map.py:56-84): the tiles of the viewed depth --
    here cut out around the viewer, rows y and columns x, 0 outside the grid --
    then every entity of that depth on top; the viewer itself is not drawn."""
    R, V = radius, 2 * radius + 1
    viewer = gs.iden_lookup[1 + player]
    tiles = np.asarray(gs.world.get_at_depth(viewer.depth).tiles)
    W, H = tiles.shape
    padded = np.zeros((W + 2 * R, H + 2 * R), np.int64)
    padded[R:R + W, R:R + H] = tiles
    cells = padded[viewer.x:viewer.x + V, viewer.y:viewer.y + V].T.astype(np.uint8).copy()
    health = np.zeros((V, V), np.uint8)
    for ent in gs.entities:
        if ent.depth != viewer.depth or ent.iden == viewer.iden:
            continue
        i, j = ent.x - viewer.x + R, ent.y - viewer.y + R
        if not (0 <= i < V and 0 <= j < V):
            continue
        is_player = ent.iden in (gs.player_1_iden, gs.player_2_iden)
        cells[j, i] |= 4 if is_player else 8
        if is_player or not cells[j, i] & 4:
            health[j, i] = min(max(ent.health, 0), 255)
    return cells, health
