"""Shared by tests/test_npc_given.py (CPU) and tests/test_gpu_npc_given.py: the
given-NPC-move fixtures (tests/golden/given/, made from the reference by
tests/golden/make_given.py) and the CPU restatements the GPU tests compare
larger sweeps against -- oracle/pyref.py's Game with its decide_npc_move hook
replaced by a table (GivenGame, pinned to the fixtures by test_npc_given.py)
or recorded into one (RecordingGame)."""
from __future__ import annotations

import numpy as np

from golden_util import Fixture
from oracle import pyref

GIVEN_CASES = ("given_regs_8x8", "given_dense_12x12", "given_bank_9x8", "given_stock_8x8")
KEYED_CASES = tuple(n for n in GIVEN_CASES if "stock" not in n)

BASE_CFG = dict(width=8, height=8, despawn=1, max_ticks=30, start_mode=1, p1_depth=0, p2_depth=0,
                n_npcs=6, npc_health=3, npc_damage=1, npc_armor=0, player_health=10,
                player_damage=2, player_armor=1, autoreset=1, flags=0, rng=0, npc_policy=0)


def given_fixture(name: str) -> Fixture:
    """tests/golden/given/<name>.npz; ``fx.z["npc_moves"]`` is int8 [T][K][G]."""
    return Fixture("given/" + name)


def bank(W, H, L, seed):
    """A deterministic bank of L layouts [L, W, H] (Tile codes): a Wall border,
    ~15% interior walls, one staircase; every layout keeps most of its Ground."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(L):
        t = np.ones((W, H), np.uint8)
        t[[0, -1], :] = 2
        t[:, [0, -1]] = 2
        inner = rs.rand(W, H) < 0.15
        inner[[0, -1], :] = False
        inner[:, [0, -1]] = False
        t[inner] = 2
        ground = np.argwhere(t == 1)
        t[tuple(ground[rs.randint(len(ground))])] = 3
        out.append(t)
    return np.stack(out)


def random_table(T, K, G, seed):
    return np.random.default_rng(seed).integers(1, 6, size=(T, K, G), dtype=np.int8)


def guarded(gs, e, move):
    """include/orx_npc.h's guards on ``move`` of NPC ``e``: Stay on a depth
    without a dungeon, Stay while a player of that depth stands next to a
    staircase tile, Stay instead of a move into a blocked cell."""
    if e.depth not in gs.world:
        return pyref.STAY
    d = gs.world[e.depth]
    W, H = d.tiles.shape
    for p in (gs.iden_lookup[1], gs.iden_lookup[2]):
        if p.depth != e.depth:
            continue
        for m in (pyref.UP, pyref.RIGHT, pyref.DOWN, pyref.LEFT):
            x, y = pyref.calculate_pos(p.x, p.y, m)
            if 0 <= x < W and 0 <= y < H and d.tiles[x, y] == pyref.STAIRS:
                return pyref.STAY
    if d.is_blocked(*pyref.calculate_pos(e.x, e.y, move)):
        return pyref.STAY
    return move


class GivenGame(pyref.Game):
    """pyref.Game whose decide_npc_move is the guards plus ``table[t][iden -
    3][g]`` (t: the step of the run, autoreset steps included; g: the game's
    column).  Nothing is drawn for the NPCs' moves."""

    def __init__(self, cfg, seed, gid, table, g, layouts=None):
        self.table, self.g, self.t = table, g, 0
        super().__init__(dict(cfg, npc_policy=0), seed, gid, layouts=layouts)

    def decide_npc_move(self, gs, e, ai):
        return guarded(gs, e, int(self.table[self.t, e.iden - 3, self.g]))

    def step(self, m1, m2):
        try:
            return super().step(m1, m2)
        finally:
            self.t += 1


class RecordingGame(pyref.Game):
    """pyref.Game (cfg npc_policy 1 / 2) that writes every tick's AI decisions
    into ``table[t][iden - 3][g]`` (slots without a decision keep Stay)."""

    def __init__(self, cfg, seed, gid, table, g, layouts=None):
        self.table, self.g, self.t = table, g, 0
        super().__init__(cfg, seed, gid, layouts=layouts)

    def decide_npc_move(self, gs, e, ai):
        m = super().decide_npc_move(gs, e, ai)
        self.table[self.t, e.iden - 3, self.g] = m
        return m

    def step(self, m1, m2):
        try:
            return super().step(m1, m2)
        finally:
            self.t += 1
