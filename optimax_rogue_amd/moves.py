"""What each move would do, on the host: ``outcomes`` in numpy.

The reference's learned-bot interface asks ``StateActionBot.evaluate(state,
move)`` once per supported move (optimax_rogue_bots/gui/state_action_bot.py:29,
gui/main.py:149).  What a move does is the updater's rule alone: ``update()``
turns a move into a blocked cell into a Stay (optimax_rogue/logic/
updater.py:89-98) and ``handle_move`` then attacks whatever ``pos_lookup``
holds at the target, descends on a StaircaseDown, or moves (:196-216).
``BatchedEngine.moves`` / ``VecEnv.moves`` answer that on the GPU for every
move at once (``orx_moves``, include/orx_moves.h); this module is the same
contract restated from the rules for a ``snapshot()``-shaped dict -- the slow
path for saved states, and the truth the GPU tests compare against (itself
checked against the CPU oracle move by move, tests/test_moves.py).  It needs
numpy only (no torch, no built library).

All three arrays are [B, MOVES_COLS = 8]; column ``m`` belongs to Move ``m``
(1..5, and MOVE_HEAL = 6 with EXT_HEAL), every other column holds kind 0,
target -1, amount 0.

  kind    uint8: an outcome OUT_* in bits 0-2 (OUT_MASK), ORed with OUT_LETHAL,
          OUT_ITEM, OUT_COOLDOWN
  target  int16: the iden an attack hits (1 / 2 a player, 3 + k NPC slot k),
          -1 otherwise
  amount  int16: an attack's damage, a heal's points, 0 otherwise

The answer is exact when the other player Stays; against its own move a STEP
can become an attack and an attack a step (include/orx_moves.h).
"""
from __future__ import annotations

import numpy as np

from .enums import (EXT_CHARACTER, EXT_HEAL, EXT_ITEMS, EXT_MANA, EXT_README_COMBAT, MOVE_HEAL,
                    Move, RPG_FIELDS, Tile)
from .query import MOVE_DELTAS, check_player, i64, item_rows, npc_depth, npc_rows, tile_at

# include/orx_moves.h ORX_MOVES_COLS, ORX_OUT_*
MOVES_COLS = 8
OUT_MASK = 7
OUT_NONE = 0
OUT_REST = 1
OUT_BLOCKED = 2
OUT_STEP = 3
OUT_DESCEND = 4
OUT_ATTACK_NPC = 5
OUT_ATTACK_PLAYER = 6
OUT_HEAL = 7
OUT_LETHAL = 8
OUT_ITEM = 16
OUT_COOLDOWN = 32

OUT_NAMES = ("NONE", "REST", "BLOCKED", "STEP", "DESCEND", "ATTACK_NPC", "ATTACK_PLAYER", "HEAL")


def move_count(cfg) -> int:
    """M: the moves of a configuration, 5, or 6 with EXT_HEAL."""
    return MOVE_HEAL if int(cfg.flags) & EXT_HEAL else int(Move.Stay)


def check_moves_args(player: int) -> None:
    """ValueError for a player other than 0 / 1 (what orx_moves refuses with
    ORX_EINVAL)."""
    check_player(player)


def outcomes(cfg, state: dict, player: int, layouts=None):
    """``(kind, target, amount)`` of ``player`` (0 / 1) of every game of a state
    dict in the layout of ``Oracle.export()`` / ``engine.snapshot()``.
    ``layouts``: the [L, W, H] Tile codes of a configuration with a bank (or a
    DungeonBank; ``cfg.layouts`` when omitted; the state then has
    ``p_layout``)."""
    check_moves_args(player)
    K, flags = int(cfg.n_npcs), int(cfg.flags)
    if layouts is None:
        layouts = getattr(cfg, "layouts", None)
    if layouts is not None:
        layouts = np.asarray(getattr(layouts, "layouts", layouts))
    p, q = int(player), 1 - int(player)
    x, y, d, hp = (i64(state[f][p]) for f in ("p_x", "p_y", "p_depth", "p_health"))
    ox, oy, od, ohp = (i64(state[f][q]) for f in ("p_x", "p_y", "p_depth", "p_health"))
    B = len(x)
    kind = np.zeros((B, MOVES_COLS), np.uint8)
    target = np.full((B, MOVES_COLS), -1, np.int64)
    amount = np.zeros((B, MOVES_COLS), np.int64)

    # the player's own attributes (Entity.damage / armor; the character's p_rpg)
    damage = np.full(B, int(cfg.player_damage), np.int64)
    mana = max_hp = held = cooldown = np.zeros(B, np.int64)
    if flags & EXT_CHARACTER:
        rpg = {f: i64(state["p_rpg"][i][p]) for i, f in enumerate(RPG_FIELDS)}
        damage, mana, max_hp = rpg["damage"], rpg["mana"], rpg["max_health"]
        held, cooldown = rpg["items"], rpg["cooldown"]
    # mana_points: whole points from up to a third of the manabar
    pts = np.zeros(B, np.int64)
    if flags & EXT_MANA:
        pts = np.minimum(mana, int(cfg.mana_max) // 3) // max(int(cfg.mana_per_point), 1)
    attack = np.maximum(damage - int(cfg.player_armor) + pts, 0)      # updater.py:313
    on_cooldown = (cooldown > 0) if flags & EXT_README_COMBAT else np.zeros(B, bool)

    on_npc_depth = d == npc_depth(cfg)
    if K:
        alive, nx, ny, nhp = npc_rows(state, K)
    items = bool(K and flags & EXT_ITEMS and "item_mask" in state)
    if items:
        on_floor, ix, iy, _ = item_rows(state, K)

    games = np.arange(B)
    for m, dx, dy in MOVE_DELTAS:
        tx, ty = x + dx, y + dy
        inside, tile = tile_at(cfg, state, p, tx, ty, layouts)
        blocked = ~inside | (tile == int(Tile.Wall))                   # Dungeon.is_blocked
        at_player = ~blocked & (od == d) & (tx == ox) & (ty == oy)
        # the first live NPC on the target, in slot order (pos_lookup)
        slot = np.full(B, -1, np.int64)
        for k in range(K - 1, -1, -1):
            hit = on_npc_depth & alive[k] & (nx[k] == tx) & (ny[k] == ty)
            slot[hit] = k
        at_npc = ~blocked & ~at_player & (slot >= 0)
        free = ~blocked & ~at_player & ~at_npc
        descend = free & (tile == int(Tile.StaircaseDown))
        step = free & ~descend

        k_m = np.zeros(B, np.int64)
        k_m[blocked] = OUT_BLOCKED
        k_m[step] = OUT_STEP
        k_m[descend] = OUT_DESCEND
        # the other player: the readme's table measures an attack on cooldown as a Stay
        amt = np.where(on_cooldown, 0, attack)
        k_m[at_player] = OUT_ATTACK_PLAYER
        k_m[at_player & on_cooldown] |= OUT_COOLDOWN
        k_m[at_player & (ohp > 0) & (amt >= ohp)] |= OUT_LETHAL
        target[at_player, m] = 2 - p
        amount[at_player, m] = amt[at_player]
        # an NPC
        if K:
            victim = nhp[np.maximum(slot, 0), games]
            k_m[at_npc] = OUT_ATTACK_NPC
            k_m[at_npc & (victim > 0) & (attack >= victim)] |= OUT_LETHAL
            target[at_npc, m] = 3 + slot[at_npc]
            amount[at_npc, m] = attack[at_npc]
        if items:
            lies = np.zeros(B, bool)
            for k in range(K):
                lies |= on_floor[k] & (ix[k] == tx) & (iy[k] == ty)
            k_m[step & on_npc_depth & lies & (held < int(cfg.item_slots))] |= OUT_ITEM
        kind[:, m] = k_m

    kind[:, int(Move.Stay)] = OUT_REST
    if flags & EXT_HEAL:                                              # readme.md:74
        kind[:, MOVE_HEAL] = OUT_HEAL
        amount[:, MOVE_HEAL] = np.where(hp > 0, np.minimum(pts, np.maximum(max_hp - hp, 0)), 0)
    return kind, target.astype(np.int16), np.clip(amount, 0, 32767).astype(np.int16)


def action_mask(kind, n_moves: int):
    """bool [B, n_moves] from a ``kind`` array (numpy, or a torch tensor):
    column ``j`` is Move ``j + 1``, False exactly where the updater would play
    a Stay in the move's place -- OUT_BLOCKED, or the OUT_COOLDOWN flag -- so
    ``masked_logits.argmax(1) + 1`` is a valid action that is not wasted."""
    k = kind[:, 1:int(n_moves) + 1]
    return ((k & OUT_MASK) != OUT_BLOCKED) & ((k & OUT_COOLDOWN) == 0)
