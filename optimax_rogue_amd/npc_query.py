"""The enemies' queries on the host: ``options`` and ``seek`` in numpy.

``BatchedEngine.step(npc_moves=...)`` plays every NPC from a table (the
reference's hook ``Updater.decide_npc_move``, optimax_rogue/logic/
updater.py:165-178, batched: include/orx_npc.h).  A move of that table passes
the engine's guards -- Stay on a depth without a dungeon, Stay while a player
of that depth stands next to a staircase tile, Stay instead of a move into a
blocked cell -- and then ``handle_move`` (:196-216): it attacks whatever
``pos_lookup`` holds at the target, is removed on a free StaircaseDown
(:263-270), or moves.  ``BatchedEngine.npc_options`` / ``npc_seek`` answer on
the GPU, for every NPC of every game, what each move would do and how far the
players are along walkable cells (``orx_npc_options`` / ``orx_npc_seek``,
include/orx_npc_query.h); this module is the same contract restated for a
``snapshot()``-shaped dict, and the truth the GPU tests compare against
(itself checked against the guards and the CPU restatement of the tick move by
move, tests/test_npc_query.py).  It needs numpy only (no torch, no built
library).

Every row is slot-major: ``[K, B, ...]``, row ``k`` NPC slot ``k`` (iden 3 +
``k``).  The freeze rule is the engine's, not the reference's (orx_npc.h).
"""
from __future__ import annotations

import numpy as np

from .enums import (DungeonDespawningStrategy, Move, NPC_DEPTH_GONE, NPC_DEPTH_UNWATCHED,
                    NPC_DEPTH_WATCHED, NPC_OUT_ATTACK_NPC, NPC_OUT_ATTACK_PLAYER, NPC_OUT_BLOCKED,
                    NPC_OUT_FROZEN, NPC_OUT_LETHAL, NPC_OUT_MASK, NPC_OUT_NONE, NPC_OUT_REST,
                    NPC_OUT_STAIRS, NPC_OUT_STEP, NPC_SEEK_NEAREST, Tile)
from .moves import MOVES_COLS
from .path import PATH_UNREACHABLE, PATH_WALL, Walk, fill_column, seek_columns
from .query import MOVE_DELTAS, bank_of, i64, inside_grid, npc_depth, npc_rows, tile_at


def _check(cfg) -> int:
    K = int(cfg.n_npcs)
    if K <= 0:
        raise ValueError("the NPC queries need a configuration with NPCs (n_npcs > 0)")
    return K


def _layouts(cfg, bank):
    """``(bank, layouts)``: the DungeonBank of a configuration with one (made
    from ``cfg.layouts`` when omitted) and its [L, W, H] Tile codes."""
    bank = bank_of(cfg, bank)
    return bank, None if bank is None else np.asarray(bank.layouts)


def depth_state(snap: dict, cfg) -> np.ndarray:
    """uint8 [B]: NPC_DEPTH_WATCHED where a player's depth is the NPCs' depth
    nd, NPC_DEPTH_UNWATCHED where none is but the dungeon of nd still exists
    (Unreachable despawning with player 2 above nd), else NPC_DEPTH_GONE."""
    nd = npc_depth(cfg)
    d1, d2 = i64(snap["p_depth"][0]), i64(snap["p_depth"][1])
    watched = (d1 == nd) | (d2 == nd)
    kept = (int(cfg.despawn) == int(DungeonDespawningStrategy.Unreachable)) & (d2 < nd)
    return np.where(watched, NPC_DEPTH_WATCHED,
                    np.where(kept, NPC_DEPTH_UNWATCHED, NPC_DEPTH_GONE)).astype(np.uint8)


def _depth_dungeon(snap: dict, cfg, layouts):
    """The dungeon of the NPCs' depth as a one-row snapshot for ``tile_at``:
    player 1's staircase and layout where it stands on nd, else player 2's."""
    on1 = i64(snap["p_depth"][0]) == npc_depth(cfg)
    pick = lambda f: np.where(on1, i64(snap[f][0]), i64(snap[f][1]))[None]
    dung = {}
    if layouts is None:
        dung["st_x"], dung["st_y"] = pick("st_x"), pick("st_y")
    else:
        dung["p_layout"] = pick("p_layout")
    return dung


def options(snap: dict, cfg, bank=None):
    """``(kind, target, amount, where)`` of every NPC of every game of a
    ``snapshot()``-shaped dict: uint8, int16 and int16 [K, B, MOVES_COLS = 8],
    column ``m`` for Move ``m`` (columns 0, 6 and 7 hold 0 / -1 / 0), and
    ``where = depth_state(snap, cfg)``.

    kind    NPC_OUT_*: REST for Stay; for the other moves of a live slot NONE
            on an UNWATCHED depth, FROZEN where the engine plays Stay whatever
            the byte (the depth is GONE, or a player on it stands next to a
            staircase tile), else BLOCKED, ATTACK_PLAYER, ATTACK_NPC, STAIRS
            or STEP, the attacks ORed with NPC_OUT_LETHAL; all 0 for a dead slot
    target  the iden an attack hits (1 / 2 a player, 3 + j NPC slot j), else -1
    amount  an attack's ``max(npc_damage - npc_armor, 0)``, else 0"""
    K = _check(cfg)
    bank, layouts = _layouts(cfg, bank)
    nd = npc_depth(cfg)
    where = depth_state(snap, cfg)
    B = len(where)
    dung = _depth_dungeon(snap, cfg, layouts)
    px, py, pd, php = (i64(snap[f]) for f in ("p_x", "p_y", "p_depth", "p_health"))
    on = pd == nd                                                    # [2, B]
    alive, nx, ny, nhp = (a.T for a in npc_rows(snap, K))            # [B, K]

    def stairs_next_to(p):   # the engine's next_to_stairs for player row p
        if layouts is None:
            return np.abs(px[p] - dung["st_x"][0]) + np.abs(py[p] - dung["st_y"][0]) == 1
        near = np.zeros(B, bool)
        for _, dx, dy in MOVE_DELTAS:
            inside, tile = tile_at(cfg, dung, 0, px[p] + dx, py[p] + dy, layouts)
            near |= inside & (tile == int(Tile.StaircaseDown))
        return near
    watched = where == NPC_DEPTH_WATCHED
    frozen = (where == NPC_DEPTH_GONE) | \
        (watched & ((on[0] & stairs_next_to(0)) | (on[1] & stairs_next_to(1))))
    answers = alive & (watched & ~frozen)[:, None]                   # [B, K]

    attack = min(max(int(cfg.npc_damage) - int(cfg.npc_armor), 0), 32767)   # updater.py:313
    kind = np.zeros((B, K, MOVES_COLS), np.int64)
    target = np.full((B, K, MOVES_COLS), -1, np.int64)
    amount = np.zeros((B, K, MOVES_COLS), np.int64)
    games = np.arange(B)[:, None]
    for m, dx, dy in MOVE_DELTAS:
        tx, ty = nx + dx, ny + dy
        inside, tile = tile_at(cfg, dung, 0, tx, ty, layouts)
        blocked = ~inside | (tile == int(Tile.Wall))                 # Dungeon.is_blocked
        at = [on[p][:, None] & (tx == px[p][:, None]) & (ty == py[p][:, None]) for p in (0, 1)]
        at[1] &= ~at[0]
        # the first live NPC on the target, in slot order (pos_lookup)
        slot = np.full((B, K), -1, np.int64)
        for j in range(K - 1, -1, -1):
            hit = alive[:, j:j + 1] & (nx[:, j:j + 1] == tx) & (ny[:, j:j + 1] == ty)
            slot[hit] = j
        at_player = ~blocked & (at[0] | at[1])
        at_npc = ~blocked & ~at_player & (slot >= 0)
        free = ~blocked & ~at_player & ~at_npc
        victim = np.where(at[0], php[0][:, None], np.where(
            at[1], php[1][:, None], nhp[games, np.maximum(slot, 0)]))
        lethal = (at_player | at_npc) & (victim > 0) & (attack >= victim)
        k_m = np.where(blocked, NPC_OUT_BLOCKED, np.where(
            at_player, NPC_OUT_ATTACK_PLAYER, np.where(at_npc, NPC_OUT_ATTACK_NPC, np.where(
                free & (tile == int(Tile.StaircaseDown)), NPC_OUT_STAIRS, NPC_OUT_STEP))))
        k_m = k_m | np.where(lethal, NPC_OUT_LETHAL, 0)
        k_m = np.where(answers, k_m, np.where(alive & frozen[:, None], NPC_OUT_FROZEN,
                                              NPC_OUT_NONE))
        hits = answers & (at_player | at_npc)
        kind[:, :, m] = k_m
        target[:, :, m] = np.where(hits, np.where(at[0], 1, np.where(at[1], 2, 3 + slot)), -1)
        amount[:, :, m] = np.where(hits, attack, 0)
    kind[:, :, int(Move.Stay)] = np.where(alive, NPC_OUT_REST, NPC_OUT_NONE)
    t = lambda a, dt: np.ascontiguousarray(a.transpose(1, 0, 2).astype(dt))
    return t(kind, np.uint8), t(target, np.int16), t(amount, np.int16), where


def action_mask(kind, where):
    """bool [K, B, 5] from ``options``' kind and where (numpy, or torch
    tensors): column ``j`` is Move ``j + 1``, True where the engine would play
    the byte as given -- not NPC_OUT_FROZEN, not NPC_OUT_BLOCKED.  Stay is
    always True; a dead slot has only Stay True (a masked softmax is never
    empty); the live slots of an UNWATCHED game, about which there is no
    answer, are all True."""
    k = kind[:, :, 1:int(Move.Stay) + 1] & NPC_OUT_MASK
    live = k[:, :, int(Move.Stay) - 1:] == NPC_OUT_REST   # (a dead slot's row is all 0)
    unwatched = (where == NPC_DEPTH_UNWATCHED)[None, :, None]
    plays = (k != NPC_OUT_FROZEN) & (k != NPC_OUT_BLOCKED) & (k != NPC_OUT_NONE)
    mask = live & (plays | unwatched)
    mask[:, :, int(Move.Stay) - 1] = True
    return mask


def seek(snap: dict, cfg, bank=None):
    """``(dist, move, target)``, int32, int8 and int16 [K, B, SEEK_COLS = 4], of
    every NPC of every game of a ``snapshot()``-shaped dict: column
    NPC_SEEK_P1 player 1, NPC_SEEK_P2 player 2 (a target when it is on the
    NPCs' depth, whatever its health), NPC_SEEK_NEAREST the nearer of the two
    (less distance wins, reachable beats unreachable, player 1 wins a tie);
    column 3 pads.  Dead slots, and games whose depth is not WATCHED, have no
    target.

    dist    ``path.seek``'s walking distance from the NPC's cell on the
            dungeon of the NPCs' depth (``bank.pair_field()``, else
            ``room_distance``); SEEK_UNREACHABLE, SEEK_ABSENT
    move    the first of Up, Right, Down, Left whose neighbour cell is at
            ``dist - 1`` from the target -- a staircase neighbour only if it
            is the target's own cell; Stay when ``dist <= 0``
    target  the player's iden, 1 or 2; -1 when absent"""
    K = _check(cfg)
    bank, layouts = _layouts(cfg, bank)
    nd = npc_depth(cfg)
    watched = depth_state(snap, cfg) == NPC_DEPTH_WATCHED
    walk = Walk(cfg, _depth_dungeon(snap, cfg, layouts), 0, bank)
    px, py, pd = (i64(snap[f]) for f in ("p_x", "p_y", "p_depth"))
    alive, nx, ny, _ = (a.T for a in npc_rows(snap, K))               # [B, K]
    here = alive & watched[:, None] & inside_grid(cfg, nx, ny)
    has, own, move = [], [], []
    for p in (0, 1):
        tx, ty = px[p][:, None], py[p][:, None]
        has.append(here & (pd[p] == nd)[:, None])
        own.append(np.minimum(walk.between(nx, ny, tx, ty), PATH_UNREACHABLE))
        move.append(walk.first_move(nx, ny, tx, ty, own[p]))
    # absent above unreachable above every distance; player 1 wins a tie
    nearer = np.where(has[1], own[1], PATH_WALL) < np.where(has[0], own[0], PATH_WALL)
    out = seek_columns(nx.shape, np.int16)
    for col in range(NPC_SEEK_NEAREST + 1):
        p = np.full(nx.shape, col) if col < NPC_SEEK_NEAREST else nearer.astype(np.int64)
        pick = lambda pair: np.where(p == 0, pair[0], pair[1])
        fill_column(out, col, pick(has), pick(own), pick(move), p + 1)
    return tuple(np.ascontiguousarray(a.transpose(1, 0, 2)) for a in out)


def hunt_moves(kind, move, target=None) -> np.ndarray:
    """int8 [K, B], ready to pass as ``npc_moves``: the move of ``seek``'s
    column NPC_SEEK_NEAREST where ``options`` calls that move STEP or
    ATTACK_PLAYER, else Stay -- so the pursuit never walks onto a staircase
    and never hits a fellow NPC.  (``target``, ``seek``'s third array, is not
    needed: a slot without prey has the move Stay.)"""
    m = np.asarray(move)[:, :, NPC_SEEK_NEAREST].astype(np.int64)
    k = np.take_along_axis(np.asarray(kind).astype(np.int64), m[:, :, None], axis=2)[:, :, 0]
    k &= NPC_OUT_MASK
    ok = (k == NPC_OUT_STEP) | (k == NPC_OUT_ATTACK_PLAYER)
    return np.where(ok, m, int(Move.Stay)).astype(np.int8)
