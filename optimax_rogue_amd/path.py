"""The staircase distance field on the host: ``stair_field`` and ``query`` in
numpy.

The reference's StaircaseBot "rushes as quickly as possible to the staircase"
(optimax_rogue_bots/staircasebot.py:1-21) by stepping along the larger delta;
the updater turns a step into a Wall into Stay (updater.py:89-98), so on a
layout with interior walls it stops at the first one in its way.  What a
walking entity has to cover is the breadth-first distance over tiles that
``is_blocked`` lets through (world.py:41-46: in the grid and not Wall) with
``calculate_pos``'s four moves (updater.py:340-351), to the nearest
StaircaseDown -- any of them descends (updater.py:205-206).

``BatchedEngine.path`` / ``VecEnv.path`` answer that on the GPU
(``orx_path_field`` / ``orx_path_query``, include/orx_path.h); this module is
the same contract restated for layouts and a ``snapshot()``-shaped dict, and
the truth the GPU tests compare against.  It needs numpy only (no torch, no
built library).

One cell of a field (uint16): 0 on a StaircaseDown, else the number of moves
to the nearest one, ``PATH_WALL`` on a Wall tile or outside the grid,
``PATH_UNREACHABLE`` on a tile that is not Wall but has no walkable path.

``source_rows`` / ``pair_field`` and ``seek`` are the same for targets that
move (``orx_path_rows`` / ``orx_path_seek``): the walking distance between two
cells, and from a player to the other player, the nearest NPC and the nearest
item.  The updater descends an entity that steps onto a free StaircaseDown
(updater.py:205-206), so a walk that stays on its depth may start or end on a
staircase but not cross one: the interior cells of a path are all Ground.

``threat`` (``orx_path_threat``) turns ``seek`` round: the least of those
distances from what hunts a player -- the other player, the live NPCs -- to its
own cell, to each move's cell and to every cell of a window, and the move after
which it is largest (``flee_moves``).

``ticks`` (``orx_path_ticks``) is ``query`` with the enemies in the way: a step
onto a live NPC's cell is an attack that leaves the mover where it is
(updater.py:218-227), so entering a held cell costs one tick per blow and one
for the step -- a shortest path with small integer entry costs, per game.
"""
from __future__ import annotations

import numpy as np

from .enums import EXT_CHARACTER, RPG_FIELDS, Move, Tile
from .query import (MOVE_DELTAS, bank_at, bank_of, check_player, check_radius, i64, inside_grid,
                    item_rows, npc_depth, npc_rows, per_game, tile_at, window_cells)

# include/orx_path.h ORX_PATH_* and ORX_SEEK_*
PATH_WALL = 0xFFFF
PATH_UNREACHABLE = 0xFFFE
SEEK_PLAYER, SEEK_NPC, SEEK_ITEM, SEEK_COLS = 0, 1, 2, 4
SEEK_UNREACHABLE = -1
SEEK_ABSENT = -2
# include/orx_path.h ORX_THREAT_*
THREAT_PLAYER, THREAT_NPC, THREAT_ANY = 0, 1, 2
THREAT_AFTER_COLS = 8


def check_path_args(player: int, radius=None, cfg=None) -> None:
    """ValueError for a player other than 0 / 1, a radius (when one is given)
    outside 1..VIEW_MAX_RADIUS, or an EmptyDungeonGenerator grid whose largest
    distance (W - 3) + (H - 3) would reach the sentinels (what orx_path_query
    refuses with ORX_EINVAL)."""
    check_player(player)
    if radius is not None:
        check_radius(radius)
    if cfg is not None and getattr(cfg, "layouts", None) is None \
            and int(cfg.width) + int(cfg.height) - 6 >= PATH_UNREACHABLE:
        raise ValueError("width + height too large for uint16 distances")


def stair_field(layouts) -> np.ndarray:
    """uint16 [L, W, H]: the field of every layout of ``layouts`` ([L, W, H] or
    [W, H] Tile codes).  A frontier breadth-first search over all layouts at
    once: each level touches only the cells it reaches, so the cost follows
    the cells (plus a few numpy calls per level), not levels x cells."""
    a = np.asarray(layouts)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("layouts must be [L, W, H] Tile codes")
    L, W, H = a.shape
    # one Wall ring around every layout: a step off the grid lands on it
    pad = np.full((L, W + 2, H + 2), int(Tile.Wall), np.uint8)
    pad[:, 1:-1, 1:-1] = a
    flat = pad.reshape(-1)
    dist = np.full(flat.shape, -1, np.int64)          # -1: not reached
    steps = np.array([-1, 1, -(H + 2), H + 2], np.int64)
    frontier = np.flatnonzero(flat == int(Tile.StaircaseDown))
    open_ = flat != int(Tile.Wall)
    dist[frontier] = 0
    d = 0
    while len(frontier):
        d += 1
        nxt = (frontier[:, None] + steps[None, :]).reshape(-1)
        nxt = nxt[open_[nxt] & (dist[nxt] < 0)]
        frontier = np.unique(nxt)
        dist[frontier] = d
    if d > PATH_UNREACHABLE:   # (cannot happen with at most 65,536 tiles)
        raise ValueError("a distance reaches the sentinels")
    out = np.where(open_, np.where(dist < 0, PATH_UNREACHABLE, dist), PATH_WALL)
    return np.ascontiguousarray(out.reshape(L, W + 2, H + 2)[:, 1:-1, 1:-1].astype(np.uint16))


def closed_form(cfg, sx, sy) -> np.ndarray:
    """uint16 [..., W, H]: the field of EmptyDungeonGenerator's dungeon
    (worldgen.py:33-43: the border is Wall, the interior open) with its
    staircase at (sx, sy) -- scalars, or arrays of one shape: PATH_WALL on the
    border, |x - sx| + |y - sy| inside.  Exact because the interior has no
    walls: the Manhattan distance is a lower bound and an L-shaped walk
    inside the interior attains it."""
    W, H = int(cfg.width), int(cfg.height)
    sx, sy = np.asarray(sx, np.int64), np.asarray(sy, np.int64)
    x = np.arange(W, dtype=np.int64)[:, None]
    y = np.arange(H, dtype=np.int64)[None, :]
    d = np.abs(x - sx[..., None, None]) + np.abs(y - sy[..., None, None])
    border = (x == 0) | (x == W - 1) | (y == 0) | (y == H - 1)
    return np.where(border, PATH_WALL, d).astype(np.uint16)


def move_toward(own, up, right, down, left) -> np.ndarray:
    """int8: the first of Up, Right, Down, Left whose target value is ``own`` -
    1; Stay where ``own`` is 0 or a sentinel (arrays of one shape)."""
    own = np.asarray(own, np.int64)
    want = own - 1
    move = np.full(own.shape, int(Move.Stay), np.int8)
    for (code, _, _), val in reversed(list(zip(MOVE_DELTAS, (up, right, down, left)))):
        move = np.where(np.asarray(val, np.int64) == want, code, move)
    return np.where((own == 0) | (own >= PATH_UNREACHABLE), int(Move.Stay), move).astype(np.int8)


def query(snap: dict, cfg, player: int, radius=None, bank=None):
    """``(dist, move)`` of ``player`` (0 / 1) of every game of a
    ``snapshot()``-shaped dict, and with a ``radius`` ``(dist, move, window)``.

    dist    int32 [B]: the value of the player's own cell, -1 where it is
            PATH_UNREACHABLE
    move    int8 [B]: the Move that gets one step closer (``move_toward``)
    window  uint16 [B, V, V], V = 2 * radius + 1: ``window[b, j, i]`` is the
            value of grid cell (px + i - radius, py + j - radius), PATH_WALL
            outside the grid (``render_view``'s geometry)

    The value of a cell is ``bank.stair_field()[p_layout[player]][x, y]`` with
    a bank (made from ``cfg.layouts`` when omitted), else ``closed_form`` with
    the staircase (st_x, st_y)[player] of the player's depth."""
    check_path_args(player, radius, cfg)
    bank = bank_of(cfg, bank)
    p = int(player)
    px, py = i64(snap["p_x"][p]), i64(snap["p_y"][p])
    if bank is None:
        sx, sy = i64(snap["st_x"][p]), i64(snap["st_y"][p])
    else:
        field = bank.stair_field()

    def value(x, y):
        """The values of cells (x, y), arrays of shape [B, ...]."""
        if bank is None:
            g = (slice(None),) + (None,) * (x.ndim - 1)
            inside, tile = tile_at(cfg, snap, p, x, y)
            v = np.where(tile == int(Tile.Wall), PATH_WALL, np.abs(x - sx[g]) + np.abs(y - sy[g]))
        else:
            inside, v = inside_grid(cfg, x, y), bank_at(field, snap, p, x, y).astype(np.int64)
        return np.where(inside, v, PATH_WALL)

    own = value(px, py)
    dist = np.where(own == PATH_UNREACHABLE, -1, own).astype(np.int32)
    move = move_toward(own, *(value(px + dx, py + dy) for _, dx, dy in MOVE_DELTAS))
    if radius is None:
        return dist, move
    return dist, move, value(*window_cells(px, py, int(radius))).astype(np.uint16)


def source_rows(layouts, layout, cell) -> np.ndarray:
    """uint16 [n, W * H]: row ``i`` is the walking distance from flat cell
    ``cell[i]`` (= x * H + y) of layout ``layout[i]`` of ``layouts`` ([L, W, H]
    or [W, H] Tile codes) to every tile of that layout: PATH_WALL on Wall
    tiles, PATH_UNREACHABLE where there is no walk, else the moves of the
    shortest path whose interior cells are all Ground (its end cells may be
    staircases).  A source on a Wall, or an index outside the bank, seeds
    nothing (its row shows the Walls of the layout index clamped into the
    bank).  A frontier breadth-first search over all rows at once on "Ground
    plus the source"; the other staircases then take 1 + the least of their
    reached neighbours."""
    a = np.asarray(layouts)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("layouts must be [L, W, H] Tile codes")
    L, W, H = a.shape
    lay, cell = i64(layout).reshape(-1), i64(cell).reshape(-1)
    if lay.shape != cell.shape:
        raise ValueError("layout and cell must have one length")
    n, P = len(lay), (W + 2) * (H + 2)
    pad = np.full((L, W + 2, H + 2), int(Tile.Wall), np.uint8)
    pad[:, 1:-1, 1:-1] = a
    tiles = pad[np.clip(lay, 0, L - 1)].reshape(-1)          # [n * P]: every row's own copy
    wall, stair = tiles == int(Tile.Wall), tiles == int(Tile.StaircaseDown)
    ground = ~wall & ~stair
    dist = np.full(n * P, -1, np.int32)                       # -1: not reached
    ok = (lay >= 0) & (lay < L) & (cell >= 0) & (cell < W * H)
    c = np.where(ok, cell, 0)
    frontier = np.arange(n) * P + (c // H + 1) * (H + 2) + c % H + 1
    frontier = frontier[ok & ~wall[frontier]]
    dist[frontier] = 0
    steps = np.array([-1, 1, -(H + 2), H + 2], np.int64)
    d = 0
    while len(frontier):
        d += 1
        nxt = (frontier[:, None] + steps[None, :]).reshape(-1)
        nxt = nxt[ground[nxt] & (dist[nxt] < 0)]
        frontier = np.unique(nxt)
        dist[frontier] = d
    # a staircase that is not the source: one move from its nearest reached neighbour
    plane = dist.reshape(n, W + 2, H + 2)
    far = np.int32(PATH_UNREACHABLE)
    seen = np.where(plane < 0, far, plane)
    near = np.full_like(plane, far)
    near[:, 1:-1, 1:-1] = np.minimum(np.minimum(seen[:, :-2, 1:-1], seen[:, 2:, 1:-1]),
                                     np.minimum(seen[:, 1:-1, :-2], seen[:, 1:-1, 2:]))
    end = stair.reshape(plane.shape) & (plane < 0) & (near < far)
    out = np.where(wall.reshape(plane.shape), PATH_WALL, np.where(end, near + 1, seen))
    return np.ascontiguousarray(out[:, 1:-1, 1:-1].reshape(n, W * H).astype(np.uint16))


def pair_field(layouts) -> np.ndarray:
    """uint16 [L, W * H, W * H]: ``pairs[l, s, c]`` is the walking distance
    between flat cells ``s`` and ``c`` of layout ``l`` -- ``source_rows`` over
    every source of every layout, symmetric in ``s`` and ``c``."""
    a = np.asarray(layouts)
    if a.ndim == 2:
        a = a[None]
    L, W, H = a.shape
    cells = np.arange(W * H)
    return np.stack([source_rows(a, np.full(W * H, l), cells) for l in range(L)])


def room_distance(cfg, sx, sy, ax, ay, bx, by) -> np.ndarray:
    """int64: the walking distance between cells (ax, ay) and (bx, by) of
    EmptyDungeonGenerator's dungeon with its staircase at (sx, sy) (arrays
    that broadcast): |dx| + |dy|, plus 2 when the two cells share a row or
    column and the staircase lies strictly between them; PATH_WALL when either
    cell is on the border or outside the grid.  Exact, because the interior is
    at least two cells wide each way: a bent walk has two L-shaped routes and
    the staircase can lie inside one of them only."""
    W, H = int(cfg.width), int(cfg.height)
    sx, sy, ax, ay, bx, by = np.broadcast_arrays(*(i64(v) for v in (sx, sy, ax, ay, bx, by)))
    inner = lambda x, y: (x >= 1) & (x <= W - 2) & (y >= 1) & (y <= H - 2)
    between = lambda s, a, b: ((a < s) & (s < b)) | ((b < s) & (s < a))
    detour = ((ax == bx) & (sx == ax) & between(sy, ay, by)) \
        | ((ay == by) & (sy == ay) & between(sx, ax, bx))
    d = np.abs(ax - bx) + np.abs(ay - by) + 2 * detour
    return np.where(inner(ax, ay) & inner(bx, by), d, PATH_WALL)


# -- what the seek-shaped queries share (the host twin of csrc/orx_seek.h) -----
class Walk:
    """The dungeon that row ``p`` of a ``snapshot()``-shaped dict walks on: the
    layout ``p_layout[p]`` (clamped into the bank) of ``bank``, else
    EmptyDungeonGenerator's room with its staircase at (st_x, st_y)[p].  Cells
    are int64 arrays [B, ...] that broadcast, the games on the first axis."""

    def __init__(self, cfg, snap: dict, p: int, bank=None):
        self.cfg, self.snap, self.p, self.bank = cfg, snap, p, bank
        if bank is not None:
            self.pairs = bank.pair_field()
            self.lay = np.clip(i64(snap["p_layout"][p]), 0, len(self.pairs) - 1)

    def between(self, x, y, tx, ty):
        """The walking distance between cells (x, y) and (tx, ty): the pair
        table, else ``room_distance``; PATH_WALL where either is off the grid."""
        W, H = int(self.cfg.width), int(self.cfg.height)
        x, y, tx, ty = np.broadcast_arrays(x, y, tx, ty)
        if self.bank is None:
            sx, sy = (per_game(i64(self.snap[f][self.p]), x) for f in ("st_x", "st_y"))
            v = room_distance(self.cfg, sx, sy, x, y, tx, ty)
        else:
            flat = lambda u, v: np.clip(u, 0, W - 1) * H + np.clip(v, 0, H - 1)
            v = self.pairs[per_game(self.lay, x), flat(tx, ty), flat(x, y)].astype(np.int64)
        return np.where(inside_grid(self.cfg, x, y) & inside_grid(self.cfg, tx, ty), v, PATH_WALL)

    def is_stair(self, x, y):
        inside, tile = tile_at(self.cfg, self.snap, self.p, x, y,
                               None if self.bank is None else self.bank.layouts)
        return inside & (tile == int(Tile.StaircaseDown))

    def first_move(self, x, y, tx, ty, own):
        """int8: from cells (x, y) at distance ``own`` from their targets (tx,
        ty), the first of Up, Right, Down, Left whose neighbour cell is at
        ``own - 1`` -- a staircase neighbour only if it is the target's own
        cell (``move_toward``)."""
        near = []
        for _, dx, dy in MOVE_DELTAS:
            nx, ny = x + dx, y + dy
            near.append(np.where(self.is_stair(nx, ny) & ~((nx == tx) & (ny == ty)), PATH_WALL,
                                 self.between(nx, ny, tx, ty)))
        return move_toward(own, *near)


def seek_columns(shape, target_dtype):
    """``(dist, move, target)`` [*shape, SEEK_COLS] with every column absent."""
    shape = tuple(shape) + (SEEK_COLS,)
    return (np.full(shape, SEEK_ABSENT, np.int32), np.full(shape, int(Move.Stay), np.int8),
            np.full(shape, -1, target_dtype))


def fill_column(out, col: int, has, own, move, chosen) -> None:
    """Column ``col`` of ``out = (dist, move, target)``: where the column ``has``
    a target, its distance ``own`` (SEEK_UNREACHABLE from PATH_UNREACHABLE up),
    ``move`` and the ``chosen`` slot or cell; elsewhere SEEK_ABSENT, Stay, -1."""
    dist, mv, target = out
    dist[..., col] = np.where(has, np.where(own >= PATH_UNREACHABLE, SEEK_UNREACHABLE, own),
                              SEEK_ABSENT)
    mv[..., col] = np.where(has, move, int(Move.Stay))
    target[..., col] = np.where(has, chosen, -1)


def seek(snap: dict, cfg, player: int, bank=None):
    """``(dist, move, target)``, int32, int8 and int16 [B, SEEK_COLS], of
    ``player`` (0 / 1) of every game of a ``snapshot()``-shaped dict: column
    SEEK_PLAYER the other player (a target when it is on the viewer's depth),
    SEEK_NPC the NPCs whose alive bit is set and SEEK_ITEM the items on the
    floor (both only when the viewer is on the NPCs' depth); column 3 pads.

    dist    the least walking distance over the column's targets --
            ``bank.pair_field()`` on the viewer's layout with a bank (made
            from ``cfg.layouts`` when omitted), else ``room_distance``;
            SEEK_UNREACHABLE when none can be reached, SEEK_ABSENT without a
            target
    target  the lowest slot attaining it (NPC slot, item slot, ``1 - player``
            for the other player); -1 when absent
    move    the first of Up, Right, Down, Left whose neighbour cell is at
            ``dist - 1`` from that target -- a staircase neighbour only if it
            is the target's own cell; Stay when ``dist <= 0``"""
    check_player(player)
    p, q = int(player), 1 - int(player)
    K = int(cfg.n_npcs)
    walk = Walk(cfg, snap, p, bank_of(cfg, bank))
    px, py = i64(snap["p_x"][p]), i64(snap["p_y"][p])
    B = len(px)
    depth = i64(snap["p_depth"][p])
    here = inside_grid(cfg, px, py)
    on_npc_depth = here & (depth == npc_depth(cfg))
    columns = [((here & (i64(snap["p_depth"][q]) == depth))[None],
                i64(snap["p_x"][q])[None], i64(snap["p_y"][q])[None], np.array([q]))]
    if K > 0:
        alive, nx, ny, _ = npc_rows(snap, K)
        columns.append((alive & on_npc_depth, nx, ny, np.arange(K)))
        if snap.get("item_mask") is not None:
            on, ix, iy, _ = item_rows(snap, K)
            columns.append((on & on_npc_depth, ix, iy, np.arange(K)))
    out = seek_columns((B,), np.int16)
    games = np.arange(B)
    for col, (present, tx, ty, slots) in enumerate(columns):
        # absent above unreachable above every distance: argmin takes the lowest slot
        present, tx, ty = present.T, tx.T, ty.T                      # [B, slots]
        v = np.minimum(walk.between(px[:, None], py[:, None], tx, ty), PATH_UNREACHABLE)
        v = np.where(present, v, PATH_WALL)
        best = v.argmin(axis=1)
        own, bx, by = v[games, best], tx[games, best], ty[games, best]
        fill_column(out, col, own != PATH_WALL, own, walk.first_move(px, py, bx, by, own),
                    slots[best])
    return out


# -- the danger field (orx_path_threat) ----------------------------------------
def _least(walk: Walk, x, y, present, tx, ty):
    """int64, the shape of cells (x, y) [B, ...]: the least walking distance to
    the threats ``present`` [T, B] at (tx, ty) [T, B], PATH_UNREACHABLE where
    none reaches the cell (or there is none).  A Wall or off-grid cell is the
    caller's to mark."""
    out = np.full(np.broadcast(x, y).shape, PATH_UNREACHABLE, np.int64)
    for k in np.flatnonzero(present.any(axis=1)):
        v = np.minimum(walk.between(x, y, per_game(tx[k], x), per_game(ty[k], x)), PATH_UNREACHABLE)
        out = np.where(per_game(present[k], x), np.minimum(out, v), out)
    return out


def threat(snap: dict, cfg, player: int, radius=None, bank=None):
    """``(dist, move, target, after, window)`` of ``player`` (0 / 1) of every
    game of a ``snapshot()``-shaped dict: the danger field, the flip side of
    ``seek``.  A threat is the other player (on the viewer's depth) and every
    NPC whose alive bit is set (when the viewer is on the NPCs' depth): the
    targets of ``seek``'s SEEK_PLAYER and SEEK_NPC columns.  The value of a
    cell for a column is the least walking distance (``seek``'s) from a threat
    of the column to it, in the field's format: PATH_WALL on a Wall or outside
    the grid, PATH_UNREACHABLE where no threat can walk to it.

    dist    int32 [B, SEEK_COLS], columns THREAT_PLAYER, THREAT_NPC, THREAT_ANY
            (the union) and one of padding: the value of the own cell,
            SEEK_UNREACHABLE from PATH_UNREACHABLE up, SEEK_ABSENT without a
            threat
    move    int8 [B, SEEK_COLS]: the greedy flee move -- of Stay, then Up,
            Right, Down, Left where the neighbour cell is Ground (not a Wall,
            not a staircase), the first with the largest value, so a move is
            taken only when it strictly gains; Stay when absent
    target  int16 [B, SEEK_COLS]: the nearest threat -- ``1 - player``, the
            lowest NPC slot attaining ``dist``, and for THREAT_ANY an iden (1 /
            2 a player, 3 + slot an NPC; the player on a tie); -1 when absent
    after   int32 [B, THREAT_AFTER_COLS]: column ``m`` is Move ``m``'s value for
            THREAT_ANY in ``dist``'s convention (column Stay is ``dist[:,
            THREAT_ANY]``), SEEK_ABSENT where the move is no candidate or there
            is no threat
    window  with a ``radius``, uint16 [B, V, V]: THREAT_ANY's value of every
            cell in ``render_view``'s geometry; else None"""
    check_player(player)
    if radius is not None:
        check_radius(radius)
    p, q = int(player), 1 - int(player)
    K = int(cfg.n_npcs)
    bank = bank_of(cfg, bank)
    walk = Walk(cfg, snap, p, bank)
    layouts = None if bank is None else bank.layouts
    px, py = i64(snap["p_x"][p]), i64(snap["p_y"][p])
    B = len(px)
    depth = i64(snap["p_depth"][p])
    here = inside_grid(cfg, px, py)
    # the threats, [T, B]: the other player, then the NPC slots
    present = [(here & (i64(snap["p_depth"][q]) == depth))[None]]
    tx, ty = [i64(snap["p_x"][q])[None]], [i64(snap["p_y"][q])[None]]
    if K > 0:
        alive, nx, ny, _ = npc_rows(snap, K)
        present.append(alive & (here & (depth == npc_depth(cfg))))
        tx.append(nx)
        ty.append(ny)
    present, tx, ty = (np.concatenate(a) for a in (present, tx, ty))
    columns = {THREAT_PLAYER: slice(0, 1), THREAT_NPC: slice(1, 1 + K)}

    # the five cells a move chooses among: the own cell, then Up, Right, Down, Left
    cx = np.stack([px] + [px + dx for _, dx, _ in MOVE_DELTAS], axis=1)          # [B, 5]
    cy = np.stack([py] + [py + dy for _, _, dy in MOVE_DELTAS], axis=1)
    inside, tile = tile_at(cfg, snap, p, cx, cy, layouts)
    cand = inside & (tile == int(Tile.Ground))
    cand[:, 0] = True

    out = seek_columns((B,), np.int16)
    vals, has, slot = {}, {}, {}
    for col, sl in columns.items():
        pr = present[sl]
        vals[col] = _least(walk, cx, cy, pr, tx[sl], ty[sl])
        has[col] = pr.any(axis=0)
        # the lowest slot attaining the own cell's value (absent above unreachable)
        own = np.minimum(walk.between(px[:, None], py[:, None], tx[sl].T, ty[sl].T),
                         PATH_UNREACHABLE)
        slot[col] = np.where(pr.T, own, PATH_WALL).argmin(axis=1) if pr.shape[0] else np.zeros(B, int)
    P, N, A = THREAT_PLAYER, THREAT_NPC, THREAT_ANY
    vals[A], has[A] = np.minimum(vals[P], vals[N]), has[P] | has[N]
    player_first = has[P] & (~has[N] | (vals[P][:, 0] <= vals[N][:, 0]))
    chosen = {P: np.full(B, q), N: slot[N], A: np.where(player_first, 1 + q, 3 + slot[N])}
    for col in (P, N, A):
        best, move = vals[col][:, 0], np.full(B, int(Move.Stay))
        for j, (code, _, _) in enumerate(MOVE_DELTAS, start=1):
            gains = cand[:, j] & (vals[col][:, j] > best)
            move, best = np.where(gains, code, move), np.where(gains, vals[col][:, j], best)
        fill_column(out, col, has[col], vals[col][:, 0], move, chosen[col])
    dist, move, target = out
    after = np.full((B, THREAT_AFTER_COLS), SEEK_ABSENT, np.int32)
    shown = np.where(vals[A] >= PATH_UNREACHABLE, SEEK_UNREACHABLE, vals[A])
    for j, code in enumerate([int(Move.Stay)] + [c for c, _, _ in MOVE_DELTAS]):
        after[:, code] = np.where(has[A] & cand[:, j], shown[:, j], SEEK_ABSENT)
    if radius is None:
        return dist, move, target, after, None
    wx, wy = window_cells(px, py, int(radius))
    inside, tile = tile_at(cfg, snap, p, wx, wy, layouts)
    window = np.where(inside & (tile != int(Tile.Wall)), _least(walk, wx, wy, present, tx, ty),
                      PATH_WALL)
    return dist, move, target, after, window.astype(np.uint16)


def flee_moves(move) -> np.ndarray:
    """int8 [B]: column THREAT_ANY of ``threat``'s ``move`` -- the step that
    puts the most walking distance between the player and what hunts it."""
    return np.asarray(move)[:, THREAT_ANY].astype(np.int8)


# -- ticks to the staircase through the enemies (orx_path_ticks) ---------------
def ticks(snap: dict, cfg, player: int, radius=None, bank=None):
    """``(ticks, move)`` of ``player`` (0 / 1) of every game of a
    ``snapshot()``-shaped dict, and with a ``radius`` ``(ticks, move, window)``:
    ``query`` with the live NPCs of the player's depth in the way.

    A live NPC (alive bit set, in the grid, the player on the NPCs' depth) holds
    its cell: with ``a = max(damage - player_armor, 0)`` -- ``damage`` the
    player's ``p_rpg`` row under a character flag, ``cfg.player_damage``
    otherwise -- entering it costs ``1 + ceil(max(health, 1) / a)`` ticks, and
    it cannot be entered when ``a == 0``; every other cell costs 1.  ``T`` of a
    cell is the least total over a walk from it to a StaircaseDown (every cell
    stepped onto, the staircase included; interior cells all Ground), 0 on a
    staircase.

    ticks   int32 [B]: ``T`` of the own cell; -1 where there is no walk, or the
            own cell is a Wall or outside the grid
    move    int8 [B]: the first of Up, Right, Down, Left whose neighbour's entry
            cost plus ``T`` is ``ticks``; Stay when ``ticks <= 0``
    window  uint16 [B, V, V]: ``T`` in ``query``'s format and geometry
            (PATH_WALL, PATH_UNREACHABLE)

    Exact with flags 0 against NPCs that stay: playing ``move`` lowers ``ticks``
    by one per tick and descends where it was 1.  A Dijkstra over all games at
    once, by steps of game time: the cells that emit at step t give t to their
    open neighbours, which emit ``enter`` steps later."""
    import heapq
    check_player(player)
    if radius is not None:
        check_radius(radius)
    bank = bank_of(cfg, bank)
    p, K = int(player), int(cfg.n_npcs)
    W, H = int(cfg.width), int(cfg.height)
    px, py = i64(snap["p_x"][p]), i64(snap["p_y"][p])
    B = len(px)
    if radius is not None and W * H + 127 * K >= PATH_UNREACHABLE:
        raise ValueError("width * height + 127 * n_npcs too large for a window of uint16 values")
    X, Y = (np.broadcast_to(a, (B, W, H)) for a in np.indices((W, H)))
    _, tile = tile_at(cfg, snap, p, X, Y, None if bank is None else bank.layouts)
    # one Wall ring around every game's grid: a step off the grid lands on it
    P = (W + 2) * (H + 2)
    pad = np.full((B, W + 2, H + 2), int(Tile.Wall), np.int8)
    pad[:, 1:-1, 1:-1] = tile
    flat = pad.reshape(-1)
    ground, stair = flat == int(Tile.Ground), flat == int(Tile.StaircaseDown)

    # the held cells: hits per cell (the least over the slots on it), and
    # whether it can be entered at all
    damage = np.full(B, int(cfg.player_damage), np.int64)
    if int(cfg.flags) & EXT_CHARACTER:
        damage = i64(snap["p_rpg"][RPG_FIELDS.index("damage")][p])
    a = np.maximum(damage - int(cfg.player_armor), 0)
    never = np.int32(1) << 30
    hits = np.full(B * P, never, np.int32)
    if K > 0:
        alive, nx, ny, hp = npc_rows(snap, K)
        on = alive & (i64(snap["p_depth"][p]) == npc_depth(cfg))[None] & inside_grid(cfg, nx, ny)
        blows = -(-np.maximum(hp, 1) // np.maximum(a, 1))                 # [K, B]
        k, b = np.nonzero(on)
        np.minimum.at(hits, b * P + (nx[k, b] + 1) * (H + 2) + ny[k, b] + 1, blows[k, b])
    held = hits < never
    barred = held & (np.repeat(a, P) == 0)
    hits = np.where(held & ~barred, hits, 0)

    T = np.full(B * P, -1, np.int32)
    steps = np.array([-1, 1, -(H + 2), H + 2], np.int64)
    due, order = {}, []                 # step -> the cells that emit then

    def emit(cells, t):
        cells = cells[~barred[cells]]
        at = t + 1 + hits[cells].astype(np.int64)
        for step in (np.unique(at) if held[cells].any() else at[:1]):
            if int(step) not in due:
                due[int(step)] = []
                heapq.heappush(order, int(step))
            due[int(step)].append(cells[at == step])

    seeds = np.flatnonzero(stair)
    T[seeds] = 0
    emit(seeds, 0)
    while order:
        t = heapq.heappop(order)
        nxt = (np.concatenate(due.pop(t))[:, None] + steps[None, :]).reshape(-1)
        nxt = np.unique(nxt[ground[nxt] & (T[nxt] < 0)])
        T[nxt] = t
        emit(nxt, t)

    T, hits, barred = (v.reshape(B, W + 2, H + 2) for v in (T, hits, barred))

    def read(plane, x, y):
        return plane[per_game(np.arange(B), x), np.clip(x, -1, W) + 1, np.clip(y, -1, H) + 1]

    own = read(T, px, py)
    out = np.where(inside_grid(cfg, px, py), own, -1).astype(np.int64)
    move = np.full(B, int(Move.Stay), np.int8)
    for code, dx, dy in reversed(MOVE_DELTAS):
        x, y = px + dx, py + dy
        via = inside_grid(cfg, x, y) & (read(T, x, y) >= 0) & ~read(barred, x, y)
        cost = 1 + read(hits, x, y).astype(np.int64) + read(T, x, y)
        move = np.where(via & (out > 0) & (cost == out), code, move)
    out = out.astype(np.int32)
    if radius is None:
        return out, move.astype(np.int8)
    wx, wy = window_cells(px, py, int(radius))
    cell = inside_grid(cfg, wx, wy) & np.isin(read(pad, wx, wy), (int(Tile.Ground), int(Tile.StaircaseDown)))
    value = read(T, wx, wy).astype(np.int64)
    window = np.where(cell, np.where(value < 0, PATH_UNREACHABLE, value), PATH_WALL)
    return out, move.astype(np.int8), window.astype(np.uint16)

