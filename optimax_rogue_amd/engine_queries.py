"""The queries of BatchedEngine: read-only launches over the resident state.

``EngineQueries`` is the mixin ``BatchedEngine`` inherits them from; the state,
``_call``, ``_require`` and ``_stream`` are the engine's (engine.py).
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class EngineQueries:
    # the bank's tables on the device, each made at its first use (_bank_table);
    # the remembered maps, player -> (memory, key), are a dict per engine
    _stair_field = _pair_field = _route_planes = _explore_maps = None

    def _outs(self, out, specs, what: str, align: int = 0, distinct=None) -> list:
        """A query's output tensors: fresh ones for ``specs`` ((dtype, shape)
        each), or ``out`` (a tensor or a tuple, ``what``) checked against them.
        The kernels write these shapes blindly (with ``align``, a row per
        vector store): a wrong buffer would be an out-of-bounds or misaligned
        device access.  ``distinct``: the names of outputs that must differ."""
        if out is None:
            return [torch.empty(shape, dtype=dt, device=self.device) for dt, shape in specs]
        outs = list(out) if isinstance(out, (tuple, list)) else [out]
        if len(outs) != len(specs):
            raise ValueError(f"out must be {what}")
        aligned = f", {align}-byte aligned" if align else ""
        for t, (dt, shape) in zip(outs, specs):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != shape \
                    or not t.is_contiguous() or t.device != self.device \
                    or (align and t.data_ptr() % align):
                raise ValueError(f"out must hold a contiguous{aligned} {dt} {shape} tensor on "
                                 f"{self.device}")
        if distinct and len({t.data_ptr() for t in outs}) != len(outs):
            raise ValueError(f"out: {', '.join(distinct[:-1])} and {distinct[-1]} must be "
                             "different tensors")
        return outs

    def _seek_outs(self, out, target_dtype, *lead) -> list:
        """``_outs`` for the seek-shaped ``(dist, move, target)``: int32, int8 and
        ``target_dtype`` [*lead, n_games, SEEK_COLS], a row per vector store."""
        from .path import SEEK_COLS
        shape = (*lead, self.B, SEEK_COLS)
        return self._outs(out, [(torch.int32, shape), (torch.int8, shape), (target_dtype, shape)],
                          "(dist, move, target)", align=16, distinct=("dist", "move", "target"))

    def _refuse_wide_cells(self, who: str) -> None:
        if int(self.cfg.width) * int(self.cfg.height) > 65536:
            raise ValueError(f"{who} needs width * height <= 65536 (a flat cell in 16 bits)")

    def _bank_table(self, attr: str, name: str, capture: str, make):
        """The bank's table cached as ``attr``: None without a bank, else made
        at the first use by one call of ``name`` with cfg, the bank's tiles,
        ``make()``'s arguments (tensors as their pointers) and the stream --
        ``make`` allocates and returns ``(table, arguments)``.  Under stream
        capture that first use is refused with ``capture``."""
        if self.bank is None:
            return None
        if getattr(self, attr) is None:
            self._require(name)
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(capture)
            table, args = make()
            ptrs = [_ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
            with torch.cuda.device(self.device):
                code = getattr(self.lib, name)(self._pcfg, _ptr(self.bank_tiles), *ptrs,
                                               self._stream())
            _lib.check(name, code)
            setattr(self, attr, table)
        return getattr(self, attr)

    def view(self, radius: int, player: int = 0, health: bool = False, out=None):
        """orx_view (include/orx_view.h): the egocentric map window of
        ``player`` (0 / 1) of every game, uint8 [n_games, V, V] with V = 2 *
        radius + 1 (1 <= radius <= 15), written by one launch on the current
        stream from the resident state (no host sync, no state change; it can
        be captured in a graph behind a step).  ``cells[b, j, i]`` is grid cell
        (px + i - radius, py + j - radius): tile bits, VIEW_PLAYER, VIEW_NPC
        and the item bits (optimax_rogue_amd.view; ``view.decode`` gives
        planes).  With ``health`` returns ``(cells, health)``, the second
        plane the flagged occupant's health.  ``out`` (a tensor, or a pair
        with ``health``) is written and returned instead of fresh tensors.
        The host reference is ``view.render_view(self.snapshot(), ...)``."""
        from .view import check_view_args
        check_view_args(player, radius)
        self._require("orx_view")
        V = 2 * int(radius) + 1
        outs = self._outs(out, [(torch.uint8, (self.B, V, V))] * (2 if health else 1),
                          "one tensor, or (cells, health) with health=True",
                          distinct=("cells", "health"))
        self._call("orx_view", int(player), int(radius), _ptr(outs[0]),
                   _ptr(outs[1]) if health else None, self.B, self._stream())
        return (outs[0], outs[1]) if health else outs[0]

    # -- line of sight (include/orx_sight.h) -----------------------------------
    def sight(self, radius: int, player: int = 0, out=None) -> torch.Tensor:
        """orx_sight (include/orx_sight.h): which cells of ``view(radius,
        player)``'s window the player sees through the dungeon's walls, as
        uint32 [n_games, V] row words: bit ``i`` of ``rows[b, j]`` is window
        cell (j, i); bits >= V are zero.  A Wall is opaque, everything else
        transparent; the rule (two digital lines per cell, far walls lit
        through their floor neighbours) is optimax_rogue_amd.sight's, symmetric
        among floor cells.  One launch on the current stream from the resident
        state, no host sync, no state change, no random words.  ``out``: the
        tensor written and returned.  The host reference is
        ``sight.pack_rows(sight.visible(self.snapshot(), cfg, player, radius))``."""
        from .view import check_view_args
        check_view_args(player, radius)
        self._require("orx_sight")
        rows, = self._outs(out, [(torch.uint32, (self.B, 2 * int(radius) + 1))], "one tensor",
                           align=4)
        self._call("orx_sight", int(player), int(radius), _ptr(rows), None, None, self.B,
                   self._stream())
        return rows

    def seen_view(self, radius: int, player: int = 0, health: bool = False, out=None):
        """``view(radius, player, health, out)`` under the player's line of
        sight: orx_view, then orx_sight on its output in place (two launches on
        the current stream, no host sync; they can be captured in a graph
        behind a step).  A seen cell is ``code | SIGHT_SEEN`` (bit 6), an
        unseen one 0; the health plane is 0 where unseen.  The host reference
        is ``sight.apply(view.render_view(...), sight.visible(...))``."""
        from .view import check_view_args
        check_view_args(player, radius)
        self._require("orx_sight")
        got = self.view(radius, player=player, health=health, out=out)
        cells, hp = got if health else (got, None)
        self._call("orx_sight", int(player), int(radius), None, _ptr(cells), _ptr(hp), self.B,
                   self._stream())
        return got

    def sees_other(self, radius: int, player: int = 0) -> torch.Tensor:
        """bool [n_games]: the other player is on ``player``'s depth, inside
        its window of this radius, and seen (``sight``'s bit of its cell).
        Symmetric in the two players at one radius."""
        rows = self.sight(radius, player=player).view(torch.int32).to(torch.int64)
        p, q, R = int(player), 1 - int(player), int(radius)
        i = (self.p_x[q] - self.p_x[p]).to(torch.int64) + R
        j = (self.p_y[q] - self.p_y[p]).to(torch.int64) + R
        near = (self.p_depth[p] == self.p_depth[q]) & (i >= 0) & (i <= 2 * R) & (j >= 0) \
            & (j <= 2 * R)
        word = rows.gather(1, j.clamp(0, 2 * R).unsqueeze(1)).squeeze(1)
        return near & (((word >> i.clamp(0, 2 * R)) & 1) != 0)

    # -- the remembered map (include/orx_explore.h) ----------------------------
    def explore_map(self, player: int = 0):
        """``(memory, key)`` of ``player``'s remembered map: uint32 [n_games, H,
        WW] with WW = (W + 31) // 32 -- bit ``x % 32`` of ``memory[b, y, x //
        32]`` is set when the player has seen cell (x, y) on its present depth
        in the present episode -- and int32 [n_games, 4], {episode, depth, tick,
        known} (include/orx_explore.h; ``explore.unpack`` gives a bool map).
        The engine's own tensors, one pair per player, allocated empty at the
        first use (not under capture) and written by ``explore``.  The map is
        not part of ``snapshot()``."""
        from .query import check_player
        check_player(player)
        maps = self._explore_maps
        if maps is None:
            maps = self._explore_maps = {}
        if int(player) not in maps:
            self._require("orx_explore_update")
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the remembered map is allocated at the first explore() call: "
                                   "call explore() (or explore_map()) once before capturing")
            W, H = int(self.cfg.width), int(self.cfg.height)
            memory = torch.zeros((self.B, H, (W + 31) // 32), dtype=torch.int32,
                                 device=self.device).view(torch.uint32)
            key = torch.full((self.B, 4), -1, dtype=torch.int32, device=self.device)
            maps[int(player)] = (memory, key)
        return maps[int(player)]

    def explore(self, radius: int, player: int = 0, view: bool = False, health: bool = False,
                out=None):
        """orx_explore_update (include/orx_explore.h): adds what ``player`` (0 /
        1) of every game sees now in its window of this radius to
        ``explore_map(player)`` and returns ``gained``, int32 [n_games]: the
        number of cells newly known -- the usual exploration reward.  A map of
        another episode or depth (or of a later tick: a reset into the same
        episode) is cleared first, so a descent and an autoreset need no call.
        With ``view`` returns ``(gained, cells)`` (and ``health``: ``(gained,
        cells, health)``): ``view(radius, player)`` as the player remembers it
        -- a seen cell is ``code | SIGHT_SEEN | EXPLORE_KNOWN``, a known cell
        out of sight ``tile | EXPLORE_KNOWN`` (occupants and items are not
        remembered, its health is 0), any other 0.  orx_view when asked, then
        orx_sight for the row words, then orx_explore_update, all on the
        current stream with no host sync; no state change, no random words.
        ``out``: the tensor, or the tuple, written and returned.  The host
        reference is ``explore.update``."""
        from .view import check_view_args
        check_view_args(player, radius)
        if health and not view:
            raise ValueError("health=True needs view=True")
        self._require("orx_explore_update")
        self._require("orx_sight")
        V = 2 * int(radius) + 1
        specs = [(torch.int32, (self.B,))] + [(torch.uint8, (self.B, V, V))] * (view + (view and health))
        outs = self._outs(out, specs, "gained, (gained, cells) with view=True, or (gained, cells, "
                          "health) with health=True too",
                          distinct=("gained", "cells", "health")[:len(specs)] if view else None)
        if outs[0].data_ptr() % 4:
            raise ValueError("out: gained must be 4-byte aligned")
        memory, key = self.explore_map(player)
        cells = outs[1] if view else None
        hp = outs[2] if view and health else None
        if view:
            self.view(radius, player=player, health=health, out=(cells, hp) if health else cells)
        rows = self.sight(radius, player=player)
        self._call("orx_explore_update", int(player), int(radius), _ptr(rows), _ptr(memory),
                   _ptr(key), _ptr(outs[0]), _ptr(cells), _ptr(hp), self.B, self._stream())
        return tuple(outs) if view else outs[0]

    def explore_seek(self, player: int = 0, out=None):
        """orx_explore_seek (include/orx_explore.h): how many moves ``player``
        (0 / 1) of every game is from the nearest frontier cell of its
        remembered map -- a known Ground cell with a neighbour it has not seen
        -- and from the nearest StaircaseDown it has seen, and the move that
        gets one step closer.  Returns ``(dist, move, target)``: int32, int8 and
        int32 [n_games, SEEK_COLS = 4], columns EXPLORE_FRONTIER,
        EXPLORE_STAIRS and two of padding; ``dist`` is SEEK_ABSENT (-2) where
        the column has no target (nothing left to explore; no staircase seen
        yet) or the map is not of this state, SEEK_UNREACHABLE (-1) where no
        target can be walked to; ``target`` the flat cell ``x * H + y``.  Every
        shortest walk to the nearest frontier cell passes only known cells.
        One launch, no host sync, no state change; with a bank the first call
        also builds ``pair_field``.  ``out``: a ``(dist, move, target)`` tuple
        written and returned.  The host reference is ``explore.seek``."""
        from .query import check_player
        check_player(player)
        self._require("orx_explore_seek")
        outs = self._seek_outs(out, torch.int32)
        self._refuse_wide_cells("explore_seek")
        memory, key = self.explore_map(player)
        pairs = self.pair_field
        self._call("orx_explore_seek", _ptr(pairs), int(player), _ptr(memory), _ptr(key),
                   _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), self.B, self._stream())
        return tuple(outs)

    def explore_forget(self, player: Optional[int] = None) -> None:
        """Clears the remembered map of ``player`` (both players' when None):
        all-zero memory, the key -1 (two fills on the current stream)."""
        if player not in (None, 0, 1):
            raise ValueError(f"player must be None, 0 or 1, got {player!r}")
        for p, (memory, key) in (self._explore_maps or {}).items():
            if player is None or p == int(player):
                memory.view(torch.int32).zero_()
                key.fill_(-1)

    # -- walks over the remembered map (include/orx_route.h) -------------------
    @property
    def route_planes(self):
        """The bank's Ground and StaircaseDown bits on the device, uint32 [L, 2,
        H, WW] in the remembered map's layout (orx_route_planes,
        include/orx_route.h; ``route.planes`` is its host twin), packed by one
        launch at the first use.  None without a bank."""
        def make():
            W, H = int(self.cfg.width), int(self.cfg.height)
            planes = torch.empty((len(self.bank), 2, H, (W + 31) // 32), dtype=torch.int32,
                                 device=self.device).view(torch.uint32)
            return planes, (planes,)
        return self._bank_table(
            "_route_planes", "orx_route_planes", "the bank's bit planes are packed at the first "
            "explore_route() call: call explore_route() (or read route_planes) once before "
            "capturing", make)

    def explore_route(self, player: int = 0, goal=None, out=None):
        """orx_route (include/orx_route.h): how many moves ``player`` (0 / 1)
        of every game is from the nearest frontier cell of its remembered map,
        from the nearest StaircaseDown it has seen and from the cell
        ``goal[b]``, walking through cells it KNOWS only, and the move that
        gets one step closer.  Returns ``(dist, move, target)``: int32, int8
        and int32 [n_games, SEEK_COLS = 4], columns ROUTE_FRONTIER,
        ROUTE_STAIRS, ROUTE_GOAL and one of padding, in ``explore_seek``'s
        conventions (SEEK_ABSENT, SEEK_UNREACHABLE; ``target`` the flat cell
        ``x * H + y``).  ``goal``: an integer tensor [n_games] of flat cells
        (cast to int32 on the device), or None -- the column is then absent,
        as where a goal is outside ``[0, W * H)``; a goal the player has not
        seen, or a Wall, is unreachable.  A breadth-first search over the map
        itself: no pair table, so it runs on every bank the engine accepts.
        One launch, no host sync, no state change; with a bank the first call
        also packs ``route_planes``.  ``out``: a ``(dist, move, target)`` tuple
        written and returned.  The host reference is ``route.route``."""
        from .query import check_player
        check_player(player)
        self._require("orx_route")
        outs = self._seek_outs(out, torch.int32)
        self._refuse_wide_cells("explore_route")
        if goal is not None:
            if not isinstance(goal, torch.Tensor) or goal.dtype not in (
                    torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) \
                    or tuple(goal.shape) != (self.B,):
                raise ValueError(f"goal must be an integer tensor of shape ({self.B},)")
            if goal.device != self.device:
                raise ValueError(f"goal is on {goal.device}, the engine on {self.device}")
            goal = goal.to(torch.int32).contiguous()
        memory, key = self.explore_map(player)
        planes = self.route_planes
        self._call("orx_route", _ptr(planes), int(player), _ptr(memory), _ptr(key), _ptr(goal),
                   _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), self.B, self._stream())
        return tuple(outs)

    def explore_route_moves(self, player: int = 0) -> torch.Tensor:
        """int8 [n_games], ready as ``actions``: ``explore_route``'s frontier
        move where a frontier cell is left to walk to, else its stairs move
        where a known walk leads to a staircase, else Stay -- the explorer
        that needs no pair table and never leaves what the player knows
        (``route.router_moves``).  Call ``explore`` first in every state."""
        from .enums import Move
        from .route import ROUTE_FRONTIER as F, ROUTE_STAIRS as S
        dist, move, _ = self.explore_route(player=player)
        stairs = torch.where(dist[:, S] > 0, move[:, S], int(Move.Stay))
        return torch.where(dist[:, F] > 0, move[:, F], stairs)

    @property
    def stair_field(self):
        """The bank's staircase distance field on the device, uint16 [L, W, H]
        (orx_path_field, include/orx_path.h; ``DungeonBank.stair_field`` is its
        host twin), computed by one launch at the first use -- ``__init__`` and
        every other path keep their cost.  None without a bank."""
        def make():
            field = torch.empty((len(self.bank), int(self.cfg.width), int(self.cfg.height)),
                                dtype=torch.uint16, device=self.device)
            return field, (field,)
        return self._bank_table(
            "_stair_field", "orx_path_field", "the staircase field is computed at the first "
            "path() call: call path() (or read stair_field) once before capturing", make)

    def path(self, player: int = 0, radius: Optional[int] = None, out=None):
        """orx_path_query (include/orx_path.h): how far ``player`` (0 / 1) of
        every game is from the nearest staircase of its depth along walkable
        cells, and the move that gets it one step closer.  Returns ``(dist,
        move)``: int32 [n_games], -1 where no staircase can be reached, and
        int8 [n_games], the first of Up, Right, Down, Left whose target is one
        step closer (Stay on a staircase or where none can be reached; ready
        as ``actions``).  With a ``radius`` (1..15) also ``window``, uint16
        [n_games, V, V] with V = 2 * radius + 1: the distances in ``view``'s
        geometry (PATH_WALL on walls and outside the grid, PATH_UNREACHABLE in
        sealed pockets; optimax_rogue_amd.path).  One launch on the current
        stream from the resident state, no host sync, no state change; with a
        bank the first call also computes ``stair_field``.  ``out``: a
        ``(dist, move)`` or ``(dist, move, window)`` tuple of tensors written
        and returned instead of fresh ones.  The host reference is
        ``path.query(self.snapshot(), ...)``."""
        from .path import check_path_args
        check_path_args(player, radius, self.cfg)
        self._require("orx_path_query")
        specs = [(torch.int32, (self.B,)), (torch.int8, (self.B,))]
        if radius is not None:
            V = 2 * int(radius) + 1
            specs.append((torch.uint16, (self.B, V, V)))
        outs = self._outs(out, specs, "(dist, move), or (dist, move, window) with a radius")
        field = self.stair_field
        self._call("orx_path_query", _ptr(field), int(player), int(radius or 0), _ptr(outs[0]),
                   _ptr(outs[1]), _ptr(outs[2]) if radius is not None else None, self.B,
                   self._stream())
        return tuple(outs)

    def path_ticks(self, player: int = 0, radius: Optional[int] = None, out=None):
        """orx_path_ticks (include/orx_path.h): in how many ticks ``player`` (0
        / 1) of every game can descend, with the live NPCs of its depth in the
        way -- ``path`` where a step onto an NPC's cell is the attack it is:
        entering a held cell costs a tick per blow (``ceil(health / (damage -
        armor))``) and one for the step, and the cheaper of fighting through
        and walking round is taken.  Returns ``(ticks, move)``: int32
        [n_games], -1 where no staircase can be reached, and int8 [n_games],
        the first of Up, Right, Down, Left that is on a fastest way (an attack
        where that way goes through an NPC; Stay on a staircase or where none
        can be reached; ready as ``actions``).  With a ``radius`` (1..15) also
        ``window``, uint16 [n_games, V, V]: the ticks of every cell in
        ``view``'s geometry and ``path``'s format.  Exact with flags 0 against
        NPCs that stay and the other player out of the way: playing ``move``
        lowers ``ticks`` by one per tick; an upper bound under EXT_MANA and
        EXT_ITEMS, an estimate against moving NPCs.  Always ``ticks >= path's
        dist``, equal where no NPC lives.  One launch on the current stream, a
        search per game on the device, no host sync, no state change, no
        random words; with a bank the first call also packs ``route_planes``.
        ``out``: a ``(ticks, move)`` or ``(ticks, move, window)`` tuple of
        tensors written and returned instead of fresh ones.  The host
        reference is ``path.ticks(self.snapshot(), ...)``."""
        from .query import check_player, check_radius
        check_player(player)
        if radius is not None:
            check_radius(radius)
        self._require("orx_path_ticks")
        specs = [(torch.int32, (self.B,)), (torch.int8, (self.B,))]
        if radius is not None:
            V = 2 * int(radius) + 1
            specs.append((torch.uint16, (self.B, V, V)))
        outs = self._outs(out, specs, "(ticks, move), or (ticks, move, window) with a radius")
        self._refuse_wide_cells("path_ticks")
        if radius is not None and int(self.cfg.width) * int(self.cfg.height) \
                + 127 * int(self.cfg.n_npcs) >= 0xFFFE:
            raise ValueError("path_ticks: width * height + 127 * n_npcs too large for a window of "
                             "uint16 values")
        planes = self.route_planes
        self._call("orx_path_ticks", _ptr(planes), int(player), int(radius or 0), _ptr(outs[0]),
                   _ptr(outs[1]), _ptr(outs[2]) if radius is not None else None, self.B,
                   self._stream())
        return tuple(outs)

    def rush_moves(self, player: int = 0) -> torch.Tensor:
        """int8 [n_games], ready as ``actions``: ``path_ticks``'s move alone
        (orx_path_ticks with its other outputs NULL) -- the fastest way down,
        through an NPC where the fight is quicker than the way round."""
        from .query import check_player
        check_player(player)
        self._require("orx_path_ticks")
        self._refuse_wide_cells("rush_moves")
        move = torch.empty((self.B,), dtype=torch.int8, device=self.device)
        self._call("orx_path_ticks", _ptr(self.route_planes), int(player), 0, None, _ptr(move), None,
                   self.B, self._stream())
        return move

    # the largest pair table ``pair_field`` builds: 2 * L * (W * H)^2 bytes
    PAIR_FIELD_MAX_BYTES = 1 << 30

    @property
    def pair_field(self):
        """The bank's pair table on the device, uint16 [L, W * H, W * H]: the
        walking distance between every two cells of a layout (orx_path_rows
        over every source, include/orx_path.h; ``DungeonBank.pair_field`` is
        its host twin), built by one launch at the first use.  None without a
        bank; a table above ``PAIR_FIELD_MAX_BYTES`` is refused."""
        def make():
            L, WH = len(self.bank), int(self.cfg.width) * int(self.cfg.height)
            nbytes = 2 * L * WH * WH
            if nbytes > self.PAIR_FIELD_MAX_BYTES:
                raise ValueError(f"the pair table of {L} layouts of {self.cfg.width} x "
                                 f"{self.cfg.height} tiles needs {nbytes} bytes "
                                 f"({nbytes / 2**20:.0f} MiB), above PAIR_FIELD_MAX_BYTES = "
                                 f"{self.PAIR_FIELD_MAX_BYTES}")
            cells = torch.arange(L * WH, dtype=torch.int32, device=self.device)
            layout, cell = cells // WH, cells % WH
            pairs = torch.empty((L, WH, WH), dtype=torch.uint16, device=self.device)
            return pairs, (layout, cell, pairs, L * WH)
        return self._bank_table(
            "_pair_field", "orx_path_rows", "the pair table is built at the first seek() call: "
            "call seek() (or read pair_field) once before capturing", make)

    def seek(self, player: int = 0, out=None):
        """orx_path_seek (include/orx_path.h): how many moves ``player`` (0 /
        1) of every game is from the other player, the nearest live NPC and
        the nearest floor item along walkable cells of its depth, and the move
        that gets it one step closer.  Returns ``(dist, move, target)``: int32,
        int8 and int16 [n_games, SEEK_COLS = 4], columns SEEK_PLAYER, SEEK_NPC,
        SEEK_ITEM and one of padding.  ``dist`` is SEEK_UNREACHABLE (-1) where
        no target of the column can be reached and SEEK_ABSENT (-2) where it
        has none; ``target`` the slot of the nearest (-1: none); ``move`` the
        first of Up, Right, Down, Left that is one step closer to it, Stay
        when ``dist <= 0``.  A walk may start or end on a staircase but not
        cross one; entities are not obstacles (a move onto one is an attack).
        One launch on the current stream from the resident state, no host
        sync, no state change, no random words; with a bank the first call
        also builds ``pair_field``.  ``out``: a ``(dist, move, target)`` tuple
        of tensors written and returned instead of fresh ones.  The host
        reference is ``path.seek(self.snapshot(), ...)``."""
        from .query import check_player
        check_player(player)
        self._require("orx_path_seek")
        outs = self._seek_outs(out, torch.int16)
        pairs = self.pair_field
        self._call("orx_path_seek", _ptr(pairs), int(player), _ptr(outs[0]), _ptr(outs[1]),
                   _ptr(outs[2]), self.B, self._stream())
        return tuple(outs)

    def threat(self, player: int = 0, radius: Optional[int] = None, out=None):
        """orx_path_threat (include/orx_path.h): the danger field of ``player``
        (0 / 1) of every game -- how many moves away what hunts it is along
        walkable cells of its depth, and the move that flees.  A threat is the
        other player and every live NPC (``seek``'s SEEK_PLAYER and SEEK_NPC
        targets).  Returns ``(dist, move, target, after)``: int32, int8 and
        int16 [n_games, SEEK_COLS = 4], columns THREAT_PLAYER, THREAT_NPC,
        THREAT_ANY (the union) and one of padding, and int32 [n_games,
        THREAT_AFTER_COLS = 8].  ``dist`` is the least distance from a threat
        of the column (SEEK_UNREACHABLE / SEEK_ABSENT as in ``seek``),
        ``target`` the nearest one (THREAT_ANY: an iden), ``move`` the first of
        Stay, Up, Right, Down, Left -- a move only onto Ground -- after which
        that distance is largest (Stay on every tie), and column ``m`` of
        ``after`` what Move ``m`` would leave of ``dist[:, THREAT_ANY]``
        (SEEK_ABSENT: not a candidate), a mask or a shaping term for a policy's
        logits.  With a ``radius`` (1..15) also ``window``, uint16 [n_games, V,
        V]: THREAT_ANY's value of every cell in ``view``'s geometry, the
        danger map (PATH_WALL on walls and outside the grid, PATH_UNREACHABLE
        where nothing hunts).  One launch on the current stream from the
        resident state, no host sync, no state change, no random words; with a
        bank the first call also builds ``pair_field``.  ``out``: a tuple of
        the four (five with a radius) tensors written and returned instead of
        fresh ones.  The host reference is ``path.threat(self.snapshot(),
        ...)``."""
        from .path import SEEK_COLS, THREAT_AFTER_COLS
        from .query import check_player, check_radius
        check_player(player)
        if radius is not None:
            check_radius(radius)
        self._require("orx_path_threat")
        row = (self.B, SEEK_COLS)
        specs = [(torch.int32, row), (torch.int8, row), (torch.int16, row),
                 (torch.int32, (self.B, THREAT_AFTER_COLS))]
        names = ("dist", "move", "target", "after")
        if radius is not None:
            V = 2 * int(radius) + 1
            specs.append((torch.uint16, (self.B, V, V)))
            names += ("window",)
        outs = self._outs(out, specs, "(dist, move, target, after), or (dist, move, target, "
                          "after, window) with a radius", distinct=names)
        # (a row is one vector store, after's two; the window may start at any uint16)
        if any(t.data_ptr() % 16 for t in outs[:4]):
            raise ValueError("out: dist, move, target and after must be 16-byte aligned")
        pairs = self.pair_field
        self._call("orx_path_threat", _ptr(pairs), int(player), int(radius or 0), *map(_ptr, outs),
                   *([None] if radius is None else []), self.B, self._stream())
        return tuple(outs)

    def threat_view(self, radius: int, player: int = 0) -> torch.Tensor:
        """``threat(player, radius)``'s window alone, uint16 [n_games, V, V]:
        orx_path_threat with its other outputs NULL (the danger map as an
        observation plane beside ``view``)."""
        from .query import check_player, check_radius
        check_player(player)
        check_radius(radius)
        self._require("orx_path_threat")
        V = 2 * int(radius) + 1
        window = torch.empty((self.B, V, V), dtype=torch.uint16, device=self.device)
        self._call("orx_path_threat", _ptr(self.pair_field), int(player), int(radius), None, None,
                   None, None, _ptr(window), self.B, self._stream())
        return window

    def flee_moves(self, player: int = 0) -> torch.Tensor:
        """int8 [n_games], ready as ``actions``: ``threat``'s move of column
        THREAT_ANY alone (orx_path_threat with its other outputs NULL) -- the
        step that puts the most walking distance between ``player`` and the
        nearest of what hunts it; Stay where no step gains, where nothing hunts
        and in a dead end (``path.flee_moves``)."""
        from .path import SEEK_COLS, THREAT_ANY
        from .query import check_player
        check_player(player)
        self._require("orx_path_threat")
        move = torch.empty((self.B, SEEK_COLS), dtype=torch.int8, device=self.device)
        self._call("orx_path_threat", _ptr(self.pair_field), int(player), 0, None, _ptr(move), None,
                   None, None, self.B, self._stream())
        return move[:, THREAT_ANY]

    def moves(self, player: int = 0, out=None):
        """orx_moves (include/orx_moves.h): what each move of ``player`` (0 / 1)
        would do in every game, as ``(kind, target, amount)``: uint8, int16 and
        int16 [n_games, MOVES_COLS = 8], column ``m`` for Move ``m`` (1..5, and
        MOVE_HEAL with EXT_HEAL).  ``kind`` is the outcome OUT_* (REST,
        BLOCKED, STEP, DESCEND, ATTACK_NPC, ATTACK_PLAYER, HEAL) with the
        OUT_LETHAL / OUT_ITEM / OUT_COOLDOWN flags, ``target`` the iden an
        attack hits (-1 otherwise), ``amount`` its damage or a heal's points
        (optimax_rogue_amd.moves; ``moves.action_mask(kind, M)`` gives the
        mask).  One launch on the current stream from the resident state, no
        host sync, no state change, no random words; it can be captured in a
        graph behind a step.  ``out``: a ``(kind, target, amount)`` tuple of
        tensors written and returned instead of fresh ones.  The host
        reference is ``moves.outcomes(cfg, self.snapshot(), player)``."""
        from .moves import MOVES_COLS, check_moves_args
        check_moves_args(player)
        self._require("orx_moves")
        shape = (self.B, MOVES_COLS)
        outs = self._outs(out, [(torch.uint8, shape), (torch.int16, shape), (torch.int16, shape)],
                          "(kind, target, amount)", align=16,
                          distinct=("kind", "target", "amount"))
        self._call("orx_moves", int(player), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), self.B,
                   self._stream())
        return tuple(outs)

    def moves_kind(self, player: int = 0) -> torch.Tensor:
        """``moves(player)[0]`` alone, uint8 [n_games, MOVES_COLS]: orx_moves
        with its optional outputs NULL (what an action mask needs; a third of
        the stores)."""
        from .moves import MOVES_COLS, check_moves_args
        check_moves_args(player)
        self._require("orx_moves")
        kind = torch.empty((self.B, MOVES_COLS), dtype=torch.uint8, device=self.device)
        self._call("orx_moves", int(player), _ptr(kind), None, None, self.B, self._stream())
        return kind

    # -- the enemies' queries (include/orx_npc_query.h) ------------------------
    def _require_npc_query(self, name: str) -> None:
        if self.K == 0:
            raise ValueError("the NPC queries need a configuration with NPCs (n_npcs > 0)")
        self._require(name)

    def npc_options(self, out=None):
        """orx_npc_options (include/orx_npc_query.h): what each move of every
        NPC would do in every game, as ``(kind, target, amount, where)``: uint8,
        int16 and int16 [n_npcs, n_games, MOVES_COLS = 8], slot-major like
        ``npc_moves`` (row k: iden 3 + k), column ``m`` for Move ``m``, and
        uint8 [n_games], the state of the NPCs' depth (NPC_DEPTH_WATCHED,
        UNWATCHED, GONE).  ``kind`` is the outcome NPC_OUT_* (REST, FROZEN,
        BLOCKED, STEP, STAIRS, ATTACK_NPC, ATTACK_PLAYER, NONE) with the
        NPC_OUT_LETHAL flag, ``target`` the iden an attack hits (-1
        otherwise), ``amount`` its damage.  FROZEN and BLOCKED are the moves
        the engine's guards (include/orx_npc.h) replace with Stay.  One launch
        on the current stream from the resident state, no host sync, no state
        change, no random words; it can be captured in a graph beside a step.
        ``out``: a ``(kind, target, amount, where)`` tuple of tensors written
        and returned instead of fresh ones.  The host reference is
        ``npc_query.options(self.snapshot(), cfg)``."""
        from .moves import MOVES_COLS
        self._require_npc_query("orx_npc_options")
        shape = (self.K, self.B, MOVES_COLS)
        outs = self._outs(out, [(torch.uint8, shape), (torch.int16, shape), (torch.int16, shape),
                                (torch.uint8, (self.B,))], "(kind, target, amount, where)",
                          align=16, distinct=("kind", "target", "amount", "where"))
        self._call("orx_npc_options", _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]),
                   self.B, self._stream())
        return tuple(outs)

    def npc_options_kind(self):
        """``(kind, where)`` of ``npc_options()`` alone: orx_npc_options with
        target and amount NULL (what a mask needs; a fifth of the stores)."""
        from .moves import MOVES_COLS
        self._require_npc_query("orx_npc_options")
        kind = torch.empty((self.K, self.B, MOVES_COLS), dtype=torch.uint8, device=self.device)
        where = torch.empty(self.B, dtype=torch.uint8, device=self.device)
        self._call("orx_npc_options", _ptr(kind), None, None, _ptr(where), self.B, self._stream())
        return kind, where

    def npc_action_mask(self) -> torch.Tensor:
        """bool [n_npcs, n_games, 5]: column ``j`` is Move ``j + 1``, True where
        the engine would play that byte of ``npc_moves`` as given (not
        NPC_OUT_FROZEN, not NPC_OUT_BLOCKED).  Stay is always True; a dead slot
        has only Stay True, so a masked softmax is never empty; the live slots
        of an UNWATCHED game are all True (``npc_query.action_mask``).  Torch
        ops on the device behind one launch, no sync."""
        from .npc_query import action_mask
        return action_mask(*self.npc_options_kind())

    def npc_seek(self, out=None):
        """orx_npc_seek (include/orx_npc_query.h): how many moves every NPC of
        every game is from player 1, player 2 and the nearer of the two along
        walkable cells of the NPCs' depth, and the move that gets it one step
        closer.  Returns ``(dist, move, target)``: int32, int8 and int16
        [n_npcs, n_games, SEEK_COLS = 4], columns NPC_SEEK_P1, NPC_SEEK_P2,
        NPC_SEEK_NEAREST and one of padding; ``dist`` is SEEK_UNREACHABLE (-1)
        or SEEK_ABSENT (-2) as in ``seek``, ``target`` the player's iden (-1:
        none).  A walk may not cross a staircase; entities and the freeze guard
        are ignored (``npc_options`` tells what the move would do).  One launch,
        no host sync, no state change; with a bank the first call also builds
        ``pair_field``.  ``out``: a ``(dist, move, target)`` tuple of tensors
        written and returned instead of fresh ones.  The host reference is
        ``npc_query.seek(self.snapshot(), cfg)``."""
        self._require_npc_query("orx_npc_seek")
        outs = self._seek_outs(out, torch.int16, self.K)
        pairs = self.pair_field
        self._call("orx_npc_seek", _ptr(pairs), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
                   self.B, self._stream())
        return tuple(outs)

    def npc_hunt_moves(self) -> torch.Tensor:
        """int8 [n_npcs, n_games], ready to pass as ``npc_moves``: every NPC's
        first move toward the nearer player (``npc_seek``'s column
        NPC_SEEK_NEAREST) where ``npc_options`` calls that move STEP or
        ATTACK_PLAYER, and Stay otherwise -- a pursuit that walks round walls,
        never steps onto a staircase and never hits a fellow NPC
        (``npc_query.hunt_moves``).  Two launches and torch ops on the device,
        no sync; with a bank, call it (or ``npc_seek``) once before capturing
        a graph."""
        from .enums import (Move, NPC_OUT_ATTACK_PLAYER, NPC_OUT_MASK, NPC_OUT_STEP,
                            NPC_SEEK_NEAREST)
        from .path import SEEK_COLS
        self._require_npc_query("orx_npc_seek")
        kind, _ = self.npc_options_kind()
        move = torch.empty((self.K, self.B, SEEK_COLS), dtype=torch.int8, device=self.device)
        self._call("orx_npc_seek", _ptr(self.pair_field), None, _ptr(move), None, self.B,
                   self._stream())
        m = move[:, :, NPC_SEEK_NEAREST]
        k = torch.gather(kind, 2, m.to(torch.int64).unsqueeze(2)).squeeze(2) & NPC_OUT_MASK
        ok = (k == NPC_OUT_STEP) | (k == NPC_OUT_ATTACK_PLAYER)
        return torch.where(ok, m, int(Move.Stay))
