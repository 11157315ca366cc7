/*
 * orx_path.h -- the staircase distance field of liborx.so: how far every tile
 * of a dungeon is from the nearest StaircaseDown along walkable cells, and
 * the move that gets a player one step closer.
 *
 * The reference's one non-random scripted player, StaircaseBot ("rushes as
 * quickly as possible to the staircase", optimax_rogue_bots/staircasebot.py:
 * 1-21), steps along the larger delta; the updater turns a step into a Wall
 * into Stay (optimax_rogue/logic/updater.py:89-98), so on a map with interior
 * walls it stops at the first one in its way.  The distance a walking entity
 * actually has to cover is a breadth-first search over is_blocked
 * (world.py:41-46) with calculate_pos's four moves (updater.py:340-351).
 * orx_path_field computes it for every layout of a dungeon bank;
 * orx_path_query reads it for one player of every game.  Nothing in the tick
 * changes: this is a definition over the tiles, not a game rule.
 *
 * The same question about targets that move -- how many moves away is the
 * other player, the nearest NPC, the nearest item, and which move gets there --
 * has one more rule built in: the updater descends an entity that steps onto a
 * free StaircaseDown (updater.py:205-206), so a walk that stays on its depth
 * may start or end on a staircase tile but cannot cross one.  orx_path_rows
 * computes that distance from arbitrary source cells (all of them: the pair
 * table of a bank); orx_path_seek reads the table for one player of every game.
 * orx_path_threat reads it the other way round: how near what hunts a player
 * is to its cell, to each move's cell and to every cell of a window -- the
 * danger map -- and the move that flees.
 *
 * All of these treat the enemies as air.  orx_path_ticks does not: a step onto
 * an NPC's cell is an attack that leaves the mover where it is, so the ticks
 * to the staircase are a shortest path with small integer entry costs over
 * the positions and health of each game's NPCs -- a per-game search on the
 * device, which no table over the bank can hold.
 *
 * It is a header of its own so that orx.h's list of entry points stays what
 * it is; the conventions (caller-owned device pointers, asynchronous on the
 * caller's stream, ORX_OK or a negative code with orx_last_error) are orx.h's.
 * ORX_ABI_VERSION is unchanged: no existing struct or entry point changes.
 */
#ifndef ORX_PATH_H
#define ORX_PATH_H

#include "orx.h"
#include "orx_view.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one cell of the field (uint16) --------------------------------------
 * 0 on a StaircaseDown tile, else the number of moves of the shortest
 * 4-connected path over in-grid tiles that are not Wall to the nearest
 * StaircaseDown (any of them descends, updater.py:205-206), or: */
#define ORX_PATH_WALL        0xFFFF   /* a Wall tile, or a cell outside the W x H grid */
#define ORX_PATH_UNREACHABLE 0xFFFE   /* not Wall, but no walkable path to any staircase */
/* A finite value never reaches the sentinels: a path of 0xFFFE moves needs
 * that many non-Wall tiles in a row, and a bank has at most 65,536 tiles. */

/* The field of every layout of a bank: cfg->n_layouts = L in 1..32767 layouts
 * of cfg->width x cfg->height tiles (W, H >= 1, W * H <= 65536: every bank
 * DungeonBank accepts; of cfg only these three fields are read).  bank_tiles
 * is uint8 [L][W * H], flat index x * H + y, as in orx_state_t; field is
 * uint16 [L][W * H] in the same layout.  The result is the unique fixed point
 * of d = min(d, 1 + min over the open neighbours) from d = 0 on the
 * staircases, so it does not depend on the order of the relaxation.  One
 * launch, no host sync; a layout's plane lives in LDS (2 * (W * H + min(W, H)
 * + 1) bytes, 128.5 KiB at the limit).  ORX_EINVAL: a NULL pointer or
 * dimensions outside the above; ORX_EIO: the device refuses that much LDS. */
int orx_path_field(const orx_cfg_t* cfg, const uint8_t* bank_tiles, uint16_t* field, void* stream);

/* For `player` (0 = player 1, 1 = player 2) of every game, on that player's
 * depth.  The value of cell (x, y):
 *   outside the W x H grid: ORX_PATH_WALL;
 *   a dungeon bank (cfg->n_layouts > 0): field[p_layout[player]][x * H + y]
 *     (field: what orx_path_field wrote for the state's bank_tiles; the layout
 *     index is clamped to the bank as orx_view clamps it);
 *   EmptyDungeonGenerator (n_layouts == 0; field is NULL and ignored):
 *     ORX_PATH_WALL on the border, else |x - st_x[player]| + |y - st_y[player]|
 *     -- exact, because the interior has no walls.
 * Outputs (each may be NULL, not all three):
 *   dist   int32 [n_games]: the value of the player's own cell; -1 where it is
 *          ORX_PATH_UNREACHABLE.
 *   move   int8 [n_games]: the first of ORX_MOVE_UP (y - 1), RIGHT (x + 1),
 *          DOWN (y + 1), LEFT (x - 1), in that order, whose target cell has
 *          the value own - 1; ORX_MOVE_STAY when the own value is 0 or a
 *          sentinel.  Entities are not part of the field: a move onto a cell
 *          holding an NPC or the other player is an attack, as handle_move
 *          resolves it.
 *   window uint16 [n_games][V][V], V = 2 * radius + 1, 1 <= radius <=
 *          ORX_VIEW_MAX_RADIUS: the values in orx_view's geometry,
 *          window[(b * V + j) * V + i] = cell (px + i - radius, py + j -
 *          radius).  When window is NULL, radius is ignored.
 * Reads the state, writes only its outputs; no host sync (it can be captured
 * in a graph behind orx_env_step), no random words; nothing depends on
 * status.  ORX_EINVAL: player not 0 / 1, a bad radius with a window, three
 * NULL outputs, n_games <= 0, a configuration orx_validate_cfg refuses, a
 * bank without field or p_layout, or a NULL state pointer that is read (p_x,
 * p_y; st_x and st_y without a bank). */
int orx_path_query(const orx_cfg_t* cfg, const orx_state_t* st, const uint16_t* field,
                   int32_t player, int32_t radius,
                   int32_t* dist, int8_t* move, uint16_t* window,
                   int64_t n_games, void* stream);

/* ---- walking distances between cells --------------------------------------
 * Row i of `rows` (uint16 [n][W * H]) is the walking distance from flat cell
 * cell[i] (= x * H + y) of layout layout[i] to every tile of that layout, in
 * the field's cell format: ORX_PATH_WALL on Wall tiles, ORX_PATH_UNREACHABLE
 * where there is no walk, else the number of moves of the shortest 4-connected
 * path whose interior cells are all Ground; its two end cells may be Ground or
 * StaircaseDown (two adjacent staircases are 1 apart; a staircase in a one-wide
 * corridor cuts it).  The distance is symmetric and 0 from a cell that is not
 * Wall to itself.  A source that is a Wall tile, or an index outside [0, L) or
 * [0, W * H), seeds nothing: its row is ORX_PATH_WALL on the Wall tiles (of the
 * layout index clamped into the bank) and ORX_PATH_UNREACHABLE elsewhere.
 * Entities are not part of the graph.  bank_tiles and the three cfg fields
 * are orx_path_field's, and so is every bank it accepts; layout and cell are
 * device int32 [n].  The pair table pairs[l][s][c], uint16 [L][W * H][W * H],
 * is this over every (l, s).  One launch, no host sync, one workgroup and one
 * LDS plane per row.  ORX_EINVAL: a NULL pointer, n <= 0 or dimensions outside
 * the above; ORX_EIO: the device refuses the LDS. */
int orx_path_rows(const orx_cfg_t* cfg, const uint8_t* bank_tiles,
                  const int32_t* layout, const int32_t* cell, uint16_t* rows,
                  int64_t n, void* stream);

/* The columns of orx_path_seek's rows, and its two negative distances. */
#define ORX_SEEK_PLAYER 0   /* column: the other player */
#define ORX_SEEK_NPC    1   /* the nearest NPC whose alive bit is set */
#define ORX_SEEK_ITEM   2   /* the nearest floor item (ORX_EXT_ITEMS) */
#define ORX_SEEK_COLS   4   /* a row; column 3 pads it */
#define ORX_SEEK_UNREACHABLE (-1)
#define ORX_SEEK_ABSENT      (-2)

/* For `player` (0 / 1) of every game, on that player's depth: how far the
 * targets of each column are along walkable cells, and the move that gets one
 * step closer.  The other player is a target when it is on the viewer's
 * depth, whatever its health; NPCs (every slot of n_npcs whose alive bit is
 * set) and floor items (ORX_EXT_ITEMS) only when the viewer is on the NPCs'
 * depth.  The distance between two cells:
 *   a dungeon bank: pairs[p_layout[player]][target cell][own cell] (pairs: the
 *     table orx_path_rows wrote for the state's bank_tiles; the layout index is
 *     clamped to the bank);
 *   EmptyDungeonGenerator (pairs is NULL and ignored): |dx| + |dy|, plus 2 when
 *     the two cells share a row or column and the staircase (st_x, st_y)[player]
 *     lies strictly between them -- exact, because the interior is at least
 *     two cells wide each way.
 * Outputs (each may be NULL, not all three), rows of ORX_SEEK_COLS columns:
 *   dist   int32 [n_games][4], 16-byte aligned: the least distance over the
 *          column's targets; ORX_SEEK_UNREACHABLE when none of them can be
 *          reached; ORX_SEEK_ABSENT when the column has no target.  0 occurs: a
 *          player can stand on an item it could not take.
 *   target int16 [n_games][4], 8-byte aligned: the lowest slot attaining dist --
 *          the NPC slot, the item slot, 1 - player for the other player; -1
 *          when absent.
 *   move   int8 [n_games][4], 4-byte aligned: the first of ORX_MOVE_UP, RIGHT,
 *          DOWN, LEFT whose neighbour cell is at dist - 1 from that target; a
 *          StaircaseDown neighbour counts only if it is the target's own cell
 *          (a step onto any other descends).  ORX_MOVE_STAY when dist <= 0.
 *          Entities are not part of the graph: a move onto a cell holding an
 *          NPC or the other player is an attack, as handle_move resolves it.
 *   Column 3 is ORX_SEEK_ABSENT, ORX_MOVE_STAY, -1.
 * Reads the state, writes only its outputs; no host sync (it can be captured
 * in a graph behind orx_env_step), no random words; nothing depends on
 * status.  ORX_EINVAL: player not 0 / 1, three NULL outputs, a misaligned
 * output, n_games <= 0, a configuration orx_validate_cfg refuses, a bank
 * without pairs, p_layout or bank_tiles, or a NULL state pointer that is read
 * (p_x, p_y, p_depth; st_x and st_y without a bank; npc_pos, npc_health and
 * npc_alive with NPCs; item_pos and item_mask with items). */
int orx_path_seek(const orx_cfg_t* cfg, const orx_state_t* st, const uint16_t* pairs,
                  int32_t player, int32_t* dist, int8_t* move, int16_t* target,
                  int64_t n_games, void* stream);

/* ---- the danger field: how near the hunters are, and the move that flees ----
 * The columns of orx_path_threat's rows (ORX_SEEK_COLS of them, seek's
 * alignments; column 3 pads). */
#define ORX_THREAT_PLAYER 0   /* column: the other player */
#define ORX_THREAT_NPC    1   /* every NPC whose alive bit is set */
#define ORX_THREAT_ANY    2   /* the union of both */
#define ORX_THREAT_AFTER_COLS 8   /* a row of `after`: column m is Move m */

/* For `player` (0 / 1) of every game, on that player's depth.  A THREAT of the
 * player is the other player when it is on the viewer's depth, whatever its
 * health, and every NPC slot of n_npcs whose alive bit is set when the viewer
 * is on the NPCs' depth: exactly orx_path_seek's targets of its PLAYER and NPC
 * columns (a viewer whose own cell is outside the grid has none).  Items are
 * not threats.
 *
 * The VALUE of a cell c for a column, in the field's uint16 format:
 *   ORX_PATH_WALL on a Wall tile or outside the W x H grid; else the unsigned
 *   minimum, over the column's threats t, of the walking distance between t's
 *   cell and c -- orx_path_seek's distance: pairs[p_layout[player]][t][c] with
 *   a bank, the closed room form without one -- and ORX_PATH_UNREACHABLE where
 *   no threat can walk to c (or the column has no threat).  The sentinels order
 *   themselves under the unsigned minimum: WALL above UNREACHABLE above every
 *   number of moves.  A threat whose cell is outside the grid reaches nothing.
 * Outputs (each may be NULL, not all five):
 *   dist   int32 [n_games][4], 16-byte aligned: the value of the player's own
 *          cell; ORX_SEEK_UNREACHABLE where it is ORX_PATH_UNREACHABLE or above,
 *          ORX_SEEK_ABSENT where the column has no threat (or the own cell is
 *          outside the grid).
 *   target int16 [n_games][4], 8-byte aligned: the nearest threat -- column
 *          PLAYER: 1 - player; NPC: the lowest slot attaining dist; ANY: an
 *          iden, 1 or 2 for a player and 3 + slot for an NPC, the player on a
 *          tie; -1 when absent.
 *   move   int8 [n_games][4], 4-byte aligned: the column's greedy flee move.
 *          The candidates are ORX_MOVE_STAY with the own cell's value, then
 *          ORX_MOVE_UP, RIGHT, DOWN, LEFT, each a candidate when its neighbour
 *          cell is in the grid and its tile is Ground (a Wall is not, and
 *          neither is a StaircaseDown: a step onto one descends -- that is
 *          orx_path_query's move).  The largest value wins, UNREACHABLE above
 *          every number; the first candidate in that order attaining it is
 *          taken, so Stay wins every tie and a move is chosen only when it
 *          strictly gains.  ORX_MOVE_STAY when absent.  Entities are not part
 *          of the graph: a neighbour holding a threat has value 0 and never wins.
 *   after  int32 [n_games][8], 16-byte aligned, for column ANY: column m is
 *          Move m's candidate value in dist's convention (column ORX_MOVE_STAY
 *          equals dist[ANY]); ORX_SEEK_ABSENT where the move is no candidate,
 *          where there is no threat, and in columns 0, 6 and 7.
 *   window uint16 [n_games][V][V], V = 2 * radius + 1, 1 <= radius <=
 *          ORX_VIEW_MAX_RADIUS: column ANY's value of every cell in orx_view's
 *          geometry (orx_path_query's window).  With no threat at all it holds
 *          ORX_PATH_WALL on Wall and off-grid cells and ORX_PATH_UNREACHABLE
 *          elsewhere.  When window is NULL, radius is ignored.
 *   Column 3 of dist, target and move is ORX_SEEK_ABSENT, -1, ORX_MOVE_STAY.
 * So: columns PLAYER and NPC of dist and target equal orx_path_seek's columns
 * of the same name; where column ANY has a threat the window's centre is
 * dist[ANY] (ORX_PATH_UNREACHABLE and above for ORX_SEEK_UNREACHABLE), and its
 * four neighbours are after's values wherever those moves are candidates.
 * Reads the state, writes only its outputs; no host sync (it can be captured
 * in a graph behind orx_env_step), no random words; nothing depends on
 * status.  ORX_EINVAL, on the host before any launch: player not 0 / 1, five
 * NULL outputs, a bad radius with a window, a misaligned output (window: 2
 * bytes), n_games <= 0, a configuration orx_validate_cfg refuses, a bank
 * without pairs, p_layout or bank_tiles, a window without a bank on a grid
 * whose largest distance (W - 3) + (H - 3) + 2 would reach the sentinels, or a
 * NULL state pointer that is read (p_x, p_y, p_depth; st_x and st_y without a
 * bank; npc_pos, npc_health and npc_alive with NPCs). */
int orx_path_threat(const orx_cfg_t* cfg, const orx_state_t* st, const uint16_t* pairs,
                    int32_t player, int32_t radius,
                    int32_t* dist, int8_t* move, int16_t* target, int32_t* after,
                    uint16_t* window, int64_t n_games, void* stream);

/* ---- ticks to the staircase through the enemies ------------------------------
 * orx_path_query treats the enemies as air, but a step onto an NPC's cell is an
 * attack (handle_move, updater.py:218-227): the mover stays where it is, the
 * NPC loses the attacker's damage - armor (updater.py:313) and is swept at the
 * end of the tick in which its health reaches 0 (updater.py:136-145); the step
 * after that is free.  For `player` (0 / 1) of every game, on that player's
 * depth d, this is the staircase distance with that term: the least number of
 * ticks in which the player descends, fighting through or walking round.
 *
 * The GRAPH.  Cells are the in-grid tiles that are not Wall (Ground or
 * StaircaseDown): with a bank planes[p_layout[player]], what orx_route_planes
 * (orx_route.h) wrote for the state's bank_tiles, the layout index clamped as
 * everywhere; without one EmptyDungeonGenerator's closed form (planes is NULL
 * and ignored).  A live NPC HOLDS a cell when d is the NPCs' depth, the slot's
 * alive bit is set and its npc_pos is in the grid.  Let a = max(damage -
 * player_armor, 0), with damage as orx_moves has it without the mana term:
 * p_rpg[ORX_RPG_DAMAGE] under any ORX_EXT_CHARACTER flag, cfg->player_damage
 * otherwise.  hits(c) is ceil(max(health, 1) / a) for a held cell when a > 0
 * (the least over the slots, should several hold one cell: the engine never
 * places two); a held cell cannot be entered when a == 0; hits(c) is 0 for
 * every other cell.  enter(c) = 1 + hits(c).  The other player and items are
 * not part of the graph, exactly as in orx_path_query.
 *
 * The COST.  T(c), the value of a cell, is the least total of enter over a
 * walk from c to any StaircaseDown tile: the sum of enter over every cell
 * stepped onto, the staircase included.  The walk's interior cells are all
 * Ground (a step onto a staircase descends, so a walk never crosses one).  T
 * is 0 on a StaircaseDown tile, whoever stands on it, and T(c) does not
 * include entering c itself.
 *
 * Outputs (each may be NULL, not all three):
 *   ticks  int32 [n_games], 4-byte aligned: T of the own cell; -1 where there
 *          is no such walk, or the own cell is a Wall or outside the grid.
 *   move   int8 [n_games]: the first of ORX_MOVE_UP, RIGHT, DOWN, LEFT whose
 *          neighbour n has enter(n) + T(n) == ticks; ORX_MOVE_STAY when ticks
 *          <= 0.
 *   window uint16 [n_games][V][V], 2-byte aligned, in orx_view's geometry and
 *          orx_path_query's format: ORX_PATH_WALL on Wall and off-grid cells,
 *          ORX_PATH_UNREACHABLE where T is infinite, T elsewhere.  When window
 *          is NULL, radius is ignored.
 *
 * What it is EXACT for.  With no ORX_EXT_CHARACTER flag set, every NPC staying
 * where it is (the reference's decide_npc_move, the default) and the other
 * player on another depth or off the cells used, playing `move` every tick
 * lowers ticks by exactly one per tick, and the player descends in the tick
 * where it was 1.  Under ORX_EXT_MANA or ORX_EXT_ITEMS it is an UPPER BOUND
 * under the same conditions (mana only adds damage, and so does a damage item
 * picked up on the way); ORX_EXT_LEVELING leaves hits as they are.  Against
 * NPCs that move it is an ESTIMATE.  Without a live NPC on the depth, ticks
 * and move equal orx_path_query's dist and move; always ticks >= dist, and
 * ticks == -1 with dist >= 0 happens only when a == 0.
 *
 * One launch, a wave per game, a per-game search in LDS (three bit planes of
 * H * ceil(W / 32) words and the window's tile).  Reads the state, writes only
 * its outputs; no host sync (it can be captured in a graph behind
 * orx_env_step), no random words; nothing depends on status.  ORX_EINVAL, on
 * the host before any launch: player not 0 / 1, three NULL outputs, a bad
 * radius with a window, a misaligned output or misaligned planes (4 bytes),
 * n_games <= 0, a configuration orx_validate_cfg refuses, width * height >
 * 65536, a bank without planes, p_layout or bank_tiles, a window when width *
 * height + 127 * n_npcs >= 0xFFFE (a value could reach the sentinels), or a
 * NULL state pointer that is read (p_x, p_y, p_depth; st_x and st_y without a
 * bank; npc_pos, npc_health and npc_alive with NPCs; p_rpg under a character
 * flag).  ORX_EIO where the device refuses the LDS (a grid narrower than 64
 * and thousands of rows tall). */
int orx_path_ticks(const orx_cfg_t* cfg, const orx_state_t* st, const uint32_t* planes,
                   int32_t player, int32_t radius,
                   int32_t* ticks, int8_t* move, uint16_t* window,
                   int64_t n_games, void* stream);

/* The id of the sources this part of the library was built from: the first 16
 * hex digits of SHA-256(orx_path.hip || orx_path.h), as orx_build_id() is of
 * the engine's and the view's files (which therefore keeps its value, and
 * with it every profile keyed on it, when only the files here change). */
const char* orx_path_build_id(void);

#ifdef __cplusplus
}
#endif

#endif /* ORX_PATH_H */
