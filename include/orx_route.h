/*
 * orx_route.h -- walking distances over the map a player remembers.
 *
 * orx_explore_seek measures its distances in the layout: the bank's pair table
 * (2 * L * (W * H)^2 bytes, which the large banks cannot afford), and for the
 * stairs column a walk that may pass cells the player has never seen.
 * orx_route answers from the remembered map alone, by a breadth-first search
 * over its known cells: how far the nearest frontier cell, the nearest known
 * staircase and one cell of the caller's choice are, and which move gets there.
 * It needs no table, works for every grid the seek accepts, and uses only what
 * the player knows.  It invents no game rule: no tick reads it.
 *
 * memory (uint32 [n_games][H][WW]), key (int32 [n_games][4]) and the rule that
 * says when a key is VALID for a state are orx_explore.h's, as are
 * ORX_SEEK_ABSENT, ORX_SEEK_UNREACHABLE and ORX_SEEK_COLS (orx_path.h).  Bits
 * of memory at x >= W are ignored, whatever the caller left there.
 *
 * The tiles are the state's, exactly as orx_explore_seek takes them -- a bank:
 * bank_tiles[p_layout[player]] (the index clamped into the bank);
 * EmptyDungeonGenerator: the border Wall, (st_x, st_y)[player] the one
 * staircase (when it is not on the border), the rest Ground.
 *
 * A KNOWN WALK from cell a to cell t is a 4-connected path in the grid whose
 * interior cells are all known and Ground.  a is the player's own cell,
 * whatever its tile and whether or not it is known; t must be known, and
 * Ground or StaircaseDown (a staircase ends a walk: a step onto one descends).
 * The KNOWN DISTANCE is the number of moves of the shortest known walk; from a
 * cell to itself it is 0, provided the cell can be a t.
 *
 * The rows are [n_games][ORX_SEEK_COLS], in the seek's formats:
 *   dist   int32, 16-byte aligned: the least known distance over the column's
 *          targets; ORX_SEEK_UNREACHABLE where targets exist but none has a
 *          known walk; ORX_SEEK_ABSENT where the column has no target, the key
 *          is not valid for the state, or the player's cell is outside the grid.
 *   target int32, 16-byte aligned: the lowest flat cell x * H + y among the
 *          targets at that distance; the lowest target where none is
 *          reachable; -1 when absent.
 *   move   int8, 4-byte aligned: the first of ORX_MOVE_UP, RIGHT, DOWN, LEFT
 *          whose neighbour cell is in the grid, is known Ground or the target
 *          itself, and is at known distance dist - 1 from the chosen target.
 *          ORX_MOVE_STAY when dist <= 0.
 * Column ORX_ROUTE_GOAL is absent when goal is NULL or goal[b] is outside
 * [0, W * H); ORX_SEEK_UNREACHABLE with target = goal[b] when the goal cell is
 * not known or its tile is neither Ground nor StaircaseDown (also when it is
 * the player's own cell); 0 / Stay when the goal is the player's own cell and
 * can be a t.  Column 3 pads: ORX_SEEK_ABSENT, ORX_MOVE_STAY, -1.
 *
 * Two properties follow (orx_explore.h defines the frontier):
 *   P1.  When the map was updated in the state it is asked about, column
 *   ORX_ROUTE_FRONTIER equals orx_explore_seek's frontier column in all three
 *   outputs.  Every shortest walk to a nearest frontier cell passes only known
 *   Ground cells (orx_explore.h's property), so the two minima are equal; a
 *   frontier cell at the least true distance is a nearest one, so the same
 *   cells attain it; and a neighbour one step closer on a true shortest walk
 *   lies on a known one, and the other way round.
 *   P2.  Where column ORX_ROUTE_FRONTIER is ABSENT or UNREACHABLE, everything
 *   the player can walk to is known, and column ORX_ROUTE_STAIRS equals
 *   orx_explore_seek's stairs column in all three outputs.  Elsewhere its
 *   distance is >= the seek's, or UNREACHABLE where the seek has a number: the
 *   staircase was seen across cells the player has not.
 *
 * A header of its own, like orx_explore.h; the conventions (caller-owned device
 * pointers, asynchronous on the caller's stream, ORX_OK or a negative code with
 * orx_last_error) are orx.h's.  ORX_ABI_VERSION is unchanged.
 */
#ifndef ORX_ROUTE_H
#define ORX_ROUTE_H

#include "orx_explore.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The columns of orx_route's rows. */
#define ORX_ROUTE_FRONTIER 0 /* the frontier cells of the player's map */
#define ORX_ROUTE_STAIRS   1 /* the known StaircaseDown cells */
#define ORX_ROUTE_GOAL     2 /* the one cell goal[b] */

/* Packs a bank once for orx_route: planes is uint32 [n_layouts][2][H][WW], WW =
 * (W + 31) / 32, in the map's own layout -- bit x % 32 of
 * planes[((l * 2 + k) * H + y) * WW + x / 32] is set when cell (x, y) of layout
 * l is Ground (k = 0) or StaircaseDown (k = 1); bits at x >= W are zero.
 * ORX_EINVAL: no bank (n_layouts == 0), bank_tiles or planes NULL, planes not
 * 4-byte aligned, a configuration orx_validate_cfg refuses. */
int orx_route_planes(const orx_cfg_t* cfg, const uint8_t* bank_tiles, uint32_t* planes,
                     void* stream);

/* The rows above for `player` (0 / 1) of every game.  planes is
 * orx_route_planes' output for the state's bank (NULL and ignored when
 * n_layouts == 0); goal is int32 [n_games], flat cells x * H + y, and may be
 * NULL.  Each output may be NULL, not all three.  Reads the state, planes,
 * memory, key and goal, writes only its outputs; no host sync (it can be
 * captured in a graph behind orx_env_step and orx_explore_update), no random
 * words; nothing depends on status.  ORX_EINVAL: player not 0 / 1, memory or
 * key NULL or misaligned (4 and 16 bytes), three NULL outputs, a misaligned
 * output (dist and target 16 bytes, move 4), goal or planes not 4-byte
 * aligned, n_games <= 0, W * H > 65536, a configuration orx_validate_cfg
 * refuses, a bank without planes, p_layout or bank_tiles, or a NULL state
 * pointer that is read (p_x, p_y, p_depth, tick, episode; st_x and st_y
 * without a bank). */
int orx_route(const orx_cfg_t* cfg, const orx_state_t* st, const uint32_t* planes,
              int32_t player, const uint32_t* memory, const int32_t* key, const int32_t* goal,
              int32_t* dist, int8_t* move, int32_t* target, int64_t n_games, void* stream);

/* The first 16 hex digits of SHA-256 over orx_route.hip, this header and the
 * queries' shared internal header, of the tree the library was built from. */
const char* orx_route_build_id(void);

#ifdef __cplusplus
}
#endif

#endif /* ORX_ROUTE_H */
