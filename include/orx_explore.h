/*
 * orx_explore.h -- the map a player remembers and the way to its edge.
 *
 * orx_sight says which cells of its window a player sees this tick.  An agent
 * behind walls also needs what it saw earlier: the corridor it came through,
 * the staircase it passed and can no longer see.  orx_explore_update keeps, per
 * game and player, one bit per grid cell -- "seen on the present depth in the
 * present episode" -- and orx_explore_seek answers from it how far the nearest
 * edge of the known map and the nearest known staircase are, and which move
 * gets there.  It invents no game rule: no tick reads it, and the map is the
 * caller's memory, not part of orx_state_t.
 *
 * The map.  memory is uint32 [n_games][H][WW], WW = (W + 31) / 32: bit x % 32
 * of memory[(b * H + y) * WW + x / 32] is set when `player` of game b has seen
 * grid cell (x, y) on its present depth in the present episode; bits at
 * x >= W are zero.  Row-major in y like orx_sight's rows, so that an update is
 * a shift and an OR.
 *
 * The key.  key is int32 [n_games][4], 16-byte aligned: {episode, depth, tick,
 * known}, known being the number of set bits of the game's map.  A key row is
 * VALID for a state when key[3] >= 0, key[0] == episode[b], key[1] ==
 * p_depth[player][b] and key[2] <= tick[b].  Players only descend, so
 * (episode, depth) names a dungeon; the tick rule catches a masked orx_reset
 * into the same episode.  A fresh map is all-zero memory with the key filled
 * with -1.
 *
 * The frontier.  A frontier cell is in the grid, known, has the tile Ground and
 * at least one in-grid 4-neighbour that is not known.  A staircase tile is
 * never a frontier cell: a step onto one descends.
 *   Property: every shortest walk (orx_path.h's: interior cells all Ground) from
 *   the player to a NEAREST frontier cell passes only known Ground cells.  The
 *   cell before the first unknown cell of such a walk would be a known Ground
 *   cell with an unknown neighbour, a frontier cell nearer than the nearest.
 *   So the frontier column of orx_explore_seek never uses knowledge the player
 *   lacks, provided the map was updated in the state it is asked about.
 *   The stairs column gives the layout's true walking distance to a staircase
 *   the player has seen; the walk itself may pass cells it has not seen.
 *
 * A header of its own so that orx.h's list of entry points stays what it is;
 * the conventions (caller-owned device pointers, asynchronous on the caller's
 * stream, ORX_OK or a negative code with orx_last_error) are orx.h's.
 * ORX_ABI_VERSION is unchanged: no existing struct or entry point changes.
 */
#ifndef ORX_EXPLORE_H
#define ORX_EXPLORE_H

#include "orx_path.h"
#include "orx_sight.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORX_EXPLORE_KNOWN 128 /* bit 7 of a remembered view cell: the cell is known */

/* Adds what `player` (0 / 1) of every game sees now to its map.
 *   rows (in, uint32 [n_games][V], V = 2 * radius + 1, required): what
 *     orx_sight wrote for the same player and radius.  Sight is not recomputed.
 *     Bits >= V and bits of cells outside the grid are ignored, whatever the
 *     caller passed: no address outside a game's map is formed.
 *   memory, key (in / out, required): the map and its key, above.  Per game:
 *     if the key is not valid the map is zeroed first; the seen cells of the
 *     grid are OR-ed in; the key becomes {episode, depth, tick, known}.  The
 *     known count of a valid key is trusted: the new count is it plus gained.
 *   gained (int32 [n_games], may be NULL): the number of bits this call set;
 *     after a clear, all of them.
 *   cells, health (uint8 [n_games][V][V], in / out, each may be NULL): hold
 *     orx_view's output for the same player and radius.  After the call a
 *     window cell is
 *       outside the grid:        0, health 0;
 *       seen now:                code | ORX_SIGHT_SEEN | ORX_EXPLORE_KNOWN,
 *                                health unchanged;
 *       known but not seen now:  (code & ORX_VIEW_TILE_MASK) | ORX_EXPLORE_KNOWN,
 *                                health 0 -- only the tile is remembered,
 *                                occupants and items would be stale;
 *       otherwise:               0, health 0.
 * Reads the state, writes only memory, key, gained, cells and health; no host
 * sync (it can be captured in a graph behind orx_env_step, orx_view and
 * orx_sight), no random words; nothing depends on status.  ORX_EINVAL: player
 * not 0 / 1, radius outside 1..ORX_VIEW_MAX_RADIUS, rows, memory or key NULL,
 * rows, memory or gained not 4-byte aligned, key not 16-byte aligned,
 * n_games <= 0, a configuration orx_validate_cfg refuses, or a NULL state
 * pointer that is read (p_x, p_y, p_depth, tick, episode). */
int orx_explore_update(const orx_cfg_t* cfg, const orx_state_t* st, int32_t player,
                       int32_t radius, const uint32_t* rows, uint32_t* memory, int32_t* key,
                       int32_t* gained, uint8_t* cells, uint8_t* health, int64_t n_games,
                       void* stream);

/* The columns of orx_explore_seek's rows (ORX_SEEK_COLS of them; 2 and 3 pad:
 * ORX_SEEK_ABSENT, ORX_MOVE_STAY, -1). */
#define ORX_EXPLORE_FRONTIER 0 /* the nearest frontier cell of the player's map */
#define ORX_EXPLORE_STAIRS   1 /* the nearest known StaircaseDown */

/* For `player` (0 / 1) of every game: how far the nearest frontier cell and the
 * nearest known staircase are from its cell, and the move that gets one step
 * closer.  The tiles are the state's -- a bank: bank_tiles[p_layout[player]]
 * (the index clamped into the bank); EmptyDungeonGenerator: the border Wall,
 * (st_x, st_y)[player] the one staircase (when it is not on the border), the
 * rest Ground.  The stairs column's targets are the known cells whose tile is
 * StaircaseDown.  The distance between two cells is orx_path_seek's:
 * pairs[layout][target][own] with a bank (the table is symmetric: the kernel
 * reads own's row), the closed room form with n_layouts == 0 (pairs is NULL
 * and ignored).  The least distance wins, the lowest flat cell on a tie.
 *   dist   int32 [n_games][4], 16-byte aligned: ORX_SEEK_ABSENT where the
 *          column has no target, the key is not valid for the state, or the
 *          player's cell is outside the grid; ORX_SEEK_UNREACHABLE where
 *          targets exist but none can be walked to.
 *   move   int8 [n_games][4], 4-byte aligned: the first of ORX_MOVE_UP, RIGHT,
 *          DOWN, LEFT whose neighbour cell is at dist - 1 from the chosen
 *          target; a StaircaseDown neighbour counts only if it is the target
 *          itself.  ORX_MOVE_STAY when dist <= 0.
 *   target int32 [n_games][4], 16-byte aligned: the chosen target's flat cell
 *          x * H + y (up to 65,535: int16 will not do); the lowest target cell
 *          where none can be reached; -1 when absent.
 * Each output may be NULL, not all three.  Reads the state, memory and key,
 * writes only its outputs; no host sync, no random words; nothing depends on
 * status.  ORX_EINVAL: player not 0 / 1, memory or key NULL or misaligned (4
 * and 16 bytes), three NULL outputs, a misaligned output, n_games <= 0,
 * W * H > 65536, a configuration orx_validate_cfg refuses, a bank without
 * pairs, p_layout or bank_tiles, or a NULL state pointer that is read (p_x,
 * p_y, p_depth, tick, episode; st_x and st_y without a bank). */
int orx_explore_seek(const orx_cfg_t* cfg, const orx_state_t* st, const uint16_t* pairs,
                     int32_t player, const uint32_t* memory, const int32_t* key,
                     int32_t* dist, int8_t* move, int32_t* target, int64_t n_games,
                     void* stream);

/* The first 16 hex digits of SHA-256 over orx_explore.hip, this header and the
 * queries' shared internal header, of the tree the library was built from. */
const char* orx_explore_build_id(void);

#ifdef __cplusplus
}
#endif

#endif /* ORX_EXPLORE_H */
