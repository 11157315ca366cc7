/*
 * orx_sight.h -- line of sight through a dungeon's walls: which cells of
 * orx_view's window a player can actually see from where it stands.
 *
 * orx_view writes every cell of the window, walls or not: the reference hands
 * a bot the whole GameState (optimax_rogue_bots/main.py:118-155), and that
 * stays the default.  With a dungeon bank the games have interior walls;
 * orx_sight answers the partially observable question from the resident SoA
 * state (orx_state_t): an ambush round a corner, a pursuer that loses its
 * target.  It invents no game rule: no tick reads it.
 *
 * The rule is integer, exact and relative to the viewer.  Window cell (j, i)
 * has the offsets dx = i - radius, dy = j - radius, as in orx_view.  A cell is
 * opaque where orx_view's tile bits are ORX_TILE_WALL; Ground, StaircaseDown
 * and every occupant are transparent; cells outside the grid are never seen.
 *   line   n = max(|dx|, |dy|).  For s = 1 .. n - 1 the intermediate cell of
 *          variant "up" has the offsets sign(d) * ((2 s |d| + n) / (2 n)), of
 *          variant "down" sign(d) * ((2 s |d| + n - 1) / (2 n)), d being dx
 *          and dy (floor divisions: s |d| / n rounded half up and half down).
 *   clear  the cell is in the grid and at least one of the two variants -- one
 *          variant for the whole line -- has no opaque intermediate cell.  The
 *          target itself may be opaque.  n <= 1 (the centre included): clear.
 *   seen   a transparent cell: it is clear.  An opaque cell of the grid: it is
 *          clear, or one of its up to three neighbours toward the viewer,
 *          (dx - a, dy - b) with a in {0, sign dx}, b in {0, sign dy} and
 *          (a, b) != (0, 0), is in the grid, transparent and clear (the far
 *          walls of a room, which a bare digital line hides at grazing angles).
 * Among transparent cells the relation is symmetric: A sees B exactly when B
 * sees A (reversing a line swaps the two variants).  Without a bank
 * (n_layouts == 0) every cell of the window that lies in the grid is seen.
 *
 * A header of its own so that orx.h's list of entry points stays what it is;
 * the conventions (caller-owned device pointers, asynchronous on the caller's
 * stream, ORX_OK or a negative code with orx_last_error) are orx.h's.
 * ORX_ABI_VERSION is unchanged: no existing struct or entry point changes.
 */
#ifndef ORX_SIGHT_H
#define ORX_SIGHT_H

#include "orx_view.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORX_SIGHT_SEEN 64 /* bit 6 of a masked view cell: the cell is seen     */

/* What `player` (0 = player 1, 1 = player 2) of every game sees in its window
 * of side V = 2 * radius + 1 (1 <= radius <= ORX_VIEW_MAX_RADIUS).
 *   rows (uint32 [n_games][V], may be NULL): bit i of rows[b * V + j] is set
 *     when window cell (j, i) is seen; bits >= V are zero.
 *   cells (uint8 [n_games][V][V], in / out, may be NULL): holds orx_view's
 *     output for the same player and radius.  A seen cell becomes
 *     code | ORX_SIGHT_SEEN, an unseen cell 0.
 *   health (uint8 [n_games][V][V], in / out, may be NULL): an unseen cell
 *     becomes 0, a seen cell is unchanged.
 * At least one of the three is not NULL.  cells and health are only masked:
 * the opacity is computed from the state -- EmptyDungeonGenerator: the border
 * (worldgen.py:33-43 puts the staircase on an inner cell); a dungeon bank:
 * bank_tiles[p_layout[player]][x * H + y], the layout index clamped into the
 * bank as orx_view clamps it.
 * Reads state, writes only rows / cells / health; no host sync (it can be
 * captured in a graph behind orx_env_step and orx_view), no random words;
 * nothing depends on status.  ORX_EINVAL: player not 0 / 1, radius outside
 * 1..ORX_VIEW_MAX_RADIUS, all three outputs NULL, n_games <= 0, a
 * configuration orx_validate_cfg refuses, or a state pointer the configuration
 * needs that is NULL (p_x, p_y; with a bank p_layout and bank_tiles). */
int orx_sight(const orx_cfg_t* cfg, const orx_state_t* st, int32_t player, int32_t radius,
              uint32_t* rows, uint8_t* cells, uint8_t* health, int64_t n_games, void* stream);

/* The first 16 hex digits of SHA-256 over orx_sight.hip, this header and the
 * queries' shared internal header, of the tree the library was built from. */
const char* orx_sight_build_id(void);

#ifdef __cplusplus
}
#endif

#endif /* ORX_SIGHT_H */
