/*
 * orx_view.h -- the egocentric map view of liborx.so: what a bot sees, batched.
 *
 * The reference hands every bot the whole GameState each tick -- the tiles of
 * its depth, world.dungeons[depth].tiles, plus every entity
 * (optimax_rogue_bots/main.py:118-155) -- and its spectator draws exactly that
 * as a map: tiles first, then the entities of the viewed depth on top
 * (optimax_rogue_cmdspec/map.py:56-84).  orx_view writes that picture for one
 * player of every game as a window of cell codes centred on the player,
 * straight from the resident SoA state (orx_state_t), with no host copy.
 *
 * It is a header of its own so that orx.h's list of entry points stays what
 * it is; the conventions (caller-owned device pointers, asynchronous on the
 * caller's stream, ORX_OK or a negative code with orx_last_error) are orx.h's.
 * ORX_ABI_VERSION is unchanged: no existing struct or entry point changes.
 */
#ifndef ORX_VIEW_H
#define ORX_VIEW_H

#include "orx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORX_VIEW_MAX_RADIUS 15 /* window side V = 2 * radius + 1 <= 31          */

/* ---- one cell of the window (uint8) ------------------------------------- */
#define ORX_VIEW_TILE_MASK 3   /* bits 0-1: 0 = outside the W x H grid, else the
                                  Tile code (ORX_TILE_GROUND / WALL /
                                  STAIRCASE_DOWN) of dungeons[depth].tiles[x, y] */
#define ORX_VIEW_OUTSIDE 0
#define ORX_VIEW_PLAYER 4      /* bit 2: the other player stands on the cell (it
                                  is on the viewer's depth; whatever its health) */
#define ORX_VIEW_NPC 8         /* bit 3: an NPC still in GameState.entities
                                  stands on the cell                            */
#define ORX_VIEW_ITEM 16       /* bit 4: ORX_EXT_ITEMS: an item lies on the cell */
#define ORX_VIEW_ITEM_KIND 32  /* bit 5: that item's kind (item_mask row 1:
                                  0 damage, 1 max health)                       */
/* bits 6-7 are zero */

/* The window of `player` (0 = player 1, 1 = player 2) of every game, side
 * V = 2 * radius + 1 (1 <= radius <= ORX_VIEW_MAX_RADIUS).  With the viewer at
 * (px, py) on depth d, cells[(b * V + j) * V + i] describes the cell (x, y) =
 * (px + i - radius, py + j - radius): rows are y, columns are x, as map.py
 * draws them (uint8 [n_games][V][V], game-major, contiguous).
 *   tile bits:  EmptyDungeonGenerator: the closed form (border Wall, the
 *     staircase (st_x, st_y) of the viewer's depth, Ground elsewhere); a
 *     dungeon bank: bank_tiles[p_layout[player]][x * H + y].
 *   ORX_VIEW_PLAYER: the other player's cell when its depth is d.
 *   ORX_VIEW_NPC: the cell of each NPC whose alive bit is set, when d is the
 *     NPCs' depth (p1_depth for a Separated start, else 0).
 *   ORX_VIEW_ITEM (| ORX_VIEW_ITEM_KIND): item k (item_mask row 0 bit k) at
 *     item_pos[k], when d is the NPCs' depth.
 * The centre cell is the viewer's own: its tile bits and whatever else stands
 * there, never a flag for the viewer.  Nothing depends on status: a finished
 * game shows its stored state.
 * health (uint8 [n_games][V][V], may be NULL): the health of the flagged
 * occupant -- the other player where ORX_VIEW_PLAYER is set, else the NPC
 * where ORX_VIEW_NPC is set -- clamped to 0..255; 0 where neither is set.
 * Reads state, writes only cells / health; no host sync (it can be captured
 * in a graph behind orx_env_step), no random words.  ORX_EINVAL: player not
 * 0 / 1, radius outside 1..ORX_VIEW_MAX_RADIUS, cells NULL, n_games <= 0, a
 * configuration orx_validate_cfg refuses, or a state pointer the
 * configuration needs that is NULL.
 * Replaces the per-tick GameState a bot receives (optimax_rogue_bots/
 * main.py:118-155) as TextMapView.update draws it (cmdspec/map.py:56-84). */
int orx_view(const orx_cfg_t* cfg, const orx_state_t* st, int32_t player, int32_t radius,
             uint8_t* cells, uint8_t* health, int64_t n_games, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ORX_VIEW_H */
