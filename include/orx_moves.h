/*
 * orx_moves.h -- what each move would do, batched: the per-move outcomes of
 * one player of every game, read from the resident SoA state (orx_state_t).
 *
 * The reference's learned-bot interface asks one question per supported move:
 * StateActionBot.evaluate(game_state, move) (optimax_rogue_bots/gui/
 * state_action_bot.py:29, gui/main.py:149).  What a move does is decided by
 * the updater alone: update() turns a move into a blocked cell into a Stay
 * (optimax_rogue/logic/updater.py:89-98), and handle_move then attacks
 * whatever pos_lookup holds at the target, descends on a StaircaseDown, or
 * moves (:196-216).  orx_moves states that answer for every move at once, and
 * with it the action mask a masked policy needs.
 *
 * It is a header of its own so that orx.h's list of entry points stays what
 * it is; the conventions (caller-owned device pointers, asynchronous on the
 * caller's stream, ORX_OK or a negative code with orx_last_error) are orx.h's.
 * ORX_ABI_VERSION is unchanged: no existing struct or entry point changes.
 */
#ifndef ORX_MOVES_H
#define ORX_MOVES_H

#include "orx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORX_MOVES_COLS 8 /* columns of every output row: column m = Move m      */

/* ---- kind (uint8): the outcome in bits 0-2, flags above ------------------- */
#define ORX_OUT_MASK 7
#define ORX_OUT_NONE 0          /* not a move of this configuration              */
#define ORX_OUT_REST 1          /* Move.Stay                                     */
#define ORX_OUT_BLOCKED 2       /* the target cell is outside the grid or a Wall
                                   (Dungeon.is_blocked, world.py:41-46): the
                                   updater plays a Stay (updater.py:89-98)       */
#define ORX_OUT_STEP 3          /* the target is free ground: the player moves   */
#define ORX_OUT_DESCEND 4       /* the target is free and a StaircaseDown        */
#define ORX_OUT_ATTACK_NPC 5    /* an NPC still in GameState.entities stands on
                                   the target                                    */
#define ORX_OUT_ATTACK_PLAYER 6 /* the other player stands on the target         */
#define ORX_OUT_HEAL 7          /* ORX_MOVE_HEAL with ORX_EXT_HEAL               */
#define ORX_OUT_LETHAL 8        /* an attack whose amount is at least the
                                   target's health, that health above 0          */
#define ORX_OUT_ITEM 16         /* ORX_EXT_ITEMS: a STEP onto the cell of an item
                                   on the floor while the player holds fewer
                                   than item_slots items: it is picked up        */
#define ORX_OUT_COOLDOWN 32     /* ORX_EXT_README_COMBAT: ATTACK_PLAYER while the
                                   player's ORX_RPG_COOLDOWN is above 0: the
                                   table measures that attack as a Stay; its
                                   amount is 0                                   */
/* bits 6-7 are zero */

/* For `player` (0 = player 1, 1 = player 2) of every game, what each move m in
 * 1..M would do (M = 5, or 6 with ORX_EXT_HEAL), decided in the updater's
 * order from the state as it stands at the start of the tick.  The three
 * outputs are [n_games][ORX_MOVES_COLS], game-major; column m belongs to Move
 * m, and columns 0, 7 and an unused column 6 hold kind 0, target -1, amount 0
 * (eight columns make a game's row one aligned 8- or 16-byte store: kind must
 * be 8-byte aligned, target and amount 16-byte aligned).
 *
 * kind (uint8, must not be NULL).  With (tx, ty) = calculate_pos(x, y, m)
 * (updater.py:340-351) and d the player's depth, the first that holds:
 *   m == ORX_MOVE_STAY                          -> ORX_OUT_REST
 *   m == ORX_MOVE_HEAL                          -> ORX_OUT_HEAL
 *   (tx, ty) outside the W x H grid or a Wall   -> ORX_OUT_BLOCKED
 *     (tested first, as update() does; EmptyDungeonGenerator: the closed form,
 *     border Wall; a bank: bank_tiles[p_layout[player]][tx * H + ty], the
 *     layout index clamped into the bank as orx_view clamps it)
 *   the other player's depth is d and it stands on (tx, ty), whatever its
 *     health                                    -> ORX_OUT_ATTACK_PLAYER
 *   d is the NPCs' depth (p1_depth for a Separated start, else 0) and an NPC
 *     whose alive bit is set stands on (tx, ty) -> ORX_OUT_ATTACK_NPC
 *   (tx, ty) is a StaircaseDown (closed form: (st_x, st_y) of the player; a
 *     bank: tile code 3)                        -> ORX_OUT_DESCEND
 *   otherwise                                   -> ORX_OUT_STEP
 * ORed with ORX_OUT_LETHAL, ORX_OUT_ITEM (the item lies on the NPCs' depth)
 * and ORX_OUT_COOLDOWN as defined above.
 *
 * target (int16, may be NULL): the entity iden an attack hits -- 1 or 2 for a
 * player, 3 + k for NPC slot k; also under ORX_OUT_COOLDOWN, where it names
 * the player the refused attack was aimed at -- and -1 otherwise.
 *
 * amount (int16, may be NULL; clamped to 0..32767):
 *   an attack: max(dmg, 0) with dmg = the player's damage
 *     (p_rpg[ORX_RPG_DAMAGE] with any ORX_EXT_CHARACTER flag, else
 *     cfg->player_damage) minus its own player_armor (updater.py:313), plus,
 *     with ORX_EXT_MANA, min(mana, mana_max / 3) / mana_per_point; 0 under
 *     ORX_OUT_COOLDOWN;
 *   ORX_OUT_HEAL: min(min(mana, mana_max / 3) / mana_per_point,
 *     max(max_health - health, 0)), and 0 when health is not above 0;
 *   otherwise 0.
 *
 * What the answer is.  It is exact when the other player Stays (tested
 * against the oracle move by move).  ORX_OUT_ATTACK_NPC holds under any NPC
 * policy: the players resolve before the NPCs and the dead are swept only at
 * the end of the tick, so only the combat flag can differ.  Against the other
 * player's own move a STEP can become an attack (both move into one cell, or
 * it steps onto the target first) and an attack can become a step (it moved
 * away first), and ORX_OUT_LETHAL / ORX_OUT_ITEM hold only if the other player
 * does not get there first.  With ORX_EXT_README_COMBAT amount is the
 * full-damage entry of the table (a staying defender that is not on cooldown
 * negates it, a mutual attack halves it).
 *
 * Nothing depends on status: a finished game answers for its stored state.
 * Reads state, writes only the outputs; no host sync (it can be captured in a
 * graph behind orx_env_step), no random words (stock-seed mode works).
 *
 * ORX_EINVAL, on the host before any launch: player not 0 / 1, kind NULL, a
 * misaligned output, n_games <= 0, a configuration orx_validate_cfg refuses,
 * st NULL, or a state pointer NULL that the configuration makes it read:
 *   p_x, p_y, p_depth, p_health          always
 *   st_x, st_y                           without a bank (n_layouts == 0)
 *   p_layout, bank_tiles                 with a bank
 *   npc_pos, npc_health, npc_alive       n_npcs > 0
 *   npc_grid                             n_npcs > ORX_MAX_REG_NPCS
 *   p_rpg                                any ORX_EXT_CHARACTER flag
 *   item_pos, item_mask                  ORX_EXT_ITEMS and n_npcs > 0
 * Replaces the per-move question of StateActionBot.evaluate
 * (optimax_rogue_bots/gui/state_action_bot.py:29), answered by
 * Updater.update / handle_move (updater.py:89-98, 196-216). */
int orx_moves(const orx_cfg_t* cfg, const orx_state_t* st, int32_t player,
              uint8_t* kind, int16_t* target, int16_t* amount,
              int64_t n_games, void* stream);

/* Source hash of this part of the library: the first 16 hex digits of
 * SHA-256(orx_moves.hip || orx_moves.h) (build.moves_id()), "unknown" for a
 * build made outside build.py.  An id of its own, so that orx_build_id() and
 * orx_path_build_id() stay the hashes of the kernels they name. */
const char* orx_moves_build_id(void);

#ifdef __cplusplus
}
#endif

#endif /* ORX_MOVES_H */
