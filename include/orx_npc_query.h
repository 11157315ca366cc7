/*
 * orx_npc_query.h -- the enemies' side of the queries: for every NPC of every
 * game, what each of its moves would do (orx_npc_options) and how far its
 * prey is along walkable cells (orx_npc_seek), read from the resident SoA
 * state (orx_state_t).
 *
 * orx_npc.h lets a caller drive every NPC from a table, the batched form of
 * the reference's hook Updater.decide_npc_move(game_state, ent, result)
 * (optimax_rogue/logic/updater.py:165-178).  The hook is handed the whole
 * GameState; a caller of the table had x, y, health and alive.  These two
 * functions give it what orx_moves and orx_path_seek give a player: which of
 * its moves the engine's guards (orx_npc.h) replace with Stay, what the others
 * do under handle_move (:196-216) -- a free step, an attack, or a step onto a
 * StaircaseDown, which removes the NPC (:263-270) -- and the walking distance
 * and first move to each player.  They are questions about the state: no tick
 * changes, and cfg->npc_policy and cfg->flags are not restricted.
 *
 * Rows are slot-major like orx_npc.h's npc_moves table: row k * n_games + b
 * belongs to NPC slot k (iden 3 + k) of game b.
 *
 * The NPCs' depth nd is p1_depth for a Separated start, else 0.  Its dungeon
 * at the start of the tick (the engine's rule for the given-move tick):
 *   ORX_NPC_DEPTH_WATCHED    a player's p_depth is nd: that player's dungeon
 *                            (st_x, st_y, p_layout; player 1's if it is there,
 *                            else player 2's; the layout index clamped into
 *                            the bank as orx_view clamps it);
 *   ORX_NPC_DEPTH_UNWATCHED  otherwise, with despawn == ORX_DESPAWN_UNREACHABLE
 *                            and p_depth[1] < nd: the dungeon exists, but it is
 *                            keyed (or held in dstore) and these queries do not
 *                            rebuild it;
 *   ORX_NPC_DEPTH_GONE       otherwise: despawned.
 *
 * A header of its own so that orx.h's list of entry points stays what it is;
 * the conventions (caller-owned device pointers, asynchronous on the caller's
 * stream, ORX_OK or a negative code with orx_last_error) are orx.h's.
 * ORX_ABI_VERSION is unchanged: no existing struct or entry point changes.
 */
#ifndef ORX_NPC_QUERY_H
#define ORX_NPC_QUERY_H

#include "orx.h"
#include "orx_moves.h"
#include "orx_path.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- where (uint8): the state of the NPCs' depth -------------------------- */
#define ORX_NPC_DEPTH_GONE 0
#define ORX_NPC_DEPTH_WATCHED 1
#define ORX_NPC_DEPTH_UNWATCHED 2

/* ---- kind (uint8): the outcome in bits 0-2 (ORX_OUT_MASK), ORX_NPC_OUT_LETHAL
 * above.  The numbers are ORX_OUT_*'s wherever the meaning coincides. -------- */
#define ORX_NPC_OUT_NONE 0          /* no answer: a dead slot, a padding column,
                                       or a move on an UNWATCHED depth            */
#define ORX_NPC_OUT_REST 1          /* Move.Stay                                  */
#define ORX_NPC_OUT_BLOCKED 2       /* the target is outside the grid or a Wall:
                                       guard 3 of orx_npc.h plays a Stay          */
#define ORX_NPC_OUT_STEP 3          /* the target is free ground: the NPC moves   */
#define ORX_NPC_OUT_STAIRS 4        /* the target is a free StaircaseDown: the NPC
                                       is removed (updater.py:263-270)            */
#define ORX_NPC_OUT_ATTACK_NPC 5    /* a fellow NPC whose alive bit is set stands
                                       on the target                              */
#define ORX_NPC_OUT_ATTACK_PLAYER 6 /* a player on depth nd stands on the target  */
#define ORX_NPC_OUT_FROZEN 7        /* guards 1 and 2 of orx_npc.h: whatever the
                                       byte of the table, a Stay is played        */
#define ORX_NPC_OUT_LETHAL 8        /* an attack whose amount is at least the
                                       occupant's health, that health above 0     */
/* bits 4-7 are zero */

/* What each move of every NPC would do.  kind, target and amount are
 * [n_npcs][n_games][ORX_MOVES_COLS]; column m belongs to Move m, and columns
 * 0, 6 and 7 hold kind 0, target -1, amount 0 (a row is one aligned 8- or
 * 16-byte store: kind, required, must be 8-byte aligned; target and amount,
 * each of which may be NULL, 16-byte aligned).  where is uint8 [n_games], may
 * be NULL, and holds the game's ORX_NPC_DEPTH_*.
 *
 * The row of a slot whose alive bit is clear is all 0 / -1 / 0, and its stale
 * cell is never an occupant.  For a live slot on cell (x, y), with (tx, ty) =
 * calculate_pos(x, y, m) (updater.py:340-351), from the state as it stands at
 * the start of the tick, the first that holds:
 *   m == ORX_MOVE_STAY                            -> ORX_NPC_OUT_REST
 *   the depth is UNWATCHED                        -> ORX_NPC_OUT_NONE (m in 1..4)
 *   the depth is GONE, or WATCHED and a player whose p_depth is nd, whatever
 *     its health, stands next to a StaircaseDown tile of that dungeon (one of
 *     its four neighbour cells; without a bank: |dx| + |dy| == 1 from (st_x,
 *     st_y))                                      -> ORX_NPC_OUT_FROZEN (m in 1..4)
 *   (tx, ty) outside the W x H grid or a Wall     -> ORX_NPC_OUT_BLOCKED
 *   a player whose p_depth is nd stands on (tx, ty), whatever its health
 *                                                 -> ORX_NPC_OUT_ATTACK_PLAYER,
 *     target 1 or 2 (the two cannot share a cell)
 *   an NPC whose alive bit is set stands on (tx, ty)
 *                                                 -> ORX_NPC_OUT_ATTACK_NPC,
 *     target 3 + its slot
 *   (tx, ty) is a StaircaseDown                   -> ORX_NPC_OUT_STAIRS
 *   otherwise                                     -> ORX_NPC_OUT_STEP
 * Occupancy is tested before the tile, as handle_move does: an occupant that
 * stands on a staircase is attacked.  Up to ORX_MAX_REG_NPCS slots are
 * scanned; dense NPCs read npc_grid at the four targets, and the hit slot's
 * alive bit and health.
 *
 * target (int16): the iden an attack hits, -1 otherwise.  amount (int16): of
 * an attack max(npc_damage - npc_armor, 0) (the attacker's own armor,
 * updater.py:313), clamped to 0..32767; 0 otherwise.
 *
 * The freeze rule is the engine's (orx_npc.h, "The guards"), not the
 * reference's.
 *
 * What the answer is exact for.  ORX_NPC_OUT_FROZEN and ORX_NPC_OUT_BLOCKED
 * hold whatever anyone else does: the guards read only the start of the tick.
 * The other kinds are exact when every other entity Stays (tested against the
 * engine move by move).  Players act before NPCs, the NPCs in shuffled order,
 * and the dead are swept last: against other movers a STEP can become an
 * attack (something moved onto the target first), an attack a STEP or STAIRS
 * (the occupant moved away first), and LETHAL holds only if nobody hits the
 * occupant first -- as orx_moves.h says for the players.
 *
 * Nothing depends on status.  Reads the state, writes only the outputs; no
 * host sync (it can be captured in a graph beside orx_npc_env_step), no
 * random words (stock-seed mode works).
 *
 * ORX_EINVAL, on the host before any launch: n_npcs == 0, kind NULL, a
 * misaligned output, n_games <= 0, a configuration orx_validate_cfg refuses,
 * st NULL, or a state pointer NULL that the configuration makes it read:
 *   p_x, p_y, p_depth, p_health, npc_pos, npc_health, npc_alive   always
 *   st_x, st_y                           without a bank (n_layouts == 0)
 *   p_layout, bank_tiles                 with a bank
 *   npc_grid                             n_npcs > ORX_MAX_REG_NPCS */
int orx_npc_options(const orx_cfg_t* cfg, const orx_state_t* st, uint8_t* kind, int16_t* target,
                    int16_t* amount, uint8_t* where, int64_t n_games, void* stream);

/* The columns of orx_npc_seek's rows (column 3 pads a row). */
#define ORX_NPC_SEEK_P1 0      /* player 1 */
#define ORX_NPC_SEEK_P2 1      /* player 2 */
#define ORX_NPC_SEEK_NEAREST 2 /* the nearer of the two */

/* How far every NPC is from the players along walkable cells, and the move
 * that gets it one step closer.  Rows are [n_npcs][n_games][ORX_SEEK_COLS]
 * with orx_path_seek's alignments (dist int32, 16-byte; move int8, 4-byte;
 * target int16, 8-byte); each output may be NULL, but not all three.
 *
 * A player is a target when its p_depth is nd, whatever its health.  A slot
 * whose alive bit is clear, and every slot of a game whose depth is not
 * ORX_NPC_DEPTH_WATCHED, has no target: every column is ORX_SEEK_ABSENT,
 * ORX_MOVE_STAY, -1.  Otherwise, on the dungeon of nd as defined above:
 *   the distance is orx_path_seek's, from the NPC's cell: with a bank
 *     pairs[layout of nd][player cell][own cell] (pairs: the table
 *     orx_path_rows wrote for the state's bank_tiles); without one (pairs is
 *     NULL and ignored) |dx| + |dy|, plus 2 when the two cells share a row or
 *     column and the staircase lies strictly between them;
 *   dist    the distance, ORX_SEEK_UNREACHABLE where there is no walk,
 *           ORX_SEEK_ABSENT where the column has no target;
 *   move    the first of ORX_MOVE_UP, RIGHT, DOWN, LEFT whose neighbour cell is
 *           at dist - 1 from the target; a StaircaseDown neighbour counts only
 *           if it is the target's own cell; ORX_MOVE_STAY when dist <= 0;
 *   target  the player's iden, 1 or 2; -1 when absent.
 * Column ORX_NPC_SEEK_NEAREST repeats the column of the nearer player: the
 * lesser distance wins, a reachable player beats an unreachable one, an
 * unreachable one an absent one, and player 1 wins a tie.  Column 3 is
 * ORX_SEEK_ABSENT, ORX_MOVE_STAY, -1.
 * The move ignores entities and the freeze guard: orx_npc_options tells what
 * it would do.
 *
 * Reads the state, writes only the outputs; no host sync, no random words;
 * nothing depends on status.  ORX_EINVAL, on the host before any launch:
 * n_npcs == 0, three NULL outputs, a misaligned output, n_games <= 0, a
 * configuration orx_validate_cfg refuses, a bank without pairs, p_layout or
 * bank_tiles, st NULL, or a NULL state pointer that is read (p_x, p_y,
 * p_depth, npc_pos, npc_health, npc_alive; st_x and st_y without a bank). */
int orx_npc_seek(const orx_cfg_t* cfg, const orx_state_t* st, const uint16_t* pairs,
                 int32_t* dist, int8_t* move, int16_t* target, int64_t n_games, void* stream);

/* Source hash of this part of the library: the first 16 hex digits of
 * SHA-256(orx_npc_query.hip || orx_npc_query.h || orx_query.h)
 * (build.npc_query_id()), "unknown" for a build made outside build.py.  An id
 * of its own, so that every other id keeps its value. */
const char* orx_npc_query_build_id(void);

#ifdef __cplusplus
}
#endif

#endif /* ORX_NPC_QUERY_H */
