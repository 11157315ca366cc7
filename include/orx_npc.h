/*
 * orx_npc.h -- the tick with the NPCs' moves supplied by the caller: the
 * batched form of the reference's override hook
 * Updater.decide_npc_move(game_state, ent, result)
 * (optimax_rogue/logic/updater.py:165-178, called at :121).
 *
 * The reference lets any caller drive the enemies: whatever the hook returns
 * is resolved through the NPC shuffle, handle_move and the death sweep
 * (:116-145, 180-243, 263-270).  orx.h feeds that resolution from two
 * built-in AIs (cfg.npc_policy, ORX_NPC_*).  These entry points feed it from
 * a table in device memory instead, so a learned enemy, a scripted scenario
 * or a recorded game can be played.  A given-move tick is the moving-NPC tick
 * of orx_step with decide_npc_move replaced by a table lookup; nothing else
 * of the tick changes.
 *
 * The table.  npc_moves is int8 [n_npcs][n_games], slot-major like npc_pos
 * (consecutive games are consecutive bytes): npc_moves[k * n_games + b] is the
 * Move (1..5) of NPC slot k (iden 3 + k) of game b.  orx_npc_step_n takes
 * [n_ticks][n_npcs][n_games], indexed by the step of the call, not by the
 * game's tick.
 *
 * The guards.  The given move passes the guards of the built-in AIs (orx.h,
 * ORX_NPC_*), in their order:
 *   1. an NPC on a depth without a dungeon (despawned) stays;
 *   2. an NPC on a depth where a player stands next to a staircase tile stays;
 *   3. a move into a blocked cell (Dungeon.is_blocked, world.py:41-46) becomes
 *      Stay.
 * They are the engine's, not the reference's: for the first the reference
 * raises KeyError (the depth's dungeon is gone, :203), for the third it walks
 * the NPC into the wall (handle_move tests occupancy, not tiles: update()
 * filters only the players' moves, :89-98).  The second keeps the first from
 * arising in the middle of a tick (a descend that despawns the depth, then an
 * NPC stepping onto a free cell), as it does for the AIs.  A caller that
 * wants the reference's literal behaviour applies the guards itself before
 * it compares (tests/golden/make_given.py does).
 *
 * Validity.  A byte outside 1..5 in the slot of an NPC that is alive stops
 * that game with ORX_STATUS_BAD_ACTION, exactly as a bad player action does:
 * nothing is played, no events are recorded, and the game restarts on the
 * next step under autoreset.  Bytes of dead slots are never looked at.  On a
 * step that resets a game (autoreset) the table is ignored, as the actions
 * are.
 *
 * Random draws.  The SHUFFLE stream is consumed as in the moving-NPC tick
 * (the player shuffle, then the NPC Fisher-Yates).  Nothing is drawn from the
 * NPC stream (Philox purpose 9); in stock-seed mode nothing is drawn between
 * the two shuffles.  Hence an all-Stay table plays the ORX_NPC_STAY game, and
 * (keyed mode) a table holding a built-in AI's decisions plays that AI's game
 * (both tested).
 *
 * The cfg.  Every function takes the caller's ordinary cfg.  It must pass
 * orx_validate_cfg, have n_npcs > 0 and flags within
 * ORX_EXT_SEPARATION_DAMAGE | ORX_EXT_RANDOM_DOUBLE_DEATH (the moving-NPC
 * tick's limit); otherwise ORX_EINVAL, as for a NULL npc_moves, on the host
 * before any device call.  cfg->npc_policy is validated and otherwise not
 * read, so one state may be advanced by orx_step (the built-in AI, or Stay)
 * on one tick and by orx_npc_step on the next.
 *
 * A header of its own so that orx.h's list of entry points stays what it is;
 * the conventions (caller-owned device pointers, asynchronous on the caller's
 * stream, ORX_OK or a negative code with orx_last_error) are orx.h's.
 * ORX_ABI_VERSION is unchanged: no existing struct or entry point changes.
 */
#ifndef ORX_NPC_H
#define ORX_NPC_H

#include "orx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Event records per game-tick of orx_npc_step_events: 6 + 2 * n_npcs, or
 * ORX_MAX_EVENTS where that is larger, whatever cfg->npc_policy is (what
 * orx_max_events returns for a moving npc_policy).  ORX_EINVAL for a cfg
 * these entry points refuse. */
int orx_npc_max_events(const orx_cfg_t* cfg);

/* orx_step with the NPCs' moves from npc_moves [n_npcs][n_games].  Keyed and
 * stock-seed mode.  Replaces Updater.update (updater.py:76-162) of an updater
 * whose decide_npc_move is overridden (:165-178). */
int orx_npc_step(const orx_cfg_t* cfg, const orx_state_t* st, const int8_t* actions,
                 const int8_t* npc_moves, int64_t n_games, uint64_t seed, int64_t game_offset,
                 void* stream);

/* orx_step_events likewise: for game b, events[(b * orx_npc_max_events(cfg) +
 * j) * 4 + 0..3], j < n_events[b].  Keyed and stock-seed mode. */
int orx_npc_step_events(const orx_cfg_t* cfg, const orx_state_t* st, const int8_t* actions,
                        const int8_t* npc_moves, int32_t* events, int32_t* n_events,
                        int64_t n_games, uint64_t seed, int64_t game_offset, void* stream);

/* orx_step_n_ex likewise: step t plays actions[t] and npc_moves[(t * n_npcs +
 * k) * n_games + b].  Identical to n_ticks x orx_npc_step (tested).  Keyed
 * mode only, as orx_step_n. */
int orx_npc_step_n(const orx_cfg_t* cfg, const orx_state_t* st, const int8_t* actions,
                   const int8_t* npc_moves, int32_t n_ticks, int32_t* obs, int32_t obs_format,
                   int64_t n_games, uint64_t seed, int64_t game_offset, int32_t concurrency,
                   void* stream);

/* orx_env_step_args likewise (a learner's tick in one launch, no host sync):
 * the block's arguments plus the table [n_npcs][n_games].  A game stopped by
 * a bad byte of the table counts in args->bad_actions too.  Keyed mode only,
 * as orx_env_step. */
int orx_npc_env_step(const orx_env_step_args_t* args, const int8_t* npc_moves);

/* Source hash of this part of the library: the first 16 hex digits of
 * SHA-256(orx_npc.h || orx_engine.hip) (build.npc_id()), "unknown" for a
 * build made outside build.py.  An id of its own, so that orx_build_id()
 * stays the hash of the files it names. */
const char* orx_npc_build_id(void);

#ifdef __cplusplus
}
#endif

#endif /* ORX_NPC_H */
