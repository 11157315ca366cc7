// orx_moves.hip -- what each move would do (include/orx_moves.h) for gfx950.
//
// The reference's learned-bot interface asks StateActionBot.evaluate(state,
// move) once per move (optimax_rogue_bots/gui/state_action_bot.py:29); what a
// move does is the updater's rule: update() turns a move into a blocked cell
// into a Stay (optimax_rogue/logic/updater.py:89-98), handle_move attacks what
// pos_lookup holds at the target, descends on a StaircaseDown, or moves
// (:196-216).  moves_kernel answers for all moves of one player of every game
// from the resident SoA state.  It needs nothing of the tick machinery: only
// orx.h's structs, and the host side's error path (fail / launch_status of
// orx_engine.hip's host part, linked into the same library).
//
// Shape.  One lane per game, 256-thread workgroups, no LDS.  Every state field
// is a batch-contiguous row, so a wave's load of a field is one coalesced
// segment; each output row is eight columns, so a lane writes its game's kind
// row as one 8-byte store and its target / amount rows as one 16-byte store
// each.  The four targets are tested together:
//   tiles: EmptyDungeonGenerator is arithmetic (border Wall, the staircase of
//     the player's depth); a bank is four byte reads of the layout (a bank is
//     a few KiB shared by all games: L2-resident);
//   NPCs: up to ORX_MAX_REG_NPCS slots are scanned once, each packed position
//     compared against the four packed targets; dense NPCs are four byte reads
//     of the game's occupancy grid, as the tick does (one load per target, not
//     255), and the slot's alive bit and health only where a target is hit;
//   items: the on-floor slots are scanned only in games that have any.
// Plain C++ and vector stores only.
#include "../../include/orx_moves.h"
#include "orx_query.h"

namespace orx_moves_dev {

using namespace orx_query;

constexpr uint32_t kNoCell = 0xFFFFFFFFu;  // the packed key of a target outside the grid

struct MovesArgs {
  const int32_t *p_x, *p_y, *p_depth, *p_health, *st_x, *st_y;
  const uint16_t* npc_pos;
  const int8_t* npc_health;
  const uint32_t* npc_alive;
  const uint8_t* npc_grid;
  const int16_t* p_layout;
  const uint8_t* bank_tiles;
  const int32_t* p_rpg;
  const uint16_t* item_pos;
  const uint32_t* item_mask;
  uint8_t* kind;
  int16_t* target;
  int16_t* amount;
  int64_t B;
  int32_t W, H, K, L, player, npc_depth, flags;
  int32_t damage, armor, mana_third, mana_per_point, item_slots;
  int32_t character, items;  // p_rpg is read; item_pos / item_mask are read
};

__device__ __forceinline__ uint32_t clamp_i16(int32_t v) {
  return (uint32_t)(v < 0 ? 0 : v > 32767 ? 32767 : v);
}

__global__ __launch_bounds__(kBlock) void moves_kernel(const MovesArgs a) {
  const int64_t B = a.B;
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const int W = a.W, H = a.H, K = a.K;
  const auto [me, ot] = player_rows(a.player, B, b);

  // the game's header: both players (coalesced rows)
  const int32_t x = a.p_x[me], y = a.p_y[me], d = a.p_depth[me], hp = a.p_health[me];
  const int32_t ox = a.p_x[ot], oy = a.p_y[ot], ohp = a.p_health[ot];
  const bool other_here = a.p_depth[ot] == d;
  const bool npc_here = K > 0 && d == a.npc_depth;

  // the four targets, calculate_pos (updater.py:340-351): Up, Right, Down, Left
  int32_t tx[4] = {x, x + 1, x, x - 1}, ty[4] = {y - 1, y, y + 1, y};
  uint32_t key[4];      // x | y << 8 as npc_pos / item_pos pack it; kNoCell outside the grid
  bool blocked[4], stair[4];
  if (a.L == 0) {
    // EmptyDungeonGenerator (worldgen.py:33-43): border Wall, one staircase
    const int32_t sx = a.st_x[me], sy = a.st_y[me];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = tx[j] >= 0 && tx[j] < W && ty[j] >= 0 && ty[j] < H;
      const bool wall = tx[j] == 0 || tx[j] == W - 1 || ty[j] == 0 || ty[j] == H - 1;
      blocked[j] = !in || wall;
      stair[j] = !blocked[j] && tx[j] == sx && ty[j] == sy;
      key[j] = in ? (uint32_t)tx[j] | (uint32_t)ty[j] << 8 : kNoCell;
    }
  } else {
    const uint8_t* bt =
        a.bank_tiles + (size_t)clamp_layout(a.p_layout[me], a.L) * ((size_t)W * (size_t)H);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = tx[j] >= 0 && tx[j] < W && ty[j] >= 0 && ty[j] < H;
      const uint32_t code =
          in ? bt[(size_t)tx[j] * (size_t)H + (size_t)ty[j]] & 3u : (uint32_t)ORX_TILE_WALL;
      blocked[j] = code == ORX_TILE_WALL;
      stair[j] = code == ORX_TILE_STAIRCASE_DOWN;
      key[j] = in ? (uint32_t)tx[j] | (uint32_t)ty[j] << 8 : kNoCell;
    }
  }

  // the NPC on each target: its slot (-1: none) and health
  int32_t slot[4] = {-1, -1, -1, -1}, nhp[4] = {0, 0, 0, 0};
  if (npc_here) {
    if (K <= ORX_MAX_REG_NPCS) {
      const uint32_t alive = a.npc_alive[b];
#pragma unroll 4
      for (int k = 0; k < K; ++k) {
        const uint32_t pos = a.npc_pos[(int64_t)k * B + b];
        const int32_t h = a.npc_health[(int64_t)k * B + b];
        if (!((alive >> k) & 1u)) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (pos == key[j] && slot[j] < 0) slot[j] = k, nhp[j] = h;
      }
    } else {
      const uint8_t* grid = a.npc_grid + (size_t)b * ((size_t)W * (size_t)H);
      uint32_t g[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        g[j] = key[j] != kNoCell ? grid[(size_t)tx[j] * (size_t)H + (size_t)ty[j]] : 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = (int)g[j] - 1;
        if (k < 0 || k >= K) continue;
        if (!((a.npc_alive[(int64_t)(k >> 5) * B + b] >> (k & 31)) & 1u)) continue;
        slot[j] = k;
        nhp[j] = a.npc_health[(int64_t)k * B + b];
      }
    }
  }

  // the player's own attributes
  int32_t dmg = a.damage, mana = 0, max_hp = 0, held = 0, cooldown = 0;
  if (a.character) {
    const int64_t row = 2 * B, at = (int64_t)a.player * B + b;
    mana = a.p_rpg[ORX_RPG_MANA * row + at];
    dmg = a.p_rpg[ORX_RPG_DAMAGE * row + at];
    max_hp = a.p_rpg[ORX_RPG_MAX_HEALTH * row + at];
    held = a.p_rpg[ORX_RPG_ITEMS * row + at];
    cooldown = a.p_rpg[ORX_RPG_COOLDOWN * row + at];
  }
  // whole points from up to a third of the manabar (attack bonus, heal)
  const int32_t pts =
      (a.flags & ORX_EXT_MANA) ? (mana < a.mana_third ? mana : a.mana_third) / a.mana_per_point : 0;
  dmg = dmg - a.armor + pts;  // (updater.py:313, readme.md:72)
  const int32_t atk = dmg > 0 ? dmg : 0;

  // items on the floor under the targets: bit j
  uint32_t item_hit = 0;
  if (a.items && npc_here && held < a.item_slots) {
    const uint32_t on = a.item_mask[b];
    if (on) {
      for (int k = 0; k < K; ++k) {
        if (!((on >> k) & 1u)) continue;
        const uint32_t pos = a.item_pos[(int64_t)k * B + b];
#pragma unroll
        for (int j = 0; j < 4; ++j) item_hit |= pos == key[j] ? 1u << j : 0u;
      }
    }
  }

  // one move after the other, in the updater's order
  uint32_t kd[ORX_MOVES_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t tg[ORX_MOVES_COLS], am[ORX_MOVES_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int m = 0; m < ORX_MOVES_COLS; ++m) tg[m] = 0xFFFFu;
  const bool on_cooldown = (a.flags & ORX_EXT_README_COMBAT) && cooldown > 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = j + 1;
    if (blocked[j]) {
      kd[m] = ORX_OUT_BLOCKED;
    } else if (other_here && tx[j] == ox && ty[j] == oy) {
      const int32_t amt = on_cooldown ? 0 : atk;
      kd[m] = ORX_OUT_ATTACK_PLAYER | (on_cooldown ? ORX_OUT_COOLDOWN : 0) |
              (ohp > 0 && amt >= ohp ? ORX_OUT_LETHAL : 0);
      tg[m] = (uint32_t)(2 - a.player);
      am[m] = clamp_i16(amt);
    } else if (slot[j] >= 0) {
      kd[m] = ORX_OUT_ATTACK_NPC | (nhp[j] > 0 && atk >= nhp[j] ? ORX_OUT_LETHAL : 0);
      tg[m] = (uint32_t)(3 + slot[j]);
      am[m] = clamp_i16(atk);
    } else if (stair[j]) {
      kd[m] = ORX_OUT_DESCEND;
    } else {
      kd[m] = ORX_OUT_STEP | ((item_hit >> j) & 1u ? ORX_OUT_ITEM : 0);
    }
  }
  kd[ORX_MOVE_STAY] = ORX_OUT_REST;
  if (a.flags & ORX_EXT_HEAL) {  // readme.md:74
    const int32_t room = max_hp - hp > 0 ? max_hp - hp : 0;
    kd[ORX_MOVE_HEAL] = ORX_OUT_HEAL;
    am[ORX_MOVE_HEAL] = clamp_i16(hp > 0 ? (pts < room ? pts : room) : 0);
  }

  // a game's row of each output: one store
  reinterpret_cast<uint2*>(a.kind)[b] =
      make_uint2(kd[0] | kd[1] << 8 | kd[2] << 16 | kd[3] << 24,
                 kd[4] | kd[5] << 8 | kd[6] << 16 | kd[7] << 24);
  if (a.target)
    reinterpret_cast<uint4*>(a.target)[b] = make_uint4(tg[0] | tg[1] << 16, tg[2] | tg[3] << 16,
                                                       tg[4] | tg[5] << 16, tg[6] | tg[7] << 16);
  if (a.amount)
    reinterpret_cast<uint4*>(a.amount)[b] = make_uint4(am[0] | am[1] << 16, am[2] | am[3] << 16,
                                                       am[4] | am[5] << 16, am[6] | am[7] << 16);
}

}  // namespace orx_moves_dev

#ifndef ORX_MOVES_BUILD_ID
#define ORX_MOVES_BUILD_ID "unknown"
#endif

extern "C" const char* orx_moves_build_id(void) { return ORX_MOVES_BUILD_ID; }

extern "C" int orx_moves(const orx_cfg_t* cfg, const orx_state_t* st, int32_t player, uint8_t* kind,
                         int16_t* target, int16_t* amount, int64_t n_games, void* stream) {
  using namespace orx_moves_dev;
  using orx_dev::fail;
  int r;
  if ((r = orx_validate_cfg(cfg)) || (r = check_player("orx_moves", player))) return r;
  if (!kind) return fail(ORX_EINVAL, "orx_moves: kind is NULL");
  if ((r = check_games("orx_moves", n_games))) return r;
  // (a row is one vector store)
  if (misaligned(kind, 8) || misaligned(target, 16) || misaligned(amount, 16))
    return fail(ORX_EINVAL, "orx_moves: kind must be 8-byte, target and amount 16-byte aligned");
  if ((r = check_state(cfg, st, kPlayers | kStairsNoBank | kBank | kNpcs | kGrid | kCharacter |
                                    kItems)))
    return r;
  // (orx_validate_cfg holds ORX_EXT_ITEMS to n_npcs <= ORX_MAX_REG_NPCS: the
  // on-floor bits are one word)
  const bool character = (cfg->flags & ORX_EXT_CHARACTER) != 0, items = has_items(cfg);

  MovesArgs a;
  a.p_x = st->p_x, a.p_y = st->p_y, a.p_depth = st->p_depth, a.p_health = st->p_health;
  a.st_x = st->st_x, a.st_y = st->st_y;
  a.npc_pos = st->npc_pos, a.npc_health = st->npc_health, a.npc_alive = st->npc_alive;
  a.npc_grid = st->npc_grid;
  a.p_layout = st->p_layout, a.bank_tiles = st->bank_tiles;
  a.p_rpg = st->p_rpg, a.item_pos = st->item_pos, a.item_mask = st->item_mask;
  a.kind = kind, a.target = target, a.amount = amount;
  a.B = n_games;
  a.W = cfg->width, a.H = cfg->height, a.K = cfg->n_npcs, a.L = cfg->n_layouts;
  a.player = player;
  a.npc_depth = npc_depth(cfg);
  a.flags = cfg->flags;
  a.damage = cfg->player_damage, a.armor = cfg->player_armor;
  a.mana_third = cfg->mana_max / 3;
  a.mana_per_point = cfg->mana_per_point > 0 ? cfg->mana_per_point : 1;
  a.item_slots = cfg->item_slots;
  a.character = character ? 1 : 0, a.items = items ? 1 : 0;
  const unsigned grid = (unsigned)((n_games + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(moves_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a);
  return orx_dev::launch_status("orx_moves");
}
