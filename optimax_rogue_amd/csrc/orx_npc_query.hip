// orx_npc_query.hip -- the enemies' queries (include/orx_npc_query.h) for
// gfx950: what each move of every NPC would do, and every NPC's walking
// distance and first move to the players.
//
// The given-move tick (include/orx_npc.h) passes the caller's byte through
// the AI's guards and then through handle_move (updater.py:196-216);
// options_kernel restates both from the resident SoA state, seek_kernel
// answers orx_path_seek's question from an NPC's cell.  Neither needs the tick
// machinery: only orx.h's structs and the host side's error path (fail /
// launch_status of orx_engine.hip's host part, linked into the same library).
//
// Shape.  One lane per (slot, game): blockIdx.y is the slot, the game index
// runs along x, 256-thread workgroups, no LDS.  npc_pos / npc_health rows and
// the player rows are batch-contiguous, so a wave's load of a field is one
// coalesced segment, and slot-major outputs make consecutive lanes write
// consecutive rows: a lane's kind row is one 8-byte store, its target / amount
// / dist rows one 16-byte store each.  The game's header (both players, the
// staircase or layout of the NPCs' depth) is read again by each of a game's K
// lanes; they sit in different workgroups, so all but the first come from L2
// (44 bytes per lane against 40 written).  A lane per game with the K
// positions in registers would read the header once, but it has 1 / K of the
// lanes (at 65,536 games one wave per SIMD, nothing to hide the loads behind),
// a loop over the slots around the four targets, and no bound on K for the
// dense form; it was not built.  At K = 8 the stores are most of the bytes
// either way.
//   tiles: EmptyDungeonGenerator is arithmetic; a bank is byte reads of the
//     layout (a few KiB shared by all games: L2-resident);
//   fellow NPCs: up to ORX_MAX_REG_NPCS slots are scanned, each packed
//     position compared against the four packed targets; dense NPCs are four
//     byte reads of the game's occupancy grid, and the hit slot's alive bit
//     and health only where a target is hit (as orx_moves does).
// The seek helpers (the closed-form room distance and the first-move rule) are
// orx_seek.h's, the ones orx_path_seek uses.
// Plain C++ and vector stores only.
#include "../../include/orx_npc_query.h"
#include "orx_query.h"
#include "orx_seek.h"

namespace orx_npc_query_dev {

using namespace orx_query;

constexpr uint32_t kNoCell = 0xFFFFFFFFu;  // the packed key of a target outside the grid
constexpr uint32_t kAbsent = 0xFFFFFFFFu;  // no target at all (above orx_seek.h's kNoPath)

// What both kernels read of a game: the players and the NPCs' depth.
struct GameArgs {
  const int32_t *p_x, *p_y, *p_depth, *p_health, *st_x, *st_y;
  const uint16_t* npc_pos;
  const int8_t* npc_health;
  const uint32_t* npc_alive;
  const uint8_t* npc_grid;
  const int16_t* p_layout;
  const uint8_t* bank_tiles;
  int64_t B;
  int32_t W, H, K, L, npc_depth, unreachable;  // unreachable: despawn == ORX_DESPAWN_UNREACHABLE
};

struct OptionsArgs {
  GameArgs g;
  uint8_t* kind;
  int16_t* target;
  int16_t* amount;
  uint8_t* where;
  int32_t attack;  // max(npc_damage - npc_armor, 0), clamped to int16
};

struct SeekArgs {
  GameArgs g;
  const uint16_t* pairs;
  int32_t* dist;
  int8_t* move;
  int16_t* target;
};

// The NPCs' depth of game b at the start of the tick (the engine's npc_depth):
// its state, which players stand on it, and the player row whose dungeon it is.
struct Depth {
  int32_t state;
  bool on1, on2;
  int64_t row;
};
__device__ __forceinline__ Depth depth_of(const GameArgs& g, int64_t b) {
  const int32_t d1 = g.p_depth[b], d2 = g.p_depth[g.B + b];
  Depth d;
  d.on1 = d1 == g.npc_depth, d.on2 = d2 == g.npc_depth;
  d.row = d.on1 ? b : g.B + b;
  d.state = d.on1 || d.on2                        ? ORX_NPC_DEPTH_WATCHED
            : g.unreachable && d2 < g.npc_depth ? ORX_NPC_DEPTH_UNWATCHED
                                                : ORX_NPC_DEPTH_GONE;
  return d;
}

__device__ __forceinline__ bool alive_bit(const GameArgs& g, int k, int64_t b) {
  return (g.npc_alive[(int64_t)(k >> 5) * g.B + b] >> (k & 31)) & 1u;
}

// the layout of the NPCs' depth (a bank), clamped into the bank
__device__ __forceinline__ const uint8_t* layout_tiles(const GameArgs& g, const Depth& d,
                                                       size_t& lay) {
  lay = (size_t)clamp_layout(g.p_layout[d.row], g.L);
  return g.bank_tiles + lay * ((size_t)g.W * (size_t)g.H);
}

// A player on cell (px, py) stands next to a StaircaseDown tile of the depth
// (the engine's next_to_stairs): bt the bank's layout, else the closed form
__device__ __forceinline__ bool next_to_stairs(const GameArgs& g, const uint8_t* bt, int32_t sx,
                                               int32_t sy, int32_t px, int32_t py) {
  if (!bt) {
    const int32_t dx = px - sx, dy = py - sy;
    return (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) == 1;
  }
  const int32_t nx[4] = {px, px + 1, px, px - 1}, ny[4] = {py - 1, py, py + 1, py};
  bool any = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool in = nx[j] >= 0 && nx[j] < g.W && ny[j] >= 0 && ny[j] < g.H;
    const uint32_t code = in ? bt[(size_t)nx[j] * (size_t)g.H + (size_t)ny[j]] & 3u : 0u;
    any = any || code == ORX_TILE_STAIRCASE_DOWN;
  }
  return any;
}

__device__ __forceinline__ void store_options(const OptionsArgs& a, int64_t row, const uint32_t* kd,
                                              const uint32_t* tg, const uint32_t* am) {
  reinterpret_cast<uint2*>(a.kind)[row] =
      make_uint2(kd[0] | kd[1] << 8 | kd[2] << 16 | kd[3] << 24,
                 kd[4] | kd[5] << 8 | kd[6] << 16 | kd[7] << 24);
  if (a.target)
    reinterpret_cast<uint4*>(a.target)[row] = make_uint4(tg[0] | tg[1] << 16, tg[2] | tg[3] << 16,
                                                         tg[4] | tg[5] << 16, tg[6] | tg[7] << 16);
  if (a.amount)
    reinterpret_cast<uint4*>(a.amount)[row] = make_uint4(am[0] | am[1] << 16, am[2] | am[3] << 16,
                                                         am[4] | am[5] << 16, am[6] | am[7] << 16);
}

__global__ __launch_bounds__(kBlock) void options_kernel(const OptionsArgs a) {
  const GameArgs& g = a.g;
  const int64_t B = g.B;
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const int W = g.W, H = g.H, K = g.K, k = (int)blockIdx.y;
  const int64_t row = (int64_t)k * B + b;

  const Depth d = depth_of(g, b);
  if (k == 0 && a.where) a.where[b] = (uint8_t)d.state;

  uint32_t kd[ORX_MOVES_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t tg[ORX_MOVES_COLS], am[ORX_MOVES_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int m = 0; m < ORX_MOVES_COLS; ++m) tg[m] = 0xFFFFu;

  if (!alive_bit(g, k, b)) {  // a dead slot: no answer (its cell is stale)
    store_options(a, row, kd, tg, am);
    return;
  }
  kd[ORX_MOVE_STAY] = ORX_NPC_OUT_REST;
  if (d.state == ORX_NPC_DEPTH_UNWATCHED) {
    store_options(a, row, kd, tg, am);
    return;
  }

  // the players and the dungeon of the depth
  const int32_t p1x = g.p_x[b], p1y = g.p_y[b], p2x = g.p_x[B + b], p2y = g.p_y[B + b];
  const uint8_t* bt = nullptr;
  int32_t sx = -1, sy = -1;
  bool frozen = d.state == ORX_NPC_DEPTH_GONE;
  if (!frozen) {
    if (g.L > 0) {
      size_t lay;
      bt = layout_tiles(g, d, lay);
    } else {
      sx = g.st_x[d.row], sy = g.st_y[d.row];
    }
    frozen = (d.on1 && next_to_stairs(g, bt, sx, sy, p1x, p1y)) ||
             (d.on2 && next_to_stairs(g, bt, sx, sy, p2x, p2y));
  }
  if (frozen) {
#pragma unroll
    for (int m = ORX_MOVE_UP; m <= ORX_MOVE_LEFT; ++m) kd[m] = ORX_NPC_OUT_FROZEN;
    store_options(a, row, kd, tg, am);
    return;
  }

  // the four targets, calculate_pos (updater.py:340-351): Up, Right, Down, Left
  const uint32_t own = g.npc_pos[row];
  const int32_t x = (int32_t)(own & 0xFFu), y = (int32_t)(own >> 8);
  const int32_t tx[4] = {x, x + 1, x, x - 1}, ty[4] = {y - 1, y, y + 1, y};
  uint32_t key[4];  // x | y << 8 as npc_pos packs it; kNoCell outside the grid
  bool blocked[4], stair[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool in = tx[j] >= 0 && tx[j] < W && ty[j] >= 0 && ty[j] < H;
    if (bt) {
      const uint32_t code =
          in ? bt[(size_t)tx[j] * (size_t)H + (size_t)ty[j]] & 3u : (uint32_t)ORX_TILE_WALL;
      blocked[j] = code == ORX_TILE_WALL;
      stair[j] = code == ORX_TILE_STAIRCASE_DOWN;
    } else {
      // EmptyDungeonGenerator (worldgen.py:33-43): border Wall, one staircase
      const bool wall = tx[j] == 0 || tx[j] == W - 1 || ty[j] == 0 || ty[j] == H - 1;
      blocked[j] = !in || wall;
      stair[j] = !blocked[j] && tx[j] == sx && ty[j] == sy;
    }
    key[j] = in ? (uint32_t)tx[j] | (uint32_t)ty[j] << 8 : kNoCell;
  }

  // the fellow NPC on each target: its slot (-1: none) and health
  int32_t slot[4] = {-1, -1, -1, -1}, nhp[4] = {0, 0, 0, 0};
  if (K <= ORX_MAX_REG_NPCS) {
    const uint32_t alive = g.npc_alive[b];
#pragma unroll 4
    for (int j2 = 0; j2 < K; ++j2) {
      const uint32_t pos = g.npc_pos[(int64_t)j2 * B + b];
      const int32_t h = g.npc_health[(int64_t)j2 * B + b];
      if (!((alive >> j2) & 1u)) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (pos == key[j] && slot[j] < 0) slot[j] = j2, nhp[j] = h;
    }
  } else {
    const uint8_t* grid = g.npc_grid + (size_t)b * ((size_t)W * (size_t)H);
    uint32_t cell[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      cell[j] = key[j] != kNoCell ? grid[(size_t)tx[j] * (size_t)H + (size_t)ty[j]] : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int s = (int)cell[j] - 1;
      if (s < 0 || s >= K) continue;
      if (!alive_bit(g, s, b)) continue;
      slot[j] = s;
      nhp[j] = g.npc_health[(int64_t)s * B + b];
    }
  }

  // one move after the other, in handle_move's order: occupancy, then the tile
  const int32_t hp1 = g.p_health[b], hp2 = g.p_health[B + b];
  const int32_t atk = a.attack;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = j + 1;
    const bool at1 = d.on1 && tx[j] == p1x && ty[j] == p1y;
    const bool at2 = d.on2 && tx[j] == p2x && ty[j] == p2y;
    if (blocked[j]) {
      kd[m] = ORX_NPC_OUT_BLOCKED;
    } else if (at1 || at2) {
      const int32_t hp = at1 ? hp1 : hp2;
      kd[m] = ORX_NPC_OUT_ATTACK_PLAYER | (hp > 0 && atk >= hp ? ORX_NPC_OUT_LETHAL : 0);
      tg[m] = at1 ? 1u : 2u;
      am[m] = (uint32_t)atk;
    } else if (slot[j] >= 0) {
      kd[m] = ORX_NPC_OUT_ATTACK_NPC | (nhp[j] > 0 && atk >= nhp[j] ? ORX_NPC_OUT_LETHAL : 0);
      tg[m] = (uint32_t)(3 + slot[j]);
      am[m] = (uint32_t)atk;
    } else {
      kd[m] = stair[j] ? ORX_NPC_OUT_STAIRS : ORX_NPC_OUT_STEP;
    }
  }
  store_options(a, row, kd, tg, am);
}

__global__ __launch_bounds__(kBlock) void seek_kernel(const SeekArgs a) {
  const GameArgs& g = a.g;
  const int64_t B = g.B;
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const int k = (int)blockIdx.y;
  const int64_t row = (int64_t)k * B + b;

  // kAbsent above kNoPath above every distance: the nearer player is the lesser
  uint32_t reach[2] = {kAbsent, kAbsent}, move[2] = {ORX_MOVE_STAY, ORX_MOVE_STAY};
  const Depth d = depth_of(g, b);
  if (alive_bit(g, k, b) && d.state == ORX_NPC_DEPTH_WATCHED) {
    const uint32_t own = g.npc_pos[row];
    Seeker s;
    s.W = g.W, s.H = g.H;
    s.x = (int)(own & 0xFFu), s.y = (int)(own >> 8);
    s.sx = s.sy = -1, s.table = nullptr, s.tiles = nullptr;
    if (g.L > 0) {
      size_t lay;
      s.tiles = layout_tiles(g, d, lay);
      const size_t WH = (size_t)(g.W * g.H);
      s.table = a.pairs + lay * WH * WH;
    } else {
      s.sx = g.st_x[d.row], s.sy = g.st_y[d.row];
    }
    if (s.inside(s.x, s.y)) {  // (a cell outside the grid has no targets)
      const bool on[2] = {d.on1, d.on2};
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        if (!on[p]) continue;
        const int px = g.p_x[(int64_t)p * B + b], py = g.p_y[(int64_t)p * B + b];
        reach[p] = s.inside(px, py) ? s.between(s.x, s.y, px, py) : kNoPath;
        move[p] = s.move_to(reach[p], px, py);
      }
    }
  }

  const int near = reach[1] < reach[0] ? 1 : 0;  // (player 1 wins a tie)
  uint32_t dist[3], mv[3], target[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int p = j < 2 ? j : near;
    dist[j] = (uint32_t)(reach[p] == kAbsent   ? ORX_SEEK_ABSENT
                         : reach[p] == kNoPath ? ORX_SEEK_UNREACHABLE
                                               : (int32_t)reach[p]);
    mv[j] = move[p];
    target[j] = reach[p] == kAbsent ? 0xFFFFu : (uint32_t)(p + 1);
  }

  // a lane's row of each output: one store
  store_seek_rows(a.dist, a.move, row, dist[0], dist[1], dist[2], mv[0], mv[1], mv[2]);
  if (a.target)
    reinterpret_cast<uint2*>(a.target)[row] =
        make_uint2(target[0] | target[1] << 16, target[2] | 0xFFFFu << 16);
}

// the refusals both entry points share, and the game's part of the arguments
inline int game_args(const char* fn, const orx_cfg_t* cfg, const orx_state_t* st, int64_t n_games,
                     uint32_t needs, GameArgs& g) {
  int r;
  if ((r = orx_validate_cfg(cfg))) return r;
  if (cfg->n_npcs <= 0) return fail_in(fn, "needs a configuration with NPCs (n_npcs > 0)");
  if ((r = check_games(fn, n_games)) || (r = check_state(cfg, st, needs))) return r;
  g.p_x = st->p_x, g.p_y = st->p_y, g.p_depth = st->p_depth, g.p_health = st->p_health;
  g.st_x = st->st_x, g.st_y = st->st_y;
  g.npc_pos = st->npc_pos, g.npc_health = st->npc_health, g.npc_alive = st->npc_alive;
  g.npc_grid = st->npc_grid;
  g.p_layout = st->p_layout, g.bank_tiles = st->bank_tiles;
  g.B = n_games;
  g.W = cfg->width, g.H = cfg->height, g.K = cfg->n_npcs, g.L = cfg->n_layouts;
  g.npc_depth = npc_depth(cfg);
  g.unreachable = cfg->despawn == ORX_DESPAWN_UNREACHABLE ? 1 : 0;
  return ORX_OK;
}

inline dim3 lanes(const GameArgs& g) {
  return dim3((unsigned)((g.B + kBlock - 1) / kBlock), (unsigned)g.K);
}

}  // namespace orx_npc_query_dev

#ifndef ORX_NPC_QUERY_BUILD_ID
#define ORX_NPC_QUERY_BUILD_ID "unknown"
#endif

extern "C" const char* orx_npc_query_build_id(void) { return ORX_NPC_QUERY_BUILD_ID; }

extern "C" int orx_npc_options(const orx_cfg_t* cfg, const orx_state_t* st, uint8_t* kind,
                               int16_t* target, int16_t* amount, uint8_t* where, int64_t n_games,
                               void* stream) {
  using namespace orx_npc_query_dev;
  using orx_dev::fail;
  int r;
  OptionsArgs a;
  if ((r = game_args("orx_npc_options", cfg, st, n_games,
                     kPlayers | kStairsNoBank | kBank | kNpcs | kGrid, a.g)))
    return r;
  if (!kind) return fail(ORX_EINVAL, "orx_npc_options: kind is NULL");
  // (a row is one vector store)
  if (misaligned(kind, 8) || misaligned(target, 16) || misaligned(amount, 16))
    return fail(ORX_EINVAL,
                "orx_npc_options: kind must be 8-byte, target and amount 16-byte aligned");
  a.kind = kind, a.target = target, a.amount = amount, a.where = where;
  const int64_t atk = (int64_t)cfg->npc_damage - (int64_t)cfg->npc_armor;  // (updater.py:313)
  a.attack = (int32_t)(atk < 0 ? 0 : atk > 32767 ? 32767 : atk);
  hipLaunchKernelGGL(options_kernel, lanes(a.g), dim3(kBlock), 0, (hipStream_t)stream, a);
  return orx_dev::launch_status("orx_npc_options");
}

extern "C" int orx_npc_seek(const orx_cfg_t* cfg, const orx_state_t* st, const uint16_t* pairs,
                            int32_t* dist, int8_t* move, int16_t* target, int64_t n_games,
                            void* stream) {
  using namespace orx_npc_query_dev;
  using orx_dev::fail;
  int r;
  SeekArgs a;
  if ((r = game_args("orx_npc_seek", cfg, st, n_games, kStairsNoBank | kBank | kNpcs, a.g)))
    return r;
  if (!st->p_depth) return fail(ORX_EINVAL, "a required state pointer is NULL");
  if (!dist && !move && !target)
    return fail(ORX_EINVAL, "orx_npc_seek: dist, move and target are all NULL");
  if (misaligned(dist, 16) || misaligned(move, 4) || misaligned(target, 8))
    return fail(ORX_EINVAL,
                "orx_npc_seek: dist must be 16-byte, move 4-byte and target 8-byte aligned");
  if (cfg->n_layouts > 0 && !pairs) return fail(ORX_EINVAL, "orx_npc_seek: n_layouts > 0 needs pairs");
  a.pairs = cfg->n_layouts > 0 ? pairs : nullptr;
  a.dist = dist, a.move = move, a.target = target;
  hipLaunchKernelGGL(seek_kernel, lanes(a.g), dim3(kBlock), 0, (hipStream_t)stream, a);
  return orx_dev::launch_status("orx_npc_seek");
}
