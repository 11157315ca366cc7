// orx_query.h -- what orx_view.hip, orx_path.hip and orx_moves.hip share: each
// a read-only query of the resident state for one player of every game.
// Internal to csrc/ (the C-ABI is include/*.h) and header-only.
#ifndef ORX_QUERY_H_
#define ORX_QUERY_H_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/orx.h"

// the host side's error path (orx_engine.hip, "Host side of the C-ABI")
namespace orx_dev {
int fail(int code, const char* msg);
int launch_status(const char* what);
}  // namespace orx_dev

namespace orx_query {

constexpr int kBlock = 256;
constexpr int kTileBudget = 40 * 1024;  // LDS bytes of a workgroup's tiles (all planes)

// 2^32 / d + 1, the reciprocal the kernels divide by: __umulhi(n, recip(d)) ==
// n / d while n * d < 2^32, which holds for n < 2^16 and d <= 2^16.  (recip(d)
// = (2^32 + e) / d with 0 < e <= d, so n recip(d) / 2^32 = n / d + n e / (d 2^32):
// above n / d by less than 1 / d while n e < 2^32, too little to reach the next integer.)
inline uint32_t recip(int d) { return (uint32_t)(0x100000000ULL / (uint64_t)d) + 1u; }

// The window: V x V cells around the player, G games per workgroup.  (The
// kernels' argument blocks keep R, G and the reciprocals where they were --
// the layout is part of the device code -- and the kernel calls `of`.)
struct Window {
  int32_t R, V, VV, G;
  uint32_t inv_vv, inv_v;  // recip(VV) and recip(V)

  __host__ __device__ __forceinline__ static Window of(int R, int G, uint32_t inv_vv,
                                                       uint32_t inv_v) {
    const int V = 2 * R + 1;
    return {R, V, V * V, G, inv_vv, inv_v};
  }
  // G: the most of 64, 32, 16 (`cap` at most) whose tiles, `cell_bytes` of LDS
  // per window cell over all planes, fit kTileBudget.  (A multiple of 16: a
  // workgroup's G * VV cells are whole uint4s at a 16-byte aligned offset.)
  static Window fit(int radius, int cell_bytes, int cap = 64) {
    const int V = 2 * radius + 1, VV = V * V;
    int G = cap;
    while (G > 16 && G * VV * cell_bytes > kTileBudget) G >>= 1;
    return of(radius, G, recip(VV), recip(V));
  }

  __device__ __forceinline__ int div_v(uint32_t n) const { return (int)__umulhi(n, inv_v); }
  // flat cell index c (< 2^16) of a workgroup's tile -> game g, row j, column i
  struct Cell { int g, j, i; };
  __device__ __forceinline__ Cell split(uint32_t c) const {
    const int g = (int)__umulhi(c, inv_vv);
    const uint32_t r = c - (uint32_t)(g * VV);
    const int j = div_v(r);
    return {g, j, (int)r - j * V};
  }
};

// the window columns that lie in the grid's x range, as row-word bits (bit i:
// window column i of a viewer at x = px)
__device__ __forceinline__ uint32_t grid_columns(int px, int W, int R, int V) {
  const int i0 = R - px, i1 = W - 1 - px + R;  // window columns of x = 0 and x = W - 1
  const int lo = i0 > 0 ? i0 : 0, hi = i1 < V - 1 ? i1 : V - 1;
  return lo <= hi ? ((2u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}

// bits [i, i + 16) of the window's flat cell sequence starting at row `row`,
// column `i`, out of per-row words: the cells run over a row's end into the next
__device__ __forceinline__ uint32_t gather16(const uint32_t* words, int row, int i, int V) {
  uint32_t bits = 0;
  int filled = 0;
  while (filled < 16) {
    const int take = V - i < 16 - filled ? V - i : 16 - filled;
    bits |= ((words[row] >> i) & ((1u << take) - 1u)) << filled;
    filled += take;
    i = 0;
    ++row;
  }
  return bits;
}

// bits 0..3 of n -> the low bit of bytes 0..3 (times 0xFF: all of their bits)
__device__ __forceinline__ uint32_t spread4(uint32_t n) {
  return ((n & 15u) * 0x00204081u) & 0x01010101u;
}

// tile[0 .. n) (LDS, 16-byte aligned) -> out[0 .. n): 16 bytes per lane while
// out is 16-byte aligned, the rest (all of it, if out is not) element by element.
// t: the thread's index among the kThreads that stream (a workgroup; a wave
// that owns its tile: 64).
template <typename T, int kThreads = kBlock>
__device__ __forceinline__ void stream_out(const T* tile, T* out, int n, int t) {
  static_assert(sizeof(T) == 1 || sizeof(T) == 2, "1 or 2-byte cells");
  constexpr int kShift = sizeof(T) == 1 ? 4 : 3;  // log2 of the elements per uint4
  const int nvec = ((reinterpret_cast<uintptr_t>(out) & 15) == 0) ? n >> kShift : 0;
  const uint4* src = reinterpret_cast<const uint4*>(tile);
  uint4* dst = reinterpret_cast<uint4*>(out);
  for (int v = t; v < nvec; v += kThreads) dst[v] = src[v];
  for (int i = (nvec << kShift) + t; i < n; i += kThreads) out[i] = tile[i];
}

// a layout index clamped into a bank of L > 0 layouts (the lookup must stay
// inside it), and that of player row `me` of an argument block (0: no bank)
__device__ __forceinline__ int clamp_layout(int lay, int L) {
  return lay < 0 ? 0 : lay >= L ? L - 1 : lay;
}
template <typename Args>
__device__ __forceinline__ int layout_of(const Args& a, int64_t me) {
  if (a.L <= 0) return 0;
  return clamp_layout(a.p_layout[me], a.L);
}

// game b's index in the [2][B] player rows: the asked player's and the other's
struct PlayerRows { int64_t me, ot; };
__device__ __forceinline__ PlayerRows player_rows(int player, int64_t B, int64_t b) {
  return {(int64_t)player * B + b, (int64_t)(1 - player) * B + b};
}

// the depth the NPCs (and the items they drop) are on: player 1's start depth
inline int32_t npc_depth(const orx_cfg_t* cfg) {
  return cfg->start_mode == ORX_START_SEPARATED ? cfg->p1_depth : 0;
}
inline bool has_items(const orx_cfg_t* cfg) {
  return (cfg->flags & ORX_EXT_ITEMS) && cfg->n_npcs > 0;
}

// The entry points' shared refusals (`fn`: the entry point's name).
// p is not a multiple of n, a power of two (a NULL pointer is aligned)
inline bool misaligned(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) & (n - 1); }
inline int fail_in(const char* fn, const char* msg) {
  char buf[128];
  snprintf(buf, sizeof(buf), "%s: %s", fn, msg);
  return orx_dev::fail(ORX_EINVAL, buf);
}
inline int check_player(const char* fn, int32_t player) {
  return player == 0 || player == 1 ? ORX_OK : fail_in(fn, "player must be 0 or 1");
}
inline int check_games(const char* fn, int64_t n_games) {
  return n_games > 0 && n_games <= 0x7FFFFFFFLL ? ORX_OK : fail_in(fn, "bad n_games");
}

// What a query reads besides p_x and p_y (where the configuration has it).
enum : uint32_t {
  kPlayers = 1,       // p_depth, p_health
  kStairs = 2,        // st_x, st_y, whatever the configuration
  kStairsNoBank = 4,  // st_x, st_y without a bank
  kBank = 8,          // p_layout, bank_tiles
  kNpcs = 16,         // npc_pos, npc_health, npc_alive
  kGrid = 32,         // npc_grid (dense NPCs)
  kCharacter = 64,    // p_rpg
  kItems = 128,       // item_pos, item_mask
};
inline int check_state(const orx_cfg_t* cfg, const orx_state_t* st, uint32_t needs) {
  using orx_dev::fail;
  if (!st) return fail(ORX_EINVAL, "state is NULL");
  if (!st->p_x || !st->p_y || ((needs & kPlayers) && (!st->p_depth || !st->p_health)) ||
      ((needs & kStairs) && (!st->st_x || !st->st_y)))
    return fail(ORX_EINVAL, "a required state pointer is NULL");
  if ((needs & kStairsNoBank) && cfg->n_layouts == 0 && (!st->st_x || !st->st_y))
    return fail(ORX_EINVAL, "n_layouts == 0 needs st_x and st_y");
  if ((needs & kBank) && cfg->n_layouts > 0 && (!st->p_layout || !st->bank_tiles))
    return fail(ORX_EINVAL, "n_layouts > 0 needs p_layout and bank_tiles");
  if ((needs & kNpcs) && cfg->n_npcs > 0 && (!st->npc_pos || !st->npc_health || !st->npc_alive))
    return fail(ORX_EINVAL, "n_npcs > 0 needs npc_pos, npc_health and npc_alive");
  if ((needs & kGrid) && cfg->n_npcs > ORX_MAX_REG_NPCS && !st->npc_grid)
    return fail(ORX_EINVAL, "n_npcs > 16 needs npc_grid ([B][W * H] uint8)");
  if ((needs & kCharacter) && (cfg->flags & ORX_EXT_CHARACTER) && !st->p_rpg)
    return fail(ORX_EINVAL, "the character mechanics need p_rpg");
  if ((needs & kItems) && has_items(cfg) && (!st->item_pos || !st->item_mask))
    return fail(ORX_EINVAL, "ORX_EXT_ITEMS needs item_pos and item_mask");
  return ORX_OK;
}

}  // namespace orx_query

#endif  // ORX_QUERY_H_
