// orx_seek.h -- the seek-shaped rules, each defined once: what orx_path.hip
// (orx_path_seek), orx_npc_query.hip (orx_npc_seek), orx_explore.hip
// (orx_explore_seek) and orx_route.hip (orx_route) share beyond orx_query.h.
// Walking distances on a dungeon and the first move along them, the key and the
// frontier of a remembered map, a wave's reductions, the dist / move rows'
// stores, and the host side of the two queries over a remembered map.
// Internal to csrc/ (the C-ABI is include/*.h) and header-only.
#ifndef ORX_SEEK_H_
#define ORX_SEEK_H_

#include "../../include/orx_path.h"
#include "orx_query.h"

namespace orx_query {

constexpr uint32_t kNoPath = 0x7FFFFFFFu;  // a target that cannot be reached (above every distance)

// The walking distance between cells (ax, ay) and (tx, ty) of
// EmptyDungeonGenerator's W x H grid with its staircase at (sx, sy), kNo where
// there is no walk.  Border Wall; an open interior at least two cells wide, so
// only a staircase strictly between two cells of one row or column costs a
// detour, of two moves.  (kNo: orx_explore_seek packs distances into 16 bits
// and asks for ORX_PATH_UNREACHABLE.)
template <uint32_t kNo = kNoPath>
__device__ __forceinline__ uint32_t room(int W, int H, int sx, int sy, int ax, int ay, int tx,
                                         int ty) {
  if (ax < 1 || ax > W - 2 || ay < 1 || ay > H - 2 || tx < 1 || tx > W - 2 || ty < 1 || ty > H - 2)
    return kNo;
  const int dx = ax - tx, dy = ay - ty;
  uint32_t d = (uint32_t)((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy));
  if (dx == 0 && sx == ax && (ay < sy) != (ty < sy) && sy != ay && sy != ty) d += 2u;
  if (dy == 0 && sy == ay && (ax < sx) != (tx < sx) && sx != ax && sx != tx) d += 2u;
  return d;
}

// One game's seeker -- a player (orx_path_seek) or an NPC (orx_npc_seek) -- on
// its dungeon: its cell, and the distances from it.
struct Seeker {
  int W, H, x, y, sx, sy;
  const uint16_t* table;  // pairs[layout], or nullptr: the closed form
  const uint8_t* tiles;   // bank_tiles[layout], with the table

  __device__ __forceinline__ bool inside(int cx, int cy) const {
    return (uint32_t)cx < (uint32_t)W && (uint32_t)cy < (uint32_t)H;
  }
  // A bank's byte is masked with ORX_VIEW_TILE_MASK: orx.h documents
  // bank_tiles as Tile codes, so on every input within the contract the masked
  // and the unmasked byte agree, and a byte outside it is read as orx_view
  // reads it.
  __device__ __forceinline__ bool staircase(int cx, int cy) const {
    return tiles ? (tiles[cx * H + cy] & ORX_VIEW_TILE_MASK) == ORX_TILE_STAIRCASE_DOWN
                 : (cx == sx && cy == sy);
  }
  // the walking distance between cells (ax, ay) and (tx, ty), both in the
  // grid; kNoPath where there is no walk (or a cell is Wall)
  __device__ __forceinline__ uint32_t between(int ax, int ay, int tx, int ty) const {
    if (!table) return room(W, H, sx, sy, ax, ay, tx, ty);
    const uint32_t v = table[(size_t)(tx * H + ty) * (size_t)(W * H) + (size_t)(ax * H + ay)];
    return v >= (uint32_t)ORX_PATH_UNREACHABLE ? kNoPath : v;
  }
  // the first of Up, Right, Down, Left whose cell is at dist - 1 from the
  // target; a staircase counts only as the target's own cell
  __device__ __forceinline__ uint32_t move_to(uint32_t dist, int tx, int ty) const {
    if (dist == 0u || dist >= kNoPath) return ORX_MOVE_STAY;
    const int nx[4] = {x, x + 1, x, x - 1}, ny[4] = {y - 1, y, y + 1, y};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!inside(nx[j], ny[j])) continue;
      if (between(nx[j], ny[j], tx, ty) != dist - 1u) continue;
      if (staircase(nx[j], ny[j]) && !(nx[j] == tx && ny[j] == ty)) continue;
      return (uint32_t)(ORX_MOVE_UP + j);
    }
    return ORX_MOVE_STAY;
  }
};

// whether key row k of a remembered map is valid for a state (orx_explore.h's rule)
__device__ __forceinline__ bool key_valid(const int4 k, int32_t episode, int32_t depth,
                                          int32_t tick) {
  return k.w >= 0 && k.x == episode && k.y == depth && k.z <= tick;
}

// The cells of word i (row y, word xw of the row) of a remembered map that are
// known and have an unknown neighbour in the grid.  k: the caller's known[i],
// clipped to the columns x < W (last_word, last_bit: the word and the bit of
// column W - 1).  A cell off the grid counts as known (it is no one's frontier).
__device__ __forceinline__ uint32_t frontier_bits(const uint32_t* known, uint32_t k, int i, int y,
                                                  int xw, int WW, int H, int last_word,
                                                  uint32_t last_bit) {
  const uint32_t up = y > 0 ? known[i - WW] : ~0u, down = y < H - 1 ? known[i + WW] : ~0u;
  const uint32_t left = k << 1 | (xw > 0 ? known[i - 1] >> 31 : 1u);
  const uint32_t right = k >> 1 | (xw < last_word ? known[i + 1] << 31 : last_bit);
  return k & ~(up & down & left & right);
}

// One step of a bit-parallel search over a plane of H rows of WW words: the
// cells beside those of `cur`, for word i (row y, word xw of the row; c =
// cur[i]) -- the word shifted left and right with the carry bits of the words
// beside it, ORed with the words above and below.  orx_route's search and
// orx_path_ticks' both take their steps with it.
__device__ __forceinline__ uint32_t beside(const uint32_t* cur, uint32_t c, int i, int y, int xw,
                                           int WW, int H) {
  uint32_t nb = c << 1 | c >> 1;
  if (xw > 0) nb |= cur[i - 1] >> 31;
  if (xw < WW - 1) nb |= cur[i + 1] << 31;
  if (y > 0) nb |= cur[i - WW];
  if (y < H - 1) nb |= cur[i + WW];
  return nb;
}

// Word xw of row y of EmptyDungeonGenerator's W x H room as bit planes: the
// border Wall, the rest Ground but for the one staircase (sx, sy) off the
// border.  `in`: the word's columns x < W; last_word, last_bit: the word and
// the bit of column W - 1.
struct RoomWord { uint32_t ground, stair; };
__device__ __forceinline__ RoomWord room_word(int W, int H, int sx, int sy, int y, int xw,
                                              int last_word, uint32_t last_bit, uint32_t in) {
  RoomWord r = {0u, 0u};
  if (y > 0 && y < H - 1) {
    r.ground = in;
    if (xw == 0) r.ground &= ~1u;
    if (xw == last_word) r.ground &= ~last_bit;
    if (y == sy && sx >= 1 && sx <= W - 2 && (sx >> 5) == xw) r.stair = 1u << (sx & 31);
    r.ground &= ~r.stair;
  }
  return r;
}

// the least of a word over the wave
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}

// the wave's LDS stores so far are visible to its loads from here on
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// fn() by the lanes that say `mine`, one after the other, each seeing the LDS
// stores of those before it: how lanes change bits of one word without atomics
template <typename Fn>
__device__ __forceinline__ void lane_by_lane(bool mine, int lane, Fn fn) {
  for (uint64_t m = __ballot(mine); m; m &= m - 1) {
    if (lane == __builtin_ctzll(m)) fn();
    wave_sync();
  }
}

// Row `row` of a seek's dist ([.][ORX_SEEK_COLS] int32) and move
// ([.][ORX_SEEK_COLS] int8) outputs, one store each; the fourth column pads
// the row.  Either pointer may be NULL.
__device__ __forceinline__ void store_seek_rows(int32_t* dist, int8_t* move, int64_t row,
                                                uint32_t d0, uint32_t d1, uint32_t d2,
                                                uint32_t m0, uint32_t m1, uint32_t m2) {
  if (dist)
    reinterpret_cast<uint4*>(dist)[row] = make_uint4(d0, d1, d2, (uint32_t)ORX_SEEK_ABSENT);
  if (move)
    reinterpret_cast<uint32_t*>(move)[row] =
        m0 | m1 << 8 | m2 << 16 | (uint32_t)ORX_MOVE_STAY << 24;
}

// A wave per game: four games to a workgroup, halved while their LDS
// (`bytes_per_game` each) exceeds 32 KiB.
inline int games_per_workgroup(size_t bytes_per_game) {
  int G = 4;
  while (G > 1 && (size_t)G * bytes_per_game > 32 * 1024) G >>= 1;
  return G;
}

// The refusals the queries over a remembered map share (orx_explore_seek,
// orx_route), after the configuration's and the player's: the pointers first,
// then the games, the grid and the state (orx_route has one of its own between).
inline int check_memory_rows(const char* fn, const uint32_t* memory, const int32_t* key,
                             const int32_t* dist, const int8_t* move, const int32_t* target) {
  if (!memory || !key) return fail_in(fn, "memory or key is NULL");
  if (misaligned(memory, 4) || misaligned(key, 16))
    return fail_in(fn, "memory must be 4-byte and key 16-byte aligned");
  if (!dist && !move && !target) return fail_in(fn, "dist, move and target are all NULL");
  // (a row is one vector store)
  if (misaligned(dist, 16) || misaligned(move, 4) || misaligned(target, 16))
    return fail_in(fn, "dist and target must be 16-byte and move 4-byte aligned");
  return ORX_OK;
}
inline int check_memory_query(const char* fn, const orx_cfg_t* cfg, const orx_state_t* st,
                              int64_t n_games) {
  int r;
  if ((r = check_games(fn, n_games))) return r;
  if ((int64_t)cfg->width * cfg->height > 65536)
    return fail_in(fn, "a flat cell must fit 16 bits (W * H <= 65536)");
  if ((r = check_state(cfg, st, kStairsNoBank | kBank))) return r;
  if (!st->p_depth || !st->tick || !st->episode)
    return orx_dev::fail(ORX_EINVAL, "a required state pointer is NULL");
  return ORX_OK;
}

}  // namespace orx_query

#endif  // ORX_SEEK_H_
