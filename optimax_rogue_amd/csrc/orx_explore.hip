// orx_explore.hip -- the map a player remembers and the way to its edge
// (include/orx_explore.h) for gfx950.
//
// Two kernels, neither of which needs the tick machinery: only orx.h's structs,
// the queries' shared headers and the host side's error path.  The room distance
// is orx_seek.h's, as are the key's rule, the wave's minimum, the dist / move
// stores and the host side's refusals.  seek_kernel keeps its own Dungeon (the
// tile, the table lookup by flat cell, the first-move test over eight lanes)
// and its frontier words inline: lifted into Seeker and frontier_bits they cost
// the kernel 1-2%.
//
// update_kernel.  A THREAD IS A WINDOW ROW.  A workgroup of 256 threads takes 64
// consecutive games (their maps, row words and planes are contiguous), and
//   1. one lane per game reads the viewer, the state's (episode, depth, tick)
//      and the key row (one 16-byte load) and decides whether the key is valid;
//   2. the maps of the games whose key is not are zeroed, all threads striding
//      one map at a time (rare: a descent or a new episode);
//   3. a thread per window row: the row word, clipped to the grid's columns,
//      is shifted by px - radius as 64 bits into at most two map words; a word
//      is stored only where it gains bits; popcounts of the new bits go to the
//      game's counter in LDS.  The thread keeps the seen and the known bits of
//      its row in window coordinates (LDS) for step 5;
//   4. one lane per game stores `gained` and the new key row;
//   5. the planes are rewritten in place from those two words per row: 16
//      bytes per lane while the plane is 16-byte aligned (64 games: every
//      workgroup's slice then starts aligned), byte by byte otherwise.
// Rows of one game are rows of different y: no two threads touch one map word.
//
// seek_kernel.  A WAVE IS A GAME: its map is staged in LDS (H * WW words) and
// the lanes stride its WORDS.  A word that is zero -- most of a map, most of an
// episode -- costs one LDS read; of any other, the word above, the word below
// and its own bits shifted either way say in four ANDs which of its 32 cells
// have an unknown neighbour.  Only the known cells are then visited (their tile
// read from the layout, which every game of the layout shares), and only a
// target reads its distance, an entry of own's row of the pair table.  (The
// first form scanned all W * H cells against the whole row, coalesced: 8 KiB a
// game at 64 x 64 whatever the map held; profiles/explore.)  The two minima
// are packed words dist << 16 | cell (both parts below 2^16), reduced across
// the wave; then lanes 0..7 each try one neighbour of one column for the move.
// Plain C++ and vector stores only.
#include "../../include/orx_explore.h"
#include "orx_query.h"
#include "orx_seek.h"

namespace orx_explore_dev {

using namespace orx_query;

constexpr int kGames = 64;  // games per workgroup of update_kernel
constexpr uint32_t kFar = ORX_PATH_UNREACHABLE;  // the distance part of a packed word without a walk
constexpr uint32_t kNone = 0xFFFFFFFFu;  // a column without a target (above every packed word)

enum { H_PX, H_PY, H_VALID, H_KNOWN, H_GAIN, kHdr };  // per game ([kHdr][G] int32 in LDS)

// a coordinate held to where the window arithmetic cannot overflow
__device__ __forceinline__ int tame(int v) { return v < -64 ? -64 : v > (1 << 20) ? (1 << 20) : v; }

struct UpdateArgs {
  const int32_t *p_x, *p_y, *p_depth, *tick, *episode;
  const uint32_t* rows;
  uint32_t* memory;
  int32_t* key;
  int32_t* gained;
  uint8_t* cells;
  uint8_t* health;
  int64_t B;
  int32_t W, H, WW, R, G, player;
  uint32_t inv_vv, inv_v;  // (R, G, inv_vv, inv_v: a Window)
};

// four view codes under four seen and four known bits (seen cells are known)
__device__ __forceinline__ uint32_t remember4(uint32_t w, uint32_t seen, uint32_t known) {
  const uint32_t s = spread4(seen) * 0xFFu, k = spread4(known) * 0xFFu;
  constexpr uint32_t kSeen = (ORX_SIGHT_SEEN | ORX_EXPLORE_KNOWN) * 0x01010101u;
  constexpr uint32_t kKnown = ORX_EXPLORE_KNOWN * 0x01010101u;
  constexpr uint32_t kTile = ORX_VIEW_TILE_MASK * 0x01010101u;
  return ((w | kSeen) & s) | (((w & kTile) | kKnown) & k & ~s);
}

// plane[0 .. n) (a workgroup's cells, in place).  kCells: the view codes, else
// the health plane (kept where seen)
template <bool kCells>
__device__ __forceinline__ void remember_plane(const uint32_t* seen, const uint32_t* known,
                                               uint8_t* plane, int n, const Window& win, int t) {
  const int V = win.V;
  const int nvec = ((reinterpret_cast<uintptr_t>(plane) & 15) == 0) ? n >> 4 : 0;
  uint4* q = reinterpret_cast<uint4*>(plane);
  for (int v = t; v < nvec; v += kBlock) {
    const Window::Cell first = win.split((uint32_t)v << 4);
    const int row = first.g * V + first.j;
    const uint32_t s = gather16(seen, row, first.i, V);
    uint4 w = q[v];
    if (kCells) {
      const uint32_t k = gather16(known, row, first.i, V);
      w.x = remember4(w.x, s, k);
      w.y = remember4(w.y, s >> 4, k >> 4);
      w.z = remember4(w.z, s >> 8, k >> 8);
      w.w = remember4(w.w, s >> 12, k >> 12);
    } else {
      w.x &= spread4(s) * 0xFFu, w.y &= spread4(s >> 4) * 0xFFu;
      w.z &= spread4(s >> 8) * 0xFFu, w.w &= spread4(s >> 12) * 0xFFu;
    }
    q[v] = w;
  }
  for (int c = (nvec << 4) + t; c < n; c += kBlock) {
    const Window::Cell at = win.split((uint32_t)c);
    const int row = at.g * V + at.j;
    const bool s = (seen[row] >> at.i) & 1u, k = (known[row] >> at.i) & 1u;
    const uint32_t w = plane[c];
    if (kCells)
      plane[c] = (uint8_t)(s ? w | ORX_SIGHT_SEEN | ORX_EXPLORE_KNOWN
                             : k ? (w & ORX_VIEW_TILE_MASK) | ORX_EXPLORE_KNOWN : 0u);
    else
      plane[c] = (uint8_t)(s ? w : 0u);
  }
}

__global__ __launch_bounds__(kBlock) void update_kernel(const UpdateArgs a) {
  extern __shared__ uint4 smem[];
  const Window win = Window::of(a.R, a.G, a.inv_vv, a.inv_v);
  const int G = win.G, R = win.R, V = win.V, VV = win.VV, W = a.W, H = a.H, WW = a.WW;
  uint32_t* seen = reinterpret_cast<uint32_t*>(smem);  // [G * V] row words: seen now, in the grid
  uint32_t* known = seen + G * V;                      // ... known after this call
  int32_t* hdr = reinterpret_cast<int32_t*>(known + G * V);
  const int64_t B = a.B;
  const int64_t b0 = (int64_t)blockIdx.x * G;
  const int nb = (int)((B - b0) < (int64_t)G ? (B - b0) : (int64_t)G);
  const int t = threadIdx.x;
  const size_t map_words = (size_t)H * (size_t)WW;
  uint32_t* maps = a.memory + (size_t)b0 * map_words;  // the workgroup's nb maps

  // 1. the viewers and the keys, coalesced over the games
  int32_t ep = 0, depth = 0, tick = 0;
  if (t < nb) {
    const int64_t b = b0 + t, me = player_rows(a.player, B, b).me;
    ep = a.episode[b], depth = a.p_depth[me], tick = a.tick[b];
    const int4 k = reinterpret_cast<const int4*>(a.key)[b];
    const bool ok = key_valid(k, ep, depth, tick);
    hdr[H_PX * G + t] = tame(a.p_x[me]);
    hdr[H_PY * G + t] = tame(a.p_y[me]);
    hdr[H_VALID * G + t] = ok;
    hdr[H_KNOWN * G + t] = ok ? k.w : 0;
    hdr[H_GAIN * G + t] = 0;
  }
  __syncthreads();

  // 2. a map whose key is not valid starts empty
  for (int g = 0; g < nb; ++g) {
    if (hdr[H_VALID * G + g]) continue;
    uint32_t* m = maps + (size_t)g * map_words;
    for (size_t i = t; i < map_words; i += kBlock) m[i] = 0u;
  }
  __syncthreads();  // (the zeros are in memory before step 3 stores into those maps)

  // 3. one thread per window row
  const uint32_t vmask = (1u << V) - 1u;
  const int nrows = nb * V;
  for (int row = t; row < nrows; row += kBlock) {
    const int g = win.div_v((uint32_t)row), j = row - g * V;
    const int px = hdr[H_PX * G + g], y = hdr[H_PY * G + g] + j - R;
    uint32_t s = 0, k = 0;
    if (y >= 0 && y < H) {
      const uint32_t in = grid_columns(px, W, R, V);
      s = a.rows[(size_t)b0 * (size_t)V + (size_t)row] & vmask & in;
      if (in) {
        // window column lo is grid column xs, the first of the row in the grid
        const int x0 = px - R, lo = x0 < 0 ? -x0 : 0, xs = x0 < 0 ? 0 : x0;
        const int w0 = xs >> 5, sh = xs & 31;
        const uint64_t v = (uint64_t)(s >> lo) << sh;
        const bool two = w0 + 1 < WW;  // (in != 0: xs < W, so w0 < WW)
        const bool kept = hdr[H_VALID * G + g];
        uint32_t* m = maps + ((size_t)g * (size_t)H + (size_t)y) * (size_t)WW + (size_t)w0;
        const uint32_t old0 = kept ? m[0] : 0u, old1 = kept && two ? m[1] : 0u;
        // (s is clipped to x < W: the high word has bits only where the map has that word)
        const uint32_t new0 = (uint32_t)v & ~old0, new1 = two ? (uint32_t)(v >> 32) & ~old1 : 0u;
        if (new0) m[0] = old0 | new0;
        if (new1) m[1] = old1 | new1;
        const int gain = __popc(new0) + __popc(new1);
        if (gain) atomicAdd(&hdr[H_GAIN * G + g], gain);
        const uint64_t now = (uint64_t)(old1 | new1) << 32 | (uint64_t)(old0 | new0);
        k = ((uint32_t)(now >> sh) << lo) & vmask & in;
      }
    }
    seen[row] = s;
    known[row] = k;
  }
  __syncthreads();

  // 4. the counts and the keys
  if (t < nb) {
    const int64_t b = b0 + t;
    const int gain = hdr[H_GAIN * G + t];
    if (a.gained) a.gained[b] = gain;
    reinterpret_cast<int4*>(a.key)[b] = make_int4(ep, depth, tick, hdr[H_KNOWN * G + t] + gain);
  }

  // 5. the planes, rewritten in place
  const size_t off = (size_t)b0 * (size_t)VV;
  if (a.cells) remember_plane<true>(seen, known, a.cells + off, nb * VV, win, t);
  if (a.health) remember_plane<false>(seen, known, a.health + off, nb * VV, win, t);
}

// ---------------------------------------------------------------------------
// seek: the nearest frontier cell and the nearest known staircase
// ---------------------------------------------------------------------------
struct SeekArgs {
  const int32_t *p_x, *p_y, *p_depth, *tick, *episode, *st_x, *st_y;
  const int16_t* p_layout;
  const uint8_t* bank_tiles;
  const uint16_t* pairs;
  const uint32_t* memory;
  const int32_t* key;
  int32_t* dist;
  int8_t* move;
  int32_t* target;
  int64_t B;
  int32_t W, H, WW, L, player, G;
  uint32_t inv_h;  // recip(H): __umulhi(c, inv_h) = c / H for a flat cell c
};

// One game's viewer on its dungeon: the tiles and the distances, kFar where
// there is no walk.
struct Dungeon {
  int W, H, sx, sy;
  const uint16_t* table;  // pairs[layout], or nullptr: the closed form
  const uint8_t* tiles;   // bank_tiles[layout], with the table

  __device__ __forceinline__ bool inside(int cx, int cy) const {
    return (uint32_t)cx < (uint32_t)W && (uint32_t)cy < (uint32_t)H;
  }
  // the Tile code of a cell of the grid (a bank's may carry 0: no tile at all)
  __device__ __forceinline__ uint32_t tile(int cx, int cy) const {
    if (tiles) return tiles[cx * H + cy] & ORX_VIEW_TILE_MASK;
    // EmptyDungeonGenerator (worldgen.py:33-43): the border is Wall
    if (cx == 0 || cx == W - 1 || cy == 0 || cy == H - 1) return ORX_TILE_WALL;
    return cx == sx && cy == sy ? ORX_TILE_STAIRCASE_DOWN : ORX_TILE_GROUND;
  }
  // the closed form's distance between two cells of the grid
  __device__ __forceinline__ uint32_t closed(int ax, int ay, int tx, int ty) const {
    return room<kFar>(W, H, sx, sy, ax, ay, tx, ty);
  }
  // ... from cell (ax, ay) to the cell whose table row is `row` (flat cell tc)
  __device__ __forceinline__ uint32_t between(int ax, int ay, int tc, int tx, int ty) const {
    if (!table) return closed(ax, ay, tx, ty);
    const uint32_t v = table[(size_t)tc * (size_t)(W * H) + (size_t)(ax * H + ay)];
    return v >= kFar ? kFar : v;
  }
};

__global__ __launch_bounds__(kBlock) void seek_kernel(const SeekArgs a) {
  extern __shared__ uint4 smem[];
  const int W = a.W, H = a.H, WW = a.WW, WH = W * H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t B = a.B, b = (int64_t)blockIdx.x * a.G + wave;
  const int map_words = H * WW;
  uint32_t* map = reinterpret_cast<uint32_t*>(smem) + (size_t)wave * (size_t)map_words;
  const bool live = b < B;
  if (live) {
    const uint32_t* src = a.memory + (size_t)b * (size_t)map_words;
    for (int i = lane; i < map_words; i += 64) map[i] = src[i];
  }
  __syncthreads();
  if (!live) return;

  const int64_t me = player_rows(a.player, B, b).me;
  const int x = a.p_x[me], y = a.p_y[me];
  Dungeon s;
  s.W = W, s.H = H, s.sx = s.sy = -1, s.table = nullptr, s.tiles = nullptr;
  if (a.L > 0) {
    const size_t lay = (size_t)layout_of(a, me);
    s.table = a.pairs + lay * (size_t)WH * (size_t)WH;
    s.tiles = a.bank_tiles + lay * (size_t)WH;
  } else {
    s.sx = a.st_x[me], s.sy = a.st_y[me];
  }
  const bool valid = key_valid(reinterpret_cast<const int4*>(a.key)[b], a.episode[b],
                               a.p_depth[me], a.tick[b]);
  // the scan, a map word at a time: dist << 16 | cell of the nearest target of
  // each column.  A cell off the grid counts as known (it is no one's frontier).
  uint32_t best[2] = {kNone, kNone};
  if (valid && s.inside(x, y)) {
    const int own = x * H + y;
    const uint16_t* row = s.table ? s.table + (size_t)own * (size_t)WH : nullptr;
    const int last_word = (W - 1) >> 5;
    const uint32_t last_bit = 1u << ((W - 1) & 31);
    for (int w = lane; w < map_words; w += 64) {
      uint32_t bits = map[w];
      if (!bits) continue;
      const int cy = w / WW, xw = w - cy * WW;
      if (xw == last_word) bits &= (last_bit << 1) - 1u;  // (whatever the caller left at x >= W)
      const uint32_t up = cy > 0 ? map[w - WW] : ~0u, down = cy < H - 1 ? map[w + WW] : ~0u;
      const uint32_t left = bits << 1 | (xw > 0 ? map[w - 1] >> 31 : 1u);
      const uint32_t right = bits >> 1 | (xw < last_word ? map[w + 1] << 31 : last_bit);
      const uint32_t edge = bits & ~(up & down & left & right);  // an unknown neighbour in the grid
      for (uint32_t rest = bits; rest; rest &= rest - 1u) {
        const int i = __builtin_ctz(rest), cx = xw * 32 + i, c = cx * H + cy;
        const uint32_t tile = s.tile(cx, cy);
        int col;
        if (tile == ORX_TILE_GROUND) {
          if (!((edge >> i) & 1u)) continue;
          col = ORX_EXPLORE_FRONTIER;
        } else if (tile == ORX_TILE_STAIRCASE_DOWN) {
          col = ORX_EXPLORE_STAIRS;
        } else {
          continue;
        }
        uint32_t d = row ? (uint32_t)row[c] : s.closed(x, y, cx, cy);
        d = d >= kFar ? kFar : d;
        const uint32_t packed = d << 16 | (uint32_t)c;
        best[col] = packed < best[col] ? packed : best[col];
      }
    }
  }
  best[0] = wave_min(best[0]);
  best[1] = wave_min(best[1]);

  // the move: lane 4 * col + j tries neighbour j (Up, Right, Down, Left)
  bool step = false;
  if (lane < 8) {
    const uint32_t p = best[lane >> 2], d = p >> 16;
    if (p != kNone && d != kFar && d > 0u) {
      const int j = lane & 3, tc = (int)(p & 0xFFFFu);
      const int tx = (int)__umulhi((uint32_t)tc, a.inv_h), ty = tc - tx * H;
      const int nx = x + (j == 1) - (j == 3), ny = y + (j == 2) - (j == 0);
      step = s.inside(nx, ny) && s.between(nx, ny, tc, tx, ty) == d - 1u &&
             !(s.tile(nx, ny) == ORX_TILE_STAIRCASE_DOWN && !(nx == tx && ny == ty));
    }
  }
  const uint32_t steps = (uint32_t)__ballot(step) & 0xFFu;
  if (lane != 0) return;

  uint32_t dist[2], move[2], target[2];
#pragma unroll
  for (int col = 0; col < 2; ++col) {
    const uint32_t p = best[col], d = p >> 16, nib = (steps >> (4 * col)) & 15u;
    dist[col] = (uint32_t)(p == kNone ? ORX_SEEK_ABSENT : d == kFar ? ORX_SEEK_UNREACHABLE : (int32_t)d);
    move[col] = nib ? (uint32_t)(ORX_MOVE_UP + __builtin_ctz(nib)) : (uint32_t)ORX_MOVE_STAY;
    target[col] = p == kNone ? 0xFFFFFFFFu : (p & 0xFFFFu);
  }
  store_seek_rows(a.dist, a.move, b, dist[0], dist[1], (uint32_t)ORX_SEEK_ABSENT, move[0], move[1],
                  ORX_MOVE_STAY);
  if (a.target)
    reinterpret_cast<uint4*>(a.target)[b] = make_uint4(target[0], target[1], 0xFFFFFFFFu, 0xFFFFFFFFu);
}

}  // namespace orx_explore_dev

#ifndef ORX_EXPLORE_BUILD_ID
#define ORX_EXPLORE_BUILD_ID "unknown"
#endif

extern "C" const char* orx_explore_build_id(void) { return ORX_EXPLORE_BUILD_ID; }

extern "C" int orx_explore_update(const orx_cfg_t* cfg, const orx_state_t* st, int32_t player,
                                  int32_t radius, const uint32_t* rows, uint32_t* memory,
                                  int32_t* key, int32_t* gained, uint8_t* cells, uint8_t* health,
                                  int64_t n_games, void* stream) {
  using namespace orx_explore_dev;
  using orx_dev::fail;
  int r;
  if ((r = orx_validate_cfg(cfg)) || (r = check_player("orx_explore_update", player))) return r;
  if (radius < 1 || radius > ORX_VIEW_MAX_RADIUS)
    return fail(ORX_EINVAL, "orx_explore_update: radius must be in [1, ORX_VIEW_MAX_RADIUS]");
  if (!rows || !memory || !key)
    return fail(ORX_EINVAL, "orx_explore_update: rows, memory or key is NULL");
  if (misaligned(rows, 4) || misaligned(memory, 4) || misaligned(gained, 4) || misaligned(key, 16))
    return fail(ORX_EINVAL,
                "orx_explore_update: rows, memory and gained must be 4-byte, key 16-byte aligned");
  if ((r = check_games("orx_explore_update", n_games)) || (r = check_state(cfg, st, 0))) return r;
  if (!st->p_depth || !st->tick || !st->episode)
    return fail(ORX_EINVAL, "a required state pointer is NULL");

  UpdateArgs a;
  a.p_x = st->p_x, a.p_y = st->p_y, a.p_depth = st->p_depth;
  a.tick = st->tick, a.episode = st->episode;
  a.rows = rows, a.memory = memory, a.key = key, a.gained = gained;
  a.cells = cells, a.health = health;
  a.B = n_games;
  a.W = cfg->width, a.H = cfg->height, a.WW = (cfg->width + 31) / 32;
  a.player = player;
  const Window win = Window::fit(radius, 0, kGames);  // (no tiles: always kGames games)
  const int G = win.G;
  a.R = win.R, a.G = G, a.inv_vv = win.inv_vv, a.inv_v = win.inv_v;
  const size_t lds = sizeof(uint32_t) * (size_t)G * (size_t)(2 * win.V + kHdr);
  const unsigned grid = (unsigned)((n_games + G - 1) / G);
  hipLaunchKernelGGL(update_kernel, dim3(grid), dim3(kBlock), lds, (hipStream_t)stream, a);
  return orx_dev::launch_status("orx_explore_update");
}

extern "C" int orx_explore_seek(const orx_cfg_t* cfg, const orx_state_t* st, const uint16_t* pairs,
                                int32_t player, const uint32_t* memory, const int32_t* key,
                                int32_t* dist, int8_t* move, int32_t* target, int64_t n_games,
                                void* stream) {
  using namespace orx_explore_dev;
  using orx_dev::fail;
  int r;
  if ((r = orx_validate_cfg(cfg)) || (r = check_player("orx_explore_seek", player))) return r;
  if ((r = check_memory_rows("orx_explore_seek", memory, key, dist, move, target)) ||
      (r = check_memory_query("orx_explore_seek", cfg, st, n_games)))
    return r;
  if (cfg->n_layouts > 0 && !pairs)
    return fail(ORX_EINVAL, "orx_explore_seek: n_layouts > 0 needs pairs");

  SeekArgs a;
  a.p_x = st->p_x, a.p_y = st->p_y, a.p_depth = st->p_depth;
  a.tick = st->tick, a.episode = st->episode, a.st_x = st->st_x, a.st_y = st->st_y;
  a.p_layout = st->p_layout, a.bank_tiles = st->bank_tiles;
  a.pairs = cfg->n_layouts > 0 ? pairs : nullptr;
  a.memory = memory, a.key = key;
  a.dist = dist, a.move = move, a.target = target;
  a.B = n_games;
  a.W = cfg->width, a.H = cfg->height, a.WW = (cfg->width + 31) / 32, a.L = cfg->n_layouts;
  a.player = player;
  a.inv_h = recip(cfg->height);
  // a wave per game, its map in LDS
  // (W * H <= 65536 and W >= 4: one map is at most 64 KiB, the default limit)
  const size_t map_bytes = sizeof(uint32_t) * (size_t)a.H * (size_t)a.WW;
  const int G = a.G = games_per_workgroup(map_bytes);
  const unsigned grid = (unsigned)((n_games + G - 1) / G);
  hipLaunchKernelGGL(seek_kernel, dim3(grid), dim3(64 * G), (size_t)G * map_bytes,
                     (hipStream_t)stream, a);
  return orx_dev::launch_status("orx_explore_seek");
}
