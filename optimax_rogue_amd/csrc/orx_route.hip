// orx_route.hip -- walking distances over the map a player remembers
// (include/orx_route.h) for gfx950.
//
// planes_kernel.  A thread is one word of a layout's two bit planes (Ground,
// StaircaseDown), in the remembered map's own layout: one bank, once.
//
// route_kernel.  A WAVE IS A GAME, and the search is bit-parallel: the reached
// set is a bit plane in LDS (H * WW words, as the map), and one step over a
// row word is the word shifted left and right with the carry bits of the words
// beside it, ORed with the words above and below, ANDed with the passable
// cells (known & Ground) and with ~reached.  Only passable cells (and the
// source) are kept in the reached plane, so only they expand; a known
// staircase next to the wave is a hit, never walked through.  The reached
// plane is double-buffered (a lane reads its neighbours' words of the step
// before), and step k only visits rows within k of the source: nothing is
// further.  One search from the player serves all three columns: each records
// the first step at which the wave meets one of its targets, and the lowest
// flat cell among that step's hits.  The move then needs the distance from
// each chosen target to the player's four neighbours: a second search from
// the target, run for dist - 1 steps, after which "neighbour j is at dist - 1"
// is "its bit is reached" (it cannot be nearer).  (The other form, four more
// planes seeded at the neighbours and advanced in lockstep with the
// player's, was rejected on the listing: five times the LDS traffic on every
// step of the long search for all columns, where the searches from the
// targets stop at their own column's distance)
//
// Where the words live.  Five planes per game in LDS -- passable, stairs,
// frontier, reached x 2 -- while they fit 64 KiB; four games to a workgroup
// while they fit 32 KiB, as seek_kernel.  A grid whose five planes do not fit
// (narrow and tall: W <= 64 and H in the thousands) keeps only the two reached
// planes in LDS and recomputes the other three from global memory at every
// visit (route_kernel<false>): slow, and correct.
//
// Synchronisation is WAVE-LOCAL throughout: a wave touches only its own LDS,
// the DS operations of one wave complete in order, and a wavefront-scope fence
// keeps the compiler from reordering them.  There is no workgroup barrier in
// the kernel, so waves of one workgroup whose searches differ in length never
// wait for each other.  Every loop is bounded by the step count (<= W * H) and
// ends at a step that reaches nothing new.  The key's rule, the wave's
// reductions, the dist / move stores and the host side's refusals are
// orx_seek.h's, shared with orx_explore.hip; frontier_bits is there too, and so
// are the step itself (beside) and the room's words (room_word), which
// orx_path_ticks shares.  Plain C++ and vector stores only;
// no atomics; each output row is one store from lane 0.
#include "../../include/orx_route.h"
#include "orx_query.h"
#include "orx_seek.h"

namespace orx_route_dev {

using namespace orx_query;

constexpr uint32_t kNone = 0xFFFFFFFFu;  // no cell (above every flat cell)
constexpr int kStagedPlanes = 5, kBarePlanes = 2;

__global__ __launch_bounds__(kBlock) void planes_kernel(const uint8_t* tiles, uint32_t* planes,
                                                        int64_t n_words, int W, int H, int WW) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= n_words) return;
  const int64_t per = (int64_t)H * WW, l = idx / per;
  const int rem = (int)(idx - l * per), y = rem / WW, xw = rem - y * WW;
  const uint8_t* t = tiles + (size_t)l * (size_t)(W * H);
  uint32_t ground = 0, stair = 0;
  for (int bit = 0; bit < 32; ++bit) {
    const int x = xw * 32 + bit;
    if (x >= W) break;
    const uint32_t tile = t[x * H + y] & ORX_VIEW_TILE_MASK;
    ground |= (uint32_t)(tile == ORX_TILE_GROUND) << bit;
    stair |= (uint32_t)(tile == ORX_TILE_STAIRCASE_DOWN) << bit;
  }
  planes[(size_t)(2 * l) * (size_t)per + (size_t)rem] = ground;
  planes[(size_t)(2 * l + 1) * (size_t)per + (size_t)rem] = stair;
}

struct RouteArgs {
  const int32_t *p_x, *p_y, *p_depth, *tick, *episode, *st_x, *st_y;
  const int16_t* p_layout;
  const uint32_t* planes;
  const uint32_t* memory;
  const int32_t* key;
  const int32_t* goal;
  int32_t* dist;
  int8_t* move;
  int32_t* target;
  int64_t B;
  int32_t W, H, WW, L, player, G;
  uint32_t inv_ww, inv_h;  // recip(WW), recip(H): __umulhi(n, inv) = n / d for n < 2^16 (WW > 1)
};

// What the search needs of one map word: the known cells that are Ground, those
// that are StaircaseDown, and the frontier cells among the first.
struct Word {
  uint32_t pass, stairs, front;
};

// One game's map on its dungeon, read from global memory.
struct Map {
  const uint32_t* known;   // memory[b]
  const uint32_t* ground;  // planes[layout][0], or nullptr: the closed form
  const uint32_t* stair;   // planes[layout][1]
  int W, H, WW, sx, sy, last_word;
  uint32_t last_bit;  // of column W - 1 in the row's last word

  // word i = row y, word xw of the row
  __device__ __forceinline__ Word at(int i, int y, int xw, bool want_front) const {
    const uint32_t in = xw == last_word ? (last_bit << 1) - 1u : ~0u;  // (the columns x < W)
    const uint32_t k = known[i] & in;
    Word r = {0u, 0u, 0u};
    if (!k) return r;
    uint32_t g = 0, s = 0;
    if (ground) {
      g = ground[i], s = stair[i];
    } else {
      // EmptyDungeonGenerator: the border Wall, one staircase off the border
      const RoomWord room = room_word(W, H, sx, sy, y, xw, last_word, last_bit, in);
      g = room.ground, s = room.stair;
    }
    r.pass = k & g, r.stairs = k & s;
    if (want_front && r.pass)
      r.front = r.pass & frontier_bits(known, k, i, y, xw, WW, H, last_word, last_bit);
    return r;
  }
};

template <bool kStaged>
__global__ __launch_bounds__(kBlock) void route_kernel(const RouteArgs a) {
  extern __shared__ uint4 smem[];
  const int W = a.W, H = a.H, WW = a.WW, WH = W * H, words = H * WW;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t B = a.B, b = (int64_t)blockIdx.x * a.G + wave;
  if (b >= B) return;  // (no workgroup barrier below: a wave is on its own)
  uint32_t* lds = reinterpret_cast<uint32_t*>(smem) +
                  (size_t)wave * (size_t)(kStaged ? kStagedPlanes : kBarePlanes) * (size_t)words;
  uint32_t* const r0 = lds;
  uint32_t* const r1 = lds + words;
  uint32_t* const pass = lds + 2 * words;  // (the three below only when staged)
  uint32_t* const stairs = lds + 3 * words;
  uint32_t* const front = lds + 4 * words;

  const int64_t me = player_rows(a.player, B, b).me;
  const int x = a.p_x[me], y = a.p_y[me];
  const bool valid = key_valid(reinterpret_cast<const int4*>(a.key)[b], a.episode[b],
                               a.p_depth[me], a.tick[b]);
  const bool inside = (uint32_t)x < (uint32_t)W && (uint32_t)y < (uint32_t)H;

  int32_t found[3] = {ORX_SEEK_ABSENT, ORX_SEEK_ABSENT, ORX_SEEK_ABSENT};
  uint32_t cell[3] = {kNone, kNone, kNone};
  uint32_t steps = 0;  // the moves: a nibble of neighbour bits per column

  // row of word i (< 2^16)
  auto row_of = [&](int i) { return WW == 1 ? i : (int)__umulhi((uint32_t)i, a.inv_ww); };

  if (valid && inside) {
    Map m;
    m.known = a.memory + (size_t)b * (size_t)words;
    m.ground = m.stair = nullptr;
    m.W = W, m.H = H, m.WW = WW, m.sx = m.sy = -1;
    m.last_word = (W - 1) >> 5, m.last_bit = 1u << ((W - 1) & 31);
    if (a.L > 0) {
      const size_t lay = (size_t)layout_of(a, me);
      m.ground = a.planes + lay * 2u * (size_t)words;
      m.stair = m.ground + words;
    } else {
      m.sx = a.st_x[me], m.sy = a.st_y[me];
    }
    auto word_at = [&](int i, int yy, int xw, bool want_front) {
      if (kStaged) {
        const Word w = {pass[i], stairs[i], front[i]};
        return w;
      }
      return m.at(i, yy, xw, want_front);
    };
    // the lowest flat cell of a word's bits
    auto lowest = [&](uint32_t bits, int yy, int xw) {
      return bits ? (uint32_t)((xw * 32 + __builtin_ctz(bits)) * H + yy) : kNone;
    };
    auto lesser = [](uint32_t p, uint32_t q) { return p < q ? p : q; };

    // the map, a word at a time: the planes, and the lowest target of columns 0 and 1
    uint32_t low0 = kNone, low1 = kNone;
    for (int i = lane; i < words; i += 64) {
      const int yy = row_of(i), xw = i - yy * WW;
      const Word w = m.at(i, yy, xw, true);
      if (kStaged) pass[i] = w.pass, stairs[i] = w.stairs, front[i] = w.front;
      r0[i] = 0u, r1[i] = 0u;
      low0 = lesser(low0, lowest(w.front, yy, xw));
      low1 = lesser(low1, lowest(w.stairs, yy, xw));
    }
    low0 = wave_min(low0), low1 = wave_min(low1);

    // the goal: a cell of the grid, and whether a known walk can end on it
    const int32_t g = a.goal ? a.goal[b] : -1;
    const bool goal_in = g >= 0 && g < WH;
    const int gx = goal_in ? (int)__umulhi((uint32_t)g, a.inv_h) : 0, gy = goal_in ? g - gx * H : 0;
    const int gi = gy * WW + (gx >> 5);
    const uint32_t gbit = goal_in ? 1u << (gx & 31) : 0u;
    const Word gw = m.at(gi, gy, gx >> 5, false);
    const bool goal_ok = ((gw.pass | gw.stairs) & gbit) != 0u;

    const int own = x * H + y, oi = y * WW + (x >> 5);
    const uint32_t obit = 1u << (x & 31);
    const Word ow = m.at(oi, y, x >> 5, true);
    uint32_t pending = 0;  // the columns still looked for
    if (low0 != kNone) {
      found[0] = ORX_SEEK_UNREACHABLE, cell[0] = low0;
      if (ow.front & obit) found[0] = 0, cell[0] = (uint32_t)own; else pending |= 1u;
    }
    if (low1 != kNone) {
      found[1] = ORX_SEEK_UNREACHABLE, cell[1] = low1;
      if (ow.stairs & obit) found[1] = 0, cell[1] = (uint32_t)own; else pending |= 2u;
    }
    if (goal_in) {
      found[2] = ORX_SEEK_UNREACHABLE, cell[2] = (uint32_t)g;
      if (goal_ok) {
        if (g == own) found[2] = 0; else pending |= 4u;
      }
    }

    // one step of a search centred on row cy: cur -> nxt over rows cy - k .. cy + k
    // (`hits`: also what the wave meets; returns whether the reached set grew)
    uint32_t hit[3];
    auto advance = [&](const uint32_t* cur, uint32_t* nxt, int cy, int k, bool hits) {
      const int lo = cy - k > 0 ? cy - k : 0, hi = cy + k < H - 1 ? cy + k : H - 1;
      uint32_t grew = 0;
      hit[0] = hit[1] = hit[2] = kNone;
      for (int i = lo * WW + lane; i < (hi + 1) * WW; i += 64) {
        const int yy = row_of(i), xw = i - yy * WW;
        const uint32_t c = cur[i];
        const uint32_t nb = beside(cur, c, i, yy, xw, WW, H);
        const Word w = word_at(i, yy, xw, hits && (pending & 1u));
        const uint32_t fresh = nb & ~c & w.pass;
        nxt[i] = c | fresh;
        grew |= fresh;
        if (hits) {
          const uint32_t met = nb & w.stairs;  // (a staircase is met, never entered)
          hit[0] = lesser(hit[0], lowest(fresh & w.front, yy, xw));
          hit[1] = lesser(hit[1], lowest(met, yy, xw));
          if (i == gi && ((fresh | met) & gbit)) hit[2] = (uint32_t)g;
        }
      }
      wave_sync();
      return __ballot(grew != 0u) != 0ull;
    };

    // the search from the player
    wave_sync();
    if (lane == 0) r0[oi] = obit;
    wave_sync();
    uint32_t* cur = r0;
    uint32_t* nxt = r1;
    bool more = pending != 0u;
    for (int k = 1; more && k <= WH; ++k) {
      const bool grew = advance(cur, nxt, y, k, true);
#pragma unroll
      for (int col = 0; col < 3; ++col) {
        if (!(pending >> col & 1u)) continue;
        if (__ballot(hit[col] != kNone) == 0ull) continue;
        found[col] = k, cell[col] = wave_min(hit[col]);
        pending &= ~(1u << col);
      }
      uint32_t* const t = cur;
      cur = nxt, nxt = t;
      more = grew && pending != 0u;
    }

    // the moves: from each chosen target, dist - 1 steps; a neighbour of the
    // player that is reached then is one step closer (it cannot be nearer)
#pragma unroll
    for (int col = 0; col < 3; ++col) {
      const int d = found[col];
      if (d <= 0) continue;
      const int tc = (int)cell[col];
      const int tx = (int)__umulhi((uint32_t)tc, a.inv_h), ty = tc - tx * H;
      for (int i = lane; i < words; i += 64) r0[i] = 0u, r1[i] = 0u;
      wave_sync();
      if (lane == 0) r0[ty * WW + (tx >> 5)] = 1u << (tx & 31);
      wave_sync();
      cur = r0, nxt = r1;
      more = true;
      for (int k = 1; more && k < d && k <= WH; ++k) {
        more = advance(cur, nxt, ty, k, false);
        uint32_t* const t = cur;
        cur = nxt, nxt = t;
      }
      bool step = false;
      if (lane < 4) {
        const int nx = x + (lane == 1) - (lane == 3), ny = y + (lane == 2) - (lane == 0);
        if ((uint32_t)nx < (uint32_t)W && (uint32_t)ny < (uint32_t)H)
          step = (cur[ny * WW + (nx >> 5)] >> (nx & 31)) & 1u;
      }
      steps |= ((uint32_t)__ballot(step) & 15u) << (4 * col);
      wave_sync();  // (the planes are cleared again for the next column)
    }
  }
  if (lane != 0) return;

  uint32_t mv[3];
#pragma unroll
  for (int col = 0; col < 3; ++col) {
    const uint32_t nib = (steps >> (4 * col)) & 15u;
    mv[col] = nib ? (uint32_t)(ORX_MOVE_UP + __builtin_ctz(nib)) : (uint32_t)ORX_MOVE_STAY;
  }
  store_seek_rows(a.dist, a.move, b, (uint32_t)found[0], (uint32_t)found[1], (uint32_t)found[2],
                  mv[0], mv[1], mv[2]);
  if (a.target) reinterpret_cast<uint4*>(a.target)[b] = make_uint4(cell[0], cell[1], cell[2], kNone);
}

}  // namespace orx_route_dev

#ifndef ORX_ROUTE_BUILD_ID
#define ORX_ROUTE_BUILD_ID "unknown"
#endif

extern "C" const char* orx_route_build_id(void) { return ORX_ROUTE_BUILD_ID; }

extern "C" int orx_route_planes(const orx_cfg_t* cfg, const uint8_t* bank_tiles, uint32_t* planes,
                                void* stream) {
  using namespace orx_route_dev;
  using orx_dev::fail;
  int r;
  if ((r = orx_validate_cfg(cfg))) return r;
  if (cfg->n_layouts <= 0) return fail(ORX_EINVAL, "orx_route_planes: needs a bank (n_layouts > 0)");
  if (!bank_tiles || !planes) return fail(ORX_EINVAL, "orx_route_planes: bank_tiles or planes is NULL");
  if (misaligned(planes, 4)) return fail(ORX_EINVAL, "orx_route_planes: planes must be 4-byte aligned");
  const int W = cfg->width, H = cfg->height, WW = (W + 31) / 32;
  const int64_t n_words = (int64_t)cfg->n_layouts * H * WW;
  const unsigned grid = (unsigned)((n_words + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(planes_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, bank_tiles,
                     planes, n_words, W, H, WW);
  return orx_dev::launch_status("orx_route_planes");
}

extern "C" int orx_route(const orx_cfg_t* cfg, const orx_state_t* st, const uint32_t* planes,
                         int32_t player, const uint32_t* memory, const int32_t* key,
                         const int32_t* goal, int32_t* dist, int8_t* move, int32_t* target,
                         int64_t n_games, void* stream) {
  using namespace orx_route_dev;
  using orx_dev::fail;
  int r;
  if ((r = orx_validate_cfg(cfg)) || (r = check_player("orx_route", player))) return r;
  if ((r = check_memory_rows("orx_route", memory, key, dist, move, target))) return r;
  if (misaligned(goal, 4) || misaligned(planes, 4))
    return fail(ORX_EINVAL, "orx_route: goal and planes must be 4-byte aligned");
  if ((r = check_memory_query("orx_route", cfg, st, n_games))) return r;
  if (cfg->n_layouts > 0 && !planes) return fail(ORX_EINVAL, "orx_route: n_layouts > 0 needs planes");

  RouteArgs a;
  a.p_x = st->p_x, a.p_y = st->p_y, a.p_depth = st->p_depth;
  a.tick = st->tick, a.episode = st->episode, a.st_x = st->st_x, a.st_y = st->st_y;
  a.p_layout = st->p_layout;
  a.planes = cfg->n_layouts > 0 ? planes : nullptr;
  a.memory = memory, a.key = key, a.goal = goal;
  a.dist = dist, a.move = move, a.target = target;
  a.B = n_games;
  a.W = cfg->width, a.H = cfg->height, a.WW = (cfg->width + 31) / 32, a.L = cfg->n_layouts;
  a.player = player;
  a.inv_ww = recip(a.WW > 1 ? a.WW : 2);
  a.inv_h = recip(cfg->height);
  // a wave per game.  Five planes a game while they fit 64 KiB, four games to
  // a workgroup while theirs fit 32 KiB; else the two reached planes alone
  // (W * H <= 65536 and W >= 4: one plane is at most 64 KiB, two fit the CU's LDS)
  const size_t plane_bytes = sizeof(uint32_t) * (size_t)a.H * (size_t)a.WW;
  const bool staged = kStagedPlanes * plane_bytes <= 64 * 1024;
  const size_t game_bytes = (staged ? kStagedPlanes : kBarePlanes) * plane_bytes;
  const int G = a.G = games_per_workgroup(game_bytes);
  const unsigned grid = (unsigned)((n_games + G - 1) / G);
  const size_t lds = (size_t)G * game_bytes;
  if (staged) {
    hipLaunchKernelGGL(route_kernel<true>, dim3(grid), dim3(64 * G), lds, (hipStream_t)stream, a);
  } else {
    // (above the default limit of dynamic LDS: asked for once)
    static const hipError_t raised =
        hipFuncSetAttribute(reinterpret_cast<const void*>(route_kernel<false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    if (raised != hipSuccess) return fail(ORX_EIO,"orx_route: cannot raise the LDS limit");
    hipLaunchKernelGGL(route_kernel<false>, dim3(grid), dim3(64 * G), lds, (hipStream_t)stream, a);
  }
  return orx_dev::launch_status("orx_route");
}
