// orx_view.hip -- the egocentric map view (include/orx_view.h) for gfx950.
//
// What a bot sees, batched: the reference gives every bot the GameState of
// its depth each tick (optimax_rogue_bots/main.py:118-155) and its spectator
// draws it tiles first, entities of the viewed depth on top
// (optimax_rogue_cmdspec/map.py:56-84).  view_kernel writes that picture as a
// V x V window of cell codes around one player of every game, from the
// resident SoA state.  It needs nothing of the tick machinery: only orx.h's
// structs, and the host side's error path (fail / launch_status of
// orx_engine.hip's host part, linked into the same library).
//
// Shape.  The inputs are batch-contiguous rows (one coalesced load per field
// and wave); the output is game-major rows of V * V bytes (121 at R = 5, 961
// at R = 15: never a multiple of 16), so a lane writing its own game's row
// would scatter byte stores.  Instead a workgroup of 256 threads takes G
// consecutive games (G = 64, 32 or 16: the largest whose tiles stay within
// kTileBudget of LDS, so that four workgroups share a CU), and
//   1. loads everything it reads from HBM at once, coalesced, into LDS: the
//      games' headers (one lane per game) and the first kChunk NPCs and the
//      items of every game (one lane per (slot, game)) -- one exposed load
//      latency per workgroup;
//   2. builds the G x V*V-byte tile in LDS.  EmptyDungeonGenerator: a window
//      row is two bit masks (inside the grid; Wall); one thread gathers 16
//      consecutive cells' bits, spreads them into bytes four at a time and
//      stores them as one aligned 16-byte LDS store.  A bank: one thread per
//      window row, one tile lookup per cell;
//   3. ORs the occupant bits in from LDS, one lane per game in a fixed order
//      (items, NPCs -- further chunks of kChunk for dense NPCs, from the
//      position list -- and the other player last, whose health takes the
//      health byte);
//   4. streams the tile's contiguous G * V*V bytes to HBM, 16 bytes per lane
//      (G is a multiple of 16, so every workgroup's slice starts 16-byte
//      aligned when the buffer does), with a byte tail for the last partial
//      workgroup's unaligned end.
// Plain C++ and vector stores only.
#include <cstdlib>

#include "../../include/orx_view.h"
#include "orx_query.h"

namespace orx_view_dev {

using namespace orx_query;

constexpr int kChunk = 16;              // NPC slots staged in LDS at a time (ORX_MAX_REG_NPCS)

// header fields staged per game ([kHdr][G] int32 in LDS)
enum { H_PX, H_PY, H_FLAGS, H_OX, H_OY, H_OHP, H_SX, H_SY, H_LAYOUT, kHdr };
enum { F_OTHER = 1, F_NPC_DEPTH = 2 };  // H_FLAGS: the other player / the NPCs are on the viewer's depth
// a staged occupant ([kChunk][G] uint32 in LDS): x | y << 8 | present << 16 |
// item kind << 17 | NPC health (clamped) << 24
constexpr uint32_t kPresent = 1u << 16, kKind = 1u << 17;

struct ViewArgs {
  const int32_t *p_x, *p_y, *p_depth, *p_health, *st_x, *st_y;
  const uint16_t* npc_pos;
  const int8_t* npc_health;
  const uint32_t* npc_alive;
  const int16_t* p_layout;
  const uint8_t* bank_tiles;
  const uint16_t* item_pos;
  const uint32_t* item_mask;
  uint8_t* cells;
  uint8_t* health;
  int64_t B;
  int32_t W, H, K, L, R, G, player, npc_depth, items;
  uint32_t inv_vv, inv_v;  // (R, G, inv_vv, inv_v: a Window)
};

__device__ __forceinline__ uint32_t clamp_u8(int32_t v) {
  return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// NPC slots k0 .. k0 + kChunk of the workgroup's games -> stage, one lane per
// (slot, game): coalesced over the games
__device__ __forceinline__ void stage_npcs(const ViewArgs& a, uint32_t* stage, int k0, int64_t b0,
                                           int nb, int t) {
  const int G = a.G, n = (a.K - k0 < kChunk ? a.K - k0 : kChunk) * G;
  for (int idx = t; idx < n; idx += kBlock) {
    const int g = idx & (G - 1), k = k0 + idx / G;
    if (g >= nb) continue;
    const int64_t b = b0 + g;
    const uint32_t alive = (a.npc_alive[(int64_t)(k >> 5) * a.B + b] >> (k & 31)) & 1u;
    stage[idx] = (uint32_t)a.npc_pos[(int64_t)k * a.B + b] | (alive ? kPresent : 0u) |
                 clamp_u8(a.npc_health[(int64_t)k * a.B + b]) << 24;
  }
}

__global__ __launch_bounds__(kBlock) void view_kernel(const ViewArgs a) {
  extern __shared__ uint4 smem[];
  const Window win = Window::of(a.R, a.G, a.inv_vv, a.inv_v);
  const int G = win.G, R = win.R, V = win.V, VV = win.VV, W = a.W, H = a.H;
  const int tile_bytes = (G * VV + 15) & ~15;
  uint8_t* tile = reinterpret_cast<uint8_t*>(smem);
  uint8_t* htile = tile + tile_bytes;  // (only when a.health)
  int32_t* hdr = reinterpret_cast<int32_t*>(tile + (a.health ? 2 : 1) * tile_bytes);
  uint32_t* npc_stage = reinterpret_cast<uint32_t*>(hdr + kHdr * G);  // (only when K > 0)
  uint32_t* item_stage = npc_stage + kChunk * G;                      // (only when a.items)
  const int64_t B = a.B;
  const int64_t b0 = (int64_t)blockIdx.x * G;
  const int nb = (int)((B - b0) < (int64_t)G ? (B - b0) : (int64_t)G);
  const int t = threadIdx.x;

  // 1. everything read from HBM, coalesced over the games
  if (t < nb) {
    const auto [me, ot] = player_rows(a.player, B, b0 + t);
    const int32_t d = a.p_depth[me];
    hdr[H_PX * G + t] = a.p_x[me];
    hdr[H_PY * G + t] = a.p_y[me];
    hdr[H_FLAGS * G + t] = (a.p_depth[ot] == d ? F_OTHER : 0) | (d == a.npc_depth ? F_NPC_DEPTH : 0);
    hdr[H_OX * G + t] = a.p_x[ot];
    hdr[H_OY * G + t] = a.p_y[ot];
    hdr[H_OHP * G + t] = (int32_t)clamp_u8(a.p_health[ot]);
    hdr[H_SX * G + t] = a.st_x[me];
    hdr[H_SY * G + t] = a.st_y[me];
    hdr[H_LAYOUT * G + t] = layout_of(a, me);
  }
  if (a.K > 0) stage_npcs(a, npc_stage, 0, b0, nb, t);
  if (a.items) {  // (K <= kChunk with items)
    for (int idx = t; idx < a.K * G; idx += kBlock) {
      const int g = idx & (G - 1), k = idx / G;
      if (g >= nb) continue;
      const int64_t b = b0 + g;
      const uint32_t on = (a.item_mask[b] >> k) & 1u, kind = (a.item_mask[B + b] >> k) & 1u;
      item_stage[idx] = (uint32_t)a.item_pos[(int64_t)k * B + b] | (on ? kPresent : 0u) |
                        (kind ? kKind : 0u);
    }
  }
  if (a.health) {
    uint4* hz = reinterpret_cast<uint4*>(htile);
    for (int v = t; v < (tile_bytes >> 4); v += kBlock) hz[v] = make_uint4(0, 0, 0, 0);
  }
  __syncthreads();

  // 2. tile bits
  if (a.L == 0) {
    // EmptyDungeonGenerator (worldgen.py:33-43): the border is Wall, the rest
    // Ground (the staircase is set in step 3).  One thread per 16 consecutive
    // bytes of the tile (an aligned LDS store): they run over the end of a
    // window row into the next (and the next game's first), so the 16 cells
    // are gathered row by row as two bit strings -- bit = the cell is in the
    // grid / is Wall -- and the cell code is their sum (0, 1 or 2)
    const int nvec = (nb * VV + 15) >> 4;
    for (int v = t; v < nvec; v += kBlock) {
      const Window::Cell first = win.split((uint32_t)v << 4);
      int g = first.g, j = first.j, i = first.i;
      uint32_t inb = 0, wallb = 0;
      int filled = 0;
      while (filled < 16) {
        const int px = hdr[H_PX * G + g], y = hdr[H_PY * G + g] + j - R;
        // window columns i0 and i1 are x = 0 and x = W - 1
        const int i0 = R - px, i1 = W - 1 - px + R;
        const int lo = i0 > 0 ? i0 : 0, hi = i1 < V - 1 ? i1 : V - 1;
        const uint32_t in = (y >= 0 && y < H && lo <= hi) ? ((2u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
        const uint32_t edge = ((i0 >= 0 && i0 < V) ? 1u << i0 : 0u) | ((i1 >= 0 && i1 < V) ? 1u << i1 : 0u);
        const uint32_t wall = (y == 0 || y == H - 1) ? in : in & edge;
        const int take = V - i < 16 - filled ? V - i : 16 - filled;
        const uint32_t m = (1u << take) - 1u;
        inb |= ((in >> i) & m) << filled;
        wallb |= ((wall >> i) & m) << filled;
        filled += take;
        i = 0;
        if (++j == V) {
          j = 0;
          if (++g == G) break;
        }
      }
      reinterpret_cast<uint4*>(tile)[v] =
          make_uint4(spread4(inb) + spread4(wallb), spread4(inb >> 4) + spread4(wallb >> 4),
                     spread4(inb >> 8) + spread4(wallb >> 8), spread4(inb >> 12) + spread4(wallb >> 12));
    }
  } else {
    // a bank: one thread per window row, one tile lookup per cell
    const int rows = nb * V;
    for (int row = t; row < rows; row += kBlock) {
      const int g = row / V, j = row - g * V;
      const int px = hdr[H_PX * G + g], y = hdr[H_PY * G + g] + j - R;
      const bool yin = y >= 0 && y < H;
      uint8_t* dst = tile + g * VV + j * V;
      const uint8_t* bt = a.bank_tiles + (size_t)hdr[H_LAYOUT * G + g] * (size_t)(W * H);
      for (int i = 0; i < V; ++i) {
        const int x = px + i - R;
        uint8_t code = ORX_VIEW_OUTSIDE;
        if (yin && x >= 0 && x < W) code = bt[x * H + y] & ORX_VIEW_TILE_MASK;
        dst[i] = code;
      }
    }
  }
  __syncthreads();

  // 3. what stands on the cells: one lane per game, in a fixed order (the
  // other player last: its health takes the health byte)
  const int px = t < nb ? hdr[H_PX * G + t] : 0, py = t < nb ? hdr[H_PY * G + t] : 0;
  const int fl = t < nb ? hdr[H_FLAGS * G + t] : 0;
  uint8_t* gt = tile + t * VV;   // (used by lanes t < nb only)
  uint8_t* gh = htile + t * VV;
  // window index of grid cell (x, y), or -1 outside the window or the grid
  auto at = [&](int x, int y) -> int {
    const int i = x - px + R, j = y - py + R;
    return (i >= 0 && i < V && j >= 0 && j < V && x >= 0 && x < W && y >= 0 && y < H) ? j * V + i
                                                                                        : -1;
  };
  auto put_npcs = [&](int k0) {
    const int n = a.K - k0 < kChunk ? a.K - k0 : kChunk;
    for (int k = 0; k < n; ++k) {
      const uint32_t s = npc_stage[k * G + t];
      const int c = (s & kPresent) ? at((int)(s & 0xFF), (int)((s >> 8) & 0xFF)) : -1;
      if (c >= 0) {
        gt[c] |= ORX_VIEW_NPC;
        if (a.health) gh[c] = (uint8_t)(s >> 24);
      }
    }
  };
  if (t < nb) {
    if (a.L == 0) {
      const int c = at(hdr[H_SX * G + t], hdr[H_SY * G + t]);
      if (c >= 0) gt[c] = ORX_TILE_STAIRCASE_DOWN;
    }
    if (fl & F_NPC_DEPTH) {
      if (a.items) {
        for (int k = 0; k < a.K; ++k) {
          const uint32_t s = item_stage[k * G + t];
          const int c = (s & kPresent) ? at((int)(s & 0xFF), (int)((s >> 8) & 0xFF)) : -1;
          if (c >= 0) gt[c] |= (uint8_t)(ORX_VIEW_ITEM | ((s & kKind) ? ORX_VIEW_ITEM_KIND : 0));
        }
      }
      if (a.K > 0) put_npcs(0);
    }
  }
  for (int k0 = kChunk; k0 < a.K; k0 += kChunk) {  // dense NPCs: the further chunks
    __syncthreads();
    stage_npcs(a, npc_stage, k0, b0, nb, t);
    __syncthreads();
    if (t < nb && (fl & F_NPC_DEPTH)) put_npcs(k0);
  }
  if (t < nb && (fl & F_OTHER)) {
    const int c = at(hdr[H_OX * G + t], hdr[H_OY * G + t]);
    if (c >= 0) {
      gt[c] |= ORX_VIEW_PLAYER;
      if (a.health) gh[c] = (uint8_t)hdr[H_OHP * G + t];
    }
  }
  __syncthreads();

  // 4. the tile's nb * VV contiguous bytes to HBM
  const size_t off = (size_t)b0 * (size_t)VV;
  stream_out(tile, a.cells + off, nb * VV, t);
  if (a.health) stream_out(htile, a.health + off, nb * VV, t);
}

}  // namespace orx_view_dev

extern "C" int orx_view(const orx_cfg_t* cfg, const orx_state_t* st, int32_t player, int32_t radius,
                        uint8_t* cells, uint8_t* health, int64_t n_games, void* stream) {
  using namespace orx_view_dev;
  using orx_dev::fail;
  int r;
  if ((r = orx_validate_cfg(cfg)) || (r = check_player("orx_view", player))) return r;
  if (radius < 1 || radius > ORX_VIEW_MAX_RADIUS)
    return fail(ORX_EINVAL, "orx_view: radius must be in [1, ORX_VIEW_MAX_RADIUS]");
  if (!cells) return fail(ORX_EINVAL, "orx_view: cells is NULL");
  // (the NPCs before the bank: the order this entry point refuses in)
  if ((r = check_games("orx_view", n_games)) ||
      (r = check_state(cfg, st, kPlayers | kStairs | kNpcs)) ||
      (r = check_state(cfg, st, kBank | kItems)))
    return r;
  const bool items = has_items(cfg);

  ViewArgs a;
  a.p_x = st->p_x, a.p_y = st->p_y, a.p_depth = st->p_depth, a.p_health = st->p_health;
  a.st_x = st->st_x, a.st_y = st->st_y;
  a.npc_pos = st->npc_pos, a.npc_health = st->npc_health, a.npc_alive = st->npc_alive;
  a.p_layout = st->p_layout, a.bank_tiles = st->bank_tiles;
  a.item_pos = st->item_pos, a.item_mask = st->item_mask;
  a.cells = cells, a.health = health;
  a.B = n_games;
  a.W = cfg->width, a.H = cfg->height, a.K = cfg->n_npcs, a.L = cfg->n_layouts;
  a.player = player;
  a.npc_depth = npc_depth(cfg);
  a.items = items ? 1 : 0;
  // (env ORX_VIEW_GAMES = 16 / 32 caps the games per workgroup: measurements)
  const char* e = getenv("ORX_VIEW_GAMES");
  const int cap = e ? atoi(e) : 64, nout = health ? 2 : 1;
  const Window win = Window::fit(radius, nout, cap == 16 || cap == 32 ? cap : 64);
  const int G = win.G;
  a.R = win.R, a.G = G, a.inv_vv = win.inv_vv, a.inv_v = win.inv_v;
  const size_t lds = (size_t)((G * win.VV + 15) & ~15) * nout +
                     sizeof(int32_t) * G * (kHdr + (a.K > 0 ? kChunk : 0) + (items ? kChunk : 0));
  const unsigned grid = (unsigned)((n_games + G - 1) / G);
  hipLaunchKernelGGL(view_kernel, dim3(grid), dim3(kBlock), lds, (hipStream_t)stream, a);
  return orx_dev::launch_status("orx_view");
}
