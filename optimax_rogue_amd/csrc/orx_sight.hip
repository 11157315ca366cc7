// orx_sight.hip -- line of sight through a dungeon's walls (include/orx_sight.h)
// for gfx950: which cells of orx_view's window a player sees from its centre.
//
// The rule is the header's: two digital lines per target cell (s |d| / n
// rounded half up and half down), clear when one of them meets no Wall, and a
// Wall also seen through a clear floor neighbour toward the viewer.  Like
// orx_view it needs nothing of the tick machinery: only orx.h's structs, the
// queries' shared header and the host side's error path.
//
// Shape.  A LANE IS A GAME and a wave walks the same line in 64 games at
// once: the line's arithmetic is the same in every lane, so it runs once a
// wave on the scalar unit, and a step costs a lane an LDS read and an AND-OR.
// A workgroup of 256 threads takes 64 consecutive games, and
//   1. stages the games' px, py and layout in LDS (one lane per game);
//   2. builds the opacity of every window as V 32-bit row masks per game in
//      LDS (V <= 31), one thread per row.  EmptyDungeonGenerator: two
//      comparisons per row (orx_view's closed form); a bank: one lookup per
//      cell (the layouts are a few KiB shared by all games: L2-resident).
//      Then the same bits as column masks, one thread per column;
//   3. walks the lines.  A line advances one cell a step along its major
//      axis, exactly, so a step reads ONE word -- the column mask of that x for
//      a line that runs along x, the row mask of that y otherwise -- and tests
//      the bit of the rounded minor offset.  That offset is a running quotient
//      and remainder of s |d| / n (no division); the two roundings differ only
//      where the remainder is 0, so both variants share the read and, but for
//      those steps, the test.  The four lines to (+-dx, +-dy) share all of it:
//      two reads and four AND-ORs a step.  A game's words are V (odd) dwords
//      apart: the wave's read is free of bank conflicts.  Each lane collects
//      the bits of rows +dy and -dy and stores the two row words;
//   4. applies the neighbour rule on the row words, one thread per row:
//      opaque[j] & (the clear floor of rows j and j -/+ 1, shifted toward the
//      centre column), and writes `rows` coalesced, 4 bytes per lane;
//   5. masks `cells` and `health` in place: 16 bytes per lane where the plane
//      is 16-byte aligned (64 games: every workgroup's slice then starts
//      aligned), a byte at a time for the tail and otherwise.  Every byte is
//      read and written by exactly one thread.
// Plain C++ and vector stores only.
#include "../../include/orx_sight.h"
#include "orx_query.h"

namespace orx_sight_dev {

using namespace orx_query;

constexpr int kGames = 64;  // games per workgroup: a wave's lanes

enum { H_PX, H_PY, H_LAYOUT, kHdr };  // header fields staged per game ([kHdr][G] int32 in LDS)

struct SightArgs {
  const int32_t *p_x, *p_y;
  const int16_t* p_layout;
  const uint8_t* bank_tiles;
  uint32_t* rows;
  uint8_t* cells;
  uint8_t* health;
  int64_t B;
  int32_t W, H, L, R, G, player;
  uint32_t inv_vv, inv_v;  // (R, G, inv_vv, inv_v: a Window)
};

// four cells of a plane under four seen bits: seen -> code | flag, unseen -> 0
__device__ __forceinline__ uint32_t mask4(uint32_t w, uint32_t bits, uint32_t flag) {
  const uint32_t s = spread4(bits);
  return (w | s * flag) & (s * 0xFFu);
}

// plane[0 .. n) (a workgroup's cells, in place) under the row words `seen`:
// 16 bytes per lane while the plane is 16-byte aligned, the rest byte by byte
__device__ __forceinline__ void mask_plane(const uint32_t* seen, uint8_t* plane, int n,
                                           uint32_t flag, const Window& win, int t) {
  const int V = win.V;
  const int nvec = ((reinterpret_cast<uintptr_t>(plane) & 15) == 0) ? n >> 4 : 0;
  uint4* q = reinterpret_cast<uint4*>(plane);
  for (int v = t; v < nvec; v += kBlock) {
    // the 16 cells run over the end of a window row into the next rows
    const Window::Cell first = win.split((uint32_t)v << 4);
    const uint32_t bits = gather16(seen, first.g * V + first.j, first.i, V);
    uint4 w = q[v];
    w.x = mask4(w.x, bits, flag);
    w.y = mask4(w.y, bits >> 4, flag);
    w.z = mask4(w.z, bits >> 8, flag);
    w.w = mask4(w.w, bits >> 12, flag);
    q[v] = w;
  }
  for (int c = (nvec << 4) + t; c < n; c += kBlock) {
    const Window::Cell at = win.split((uint32_t)c);
    const bool on = (seen[at.g * V + at.j] >> at.i) & 1u;
    plane[c] = on ? (uint8_t)(plane[c] | flag) : (uint8_t)0;
  }
}

__global__ __launch_bounds__(kBlock) void sight_kernel(const SightArgs a) {
  extern __shared__ uint4 smem[];
  const Window win = Window::of(a.R, a.G, a.inv_vv, a.inv_v);
  const int G = win.G, R = win.R, V = win.V, VV = win.VV, W = a.W, H = a.H;
  uint32_t* opq = reinterpret_cast<uint32_t*>(smem);  // [G * V] row masks: Wall
  uint32_t* colw = opq + G * V;                       // ... the same bits as column masks
  uint32_t* clr = colw + G * V;                       // ... no line of the two is blocked
  uint32_t* seen = colw;                              // (step 4 on: the columns are done with)
  int32_t* hdr = reinterpret_cast<int32_t*>(clr + G * V);
  const int64_t B = a.B;
  const int64_t b0 = (int64_t)blockIdx.x * G;
  const int nb = (int)((B - b0) < (int64_t)G ? (B - b0) : (int64_t)G);
  const int t = threadIdx.x;
  const int nrows = nb * V, ncells = nb * VV;

  // 1. the viewers, coalesced over the games
  if (t < nb) {
    const int64_t me = player_rows(a.player, B, b0 + t).me;
    hdr[H_PX * G + t] = a.p_x[me];
    hdr[H_PY * G + t] = a.p_y[me];
    hdr[H_LAYOUT * G + t] = layout_of(a, me);
  }
  __syncthreads();

  // 2. opacity: one thread per window row (the rows of a partial workgroup's
  // missing games are empty: step 3's lanes read them)
  for (int row = t; row < G * V; row += kBlock) {
    const int g = win.div_v((uint32_t)row), j = row - g * V;
    uint32_t wall = 0;
    if (g < nb) {
      const int px = hdr[H_PX * G + g], y = hdr[H_PY * G + g] + j - R;
      if (y >= 0 && y < H) {
        if (a.L == 0) {
          // EmptyDungeonGenerator (worldgen.py:33-43): the border is Wall
          const int i0 = R - px, i1 = W - 1 - px + R;
          const uint32_t in = grid_columns(px, W, R, V);
          const uint32_t edge = ((i0 >= 0 && i0 < V) ? 1u << i0 : 0u) | ((i1 >= 0 && i1 < V) ? 1u << i1 : 0u);
          wall = (y == 0 || y == H - 1) ? in : in & edge;
        } else {
          const uint8_t* bt = a.bank_tiles + (size_t)hdr[H_LAYOUT * G + g] * (size_t)(W * H);
          for (int i = 0; i < V; ++i) {
            const int x = px + i - R;
            if (x >= 0 && x < W && (bt[x * H + y] & ORX_VIEW_TILE_MASK) == ORX_TILE_WALL) wall |= 1u << i;
          }
        }
      }
    }
    opq[row] = wall;
  }
  __syncthreads();
  // ... and one per window column: bit j of column i is bit i of row j
  for (int col = t; col < G * V; col += kBlock) {
    const int g = win.div_v((uint32_t)col), i = col - g * V;
    uint32_t word = 0;
    for (int j = 0; j < V; ++j) word |= ((opq[g * V + j] >> i) & 1u) << j;
    colw[col] = word;
  }
  __syncthreads();

  // 3. the lines: a lane is a game, and all of a line's arithmetic is the same
  // in every lane.  The lines to (+-dx, +-dy) mirror each other -- the same
  // steps, quotients and remainders -- so the four are walked as one: two
  // words a step (major offset +s and -s) against two masks (minor offset +q
  // and -q).  hit[major sign][minor sign] collects the Walls met; a wave takes
  // every fourth |dy|, folded (0 7 8 15 | 1 6 9 14 | ..) so that the four
  // waves walk as many steps
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const uint32_t* grow = opq + lane * V + R;  // (centred: offsets -R .. R)
  const uint32_t* gcol = colw + lane * V + R;
  uint32_t* gclr = clr + lane * V + R;
  for (int ady = 0; ady <= R; ++ady) {
    if (((ady & 4) ? 3 - (ady & 3) : (ady & 3)) != wave) continue;
    uint32_t blocked_p = 0, blocked_m = 0;  // rows +ady and -ady; bit i: both lines to the cell meet a Wall
    for (int adx = 0; adx <= R; ++adx) {
      const bool along_x = adx >= ady;
      const int n = along_x ? adx : ady, m = along_x ? ady : adx;
      if (n <= 1) continue;
      // step s stands at major offset s, minor offset (2 s m + n) / (2 n) ("up":
      // quotient q, remainder r) or, where r == 0, one less ("down")
      const uint32_t* words = along_x ? gcol : grow;
      uint32_t both_pp = 0, both_pm = 0, both_mp = 0, both_mm = 0;
      uint32_t up_pp = 0, up_pm = 0, up_mp = 0, up_mm = 0;
      uint32_t down_pp = 0, down_pm = 0, down_mp = 0, down_mm = 0;
      int q = 0, r = n;
      for (int s = 1; s < n; ++s) {
        r += 2 * m;
        if (r >= 2 * n) r -= 2 * n, ++q;
        const uint32_t wp = words[s], wm = words[-s];
        const uint32_t qp = 1u << (R + q), qm = 1u << (R - q);
        if (r == 0) {
          const uint32_t dp = 1u << (R + q - 1), dm = 1u << (R - q + 1);
          up_pp |= wp & qp, up_pm |= wp & qm, up_mp |= wm & qp, up_mm |= wm & qm;
          down_pp |= wp & dp, down_pm |= wp & dm, down_mp |= wm & dp, down_mm |= wm & dm;
        } else {
          both_pp |= wp & qp, both_pm |= wp & qm, both_mp |= wm & qp, both_mm |= wm & qm;
        }
      }
      auto shut = [](uint32_t both, uint32_t up, uint32_t down) {
        return (uint32_t)(both != 0 || (up != 0 && down != 0));
      };
      const uint32_t pp = shut(both_pp, up_pp, down_pp), pm = shut(both_pm, up_pm, down_pm);
      const uint32_t mp = shut(both_mp, up_mp, down_mp), mm = shut(both_mm, up_mm, down_mm);
      const int ip = R + adx, im = R - adx;
      if (along_x) {  // major: the column, minor: the row
        blocked_p |= pp << ip | mp << im;
        blocked_m |= pm << ip | mm << im;
      } else {        // major: the row, minor: the column
        blocked_p |= pp << ip | pm << im;
        blocked_m |= mp << ip | mm << im;
      }
    }
    gclr[ady] = ~blocked_p;  // (step 4 keeps the cells of the grid)
    gclr[-ady] = ~blocked_m;
  }
  __syncthreads();

  // 4. a Wall is also seen through a clear floor neighbour toward the viewer:
  // bitwise on the row words, one thread per row
  const uint32_t right = ((1u << V) - 1u) & ~((2u << R) - 1u), left = (1u << R) - 1u;
  auto toward = [&](uint32_t f) { return ((f << 1) & right) | ((f >> 1) & left); };
  // the clear cells of a row: those of the grid that a line reaches
  auto clear_of = [&](int row, int g) {
    const int y = hdr[H_PY * G + g] + row - g * V - R;
    return y >= 0 && y < H ? clr[row] & grid_columns(hdr[H_PX * G + g], W, R, V) : 0u;
  };
  for (int row = t; row < nrows; row += kBlock) {
    const int g = win.div_v((uint32_t)row), dy = row - g * V - R;
    const uint32_t wall = opq[row], clear = clear_of(row, g);
    uint32_t lit = toward(clear & ~wall);
    if (dy != 0) {
      const int next = dy > 0 ? row - 1 : row + 1;  // the row toward the viewer's
      const uint32_t f = clear_of(next, g) & ~opq[next];
      lit |= f | toward(f);
    }
    const uint32_t s = clear | (wall & lit);
    // (seen is colw: no thread reads the columns any more)
    seen[row] = s;
    if (a.rows) a.rows[(size_t)b0 * (size_t)V + (size_t)row] = s;
  }
  if (!a.cells && !a.health) return;
  __syncthreads();

  // 5. the planes, masked in place
  const size_t off = (size_t)b0 * (size_t)VV;
  if (a.cells) mask_plane(seen, a.cells + off, ncells, ORX_SIGHT_SEEN, win, t);
  if (a.health) mask_plane(seen, a.health + off, ncells, 0u, win, t);
}

}  // namespace orx_sight_dev

#ifndef ORX_SIGHT_BUILD_ID
#define ORX_SIGHT_BUILD_ID "unknown"
#endif

extern "C" const char* orx_sight_build_id(void) { return ORX_SIGHT_BUILD_ID; }

extern "C" int orx_sight(const orx_cfg_t* cfg, const orx_state_t* st, int32_t player, int32_t radius,
                         uint32_t* rows, uint8_t* cells, uint8_t* health, int64_t n_games,
                         void* stream) {
  using namespace orx_sight_dev;
  using orx_dev::fail;
  int r;
  if ((r = orx_validate_cfg(cfg)) || (r = check_player("orx_sight", player))) return r;
  if (radius < 1 || radius > ORX_VIEW_MAX_RADIUS)
    return fail(ORX_EINVAL, "orx_sight: radius must be in [1, ORX_VIEW_MAX_RADIUS]");
  if (!rows && !cells && !health)
    return fail(ORX_EINVAL, "orx_sight: rows, cells and health are all NULL");
  if (misaligned(rows, 4))
    return fail(ORX_EINVAL, "orx_sight: rows must be 4-byte aligned");
  if ((r = check_games("orx_sight", n_games)) || (r = check_state(cfg, st, kBank))) return r;

  SightArgs a;
  a.p_x = st->p_x, a.p_y = st->p_y;
  a.p_layout = st->p_layout, a.bank_tiles = st->bank_tiles;
  a.rows = rows, a.cells = cells, a.health = health;
  a.B = n_games;
  a.W = cfg->width, a.H = cfg->height, a.L = cfg->n_layouts;
  a.player = player;
  const Window win = Window::fit(radius, 0, kGames);  // (no tiles: always kGames games)
  const int G = win.G;
  a.R = win.R, a.G = G, a.inv_vv = win.inv_vv, a.inv_v = win.inv_v;
  const size_t lds = sizeof(uint32_t) * (size_t)G * (size_t)(3 * win.V + kHdr);
  const unsigned grid = (unsigned)((n_games + G - 1) / G);
  hipLaunchKernelGGL(sight_kernel, dim3(grid), dim3(kBlock), lds, (hipStream_t)stream, a);
  return orx_dev::launch_status("orx_sight");
}
