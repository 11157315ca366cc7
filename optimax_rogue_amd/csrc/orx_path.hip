// orx_path.hip -- the staircase distance field (include/orx_path.h) for gfx950.
//
// field_kernel: the breadth-first distance of every tile of every layout of a
// bank to its nearest StaircaseDown.  One workgroup (64 .. 1024 threads) per
// layout, grid-stride over the layouts.  The layout's uint16 plane lives in
// dynamic LDS, stored as runs along the grid's longer axis with one Wall
// sentinel between runs (and one before the first and after the last), so
// that the four neighbours of plane index i are i - 1, i + 1, i - S and i + S
// with no coordinate arithmetic: the sentinel stops a step over the end of a
// run, an index test stops one off the first or last run.  That is
// 2 * (W * H + min(W, H) + 1) bytes: 128.5 KiB for 256 x 256, above the
// default 64 KiB per workgroup, so the launch raises the kernel's limit.
//   1. tiles -> plane: Wall 0xFFFF, StaircaseDown 0, everything else 0xFFFE
//      ("not reached", which is also the final value of an unreachable tile);
//   2. relax d = min(d, 1 + min(neighbours)) in place until a workgroup-wide
//      vote finds a whole sweep without a change.  A thread owns a contiguous
//      piece of the plane and sweeps it forward, then backward, carrying the
//      last value in a register, so a straight corridor inside a piece is
//      solved in one sweep whichever way it runs.  Values only ever fall, and
//      every value written is the length of a real path, so whatever order the
//      hardware runs the threads in, the sweeps end at the one fixed point;
//      a sweep in which nobody wrote saw the final plane throughout;
//   3. plane -> HBM, 16 bytes per lane (uint16 head / tail where a layout's
//      slice does not start or end 16-byte aligned).
//
// query: point_kernel (no window) is one lane per game and five values.
// window_kernel has view_kernel's shape, from the same pieces (orx_query.h:
// the window, its split, stream_out): a workgroup of 256 threads owns G
// consecutive games (64, 32 or 16: the most whose tile stays within
// kTileBudget), stages their headers in LDS, builds the G x V*V uint16
// tile in LDS -- the closed form eight cells per thread with one aligned
// 16-byte LDS store; a bank 16 or 32 neighbouring lanes per window column,
// because a fixed x with consecutive y is consecutive uint16 in the field (a
// coalesced gather), written transposed into the tile -- takes dist and move
// from the tile's centre cells, and streams the tile's contiguous bytes out
// 16 per lane.
//
// rows_kernel: the distance plane from an arbitrary source cell, one row of
// the pair table per workgroup, grid-stride over the rows.  field_kernel's
// plane layout, sweeps and stream-out (Plane, relax_plane, stream_plane) on
// another graph: a walk that stays on its depth cannot cross a StaircaseDown (the
// updater descends whoever steps on one), so the staircases are marked kStair
// and left out of the relaxation -- "Ground plus the source" -- and a
// staircase that is not the source takes 1 + the least of its reached
// neighbours only while the plane is streamed out (it is never written back,
// so two adjacent staircases cannot see each other's value).  Thousands of
// rows are in flight where the field has L layouts, so a workgroup is sized
// by the plane (kRowsPerThread entries per thread), not fixed at 1,024.
//
// seek_kernel: moves_kernel's shape -- one lane per game, 256 per workgroup,
// no LDS.  A lane reads one table cell per target (row = the target's cell,
// column = its own: the table is symmetric), keeps the least per column, and
// reads the chosen target's row at its four neighbours for the move (the
// Seeker of orx_seek.h, which orx_npc_seek shares).
//
// threat_kernel: seek_kernel's shape with the question turned round -- a lane
// per game loops over the live threats and reads each one's row of the table
// at five cells (its own, y -+ 1 beside it, x -+ 1 at -+ H entries: at most
// three cache lines), keeping the least per cell for the other player and for
// the NPCs; the union column is their cellwise minimum, the flee move the
// first of Stay, Up, Right, Down, Left with the largest.
// threat_window_kernel: window_kernel's staging and transpose; every tile cell
// is owned by one lane through the loop over the game's threats, so the
// minimum needs no atomics and no barrier.  The rows are threat_kernel's body
// run by the first lanes after the tile has been streamed out.
//
// ticks_kernel: route_kernel's shape -- a wave per game, bit planes in LDS, no
// workgroup barrier -- for the one query here that no table can answer: a
// Dijkstra backwards from the staircases in steps of game time, in which the
// cells NPCs hold keep the wave back for the blows they cost (the comment at
// the kernel has the rest).  Its step and the room's words are orx_seek.h's,
// shared with orx_route.hip.
// Plain C++ and vector stores only.
#include <cstdlib>

#include "../../include/orx_path.h"
#include "orx_query.h"
#include "orx_seek.h"

namespace orx_path_dev {

using namespace orx_query;

constexpr uint32_t kWall = ORX_PATH_WALL, kFar = ORX_PATH_UNREACHABLE;

// ---------------------------------------------------------------------------
// the field
// ---------------------------------------------------------------------------
constexpr int kFieldBlock = 1024;
constexpr int kDefaultLds = 64 * 1024;  // dynamic LDS a kernel may use without raising its limit

struct FieldArgs {
  const uint8_t* tiles;
  uint16_t* field;
  int32_t L, W, H, WH;
  int32_t ylong;  // runs along y (H >= W), else along x
  int32_t S;      // run stride: the longer side + 1
  int32_t N;      // plane entries: (shorter side) * S + 1
};

// plane index of flat tile index c = x * H + y
__device__ __forceinline__ int plane_index(const FieldArgs& a, int c) {
  const int x = c / a.H, y = c - x * a.H;
  return a.ylong ? x * a.S + y + 1 : y * a.S + x + 1;
}

__global__ __launch_bounds__(kFieldBlock) void field_kernel(const FieldArgs a) {
  extern __shared__ uint4 smem[];
  volatile uint16_t* p = reinterpret_cast<volatile uint16_t*>(smem);
  const int t = threadIdx.x, nt = blockDim.x;
  const int S = a.S, N = a.N, WH = a.WH;
  const int per = (N + nt - 1) / nt;
  const int lo = t * per < N ? t * per : N, hi = lo + per < N ? lo + per : N;

  for (int l = blockIdx.x; l < a.L; l += gridDim.x) {
    // 1. the sentinels (every S-th entry) and the tiles
    for (int k = t * S; k < N; k += nt * S) p[k] = (uint16_t)kWall;
    const uint8_t* src = a.tiles + (size_t)l * (size_t)WH;
    for (int c = t; c < WH; c += nt) {
      const uint8_t tile = src[c];
      p[plane_index(a, c)] = (uint16_t)(tile == ORX_TILE_WALL ? kWall
                                        : tile == ORX_TILE_STAIRCASE_DOWN ? 0u : kFar);
    }
    __syncthreads();

    // 2. relax until a sweep changes nothing
    int changed;
    do {
      changed = 0;
      uint32_t carry = lo > 0 ? p[lo - 1] : kWall;
      for (int i = lo; i < hi; ++i) {  // forward: carry = the value at i - 1
        uint32_t v = p[i];
        if (v != kWall && v != 0u) {
          uint32_t m = carry;
          const uint32_t nx = i + 1 < N ? p[i + 1] : kWall;
          m = nx < m ? nx : m;
          if (i >= S) { const uint32_t u = p[i - S]; m = u < m ? u : m; }
          if (i + S < N) { const uint32_t u = p[i + S]; m = u < m ? u : m; }
          if (m + 1u < v) {  // (v <= kFar, so m < kFar - 1: a sentinel never spreads)
            v = m + 1u;
            p[i] = (uint16_t)v;
            changed = 1;
          }
        }
        carry = v;
      }
      carry = hi < N ? p[hi] : kWall;
      for (int i = hi - 1; i >= lo; --i) {  // backward: carry = the value at i + 1
        uint32_t v = p[i];
        if (v != kWall && v != 0u) {
          uint32_t m = carry;
          const uint32_t pv = i > 0 ? p[i - 1] : kWall;
          m = pv < m ? pv : m;
          if (i >= S) { const uint32_t u = p[i - S]; m = u < m ? u : m; }
          if (i + S < N) { const uint32_t u = p[i + S]; m = u < m ? u : m; }
          if (m + 1u < v) {
            v = m + 1u;
            p[i] = (uint16_t)v;
            changed = 1;
          }
        }
        carry = v;
      }
    } while (__syncthreads_or(changed));

    // 3. the plane's W * H cells, in tile order, to HBM
    uint16_t* dst = a.field + (size_t)l * (size_t)WH;
    int head = (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 1);
    head = head < WH ? head : WH;
    const int nvec = (WH - head) >> 3;
    for (int c = t; c < head; c += nt) dst[c] = p[plane_index(a, c)];
    uint4* vdst = reinterpret_cast<uint4*>(dst + head);
    for (int v = t; v < nvec; v += nt) {
      const int c0 = head + (v << 3);
      int x = c0 / a.H, y = c0 - x * a.H;
      uint32_t w[4];
      for (int k = 0; k < 4; ++k) {
        uint32_t pair = 0;
        for (int h = 0; h < 2; ++h) {
          const int i = a.ylong ? x * S + y + 1 : y * S + x + 1;
          pair |= (uint32_t)p[i] << (16 * h);
          if (++y == a.H) { y = 0; ++x; }
        }
        w[k] = pair;
      }
      vdst[v] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (int c = head + (nvec << 3) + t; c < WH; c += nt) dst[c] = p[plane_index(a, c)];
    __syncthreads();  // (the next layout overwrites the plane)
  }
}

// ---------------------------------------------------------------------------
// the rows of the pair table
// ---------------------------------------------------------------------------
// A layout's plane in LDS: runs along the grid's longer axis, one Wall
// sentinel between runs, before the first and after the last.
struct Plane {
  int32_t H, WH;
  int32_t ylong;  // runs along y (H >= W), else along x
  int32_t S;      // run stride: the longer side + 1
  int32_t N;      // plane entries: (shorter side) * S + 1

  static Plane of(int W, int H) {
    Plane g;
    g.H = H, g.WH = W * H;
    g.ylong = H >= W ? 1 : 0;
    g.S = (g.ylong ? H : W) + 1;
    g.N = (g.ylong ? W : H) * g.S + 1;
    return g;
  }
  size_t lds_bytes() const { return ((size_t)N * sizeof(uint16_t) + 15) & ~(size_t)15; }
  __device__ __forceinline__ int at(int x, int y) const {
    return ylong ? x * S + y + 1 : y * S + x + 1;
  }
  // plane index of flat tile index c = x * H + y
  __device__ __forceinline__ int index(int c) const {
    const int x = c / H;
    return at(x, c - x * H);
  }
};

// A staircase the walk may end on but not cross.  Below the sentinels and above every distance: a shortest path of
// 0xFFFD moves needs as many open tiles in a row with Walls between its turns,
// far more than the 65,536 tiles of the largest plane.
constexpr uint32_t kStair = 0xFFFD;

// Relaxes plane entries [lo, hi) of p, d = min(d, 1 + min(neighbours)), until a
// workgroup-wide vote finds a whole sweep without a change.  Wall, kStair and 0
// (a seed) keep their values; kStair and the sentinels never spread (m + 1 is
// not below kFar).  field_kernel's sweep with one more value to leave alone;
// the field keeps its own (sharing this one cost it 2.5 % of its time, measured).
__device__ __forceinline__ void relax_plane(volatile uint16_t* p, int lo, int hi, int S, int N) {
  auto open = [](uint32_t v) { return v != kWall && v != kStair && v != 0u; };
  int changed;
  do {
    changed = 0;
    uint32_t carry = lo > 0 ? p[lo - 1] : kWall;
    for (int i = lo; i < hi; ++i) {  // forward: carry = the value at i - 1
      uint32_t v = p[i];
      if (open(v)) {
        uint32_t m = carry;
        const uint32_t nx = i + 1 < N ? p[i + 1] : kWall;
        m = nx < m ? nx : m;
        if (i >= S) { const uint32_t u = p[i - S]; m = u < m ? u : m; }
        if (i + S < N) { const uint32_t u = p[i + S]; m = u < m ? u : m; }
        if (m + 1u < v) {  // (v <= kFar, so m < kFar - 1: a sentinel never spreads)
          v = m + 1u;
          p[i] = (uint16_t)v;
          changed = 1;
        }
      }
      carry = v;
    }
    carry = hi < N ? p[hi] : kWall;
    for (int i = hi - 1; i >= lo; --i) {  // backward: carry = the value at i + 1
      uint32_t v = p[i];
      if (open(v)) {
        uint32_t m = carry;
        const uint32_t pv = i > 0 ? p[i - 1] : kWall;
        m = pv < m ? pv : m;
        if (i >= S) { const uint32_t u = p[i - S]; m = u < m ? u : m; }
        if (i + S < N) { const uint32_t u = p[i + S]; m = u < m ? u : m; }
        if (m + 1u < v) {
          v = m + 1u;
          p[i] = (uint16_t)v;
          changed = 1;
        }
      }
      carry = v;
    }
  } while (__syncthreads_or(changed));
}

// The plane's W * H cells, value(plane index) each, in tile order to dst: 16
// bytes per lane, uint16 head / tail where dst does not start or end 16-byte
// aligned.
template <typename Value>
__device__ __forceinline__ void stream_plane(const Plane& g, uint16_t* dst, int t, int nt,
                                             Value value) {
  const int WH = g.WH;
  int head = (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 1);
  head = head < WH ? head : WH;
  const int nvec = (WH - head) >> 3;
  for (int c = t; c < head; c += nt) dst[c] = (uint16_t)value(g.index(c));
  uint4* vdst = reinterpret_cast<uint4*>(dst + head);
  for (int v = t; v < nvec; v += nt) {
    const int c0 = head + (v << 3);
    int x = c0 / g.H, y = c0 - x * g.H;
    uint32_t w[4];
    for (int k = 0; k < 4; ++k) {
      uint32_t pair = 0;
      for (int h = 0; h < 2; ++h) {
        pair |= (uint32_t)value(g.at(x, y)) << (16 * h);
        if (++y == g.H) { y = 0; ++x; }
      }
      w[k] = pair;
    }
    vdst[v] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  for (int c = head + (nvec << 3) + t; c < WH; c += nt) dst[c] = (uint16_t)value(g.index(c));
}

constexpr int kRowsPerThread = 64;    // plane entries a thread sweeps (ORX_ROWS_PER_THREAD=n: n)
constexpr int kRowsMaxGrid = 16384;                  // workgroups of one launch (grid-stride above)

struct RowsArgs {
  const uint8_t* tiles;
  const int32_t *layout, *cell;
  uint16_t* rows;
  int64_t n;
  int32_t L;
  Plane g;
};

__global__ __launch_bounds__(kFieldBlock) void rows_kernel(const RowsArgs a) {
  extern __shared__ uint4 smem[];
  volatile uint16_t* p = reinterpret_cast<volatile uint16_t*>(smem);
  const Plane g = a.g;
  const int t = threadIdx.x, nt = blockDim.x;
  const int S = g.S, N = g.N, WH = g.WH;
  const int per = (N + nt - 1) / nt;
  const int lo = t * per < N ? t * per : N, hi = lo + per < N ? lo + per : N;

  for (int64_t r = blockIdx.x; r < a.n; r += gridDim.x) {
    // 1. the sentinels and the tiles: Ground "not reached", the staircases
    // kStair; then the source, if it is a cell of the bank and not a Wall
    const int32_t lay = a.layout[r], c0 = a.cell[r];
    const bool in_bank = lay >= 0 && lay < a.L && c0 >= 0 && c0 < WH;
    for (int k = t * S; k < N; k += nt * S) p[k] = (uint16_t)kWall;
    const uint8_t* src = a.tiles + (size_t)clamp_layout(lay, a.L) * (size_t)WH;
    for (int c = t; c < WH; c += nt) {
      const uint8_t tile = src[c];
      p[g.index(c)] = (uint16_t)(tile == ORX_TILE_WALL ? kWall
                                 : in_bank && c == c0 ? 0u
                                 : tile == ORX_TILE_STAIRCASE_DOWN ? kStair : kFar);
    }
    __syncthreads();

    // 2. relax over Ground plus the source
    relax_plane(p, lo, hi, S, N);

    // 3. the row to HBM; a staircase other than the source ends a walk from
    // its nearest reached neighbour (the sentinels stop a step off a run; an
    // index test one off the first or last run)
    stream_plane(g, a.rows + (size_t)r * (size_t)WH, t, nt, [&](int i) -> uint32_t {
      const uint32_t v = p[i];
      if (v != kStair) return v;
      uint32_t m = p[i - 1];
      const uint32_t nx = p[i + 1];
      m = nx < m ? nx : m;
      if (i >= S) { const uint32_t u = p[i - S]; m = u < m ? u : m; }
      if (i + S < N) { const uint32_t u = p[i + S]; m = u < m ? u : m; }
      return m < kStair ? m + 1u : kFar;
    });
    __syncthreads();  // (the next row overwrites the plane)
  }
}

// ---------------------------------------------------------------------------
// the query
// ---------------------------------------------------------------------------
// header fields staged per game ([kHdr][G] int32 in LDS)
enum { H_PX, H_PY, H_SX, H_SY, H_LAYOUT, kHdr };

struct PathArgs {
  const int32_t *p_x, *p_y, *st_x, *st_y;
  const int16_t* p_layout;
  const uint16_t* field;
  int32_t* dist;
  int8_t* move;
  uint16_t* window;
  int64_t B;
  int32_t W, H, L, R, G, player;
  uint32_t inv_vv, inv_v;  // (R, G, inv_vv, inv_v: a Window, with `window`)
};

// the value of cell (x, y): `f` is the layout's plane of a bank (a.L > 0),
// (sx, sy) the staircase of the closed form
__device__ __forceinline__ uint32_t value_at(const PathArgs& a, const uint16_t* f, int x, int y,
                                             int sx, int sy) {
  if (x < 0 || x >= a.W || y < 0 || y >= a.H) return kWall;
  if (a.L > 0) return f[x * a.H + y];
  if (x == 0 || x == a.W - 1 || y == 0 || y == a.H - 1) return kWall;
  const int dx = x - sx, dy = y - sy;
  return (uint32_t)((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy));
}

__device__ __forceinline__ int32_t dist_of(uint32_t own) {
  return own == kFar ? -1 : (int32_t)own;
}

// the first of Up, Right, Down, Left whose target has the value own - 1
__device__ __forceinline__ int8_t move_of(uint32_t own, uint32_t up, uint32_t right, uint32_t down,
                                          uint32_t left) {
  if (own == 0u || own >= kFar) return ORX_MOVE_STAY;
  const uint32_t want = own - 1u;
  return up == want ? ORX_MOVE_UP : right == want ? ORX_MOVE_RIGHT : down == want ? ORX_MOVE_DOWN
         : left == want ? ORX_MOVE_LEFT : ORX_MOVE_STAY;
}

// no window: one lane per game, five values
__global__ __launch_bounds__(kBlock) void point_kernel(const PathArgs a) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= a.B) return;
  const int64_t me = player_rows(a.player, a.B, b).me;
  const int x = a.p_x[me], y = a.p_y[me];
  int sx = 0, sy = 0;
  const uint16_t* f = nullptr;
  if (a.L > 0) {
    f = a.field + (size_t)layout_of(a, me) * (size_t)(a.W * a.H);
  } else {
    sx = a.st_x[me], sy = a.st_y[me];
  }
  const uint32_t own = value_at(a, f, x, y, sx, sy);
  if (a.dist) a.dist[b] = dist_of(own);
  if (a.move)
    a.move[b] = move_of(own, value_at(a, f, x, y - 1, sx, sy), value_at(a, f, x + 1, y, sx, sy),
                        value_at(a, f, x, y + 1, sx, sy), value_at(a, f, x - 1, y, sx, sy));
}

__global__ __launch_bounds__(kBlock) void window_kernel(const PathArgs a) {
  extern __shared__ uint4 smem[];
  const Window win = Window::of(a.R, a.G, a.inv_vv, a.inv_v);
  const int G = win.G, R = win.R, V = win.V, VV = win.VV, H = a.H;
  uint16_t* tile = reinterpret_cast<uint16_t*>(smem);  // G * VV uint16 (G % 8 == 0: whole uint4s)
  int32_t* hdr = reinterpret_cast<int32_t*>(tile + G * VV);
  const int64_t B = a.B;
  const int64_t b0 = (int64_t)blockIdx.x * G;
  const int nb = (int)((B - b0) < (int64_t)G ? (B - b0) : (int64_t)G);
  const int t = threadIdx.x;

  // 1. the games' headers, coalesced over the games
  if (t < nb) {
    const int64_t me = player_rows(a.player, B, b0 + t).me;
    hdr[H_PX * G + t] = a.p_x[me];
    hdr[H_PY * G + t] = a.p_y[me];
    hdr[H_SX * G + t] = a.L > 0 ? 0 : a.st_x[me];
    hdr[H_SY * G + t] = a.L > 0 ? 0 : a.st_y[me];
    hdr[H_LAYOUT * G + t] = layout_of(a, me);
  }
  __syncthreads();

  // 2. the tile
  if (a.L == 0) {
    // the closed form: one thread per 8 consecutive cells of the tile (one
    // aligned 16-byte LDS store); they run over the end of a window row into
    // the next, and over a game's last row into the next game's first
    // (what a window row shares is computed once per row: x of its first
    // column, whether y is inside the border, |y - sy|)
    const int nvec = (nb * VV + 7) >> 3;
    const uint32_t W2 = (uint32_t)(a.W - 2), H2 = (uint32_t)(H - 2);  // interior: 1 .. W - 2
    for (int v = t; v < nvec; v += kBlock) {
      const Window::Cell first = win.split((uint32_t)v << 3);
      int g = first.g, j = first.j, i = first.i;
      int x0 = 0, sx = 0, ady = 0;
      bool yin = false;
      auto row = [&]() {
        const int y = hdr[H_PY * G + g] + j - R, dy = y - hdr[H_SY * G + g];
        x0 = hdr[H_PX * G + g] - R, sx = hdr[H_SX * G + g];
        yin = (uint32_t)(y - 1) < H2;
        ady = dy < 0 ? -dy : dy;
      };
      if (g < nb) row();
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (g < nb) {
          const int x = x0 + i, dx = x - sx;
          const uint32_t val = (yin && (uint32_t)(x - 1) < W2) ? (uint32_t)((dx < 0 ? -dx : dx) + ady)
                                                               : kWall;
          w[k >> 1] |= val << (16 * (k & 1));
          if (++i == V) {
            i = 0;
            if (++j == V) { j = 0; ++g; }
            if (g < nb) row();
          }
        }
      }
      reinterpret_cast<uint4*>(tile)[v] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  } else {
    // a bank: a fixed x with consecutive y is consecutive uint16 in the
    // field, so 16 (V <= 16) or 32 neighbouring lanes take one window column
    // -- one or two cache lines per column -- and write it down the tile's
    // column (the transpose)
    const int cols = nb * V, WH = a.W * H;
    const int shift = V <= 16 ? 4 : 5, j = t & ((1 << shift) - 1);
    if (j < V) {
      for (int col = t >> shift; col < cols; col += kBlock >> shift) {
        const int g = win.div_v((uint32_t)col), i = col - g * V;
        const int x = hdr[H_PX * G + g] + i - R, y = hdr[H_PY * G + g] + j - R;
        uint16_t val = (uint16_t)kWall;
        if ((uint32_t)x < (uint32_t)a.W && (uint32_t)y < (uint32_t)H)
          val = a.field[(size_t)hdr[H_LAYOUT * G + g] * (size_t)WH + (size_t)(x * H + y)];
        tile[g * VV + j * V + i] = val;
      }
    }
  }
  __syncthreads();

  // 3. dist and move from the tile's centre cells (R >= 1: all five are in it)
  if (t < nb) {
    const uint16_t* c = tile + t * VV + R * V + R;
    const uint32_t own = c[0];
    if (a.dist) a.dist[b0 + t] = dist_of(own);
    if (a.move) a.move[b0 + t] = move_of(own, c[-V], c[1], c[V], c[-1]);
  }

  // 4. the tile's nb * VV contiguous cells to HBM
  stream_out(tile, a.window + (size_t)b0 * (size_t)VV, nb * VV, t);
}

// ---------------------------------------------------------------------------
// seek: the walking distance and first move to the moving targets
// ---------------------------------------------------------------------------
struct SeekArgs {
  const int32_t *p_x, *p_y, *p_depth, *st_x, *st_y;
  const int16_t* p_layout;
  const uint8_t* bank_tiles;
  const uint16_t* npc_pos;
  const uint32_t* npc_alive;
  const uint16_t* item_pos;
  const uint32_t* item_mask;
  const uint16_t* pairs;
  int32_t* dist;
  int8_t* move;
  int16_t* target;
  int64_t B;
  int32_t W, H, K, L, player, npc_depth, items;
};

// the least distance of a column and the lowest slot attaining it
struct Nearest {
  uint32_t dist = kNoPath;
  int32_t slot = -1, tx = 0, ty = 0;
  __device__ __forceinline__ void offer(const Seeker& s, int32_t k, int tx_, int ty_) {
    const uint32_t d = s.inside(tx_, ty_) ? s.between(s.x, s.y, tx_, ty_) : kNoPath;
    if (slot < 0 || d < dist) dist = d, slot = k, tx = tx_, ty = ty_;
  }
};

__global__ __launch_bounds__(kBlock) void seek_kernel(const SeekArgs a) {
  const int64_t B = a.B;
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const int K = a.K;
  const auto [me, ot] = player_rows(a.player, B, b);

  Seeker s;
  s.W = a.W, s.H = a.H;
  s.x = a.p_x[me], s.y = a.p_y[me];
  s.sx = s.sy = -1, s.table = nullptr, s.tiles = nullptr;
  if (a.L > 0) {
    const size_t lay = (size_t)layout_of(a, me), WH = (size_t)(a.W * a.H);
    s.table = a.pairs + lay * WH * WH;
    s.tiles = a.bank_tiles + lay * WH;
  } else {
    s.sx = a.st_x[me], s.sy = a.st_y[me];
  }
  const int32_t d = a.p_depth[me];
  const bool here = s.inside(s.x, s.y);  // (a cell outside the grid has no targets)

  Nearest col[3];
  if (here && a.p_depth[ot] == d)
    col[ORX_SEEK_PLAYER].offer(s, 1 - a.player, a.p_x[ot], a.p_y[ot]);
  if (here && K > 0 && d == a.npc_depth) {
    // positions are x | y << 8, as npc_pos / item_pos pack them
    uint32_t alive = 0;
    for (int k = 0; k < K; ++k) {
      if ((k & 31) == 0) alive = a.npc_alive[(int64_t)(k >> 5) * B + b];
      if (!((alive >> (k & 31)) & 1u)) continue;
      const uint32_t pos = a.npc_pos[(int64_t)k * B + b];
      col[ORX_SEEK_NPC].offer(s, k, (int)(pos & 0xFFu), (int)(pos >> 8));
    }
    if (a.items) {
      const uint32_t on = a.item_mask[b];
      for (int k = 0; on >> k && k < K; ++k) {
        if (!((on >> k) & 1u)) continue;
        const uint32_t pos = a.item_pos[(int64_t)k * B + b];
        col[ORX_SEEK_ITEM].offer(s, k, (int)(pos & 0xFFu), (int)(pos >> 8));
      }
    }
  }

  uint32_t dist[3], move[3], target[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const Nearest& n = col[j];
    dist[j] = (uint32_t)(n.slot < 0 ? ORX_SEEK_ABSENT
                         : n.dist == kNoPath ? ORX_SEEK_UNREACHABLE : (int32_t)n.dist);
    move[j] = (uint32_t)(n.slot < 0 ? ORX_MOVE_STAY : s.move_to(n.dist, n.tx, n.ty));
    target[j] = (uint32_t)n.slot & 0xFFFFu;
  }

  // a game's row of each output: one store
  store_seek_rows(a.dist, a.move, b, dist[0], dist[1], dist[2], move[0], move[1], move[2]);
  if (a.target)
    reinterpret_cast<uint2*>(a.target)[b] =
        make_uint2(target[0] | target[1] << 16, target[2] | 0xFFFFu << 16);
}

// ---------------------------------------------------------------------------
// threat: the danger field and the move that flees it
// ---------------------------------------------------------------------------
struct ThreatArgs {
  const int32_t *p_x, *p_y, *p_depth, *st_x, *st_y;
  const int16_t* p_layout;
  const uint8_t* bank_tiles;
  const uint16_t* npc_pos;
  const uint32_t* npc_alive;
  const uint16_t* pairs;
  int32_t* dist;
  int8_t* move;
  int16_t* target;
  int32_t* after;
  uint16_t* window;
  int64_t B;
  int32_t W, H, K, L, player, npc_depth, R, G;
  uint32_t inv_vv, inv_v;  // (R, G, inv_vv, inv_v: a Window, with `window`)
};

// whether cell (cx, cy), in the grid, is Ground: what a flee move may step on
__device__ __forceinline__ bool ground(const Seeker& s, int cx, int cy) {
  if (s.tiles) return (s.tiles[cx * s.H + cy] & ORX_VIEW_TILE_MASK) == ORX_TILE_GROUND;
  return (uint32_t)(cx - 1) < (uint32_t)(s.W - 2) && (uint32_t)(cy - 1) < (uint32_t)(s.H - 2) &&
         !(cx == s.sx && cy == s.sy);
}

// One column's value -- the least walking distance to its threats, kNoPath
// where none reaches -- on the five cells a flee move chooses among: the own
// cell, then Up, Right, Down, Left (only the candidates of `cand`, bit j: cell
// j, are looked up); and the lowest slot attaining the own cell's.
struct Around {
  uint32_t v[5] = {kNoPath, kNoPath, kNoPath, kNoPath, kNoPath};
  int32_t slot = -1;
  __device__ __forceinline__ void offer(const Seeker& s, uint32_t cand, int32_t k, int tx, int ty) {
    const int cx[5] = {s.x, s.x, s.x + 1, s.x, s.x - 1}, cy[5] = {s.y, s.y - 1, s.y, s.y + 1, s.y};
    const bool in = s.inside(tx, ty);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const uint32_t d = in && ((cand >> j) & 1u) ? s.between(cx[j], cy[j], tx, ty) : kNoPath;
      if (j == 0 && (slot < 0 || d < v[0])) slot = k;
      v[j] = d < v[j] ? d : v[j];
    }
  }
  // a value in dist's convention
  __device__ __forceinline__ static uint32_t shown(uint32_t d) {
    return (uint32_t)(d == kNoPath ? ORX_SEEK_UNREACHABLE : (int32_t)d);
  }
  // Stay, then the first candidate that strictly gains on the best so far
  __device__ __forceinline__ uint32_t flee(uint32_t cand) const {
    uint32_t best = v[0], m = ORX_MOVE_STAY;
#pragma unroll
    for (int j = 1; j < 5; ++j)
      if (((cand >> j) & 1u) && v[j] > best) best = v[j], m = (uint32_t)(ORX_MOVE_UP + j - 1);
    return m;
  }
};

// game b's rows of dist, move, target and after: one lane, a loop over the
// live threats with five lookups in each one's row of the pair table (the own
// cell, y -+ 1 beside it, x -+ 1 at -+ H entries)
__device__ __forceinline__ void threat_rows(const ThreatArgs& a, int64_t b) {
  const int64_t B = a.B;
  const int K = a.K;
  const auto [me, ot] = player_rows(a.player, B, b);

  Seeker s;
  s.W = a.W, s.H = a.H;
  s.x = a.p_x[me], s.y = a.p_y[me];
  s.sx = s.sy = -1, s.table = nullptr, s.tiles = nullptr;
  if (a.L > 0) {
    const size_t lay = (size_t)layout_of(a, me), WH = (size_t)(a.W * a.H);
    s.table = a.pairs + lay * WH * WH;
    s.tiles = a.bank_tiles + lay * WH;
  } else {
    s.sx = a.st_x[me], s.sy = a.st_y[me];
  }
  const int32_t d = a.p_depth[me];
  const bool here = s.inside(s.x, s.y);  // (a cell outside the grid has no threats)

  // the candidates: the own cell, and the neighbours that are Ground
  uint32_t cand = 1u;
  if (here) {
    const int nx[4] = {s.x, s.x + 1, s.x, s.x - 1}, ny[4] = {s.y - 1, s.y, s.y + 1, s.y};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (s.inside(nx[j], ny[j]) && ground(s, nx[j], ny[j])) cand |= 2u << j;
  }

  Around col[3];
  if (here && a.p_depth[ot] == d)
    col[ORX_THREAT_PLAYER].offer(s, cand, 1 - a.player, a.p_x[ot], a.p_y[ot]);
  if (here && K > 0 && d == a.npc_depth) {
    uint32_t alive = 0;
    for (int k = 0; k < K; ++k) {
      if ((k & 31) == 0) alive = a.npc_alive[(int64_t)(k >> 5) * B + b];
      if (!((alive >> (k & 31)) & 1u)) continue;
      const uint32_t pos = a.npc_pos[(int64_t)k * B + b];
      col[ORX_THREAT_NPC].offer(s, cand, k, (int)(pos & 0xFFu), (int)(pos >> 8));
    }
  }
  // the union: the cellwise minimum; the player wins a tie
  const Around &p = col[ORX_THREAT_PLAYER], &n = col[ORX_THREAT_NPC];
  Around& u = col[ORX_THREAT_ANY];
#pragma unroll
  for (int j = 0; j < 5; ++j) u.v[j] = p.v[j] < n.v[j] ? p.v[j] : n.v[j];
  u.slot = p.slot >= 0 && (n.slot < 0 || p.v[0] <= n.v[0]) ? 2 - a.player
           : n.slot >= 0 ? 3 + n.slot : -1;

  uint32_t dist[3], move[3], target[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const Around& c = col[j];
    dist[j] = c.slot < 0 ? (uint32_t)ORX_SEEK_ABSENT : Around::shown(c.v[0]);
    move[j] = c.slot < 0 ? (uint32_t)ORX_MOVE_STAY : c.flee(cand);
    target[j] = (uint32_t)c.slot & 0xFFFFu;
  }

  // a game's row of each output: one store (after: two)
  store_seek_rows(a.dist, a.move, b, dist[0], dist[1], dist[2], move[0], move[1], move[2]);
  if (a.target)
    reinterpret_cast<uint2*>(a.target)[b] =
        make_uint2(target[0] | target[1] << 16, target[2] | 0xFFFFu << 16);
  if (a.after) {
    const uint32_t none = (uint32_t)ORX_SEEK_ABSENT;
    uint32_t w[5];
#pragma unroll
    for (int j = 0; j < 5; ++j)
      w[j] = u.slot >= 0 && ((cand >> j) & 1u) ? Around::shown(u.v[j]) : none;
    uint4* row = reinterpret_cast<uint4*>(a.after) + 2 * b;
    row[0] = make_uint4(none, w[1], w[2], w[3]);  // (column m: Move m; Stay is 5)
    row[1] = make_uint4(w[4], w[0], none, none);
  }
}

// no window: one lane per game
__global__ __launch_bounds__(kBlock) void threat_kernel(const ThreatArgs a) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b < a.B) threat_rows(a, b);
}

// header fields staged per game ([kThreatHdr][G] int32 in LDS)
// (T_OTHER: whether the other player hunts; T_NPCS: the live NPCs that do, in the grid)
enum { T_PX, T_PY, T_SX, T_SY, T_LAYOUT, T_OX, T_OY, T_OTHER, T_NPCS, kThreatHdr };

// LDS of a workgroup of G games: the tile, the headers, and the cells of the
// NPCs that hunt, uint16 [K][G] (x | y << 8, as npc_pos packs them)
inline size_t threat_lds(int G, int VV, int K) {
  return (size_t)G * VV * sizeof(uint16_t) + sizeof(int32_t) * G * kThreatHdr +
         sizeof(uint16_t) * G * K;
}

// window_kernel's staging.  A game's lane also lists the cells of the NPCs
// that hunt it in LDS (coalesced over the games, once per workgroup), so the
// tile's loop reads threats from LDS alone.  Every tile cell is owned by one
// lane for the whole loop over the game's threats -- it starts at Wall or
// "unreachable" and takes the minimum of each threat's distance -- so the loop
// has no atomics and no barrier.  A bank: 16 or 32 neighbouring lanes take a
// window column, which is consecutive uint16 in a threat's row of the pair
// table (window_kernel's transpose).  The room: a lane per cell, the closed
// form per threat.  The rows of the other outputs are threat_rows' by the
// first nb lanes, after the tile has left, so that the other waves retire
// meanwhile.
__global__ __launch_bounds__(kBlock) void threat_window_kernel(const ThreatArgs a) {
  extern __shared__ uint4 smem[];
  const Window win = Window::of(a.R, a.G, a.inv_vv, a.inv_v);
  const int G = win.G, R = win.R, V = win.V, VV = win.VV, W = a.W, H = a.H, K = a.K;
  uint16_t* tile = reinterpret_cast<uint16_t*>(smem);  // G * VV uint16 (G % 8 == 0: whole uint4s)
  int32_t* hdr = reinterpret_cast<int32_t*>(tile + G * VV);
  uint16_t* npcs = reinterpret_cast<uint16_t*>(hdr + kThreatHdr * G);  // [K][G]
  const int64_t B = a.B;
  const int64_t b0 = (int64_t)blockIdx.x * G;
  const int nb = (int)((B - b0) < (int64_t)G ? (B - b0) : (int64_t)G);
  const int t = threadIdx.x;

  // 1. the games' headers and threats, coalesced over the games
  if (t < nb) {
    const int64_t b = b0 + t;
    const auto [me, ot] = player_rows(a.player, B, b);
    const int x = a.p_x[me], y = a.p_y[me], ox = a.p_x[ot], oy = a.p_y[ot];
    const int32_t d = a.p_depth[me];
    const bool here = (uint32_t)x < (uint32_t)W && (uint32_t)y < (uint32_t)H;
    hdr[T_PX * G + t] = x;
    hdr[T_PY * G + t] = y;
    hdr[T_SX * G + t] = a.L > 0 ? 0 : a.st_x[me];
    hdr[T_SY * G + t] = a.L > 0 ? 0 : a.st_y[me];
    hdr[T_LAYOUT * G + t] = layout_of(a, me);
    hdr[T_OX * G + t] = ox;
    hdr[T_OY * G + t] = oy;
    hdr[T_OTHER * G + t] = here && a.p_depth[ot] == d && (uint32_t)ox < (uint32_t)W &&
                           (uint32_t)oy < (uint32_t)H;
    int n = 0;
    if (here && K > 0 && d == a.npc_depth) {
      uint32_t alive = 0;
      for (int k = 0; k < K; ++k) {
        if ((k & 31) == 0) alive = a.npc_alive[(int64_t)(k >> 5) * B + b];
        if (!((alive >> (k & 31)) & 1u)) continue;
        const uint32_t pos = a.npc_pos[(int64_t)k * B + b];
        if ((int)(pos & 0xFFu) < W && (int)(pos >> 8) < H) npcs[n++ * G + t] = (uint16_t)pos;
      }
    }
    hdr[T_NPCS * G + t] = n;
  }
  __syncthreads();

  // 2. the tile.  least(g, val, at): the least of at(tx, ty) over game g's
  // threats and of `val`
  auto least = [&](int g, uint32_t val, auto at) {
    if (hdr[T_OTHER * G + g]) {
      const uint32_t v = at(hdr[T_OX * G + g], hdr[T_OY * G + g]);
      val = v < val ? v : val;
    }
    const int n = hdr[T_NPCS * G + g];
    for (int k = 0; k < n; ++k) {
      const uint32_t pos = npcs[k * G + g];
      const uint32_t v = at((int)(pos & 0xFFu), (int)(pos >> 8));
      val = v < val ? v : val;
    }
    return val;
  };
  if (a.L == 0) {
    const int cells = nb * VV;
    for (int c = t; c < cells; c += kBlock) {
      const Window::Cell at = win.split((uint32_t)c);
      const int g = at.g, x = hdr[T_PX * G + g] + at.i - R, y = hdr[T_PY * G + g] + at.j - R;
      uint32_t val = kWall;
      if ((uint32_t)(x - 1) < (uint32_t)(W - 2) && (uint32_t)(y - 1) < (uint32_t)(H - 2)) {
        const int sx = hdr[T_SX * G + g], sy = hdr[T_SY * G + g];
        val = least(g, kFar, [&](int tx, int ty) { return room<kFar>(W, H, sx, sy, x, y, tx, ty); });
      }
      tile[c] = (uint16_t)val;
    }
  } else {
    const int cols = nb * V;
    const size_t WH = (size_t)(W * H);
    const int shift = V <= 16 ? 4 : 5, j = t & ((1 << shift) - 1);
    if (j < V) {
      for (int col = t >> shift; col < cols; col += kBlock >> shift) {
        const int g = win.div_v((uint32_t)col), i = col - g * V;
        const int x = hdr[T_PX * G + g] + i - R, y = hdr[T_PY * G + g] + j - R;
        uint32_t val = kWall;
        if ((uint32_t)x < (uint32_t)W && (uint32_t)y < (uint32_t)H) {
          const size_t lay = (size_t)hdr[T_LAYOUT * G + g], c = (size_t)(x * H + y);
          // (a game without a threat still shows its Walls)
          val = (a.bank_tiles[lay * WH + c] & ORX_VIEW_TILE_MASK) == ORX_TILE_WALL ? kWall : kFar;
          const uint16_t* column = a.pairs + lay * WH * WH + c;  // cell c of every row
          val = least(g, val, [&](int tx, int ty) -> uint32_t {
            return column[(size_t)(tx * H + ty) * WH];
          });
        }
        tile[g * VV + j * V + i] = (uint16_t)val;
      }
    }
  }
  __syncthreads();

  // 3. the tile's nb * VV contiguous cells to HBM
  stream_out(tile, a.window + (size_t)b0 * (size_t)VV, nb * VV, t);

  // 4. the other outputs' rows
  if (t < nb && (a.dist || a.move || a.target || a.after)) threat_rows(a, b0 + t);
}

// ---------------------------------------------------------------------------
// ticks: the staircase distance through the enemies
// ---------------------------------------------------------------------------
constexpr int kTicksPlanes = 3;           // open, and the emitting set twice
constexpr int kSlotPasses = 4;            // NPC slots a lane owns at most: slot k is lane k % 64's
constexpr uint32_t kWaiting = 0xFFFFFFFFu;  // a slot whose cell the wave has not met
constexpr uint32_t kNever = 0xFFFFFFFEu;    // a slot with nothing (more) to release

struct TicksArgs {
  const int32_t *p_x, *p_y, *p_depth, *st_x, *st_y, *p_rpg;
  const int16_t* p_layout;
  const uint16_t* npc_pos;
  const int8_t* npc_health;
  const uint32_t* npc_alive;
  const uint32_t* planes;
  int32_t* ticks;
  int8_t* move;
  uint16_t* window;
  int64_t B;
  int32_t W, H, WW, L, K, player, npc_depth, G, R;
  int32_t damage, armor, character;  // cfg's; character: the damage is p_rpg's
  int32_t game_words, tile_word;     // a game's LDS and its tile's offset in it, in uint32 (x 4)
  uint32_t inv_ww, inv_v;            // recip(WW) (WW > 1), recip(V)
};

// A WAVE IS A GAME, as in route_kernel, and the search is one Dijkstra
// backwards from the staircases, a bit-parallel step per tick of game time.
// Three planes of H * WW words in LDS: `open` (Ground not yet given a value)
// and the emitting set, double-buffered.  E(t), the emitting set of step t, is
// every cell c with enter(c) + T(c) == t: a free cell given its value at t - 1,
// a held cell hits(c) steps later (its RELEASE), a staircase from T = 0.  The
// cells beside E(t) that are still open get T = t and leave `open`; those no
// NPC holds are E(t + 1).  Values are given in nondecreasing order and a cell
// keeps the first, so this is Dijkstra.  Lane k % 64 owns NPC slot k (in
// kPasses passes, one while K <= 64): it sees its cell leave `open`, takes it out of the next
// emitting set and notes the step of its release, at which it puts it back --
// both lane by lane, so no two lanes change one word at once (no atomics).
// When a step gives no value, the wave jumps to the least pending release.
// The move needs no second search and no values kept: the own cell gets its
// value at the step t where a neighbour is in E(t), and the neighbours in
// E(t) are exactly those with enter + T == ticks.  Without a window the
// search ends there; with one it runs out, and every step writes t for the
// cells of the window it gives a value, into a V x V uint16 tile in LDS that
// the wave streams out at the end.  Steps only visit the rows that hold a
// valued cell, and one more each way.  Synchronisation is wave-local
// throughout (wave_sync), no workgroup barrier: searches differ in length.
template <int kPasses>
__global__ __launch_bounds__(kBlock) void ticks_kernel(const TicksArgs a) {
  extern __shared__ uint4 smem[];
  const int W = a.W, H = a.H, WW = a.WW, words = H * WW, K = a.K;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t B = a.B, b = (int64_t)blockIdx.x * a.G + wave;
  if (b >= B) return;  // (no workgroup barrier below: a wave is on its own)
  uint32_t* const lds = reinterpret_cast<uint32_t*>(smem) + (size_t)wave * (size_t)a.game_words;
  uint32_t* const open = lds;
  uint32_t* cur = lds + words;
  uint32_t* nxt = lds + 2 * words;
  uint16_t* const tile = reinterpret_cast<uint16_t*>(lds + a.tile_word);  // (16-byte aligned)

  const int64_t me = player_rows(a.player, B, b).me;
  const int px = a.p_x[me], py = a.p_y[me];
  const int R = a.R, V = 2 * R + 1, VV = V * V;
  const bool windowed = a.window != nullptr;
  const bool inside = (uint32_t)px < (uint32_t)W && (uint32_t)py < (uint32_t)H;
  // a window that holds a cell of the grid (else it is Wall throughout)
  const bool near = windowed && px >= -R && px < W + R && py >= -R && py < H + R;
  const int oi = inside ? py * WW + (px >> 5) : 0;
  const uint32_t obit = inside ? 1u << (px & 31) : 0u;

  // row of word i (< 2^16)
  auto row_of = [&](int i) { return WW == 1 ? i : (int)__umulhi((uint32_t)i, a.inv_ww); };

  int32_t ticks = -1;
  uint32_t mv = ORX_MOVE_STAY;
  if (inside || near) {
    // the planes: open = Ground, cur = the staircases; the rows that hold one
    const int last_word = (W - 1) >> 5;
    const uint32_t last_bit = 1u << ((W - 1) & 31);
    const uint32_t* ground = nullptr;
    int sx = -1, sy = -1;
    if (a.L > 0) ground = a.planes + (size_t)layout_of(a, me) * 2u * (size_t)words;
    else sx = a.st_x[me], sy = a.st_y[me];
    uint32_t first = (uint32_t)H, last_inv = ~0u;  // (the last row as its complement: a minimum)
    for (int i = lane; i < words; i += 64) {
      const int yy = row_of(i), xw = i - yy * WW;
      RoomWord w;
      if (ground) {
        w.ground = ground[i], w.stair = ground[words + i];
      } else {
        const uint32_t in = xw == last_word ? (last_bit << 1) - 1u : ~0u;
        w = room_word(W, H, sx, sy, yy, xw, last_word, last_bit, in);
      }
      open[i] = w.ground, cur[i] = w.stair, nxt[i] = 0u;
      if (w.stair) {
        first = (uint32_t)yy < first ? (uint32_t)yy : first;
        last_inv = ~(uint32_t)yy < last_inv ? ~(uint32_t)yy : last_inv;
      }
    }
    int lo = (int)wave_min(first), hi = (int)~wave_min(last_inv);
    wave_sync();

    // the window's tile as the tiles alone say it; the search fills in the rest
    if (windowed) {
      for (int c = lane; c < VV; c += 64) {
        const int j = (int)__umulhi((uint32_t)c, a.inv_v), x = px + (c - j * V) - R, y = py + j - R;
        uint32_t val = kWall;
        if (near && (uint32_t)x < (uint32_t)W && (uint32_t)y < (uint32_t)H) {
          const int wi = y * WW + (x >> 5);
          val = (cur[wi] >> (x & 31)) & 1u ? 0u : (open[wi] >> (x & 31)) & 1u ? kFar : kWall;
        }
        tile[c] = (uint16_t)val;
      }
    }
    const bool own_ground = inside && (open[oi] & obit), own_stair = inside && (cur[oi] & obit);
    if (own_stair) ticks = 0;

    // the NPC slots: a = max(damage - armor, 0) (past 127 every NPC falls at a blow)
    int64_t att = (int64_t)(a.character
                                ? a.p_rpg[(int64_t)(ORX_RPG_DAMAGE * 2 + a.player) * B + b]
                                : a.damage) - (int64_t)a.armor;
    att = att < 0 ? 0 : att > 127 ? 127 : att;
    uint32_t s_cell[kPasses], s_hits[kPasses], s_rel[kPasses];
    uint32_t on_stair = 0;  // bit p: pass p's slot stands on a staircase
    bool mine = false;
    const bool npcs_here = K > 0 && a.p_depth[me] == a.npc_depth;
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const int k = p * 64 + lane;
      s_cell[p] = 0u, s_hits[p] = 0u, s_rel[p] = kNever;
      if (!npcs_here || k >= K) continue;
      if (!((a.npc_alive[(int64_t)(k >> 5) * B + b] >> (k & 31)) & 1u)) continue;
      const uint32_t pos = a.npc_pos[(int64_t)k * B + b];
      const int x = (int)(pos & 0xFFu), y = (int)(pos >> 8);
      if (x >= W || y >= H) continue;
      const int wi = y * WW + (x >> 5);
      int h = a.npc_health[(int64_t)k * B + b];
      h = h < 1 ? 1 : h;
      s_cell[p] = (uint32_t)wi << 5 | (uint32_t)(x & 31);
      s_hits[p] = att > 0 ? (uint32_t)((h + (int)att - 1) / (int)att) : 0u;
      if ((open[wi] >> (x & 31)) & 1u) {
        s_rel[p] = kWaiting, mine = true;
      } else if ((cur[wi] >> (x & 31)) & 1u) {  // on a staircase: T = 0, held from the start
        s_rel[p] = att > 0 ? s_hits[p] + 1u : kNever, on_stair |= 1u << p, mine = true;
      }
    }
    const bool any_npc = __ballot(mine) != 0ull;
    wave_sync();  // (the tile and the slots have read the staircases)
    lane_by_lane(on_stair != 0u, lane, [&]() {
#pragma unroll
      for (int p = 0; p < kPasses; ++p)
        if ((on_stair >> p) & 1u) cur[s_cell[p] >> 5] &= ~(1u << (s_cell[p] & 31));
    });

    // The loop cannot stall.  A pass either gives a value to at least one open
    // cell -- at most W * H passes do -- or gives none; then it ends the
    // search, or jumps to the least pending release, which is then due at the
    // top of the next pass and is spent there -- at most K passes do.  t only
    // grows, by one or to a release later than t, and never passes a release:
    // one noted at step t is due at t + 2 or later.  So W * H + K + 1 passes
    // suffice; the bound below is the largest value, which is no less.
    const bool wanted = own_ground || near;
    const uint32_t bound = (uint32_t)(W * H + 128 * K + 1);
    uint32_t t = 1;
    for (uint32_t pass = 0; wanted && lo <= hi && pass < bound; ++pass) {
      // the releases due now join the emitting set
      if (any_npc) {
        bool due = false;
#pragma unroll
        for (int p = 0; p < kPasses; ++p) due |= s_rel[p] == t;
        lane_by_lane(due, lane, [&]() {
#pragma unroll
          for (int p = 0; p < kPasses; ++p)
            if (s_rel[p] == t) cur[s_cell[p] >> 5] |= 1u << (s_cell[p] & 31), s_rel[p] = kNever;
        });
      }

      // the step: the open cells beside the emitting set get T = t
      lo = lo > 0 ? lo - 1 : 0, hi = hi < H - 1 ? hi + 1 : H - 1;
      uint32_t grew = 0;
      for (int i = lo * WW + lane; i < (hi + 1) * WW; i += 64) {
        const int yy = row_of(i), xw = i - yy * WW;
        const uint32_t o = open[i];
        const uint32_t fresh = beside(cur, cur[i], i, yy, xw, WW, H) & o;
        nxt[i] = fresh;
        if (!fresh) continue;
        open[i] = o & ~fresh;
        grew |= fresh;
        const int j = yy - py + R;  // the window's row
        if (near && (uint32_t)j < (uint32_t)V) {
          const int x0 = px - R - xw * 32;  // the window's first column, as a bit of this word
          const int from = x0 > 0 ? x0 : 0, to = x0 + V - 1 < 31 ? x0 + V - 1 : 31;
          if (from <= to) {
            uint32_t m = fresh & ((2u << to) - 1u) & ~((1u << from) - 1u);
            for (; m; m &= m - 1) tile[j * V + __builtin_ctz(m) - x0] = (uint16_t)t;
          }
        }
      }
      wave_sync();

      // a held cell that got its value waits for its release
      if (any_npc) {
        bool met = false;
#pragma unroll
        for (int p = 0; p < kPasses; ++p) {
          if (s_rel[p] != kWaiting || ((open[s_cell[p] >> 5] >> (s_cell[p] & 31)) & 1u)) continue;
          s_rel[p] = t;  // (met now: marked by the step, replaced below)
          met = true;
        }
        lane_by_lane(met, lane, [&]() {
#pragma unroll
          for (int p = 0; p < kPasses; ++p)
            if (s_rel[p] == t) nxt[s_cell[p] >> 5] &= ~(1u << (s_cell[p] & 31));
        });
#pragma unroll
        for (int p = 0; p < kPasses; ++p)
          if (s_rel[p] == t) s_rel[p] = att > 0 ? t + s_hits[p] + 1u : kNever;
      }

      // the own cell: its value, and the first neighbour that emitted it
      if (own_ground && ticks < 0 && !(open[oi] & obit)) {
        ticks = (int32_t)t;
        bool step = false;
        if (lane < 4) {
          const int nx = px + (lane == 1) - (lane == 3), ny = py + (lane == 2) - (lane == 0);
          if ((uint32_t)nx < (uint32_t)W && (uint32_t)ny < (uint32_t)H)
            step = (cur[ny * WW + (nx >> 5)] >> (nx & 31)) & 1u;
        }
        const uint32_t nib = (uint32_t)__ballot(step) & 15u;
        mv = nib ? (uint32_t)(ORX_MOVE_UP + __builtin_ctz(nib)) : (uint32_t)ORX_MOVE_STAY;
        if (!near) break;
      }

      uint32_t* const swap = cur;
      cur = nxt, nxt = swap;
      if (__ballot(grew != 0u) != 0ull) {
        ++t;
        continue;
      }
      uint32_t pending = kNever;  // (a release noted is later than t)
#pragma unroll
      for (int p = 0; p < kPasses; ++p) pending = s_rel[p] < pending ? s_rel[p] : pending;
      pending = any_npc ? wave_min(pending) : kNever;
      if (pending >= kNever) break;
      t = pending;
    }
    wave_sync();
  } else if (windowed) {
    for (int c = lane; c < VV; c += 64) tile[c] = (uint16_t)kWall;
    wave_sync();
  }

  if (windowed) stream_out<uint16_t, 64>(tile, a.window + (size_t)b * (size_t)VV, VV, lane);
  if (lane != 0) return;
  if (a.ticks) a.ticks[b] = ticks;
  if (a.move) a.move[b] = (int8_t)mv;
}

}  // namespace orx_path_dev

#ifndef ORX_PATH_BUILD_ID
#define ORX_PATH_BUILD_ID "unknown"
#endif

extern "C" const char* orx_path_build_id(void) { return ORX_PATH_BUILD_ID; }

extern "C" int orx_path_field(const orx_cfg_t* cfg, const uint8_t* bank_tiles, uint16_t* field,
                              void* stream) {
  using namespace orx_path_dev;
  using orx_dev::fail;
  if (!cfg) return fail(ORX_EINVAL, "cfg is NULL");
  if (cfg->n_layouts < 1 || cfg->n_layouts > 32767)
    return fail(ORX_EINVAL, "orx_path_field: n_layouts must be in [1, 32767]");
  if (cfg->width < 1 || cfg->height < 1 || (int64_t)cfg->width * cfg->height > 65536)
    return fail(ORX_EINVAL, "orx_path_field: a bank needs W, H >= 1 and W * H <= 65536");
  if (!bank_tiles || !field) return fail(ORX_EINVAL, "orx_path_field: bank_tiles or field is NULL");

  FieldArgs a;
  a.tiles = bank_tiles, a.field = field;
  a.L = cfg->n_layouts, a.W = cfg->width, a.H = cfg->height, a.WH = a.W * a.H;
  a.ylong = a.H >= a.W ? 1 : 0;
  a.S = (a.ylong ? a.H : a.W) + 1;
  a.N = (a.ylong ? a.W : a.H) * a.S + 1;
  const size_t lds = ((size_t)a.N * sizeof(uint16_t) + 15) & ~(size_t)15;
  if (lds > (size_t)kDefaultLds &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(field_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return fail(ORX_EIO, "orx_path_field: the device refuses the LDS a layout's plane needs");
  }
  // about four plane entries per thread, whole waves, at most kFieldBlock
  int block = (((a.N + 3) / 4 + 63) / 64) * 64;
  block = block < 64 ? 64 : block > kFieldBlock ? kFieldBlock : block;
  const unsigned grid = (unsigned)(a.L < 2048 ? a.L : 2048);
  hipLaunchKernelGGL(field_kernel, dim3(grid), dim3((unsigned)block), lds, (hipStream_t)stream, a);
  return orx_dev::launch_status("orx_path_field");
}

extern "C" int orx_path_query(const orx_cfg_t* cfg, const orx_state_t* st, const uint16_t* field,
                              int32_t player, int32_t radius, int32_t* dist, int8_t* move,
                              uint16_t* window, int64_t n_games, void* stream) {
  using namespace orx_path_dev;
  using orx_dev::fail;
  int r;
  if ((r = orx_validate_cfg(cfg)) || (r = check_player("orx_path_query", player))) return r;
  if (!dist && !move && !window)
    return fail(ORX_EINVAL, "orx_path_query: dist, move and window are all NULL");
  if (window && (radius < 1 || radius > ORX_VIEW_MAX_RADIUS))
    return fail(ORX_EINVAL, "orx_path_query: radius must be in [1, ORX_VIEW_MAX_RADIUS]");
  if ((r = check_games("orx_path_query", n_games)) ||
      (r = check_state(cfg, st, cfg->n_layouts > 0 ? 0 : kStairs)))
    return r;
  if (cfg->n_layouts > 0) {
    if (!st->p_layout) return fail(ORX_EINVAL, "n_layouts > 0 needs p_layout");
    if (!field) return fail(ORX_EINVAL, "orx_path_query: n_layouts > 0 needs field");
  } else if ((int64_t)cfg->width + cfg->height - 6 >= (int64_t)ORX_PATH_UNREACHABLE) {
    // the closed form's largest value, (W - 3) + (H - 3), must stay below the sentinels
    return fail(ORX_EINVAL, "orx_path_query: W + H too large for uint16 distances");
  }

  PathArgs a;
  a.p_x = st->p_x, a.p_y = st->p_y, a.st_x = st->st_x, a.st_y = st->st_y;
  a.p_layout = st->p_layout;
  a.field = cfg->n_layouts > 0 ? field : nullptr;
  a.dist = dist, a.move = move, a.window = window;
  a.B = n_games;
  a.W = cfg->width, a.H = cfg->height, a.L = cfg->n_layouts;
  a.player = player;
  if (!window) {
    a.R = 0, a.G = 0, a.inv_vv = a.inv_v = 0;
    const unsigned grid = (unsigned)((n_games + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(point_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a);
    return orx_dev::launch_status("orx_path_query");
  }
  const Window win = Window::fit(radius, sizeof(uint16_t));
  const int G = win.G;
  a.R = win.R, a.G = G, a.inv_vv = win.inv_vv, a.inv_v = win.inv_v;
  const size_t lds = (size_t)G * win.VV * sizeof(uint16_t) + sizeof(int32_t) * G * kHdr;
  const unsigned grid = (unsigned)((n_games + G - 1) / G);
  hipLaunchKernelGGL(window_kernel, dim3(grid), dim3(kBlock), lds, (hipStream_t)stream, a);
  return orx_dev::launch_status("orx_path_query");
}

extern "C" int orx_path_rows(const orx_cfg_t* cfg, const uint8_t* bank_tiles, const int32_t* layout,
                             const int32_t* cell, uint16_t* rows, int64_t n, void* stream) {
  using namespace orx_path_dev;
  using orx_dev::fail;
  if (!cfg) return fail(ORX_EINVAL, "cfg is NULL");
  if (cfg->n_layouts < 1 || cfg->n_layouts > 32767)
    return fail(ORX_EINVAL, "orx_path_rows: n_layouts must be in [1, 32767]");
  if (cfg->width < 1 || cfg->height < 1 || (int64_t)cfg->width * cfg->height > 65536)
    return fail(ORX_EINVAL, "orx_path_rows: a bank needs W, H >= 1 and W * H <= 65536");
  if (!bank_tiles || !layout || !cell || !rows)
    return fail(ORX_EINVAL, "orx_path_rows: bank_tiles, layout, cell or rows is NULL");
  if (n <= 0) return fail(ORX_EINVAL, "orx_path_rows: n must be positive");

  RowsArgs a;
  a.tiles = bank_tiles, a.layout = layout, a.cell = cell, a.rows = rows;
  a.n = n, a.L = cfg->n_layouts;
  a.g = Plane::of(cfg->width, cfg->height);
  const size_t lds = a.g.lds_bytes();
  if (lds > (size_t)kDefaultLds &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(rows_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return fail(ORX_EIO, "orx_path_rows: the device refuses the LDS a layout's plane needs");
  }
  // kRowsPerThread plane entries per thread (tools/bench_seek.py measures
  // others through the environment), whole waves, at most kFieldBlock
  int per = kRowsPerThread;
  if (const char* e = getenv("ORX_ROWS_PER_THREAD")) per = atoi(e) >= 1 ? atoi(e) : per;
  int block = (((a.g.N + per - 1) / per + 63) / 64) * 64;
  block = block > kFieldBlock ? kFieldBlock : block;
  const unsigned grid = (unsigned)(n < kRowsMaxGrid ? n : kRowsMaxGrid);
  hipLaunchKernelGGL(rows_kernel, dim3(grid), dim3((unsigned)block), lds, (hipStream_t)stream, a);
  return orx_dev::launch_status("orx_path_rows");
}

extern "C" int orx_path_seek(const orx_cfg_t* cfg, const orx_state_t* st, const uint16_t* pairs,
                             int32_t player, int32_t* dist, int8_t* move, int16_t* target,
                             int64_t n_games, void* stream) {
  using namespace orx_path_dev;
  using orx_dev::fail;
  int r;
  if ((r = orx_validate_cfg(cfg)) || (r = check_player("orx_path_seek", player))) return r;
  if (!dist && !move && !target)
    return fail(ORX_EINVAL, "orx_path_seek: dist, move and target are all NULL");
  if ((r = check_games("orx_path_seek", n_games))) return r;
  // (a row is one vector store)
  if (misaligned(dist, 16) || misaligned(move, 4) || misaligned(target, 8))
    return fail(ORX_EINVAL,
                "orx_path_seek: dist must be 16-byte, move 4-byte and target 8-byte aligned");
  if ((r = check_state(cfg, st, kStairsNoBank | kBank | kNpcs | kItems))) return r;
  if (!st->p_depth) return fail(ORX_EINVAL, "a required state pointer is NULL");
  if (cfg->n_layouts > 0 && !pairs)
    return fail(ORX_EINVAL, "orx_path_seek: n_layouts > 0 needs pairs");

  SeekArgs a;
  a.p_x = st->p_x, a.p_y = st->p_y, a.p_depth = st->p_depth;
  a.st_x = st->st_x, a.st_y = st->st_y;
  a.p_layout = st->p_layout, a.bank_tiles = st->bank_tiles;
  a.npc_pos = st->npc_pos, a.npc_alive = st->npc_alive;
  a.item_pos = st->item_pos, a.item_mask = st->item_mask;
  a.pairs = cfg->n_layouts > 0 ? pairs : nullptr;
  a.dist = dist, a.move = move, a.target = target;
  a.B = n_games;
  a.W = cfg->width, a.H = cfg->height, a.K = cfg->n_npcs, a.L = cfg->n_layouts;
  a.player = player;
  a.npc_depth = npc_depth(cfg);
  a.items = has_items(cfg) ? 1 : 0;
  const unsigned grid = (unsigned)((n_games + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(seek_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a);
  return orx_dev::launch_status("orx_path_seek");
}

extern "C" int orx_path_threat(const orx_cfg_t* cfg, const orx_state_t* st, const uint16_t* pairs,
                               int32_t player, int32_t radius, int32_t* dist, int8_t* move,
                               int16_t* target, int32_t* after, uint16_t* window, int64_t n_games,
                               void* stream) {
  using namespace orx_path_dev;
  using orx_dev::fail;
  int r;
  if ((r = orx_validate_cfg(cfg)) || (r = check_player("orx_path_threat", player))) return r;
  if (!dist && !move && !target && !after && !window)
    return fail(ORX_EINVAL, "orx_path_threat: dist, move, target, after and window are all NULL");
  if (window && (radius < 1 || radius > ORX_VIEW_MAX_RADIUS))
    return fail(ORX_EINVAL, "orx_path_threat: radius must be in [1, ORX_VIEW_MAX_RADIUS]");
  if ((r = check_games("orx_path_threat", n_games))) return r;
  // (a row is one vector store, after's two)
  if (misaligned(dist, 16) || misaligned(move, 4) || misaligned(target, 8) ||
      misaligned(after, 16) || misaligned(window, 2))
    return fail(ORX_EINVAL,
                "orx_path_threat: dist and after must be 16-byte, move 4-byte, target 8-byte and "
                "window 2-byte aligned");
  if ((r = check_state(cfg, st, kStairsNoBank | kBank | kNpcs))) return r;
  if (!st->p_depth) return fail(ORX_EINVAL, "a required state pointer is NULL");
  if (cfg->n_layouts > 0) {
    if (!pairs) return fail(ORX_EINVAL, "orx_path_threat: n_layouts > 0 needs pairs");
  } else if (window && (int64_t)cfg->width + cfg->height - 4 >= (int64_t)ORX_PATH_UNREACHABLE) {
    // the closed form's largest value, (W - 3) + (H - 3) + 2, must stay below the sentinels
    return fail(ORX_EINVAL, "orx_path_threat: W + H too large for a window of uint16 distances");
  }

  ThreatArgs a;
  a.p_x = st->p_x, a.p_y = st->p_y, a.p_depth = st->p_depth;
  a.st_x = st->st_x, a.st_y = st->st_y;
  a.p_layout = st->p_layout, a.bank_tiles = st->bank_tiles;
  a.npc_pos = st->npc_pos, a.npc_alive = st->npc_alive;
  a.pairs = cfg->n_layouts > 0 ? pairs : nullptr;
  a.dist = dist, a.move = move, a.target = target, a.after = after, a.window = window;
  a.B = n_games;
  a.W = cfg->width, a.H = cfg->height, a.K = cfg->n_npcs, a.L = cfg->n_layouts;
  a.player = player;
  a.npc_depth = npc_depth(cfg);
  if (!window) {
    a.R = 0, a.G = 0, a.inv_vv = a.inv_v = 0;
    const unsigned grid = (unsigned)((n_games + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(threat_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a);
    return orx_dev::launch_status("orx_path_threat");
  }
  // (fewer games where the NPCs' cells would not fit beside the tile: 16 always do)
  Window win = Window::fit(radius, sizeof(uint16_t));
  while (win.G > 16 && threat_lds(win.G, win.VV, a.K) > (size_t)kDefaultLds)
    win = Window::fit(radius, sizeof(uint16_t), win.G >> 1);
  const int G = win.G;
  a.R = win.R, a.G = G, a.inv_vv = win.inv_vv, a.inv_v = win.inv_v;
  const size_t lds = threat_lds(G, win.VV, a.K);
  const unsigned grid = (unsigned)((n_games + G - 1) / G);
  hipLaunchKernelGGL(threat_window_kernel, dim3(grid), dim3(kBlock), lds, (hipStream_t)stream, a);
  return orx_dev::launch_status("orx_path_threat");
}

extern "C" int orx_path_ticks(const orx_cfg_t* cfg, const orx_state_t* st, const uint32_t* planes,
                              int32_t player, int32_t radius, int32_t* ticks, int8_t* move,
                              uint16_t* window, int64_t n_games, void* stream) {
  using namespace orx_path_dev;
  using orx_dev::fail;
  int r;
  if ((r = orx_validate_cfg(cfg)) || (r = check_player("orx_path_ticks", player))) return r;
  if (!ticks && !move && !window)
    return fail(ORX_EINVAL, "orx_path_ticks: ticks, move and window are all NULL");
  if (window && (radius < 1 || radius > ORX_VIEW_MAX_RADIUS))
    return fail(ORX_EINVAL, "orx_path_ticks: radius must be in [1, ORX_VIEW_MAX_RADIUS]");
  if (misaligned(ticks, 4) || misaligned(window, 2) || misaligned(planes, 4))
    return fail(ORX_EINVAL,
                "orx_path_ticks: ticks and planes must be 4-byte and window 2-byte aligned");
  if ((r = check_games("orx_path_ticks", n_games))) return r;
  if ((int64_t)cfg->width * cfg->height > 65536)
    return fail(ORX_EINVAL, "orx_path_ticks: a plane's words must fit 16 bits (W * H <= 65536)");
  if ((r = check_state(cfg, st, kStairsNoBank | kBank | kNpcs | kCharacter))) return r;
  if (!st->p_depth) return fail(ORX_EINVAL, "a required state pointer is NULL");
  if (cfg->n_layouts > 0 && !planes)
    return fail(ORX_EINVAL, "orx_path_ticks: n_layouts > 0 needs planes");
  // the largest value, every cell entered once and every NPC at 127 hits, must
  // stay below the sentinels
  if (window && (int64_t)cfg->width * cfg->height + 127 * (int64_t)cfg->n_npcs >=
                    (int64_t)ORX_PATH_UNREACHABLE)
    return fail(ORX_EINVAL, "orx_path_ticks: W * H + 127 * n_npcs too large for a window of "
                            "uint16 values");
  if (cfg->n_npcs > 64 * kSlotPasses) return fail(ORX_EINVAL, "orx_path_ticks: too many NPCs");

  TicksArgs a;
  a.p_x = st->p_x, a.p_y = st->p_y, a.p_depth = st->p_depth;
  a.st_x = st->st_x, a.st_y = st->st_y, a.p_rpg = st->p_rpg;
  a.p_layout = st->p_layout;
  a.npc_pos = st->npc_pos, a.npc_health = st->npc_health, a.npc_alive = st->npc_alive;
  a.planes = cfg->n_layouts > 0 ? planes : nullptr;
  a.ticks = ticks, a.move = move, a.window = window;
  a.B = n_games;
  a.W = cfg->width, a.H = cfg->height, a.WW = (cfg->width + 31) / 32, a.L = cfg->n_layouts;
  a.K = cfg->n_npcs, a.player = player, a.npc_depth = npc_depth(cfg);
  a.R = window ? radius : 0;
  a.damage = cfg->player_damage, a.armor = cfg->player_armor;
  a.character = (cfg->flags & ORX_EXT_CHARACTER) ? 1 : 0;
  a.inv_ww = recip(a.WW > 1 ? a.WW : 2);
  a.inv_v = recip(2 * a.R + 1);
  // a wave per game: three planes and the window's tile, each a whole number of uint4
  const int V = 2 * a.R + 1;
  a.tile_word = (kTicksPlanes * a.H * a.WW + 3) & ~3;
  a.game_words = a.tile_word + (window ? ((V * V + 1) / 2 + 3) & ~3 : 0);
  const size_t game_bytes = sizeof(uint32_t) * (size_t)a.game_words;
  const int G = a.G = games_per_workgroup(game_bytes);
  const size_t lds = (size_t)G * game_bytes;
  // (narrow and tall, W <= 64 and H in the thousands: three planes pass the CU's 160 KiB)
  if (lds > 160 * 1024)
    return fail(ORX_EIO, "orx_path_ticks: a game's planes need more LDS than the device has");
  if (lds > (size_t)kDefaultLds) {
    // (above the default limit of dynamic LDS: asked for once)
    static const hipError_t raised =
        hipFuncSetAttribute(reinterpret_cast<const void*>(ticks_kernel<1>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess
            ? hipErrorInvalidValue
            : hipFuncSetAttribute(reinterpret_cast<const void*>(ticks_kernel<kSlotPasses>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (raised != hipSuccess) {
      (void)hipGetLastError();
      return fail(ORX_EIO, "orx_path_ticks: the device refuses the LDS a game's planes need");
    }
  }
  const unsigned grid = (unsigned)((n_games + G - 1) / G);
  // (a lane owns one slot while K <= 64: the form without the passes' loops)
  if (a.K <= 64)
    hipLaunchKernelGGL(ticks_kernel<1>, dim3(grid), dim3(64 * G), lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(ticks_kernel<kSlotPasses>, dim3(grid), dim3(64 * G), lds,
                       (hipStream_t)stream, a);
  return orx_dev::launch_status("orx_path_ticks");
}
