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
// Plain C++ and vector stores only.
#include "../../include/orx_path.h"
#include "orx_query.h"

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
