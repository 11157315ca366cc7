// orx_plan.h -- the launch plan: the one place where the shape of an
// orx_rollout, orx_step_n or orx_env_step launch is decided (kernel family,
// policy mode, games per wave, store policy, threads, workgroups, dynamic
// LDS).  The entry points of orx_engine.hip validate, ask for a plan, pick the
// kernel instance it names and launch it; orx_rollout_shape reports the
// rollout's plan.  Plain C++17 over include/orx.h: no HIP, so a host compiler
// builds it alone (tests/test_plan.py).  Measurements behind the rules:
// DESIGN.md s7.1 "Launch plan".
#pragma once

#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/orx.h"

extern "C" char** environ;

#ifndef ORX_ROLLOUT_BLOCK  // (orx_engine.hip's compile-time switch; its one default)
#define ORX_ROLLOUT_BLOCK 256
#endif

namespace orx_dev {

constexpr int kBlock = 256;  // threads per workgroup of every launch without a plan of its own
constexpr int kDense = 256;  // NCAP of the dense-NPC instances (K > ORX_MAX_REG_NPCS)
// dynamic LDS per workgroup: the default limit (more needs the launch to
// raise the kernel's own), and the most a device is assumed to grant
inline constexpr uint32_t kMaxLdsTiles = 64 * 1024;
inline constexpr uint32_t kMaxLdsBlock = 160 * 1024;  // LDS per CU (one workgroup may take it all)
constexpr uint32_t kMinLanes = 16;  // games per one-lane wave, at least

// NPC slot capacity of the kernel instance for K NPCs.
inline int ncap_for(int K) {
  return K == 0 ? 0 : K <= 8 ? 8 : K <= ORX_MAX_REG_NPCS ? 16 : kDense;
}

// The moving-NPC kernels serve this configuration (NPCs that move) -- and,
// whatever its npc_policy, every call that brings the NPCs' moves with it
// (given_moves: the orx_npc_* entry points, include/orx_npc.h)
inline bool moving_npcs(const orx_cfg_t* c, bool given_moves = false) {
  return (c->npc_policy != ORX_NPC_STAY || given_moves) && c->n_npcs > 0;
}

// What the plan needs of the device (the engine fills it from its per-device
// caches; 1,024 SIMDs and kMaxLdsBlock without a device).
struct Device {
  int simds;
  uint32_t lds_per_block;  // dynamic LDS one workgroup may declare, with the opt-in raise
};

// The runtime overrides, for measurements and tests: every ORX_* environment
// variable that steers a launch (DESIGN.md lists them with their readers).
struct Env {
  int rollout_lanes = 0;          // ORX_ROLLOUT_LANES: games per wave, a power of two 1..64
  bool rollout_paired = true;     // ORX_ROLLOUT_PAIRED=0: never a paired form
  int rollout_threads = 0;        // ORX_ROLLOUT_THREADS: 64 / 128 / 256 (512: paired banks)
  uint32_t mov_lanes = 64;        // ORX_MOV_LANES: a power of two 1..64
  uint32_t env_lanes = 64;        // ORX_ENV_LANES: 32 / 64
  bool env_direct_rows = false;   // ORX_ENV_DIRECT_ROWS=1: orx_env_step's rows not through LDS
  bool replay_paired = true;      // ORX_REPLAY_PAIRED=0: orx_step_n's one-lane replay
  bool step_n_generic = false;    // ORX_STEP_N_GENERIC=1: orx_step_n's generic kernel
  bool no_lds_tiles = false;      // ORX_NO_LDS_TILES (set): a bank's tiles stay in global memory
  bool no_lds_bits = false;       // ORX_NO_LDS_BITS (set): no dense-NPC bitmaps in LDS
  bool refuse_lds_raise = false;  // ORX_REFUSE_LDS_RAISE=1: as if the runtime refused a raise
};

inline int lanes_value(const char* v) {
  const int x = atoi(v);
  return (x >= 1 && x <= 64 && (x & (x - 1)) == 0) ? x : 0;
}

// Read at every launch, so a sweep or a test can change them in-process: one
// pass over the environment (a launch costs less host time than with a getenv
// per variable).
inline Env read_env() {
  Env e;
  for (char** p = environ; p && *p; ++p) {
    const char* s = *p;
    if (s[0] != 'O' || s[1] != 'R' || s[2] != 'X' || s[3] != '_') continue;
    const char* v = nullptr;
    auto is = [&](const char* name) {
      const size_t len = strlen(name);
      if (strncmp(s + 4, name, len) != 0 || s[4 + len] != '=') return false;
      v = s + 5 + len;
      return true;
    };
    if (is("ROLLOUT_LANES")) e.rollout_lanes = lanes_value(v);
    else if (is("ROLLOUT_PAIRED")) e.rollout_paired = v[0] != '0';
    else if (is("ROLLOUT_THREADS")) {
      const int x = atoi(v);
      e.rollout_threads = (x == 64 || x == 128 || x == 256 || x == 512) ? x : 0;
    }
    else if (is("MOV_LANES")) e.mov_lanes = lanes_value(v) ? (uint32_t)lanes_value(v) : 64u;
    else if (is("ENV_LANES")) e.env_lanes = atoi(v) == 32 ? 32u : 64u;
    else if (is("ENV_DIRECT_ROWS")) e.env_direct_rows = v[0] == '1';
    else if (is("REPLAY_PAIRED")) e.replay_paired = v[0] != '0';
    else if (is("STEP_N_GENERIC")) e.step_n_generic = v[0] == '1';
    else if (is("NO_LDS_TILES")) e.no_lds_tiles = true;
    else if (is("NO_LDS_BITS")) e.no_lds_bits = true;
    else if (is("REFUSE_LDS_RAISE")) e.refuse_lds_raise = v[0] == '1';
  }
  return e;
}

enum class Form {
  kMoving,   // the moving-NPC kernels (lane_rollout_kernel / step_n_kernel / env_step_kernel MOV)
  kMt,       // stock-seed mode (lane_rollout_kernel<N, G, true, false>)
  kPaired,   // pair_rollout_kernel: two lanes per game
  kOneLane,  // rollout_kernel: one lane per game
  kReplay,   // replay_kernel: orx_step_n's one-lane replay under the rollout's tick
  kGeneric   // step_n_kernel / env_step_kernel
};

// Everything a launch needs besides its pointers.
struct Plan {
  Form form;
  int pm;               // the rollout kernels' policy mode (0: the generic form; 6: a move log)
  uint32_t lanes;       // games per wave
  bool nt;              // nontemporal trajectory stores (else the default policy)
  uint32_t threads;     // per workgroup
  uint32_t blocks;      // workgroups
  uint32_t lds_bytes;   // dynamic LDS per workgroup (above kMaxLdsTiles: after a limit raise)
  uint32_t lds_n;       // of them a bank's tiles (0: the kernel reads them from global memory)
  uint32_t lds_bits;    // dense NPCs: bytes of one game's occupancy bitmap in LDS (0: none)
  bool lds_rows;        // orx_env_step: the rows through LDS and 16-byte stores
};

// Workgroups for B games at `lanes` games per wave and `threads` per workgroup.
inline uint32_t blocks_for(uint64_t B, uint32_t lanes, uint32_t threads) {
  const uint64_t per_block = threads / 64u * lanes;
  return (uint32_t)((B + per_block - 1) / per_block);
}

// Games per one-lane rollout wave.  A rollout lane runs its game's whole tick
// stream, so a wave's time is set by its instruction stream, not by how many
// of its lanes are busy: a batch too small to put a wave on every SIMD is
// spread over more, narrower waves, which also take the rare block on fewer
// ticks (C5 at 16,384 games: 232 us per 128-tick launch at 64 games per wave,
// 158 at 16).  Not below 16: narrower waves share each 128-B trajectory line
// among four or more waves, and launches took twice as long (C2 at 4,096
// games: 77 us at 16, 155 at 8).  Two half-full waves per SIMD lose to one
// full one (C3: 101 us at 64, 130 at 32), so the rule is "at most one wave per
// SIMD until the wave is full".
inline uint32_t one_lane_lanes(uint32_t B, const Env& env, const Device& dev) {
  if (env.rollout_lanes) return (uint32_t)env.rollout_lanes;
  uint32_t L = 64;
  while (L > kMinLanes && (uint64_t)B < (uint64_t)dev.simds * L) L >>= 1;
  return L;
}

// Games per paired wave, rollout and replay alike: two waves per SIMD --
// counting the `concurrency` launches that share the device
// (StreamShardedEngine's shards) -- until the wave holds 32 games, at least 8
// (C5's 8-GPU share, 16,384 games: 8 per wave, 79 us per launch against 89 at
// 16 and 112 at 32; C2 at 4,096: 50 against 51; the bench's two 32,768-game
// C3 shards: 32 per wave, 96.6 us per step against 158 at 16, four waves per
// SIMD where 156 VGPRs fit three).
inline uint32_t paired_lanes(uint32_t B, uint32_t concurrency, const Env& env, const Device& dev) {
  if (env.rollout_lanes) return env.rollout_lanes < 32 ? (uint32_t)env.rollout_lanes : 32u;
  uint32_t L = 32;
  while (L > 8 && (uint64_t)B * concurrency < 2 * (uint64_t)dev.simds * L) L >>= 1;
  return L;
}

// The buffer-store forms address one tick's obs rows with 32-bit offsets.
inline bool rows_fit(uint32_t B) { return (uint64_t)B * ORX_OBS_FIELDS * 4u < (1ull << 31); }

// The policy mode of an orx_rollout launch before its form is known.
inline int rollout_pm(const orx_cfg_t* cfg, int32_t p1, int32_t p2, uint32_t B, bool traj) {
  const bool both_random = p1 == ORX_POLICY_RANDOM && p2 == ORX_POLICY_RANDOM;
  return !(traj && rows_fit(B)) ? 0
         : (cfg->flags == 0 && both_random) ? 1
         : ((cfg->flags & ~ORX_EXT_SEPARATION_DAMAGE) == 0 && p1 == ORX_POLICY_STAIRCASE &&
            p2 == ORX_POLICY_STAIRCASE) ? 2
         : ((cfg->flags | ORX_EXT_HEAL) == ORX_EXT_RPG && both_random &&
            ncap_for(cfg->n_npcs) != kDense) ? 3   // (no dense-NPC instance of PM 3)
         // one RandomBot against one StaircaseBot: paired forms only (PM 4 /
         // 5; a launch that does not pair takes the generic form)
         : (cfg->flags == 0 && p1 == ORX_POLICY_RANDOM && p2 == ORX_POLICY_STAIRCASE) ? 4
         : (cfg->flags == 0 && p1 == ORX_POLICY_STAIRCASE && p2 == ORX_POLICY_RANDOM) ? 5
         : 0;
}

struct RolloutRequest {
  const orx_cfg_t* cfg;  // (checked)
  int32_t p1, p2;        // the players' policies
  uint32_t B;            // games
  bool trajectory;       // obs and act both given
  bool compact;          // ORX_OBS_COMPACT rows
  uint32_t concurrency;  // launches that share the device
};

// The plan of an orx_rollout launch.  allow_raise false: no dynamic LDS above
// the default limit -- what a launch asks for after the runtime refused to
// raise the limit of the instance the first plan named.
inline Plan plan_rollout(const RolloutRequest& q, const Env& env, const Device& dev,
                         bool allow_raise = true) {
  const orx_cfg_t* cfg = q.cfg;
  const uint32_t B = q.B;
  Plan p{};
  p.nt = true;
  p.threads = kBlock;
  if (moving_npcs(cfg)) {  // one game per lane; 64 per wave: the tick is issue-bound, so
    p.form = Form::kMoving;  // fewer only add waves (32 / 16 / 8 measured equal or slower)
    p.lanes = env.mov_lanes;
    p.blocks = blocks_for(B, p.lanes, p.threads);
    return p;
  }
  if (cfg->rng == ORX_RNG_MT19937) {  // one game per lane, full waves
    p.form = Form::kMt;
    p.lanes = 64;
    p.blocks = blocks_for(B, p.lanes, p.threads);
    return p;
  }
  const int nc = ncap_for(cfg->n_npcs);
  const bool grid = cfg->n_layouts > 0;
  const bool sepd = (cfg->flags & ORX_EXT_SEPARATION_DAMAGE) != 0;
  p.pm = rollout_pm(cfg, q.p1, q.p2, B, q.trajectory);
  // compact rows: the buffer-store forms of PM 1 / 2 without a bank or dense
  // NPCs have compact instances; every other launch takes the generic form,
  // whose writer reads the format at run time
  if (q.compact && (p.pm >= 3 || grid || nc == kDense)) p.pm = 0;
  allow_raise = allow_raise && !env.refuse_lds_raise;
  auto fits = [&](uint32_t bytes) {
    return bytes <= kMaxLdsTiles || (allow_raise && bytes <= dev.lds_per_block);
  };
  // a bank's tiles are staged in LDS up to the device's per-workgroup limit
  const uint64_t tiles = grid ? (uint64_t)cfg->n_layouts * (uint64_t)(cfg->width * cfg->height) : 0;
  p.lds_n = (tiles && tiles <= dev.lds_per_block && !env.no_lds_tiles) ? (uint32_t)tiles : 0u;
  p.lanes = one_lane_lanes(B, env, dev);
  // The paired form: K <= 16 NPCs in registers, cells packed x | y << 8, the
  // RandomBot / StaircaseBot / character / mixed-bot trajectory forms, for
  // batches the one-lane rule leaves below 64 games per wave; a bank only as
  // PM 1 / 3 or PM 2 without separation damage, and only with its tiles in
  // LDS (the paired tick reads them nowhere else): where they need a raise
  // that is not to be had, the launch is one-lane with the tiles in global
  // memory.  StaircaseBots (PM 2) also pair where the one-lane rule fills
  // whole waves, when the batch shares the device with another launch and the
  // device's games come to at most four 32-game waves per SIMD (C5's 131,072
  // games as two stream shards: 177-179 us per 128-tick step paired against
  // 183-192 one-lane, profiles/r05_v1/c5_forms.jsonl).
  const bool bank_ok = !grid || (!(p.pm == 2 && sepd) && p.pm <= 3 && p.lds_n && fits(p.lds_n));
  const bool pm2_full = p.pm == 2 && p.lanes == 64u && q.concurrency >= 2 &&
                        (uint64_t)B * q.concurrency <= 4ull * 32ull * (uint64_t)dev.simds &&
                        !env.rollout_lanes;
  const bool paired = nc != kDense && bank_ok && p.pm >= 1 && cfg->width <= 256 &&
                      cfg->height <= 256 && (p.lanes <= 32u || pm2_full) && env.rollout_paired;
  const int x = env.rollout_threads;
  if (paired) {
    p.form = Form::kPaired;
    p.lanes = paired_lanes(B, q.concurrency, env, dev);
    p.nt = p.lanes * 4u >= 128u;  // a wave's row segment is a whole line
    // 512 threads for a bank whose tiles leave room for one workgroup per CU
    // (more than half the LDS): the CU's one copy then serves two waves per SIMD
    p.threads = (x && (x != 512 || grid)) ? (uint32_t)x
                : (grid && 2ull * p.lds_n > dev.lds_per_block) ? 512u
                : (uint32_t)ORX_ROLLOUT_BLOCK;
    p.lds_bytes = p.lds_n;
  } else {
    p.form = Form::kOneLane;
    if (p.pm >= 4) p.pm = 0;  // (the mixed-bot forms are paired only)
    p.nt = p.pm == 0 || p.lanes * 4u >= 128u;
    p.threads = (x && x != 512) ? (uint32_t)x : (uint32_t)ORX_ROLLOUT_BLOCK;
    p.lds_bytes = (p.lds_n + 15u) & ~15u;
    // dense NPCs: one occupancy bitmap per game of the block after the tiles,
    // when they fit; an optimization -- without them the kernel reads the
    // occupancy grid from HBM -- so a launch that may not have the LDS goes
    // first without the bitmaps, then without the tiles, instead of failing
    if (nc == kDense && !env.no_lds_bits) {
      const uint32_t bb = (uint32_t)((cfg->width * cfg->height + 31) / 32) * 4u;
      const uint64_t all = p.lds_bytes + (uint64_t)(p.threads / 64u * p.lanes) * bb;
      if (all <= dev.lds_per_block && fits((uint32_t)all)) {
        p.lds_bits = bb;
        p.lds_bytes = (uint32_t)all;
      }
    }
    if (!fits(p.lds_bytes)) p.lds_bytes = p.lds_n = 0u;
  }
  p.blocks = blocks_for(B, p.lanes, p.threads);
  return p;
}

// The plan of an orx_step_n launch (rows: 0 none, 1 int32, 2 compact).
// Register NPCs on empty dungeons replay the log under the rollout's tick:
// paired (pair_rollout_kernel PM 6) for rows given under the reference's
// rules, at any batch (C3, 65,536 games x 128 ticks, int32 rows: 103-104 us
// against 114-116 one-lane; as two 32,768-game stream shards at 32 games per
// wave 85-86 us, at 16 -- the plan without the concurrency -- 207,
// profiles/r06_v3 / r06_v4 ab_replay_paired.jsonl), else one lane per game
// at the one-lane rollout's games per wave.
inline Plan plan_step_n(const orx_cfg_t* cfg, uint32_t B, int rows, uint32_t concurrency,
                        const Env& env, const Device& dev, bool given_moves = false) {
  Plan p{};
  p.form = moving_npcs(cfg, given_moves) ? Form::kMoving : Form::kGeneric;
  p.lanes = 64;
  p.nt = true;
  p.threads = kBlock;
  if (p.form == Form::kGeneric && cfg->n_layouts == 0 && ncap_for(cfg->n_npcs) != kDense &&
      rows_fit(B) && !env.step_n_generic) {
    p.threads = ORX_ROLLOUT_BLOCK;
    if (rows != 0 && cfg->flags == 0 && env.rollout_paired && env.replay_paired &&
        cfg->width <= 256 && cfg->height <= 256) {
      p.form = Form::kPaired;
      p.pm = 6;
      p.lanes = paired_lanes(B, concurrency, env, dev);
      p.nt = p.lanes * 4u >= 128u;
    } else {
      p.form = Form::kReplay;
      p.lanes = one_lane_lanes(B, env, dev);
    }
  }
  p.blocks = blocks_for(B, p.lanes, p.threads);
  return p;
}

// The plan of an orx_env_step launch: 64 games per wave (32 measured no
// better); the rows through LDS and 16-byte stores when obs is 16-byte
// aligned (a torch allocation is; a view may not be: then direct stores).
inline Plan plan_env_step(const orx_cfg_t* cfg, uint32_t B, bool obs_aligned, const Env& env,
                          bool given_moves = false) {
  Plan p{};
  p.form = moving_npcs(cfg, given_moves) ? Form::kMoving : Form::kGeneric;
  p.lanes = env.env_lanes;
  p.nt = true;
  p.threads = kBlock;
  p.blocks = blocks_for(B, p.lanes, p.threads);
  p.lds_rows = obs_aligned && !env.env_direct_rows;
  return p;
}

}  // namespace orx_dev
