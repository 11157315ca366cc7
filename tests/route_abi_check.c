/* Plain-C consumer of include/orx_route.h next to include/orx.h: the header
 * compiles as C99, and orx_route_planes and orx_route link and refuse every bad
 * argument the header lists on the host, before any launch.  Built and run by
 * tests/test_route.py (no GPU calls: every call here must be refused -- each
 * passes arguments that are complete but for the one under test). */
#include <stdio.h>
#include <string.h>

#include "orx.h"
#include "orx_route.h"

static int n_ok = 0, n_all = 0;

static void refused(const char* what, int r) {
  ++n_all;
  if (r == ORX_EINVAL && strlen(orx_last_error()) > 0) ++n_ok;
  else printf("%s: returned %d\n", what, r);
}

static union { uint32_t u32[256]; int32_t i32[256]; uint8_t u8[1024]; }
    buf_memory, buf_key, buf_goal, buf_dist, buf_move, buf_target, buf_planes;

static void* aligned16(void* p) { return (void*)(((uintptr_t)p + 15) & ~(uintptr_t)15); }
static void* off(void* p, int bytes) { return (void*)((uint8_t*)aligned16(p) + bytes); }

#define MEMORY ((uint32_t*)aligned16(&buf_memory))
#define KEY ((int32_t*)aligned16(&buf_key))
#define GOAL ((int32_t*)aligned16(&buf_goal))
#define DIST ((int32_t*)aligned16(&buf_dist))
#define MOVE ((int8_t*)aligned16(&buf_move))
#define TARGET ((int32_t*)aligned16(&buf_target))
#define PLANES ((uint32_t*)aligned16(&buf_planes))

static int route(const orx_cfg_t* c, const orx_state_t* st) {
  return orx_route(c, st, PLANES, 0, MEMORY, KEY, GOAL, DIST, MOVE, TARGET, 1, NULL);
}

int main(void) {
  orx_cfg_t c, bank, big;
  orx_state_t full, st;
  int32_t i32[16];
  int16_t i16[16];
  uint8_t u8[256];
  if (orx_abi_version() != ORX_ABI_VERSION || ORX_ABI_VERSION != 7) { printf("abi\n"); return 1; }
  if (ORX_ROUTE_FRONTIER != 0 || ORX_ROUTE_STAIRS != 1 || ORX_ROUTE_GOAL != 2 ||
      ORX_ROUTE_FRONTIER != ORX_EXPLORE_FRONTIER || ORX_ROUTE_STAIRS != ORX_EXPLORE_STAIRS ||
      ORX_SEEK_COLS != 4 || ORX_SEEK_ABSENT != -2 || ORX_SEEK_UNREACHABLE != -1) {
    printf("constants\n"); return 2;
  }
  if (strlen(orx_route_build_id()) != 16) {
    printf("route build id: %s\n", orx_route_build_id()); return 3;
  }
  memset(&c, 0, sizeof c);
  c.width = 10; c.height = 8; c.despawn = ORX_DESPAWN_UNREACHABLE; c.max_ticks = 30;
  c.start_mode = ORX_START_TOGETHER; c.n_npcs = 0; c.npc_health = 3; c.npc_damage = 1;
  c.player_health = 10; c.player_damage = 2; c.player_armor = 1; c.autoreset = 1;
  bank = c; bank.n_layouts = 1;
  big = c; big.width = 300; big.height = 300;
  if (orx_validate_cfg(&c) != ORX_OK || orx_validate_cfg(&bank) != ORX_OK ||
      orx_validate_cfg(&big) != ORX_OK) {
    printf("valid cfg rejected: %s\n", orx_last_error()); return 4;
  }
  /* a state with every pointer orx_route can read (never dereferenced here) */
  memset(&full, 0, sizeof full);
  full.p_x = i32; full.p_y = i32; full.p_depth = i32; full.tick = i32; full.episode = i32;
  full.st_x = i32; full.st_y = i32; full.p_layout = i16; full.bank_tiles = u8;

  /* ---- orx_route_planes ---- */
  refused("NULL cfg", orx_route_planes(NULL, u8, PLANES, NULL));
  refused("no bank", orx_route_planes(&c, u8, PLANES, NULL));
  refused("NULL bank_tiles", orx_route_planes(&bank, NULL, PLANES, NULL));
  refused("NULL planes", orx_route_planes(&bank, u8, NULL, NULL));
  refused("misaligned planes", orx_route_planes(&bank, u8, (uint32_t*)off(&buf_planes, 2), NULL));
  bank.width = 3;
  refused("bad cfg", orx_route_planes(&bank, u8, PLANES, NULL));
  bank.width = 10;
  printf("orx_route_planes refusals: %d of %d\n", n_ok, n_all);
  if (n_ok != n_all) return 5;

  /* ---- orx_route ---- */
  n_ok = n_all = 0;
  refused("NULL cfg", route(NULL, &full));
  refused("player 2", orx_route(&c, &full, NULL, 2, MEMORY, KEY, GOAL, DIST, MOVE, TARGET, 1, NULL));
  refused("player -1", orx_route(&bank, &full, PLANES, -1, MEMORY, KEY, NULL, DIST, NULL, NULL, 1, NULL));
  refused("NULL memory", orx_route(&c, &full, NULL, 0, NULL, KEY, GOAL, DIST, MOVE, TARGET, 1, NULL));
  refused("NULL key", orx_route(&c, &full, NULL, 0, MEMORY, NULL, GOAL, DIST, MOVE, TARGET, 1, NULL));
  refused("misaligned memory", orx_route(&c, &full, NULL, 0, (uint32_t*)off(&buf_memory, 2), KEY, GOAL, DIST,
                                         MOVE, TARGET, 1, NULL));
  refused("misaligned key", orx_route(&c, &full, NULL, 0, MEMORY, (int32_t*)off(&buf_key, 4), GOAL, DIST, MOVE,
                                      TARGET, 1, NULL));
  refused("three NULL outputs", orx_route(&c, &full, NULL, 0, MEMORY, KEY, GOAL, NULL, NULL, NULL, 1, NULL));
  refused("three NULL outputs on a bank",
          orx_route(&bank, &full, PLANES, 1, MEMORY, KEY, NULL, NULL, NULL, NULL, 1, NULL));
  refused("misaligned dist", orx_route(&c, &full, NULL, 0, MEMORY, KEY, GOAL, (int32_t*)off(&buf_dist, 8), MOVE,
                                       TARGET, 1, NULL));
  refused("misaligned move", orx_route(&c, &full, NULL, 0, MEMORY, KEY, GOAL, DIST, (int8_t*)off(&buf_move, 2),
                                       TARGET, 1, NULL));
  refused("misaligned target", orx_route(&c, &full, NULL, 0, MEMORY, KEY, GOAL, DIST, MOVE,
                                         (int32_t*)off(&buf_target, 4), 1, NULL));
  refused("misaligned target alone", orx_route(&c, &full, NULL, 0, MEMORY, KEY, NULL, NULL, NULL,
                                               (int32_t*)off(&buf_target, 8), 1, NULL));
  refused("misaligned goal", orx_route(&c, &full, NULL, 0, MEMORY, KEY, (int32_t*)off(&buf_goal, 2), DIST, MOVE,
                                       TARGET, 1, NULL));
  refused("misaligned planes", orx_route(&bank, &full, (uint32_t*)off(&buf_planes, 1), 0, MEMORY, KEY, GOAL,
                                         DIST, MOVE, TARGET, 1, NULL));
  refused("zero games", orx_route(&c, &full, NULL, 0, MEMORY, KEY, GOAL, DIST, MOVE, TARGET, 0, NULL));
  refused("negative games", orx_route(&c, &full, NULL, 0, MEMORY, KEY, GOAL, DIST, MOVE, TARGET, -1, NULL));
  refused("a grid of more than 65536 cells", route(&big, &full));
  refused("NULL state", route(&c, NULL));
  refused("NULL state on a bank", route(&bank, NULL));
#define ONE_NULL(fn, cfg, field) \
  st = full; st.field = NULL; refused(#fn " " #cfg " without " #field, fn(&cfg, &st))
  ONE_NULL(route, c, p_x);
  ONE_NULL(route, c, p_y);
  ONE_NULL(route, c, p_depth);
  ONE_NULL(route, c, tick);
  ONE_NULL(route, c, episode);
  ONE_NULL(route, c, st_x);
  ONE_NULL(route, c, st_y);
  ONE_NULL(route, bank, p_layout);
  ONE_NULL(route, bank, bank_tiles);
#undef ONE_NULL
  refused("a bank without planes",
          orx_route(&bank, &full, NULL, 0, MEMORY, KEY, GOAL, DIST, MOVE, TARGET, 1, NULL));
  c.height = 3;
  refused("bad cfg", route(&c, &full));
  printf("orx_route refusals: %d of %d\n", n_ok, n_all);
  return n_ok == n_all ? 0 : 6;
}
