/* Plain-C consumer of include/orx_explore.h next to include/orx.h: the header
 * compiles as C99, and orx_explore_update and orx_explore_seek link and refuse
 * every bad argument the header lists on the host, before any launch.  Built
 * and run by tests/test_explore.py (no GPU calls: every call here must be
 * refused -- each passes arguments that are complete but for the one under
 * test). */
#include <stdio.h>
#include <string.h>

#include "orx.h"
#include "orx_explore.h"

static int n_ok = 0, n_all = 0;

static void refused(const char* what, int r) {
  ++n_all;
  if (r == ORX_EINVAL && strlen(orx_last_error()) > 0) ++n_ok;
  else printf("%s: returned %d\n", what, r);
}

/* (16-byte aligned: a union with a long double would do as well, but the
 * offsets below only need multiples of 16 from one base) */
static union { uint32_t u32[256]; int32_t i32[256]; uint16_t u16[512]; uint8_t u8[1024]; }
    buf_rows, buf_memory, buf_key, buf_gained, buf_dist, buf_move, buf_target, buf_pairs;
static uint8_t cells[32 * 32], health[32 * 32];

static void* aligned16(void* p) { return (void*)(((uintptr_t)p + 15) & ~(uintptr_t)15); }
static void* off(void* p, int bytes) { return (void*)((uint8_t*)aligned16(p) + bytes); }

#define ROWS ((uint32_t*)aligned16(&buf_rows))
#define MEMORY ((uint32_t*)aligned16(&buf_memory))
#define KEY ((int32_t*)aligned16(&buf_key))
#define GAINED ((int32_t*)aligned16(&buf_gained))
#define DIST ((int32_t*)aligned16(&buf_dist))
#define MOVE ((int8_t*)aligned16(&buf_move))
#define TARGET ((int32_t*)aligned16(&buf_target))
#define PAIRS ((uint16_t*)aligned16(&buf_pairs))

static int update(const orx_cfg_t* c, const orx_state_t* st) {
  return orx_explore_update(c, st, 0, 5, ROWS, MEMORY, KEY, GAINED, cells, health, 1, NULL);
}

static int seek(const orx_cfg_t* c, const orx_state_t* st) {
  return orx_explore_seek(c, st, PAIRS, 0, MEMORY, KEY, DIST, MOVE, TARGET, 1, NULL);
}

int main(void) {
  orx_cfg_t c, bank, big;
  orx_state_t full, st;
  int32_t i32[16];
  int16_t i16[16];
  uint8_t u8[256];
  if (orx_abi_version() != ORX_ABI_VERSION || ORX_ABI_VERSION != 7) { printf("abi\n"); return 1; }
  if (ORX_EXPLORE_KNOWN != 128 || (ORX_EXPLORE_KNOWN & (ORX_SIGHT_SEEN | ORX_VIEW_TILE_MASK |
      ORX_VIEW_PLAYER | ORX_VIEW_NPC | ORX_VIEW_ITEM | ORX_VIEW_ITEM_KIND)) != 0 ||
      ORX_EXPLORE_FRONTIER != 0 || ORX_EXPLORE_STAIRS != 1 || ORX_SEEK_COLS != 4) {
    printf("constants\n"); return 2;
  }
  if (strlen(orx_explore_build_id()) != 16) {
    printf("explore build id: %s\n", orx_explore_build_id()); return 3;
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
  /* a state with every pointer the two can read (never dereferenced here) */
  memset(&full, 0, sizeof full);
  full.p_x = i32; full.p_y = i32; full.p_depth = i32; full.tick = i32; full.episode = i32;
  full.st_x = i32; full.st_y = i32; full.p_layout = i16; full.bank_tiles = u8;

  /* ---- orx_explore_update ---- */
  refused("NULL cfg", update(NULL, &full));
  refused("player 2", orx_explore_update(&c, &full, 2, 5, ROWS, MEMORY, KEY, GAINED, cells, health, 1, NULL));
  refused("player -1", orx_explore_update(&c, &full, -1, 5, ROWS, MEMORY, KEY, NULL, NULL, NULL, 1, NULL));
  refused("radius 0", orx_explore_update(&c, &full, 0, 0, ROWS, MEMORY, KEY, GAINED, cells, health, 1, NULL));
  refused("radius 16", orx_explore_update(&c, &full, 1, 16, ROWS, MEMORY, KEY, NULL, cells, NULL, 1, NULL));
  refused("NULL rows", orx_explore_update(&c, &full, 0, 5, NULL, MEMORY, KEY, GAINED, cells, health, 1, NULL));
  refused("NULL memory", orx_explore_update(&c, &full, 0, 5, ROWS, NULL, KEY, GAINED, cells, health, 1, NULL));
  refused("NULL key", orx_explore_update(&bank, &full, 0, 5, ROWS, MEMORY, NULL, GAINED, cells, health, 1, NULL));
  refused("misaligned rows", orx_explore_update(&c, &full, 0, 5, (uint32_t*)off(&buf_rows, 2), MEMORY, KEY,
                                                GAINED, NULL, NULL, 1, NULL));
  refused("misaligned memory", orx_explore_update(&c, &full, 0, 5, ROWS, (uint32_t*)off(&buf_memory, 1), KEY,
                                                  GAINED, NULL, NULL, 1, NULL));
  refused("misaligned gained", orx_explore_update(&c, &full, 0, 5, ROWS, MEMORY, KEY,
                                                  (int32_t*)off(&buf_gained, 2), NULL, NULL, 1, NULL));
  refused("key 4 bytes past a boundary", orx_explore_update(&c, &full, 0, 5, ROWS, MEMORY,
                                                            (int32_t*)off(&buf_key, 4), GAINED, NULL, NULL, 1, NULL));
  refused("key 8 bytes past a boundary", orx_explore_update(&c, &full, 0, 5, ROWS, MEMORY,
                                                            (int32_t*)off(&buf_key, 8), NULL, NULL, NULL, 1, NULL));
  refused("zero games", orx_explore_update(&c, &full, 0, 5, ROWS, MEMORY, KEY, GAINED, cells, health, 0, NULL));
  refused("negative games", orx_explore_update(&c, &full, 0, 5, ROWS, MEMORY, KEY, NULL, NULL, health, -5, NULL));
  refused("NULL state", update(&c, NULL));
  refused("NULL state on a bank", update(&bank, NULL));
#define ONE_NULL(fn, cfg, field) \
  st = full; st.field = NULL; refused(#fn " " #cfg " without " #field, fn(&cfg, &st))
  ONE_NULL(update, c, p_x);
  ONE_NULL(update, c, p_y);
  ONE_NULL(update, c, p_depth);
  ONE_NULL(update, c, tick);
  ONE_NULL(update, c, episode);
  ONE_NULL(update, bank, episode);
  c.width = 3;
  refused("bad cfg", update(&c, &full));
  c.width = 10;
  printf("orx_explore_update refusals: %d of %d\n", n_ok, n_all);
  if (n_ok != n_all) return 5;

  /* ---- orx_explore_seek ---- */
  n_ok = n_all = 0;
  refused("NULL cfg", seek(NULL, &full));
  refused("player 2", orx_explore_seek(&c, &full, NULL, 2, MEMORY, KEY, DIST, MOVE, TARGET, 1, NULL));
  refused("player -1", orx_explore_seek(&bank, &full, PAIRS, -1, MEMORY, KEY, DIST, NULL, NULL, 1, NULL));
  refused("NULL memory", orx_explore_seek(&c, &full, NULL, 0, NULL, KEY, DIST, MOVE, TARGET, 1, NULL));
  refused("NULL key", orx_explore_seek(&c, &full, NULL, 0, MEMORY, NULL, DIST, MOVE, TARGET, 1, NULL));
  refused("misaligned memory", orx_explore_seek(&c, &full, NULL, 0, (uint32_t*)off(&buf_memory, 2), KEY, DIST,
                                                MOVE, TARGET, 1, NULL));
  refused("misaligned key", orx_explore_seek(&c, &full, NULL, 0, MEMORY, (int32_t*)off(&buf_key, 4), DIST, MOVE,
                                             TARGET, 1, NULL));
  refused("three NULL outputs", orx_explore_seek(&c, &full, NULL, 0, MEMORY, KEY, NULL, NULL, NULL, 1, NULL));
  refused("three NULL outputs on a bank",
          orx_explore_seek(&bank, &full, PAIRS, 1, MEMORY, KEY, NULL, NULL, NULL, 1, NULL));
  refused("misaligned dist", orx_explore_seek(&c, &full, NULL, 0, MEMORY, KEY, (int32_t*)off(&buf_dist, 8), MOVE,
                                              TARGET, 1, NULL));
  refused("misaligned move", orx_explore_seek(&c, &full, NULL, 0, MEMORY, KEY, DIST, (int8_t*)off(&buf_move, 2),
                                              TARGET, 1, NULL));
  refused("misaligned target", orx_explore_seek(&c, &full, NULL, 0, MEMORY, KEY, DIST, MOVE,
                                                (int32_t*)off(&buf_target, 4), 1, NULL));
  refused("misaligned target alone", orx_explore_seek(&c, &full, NULL, 0, MEMORY, KEY, NULL, NULL,
                                                      (int32_t*)off(&buf_target, 8), 1, NULL));
  refused("zero games", orx_explore_seek(&c, &full, NULL, 0, MEMORY, KEY, DIST, MOVE, TARGET, 0, NULL));
  refused("negative games", orx_explore_seek(&c, &full, NULL, 0, MEMORY, KEY, DIST, MOVE, TARGET, -1, NULL));
  refused("a grid of more than 65536 cells", seek(&big, &full));
  refused("NULL state", seek(&c, NULL));
  refused("NULL state on a bank", seek(&bank, NULL));
  ONE_NULL(seek, c, p_x);
  ONE_NULL(seek, c, p_y);
  ONE_NULL(seek, c, p_depth);
  ONE_NULL(seek, c, tick);
  ONE_NULL(seek, c, episode);
  ONE_NULL(seek, c, st_x);
  ONE_NULL(seek, c, st_y);
  ONE_NULL(seek, bank, p_layout);
  ONE_NULL(seek, bank, bank_tiles);
#undef ONE_NULL
  refused("a bank without pairs",
          orx_explore_seek(&bank, &full, NULL, 0, MEMORY, KEY, DIST, MOVE, TARGET, 1, NULL));
  c.height = 3;
  refused("bad cfg", seek(&c, &full));
  printf("orx_explore_seek refusals: %d of %d\n", n_ok, n_all);
  return n_ok == n_all ? 0 : 6;
}
