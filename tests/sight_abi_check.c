/* Plain-C consumer of include/orx_sight.h next to include/orx.h: the header
 * compiles as C99 and orx_sight links and refuses every bad argument the header
 * lists on the host, before any launch.  Built and run by tests/test_sight.py
 * (no GPU calls: every call here must be refused -- each passes a state that is
 * complete but for the one pointer under test). */
#include <stdio.h>
#include <string.h>

#include "orx.h"
#include "orx_sight.h"

static int n_ok = 0, n_all = 0;

static void refused(const char* what, int r) {
  ++n_all;
  if (r == ORX_EINVAL && strlen(orx_last_error()) > 0) ++n_ok;
  else printf("%s: returned %d\n", what, r);
}

static uint32_t rows[32];
static uint8_t cells[32 * 32], health[32 * 32];

static int sight(const orx_cfg_t* c, const orx_state_t* st) {
  return orx_sight(c, st, 0, 5, rows, cells, health, 1, NULL);
}

int main(void) {
  orx_cfg_t c, bank;
  orx_state_t full, st;
  int32_t i32[16];
  int16_t i16[16];
  uint8_t u8[256];
  if (orx_abi_version() != ORX_ABI_VERSION || ORX_ABI_VERSION != 7) { printf("abi\n"); return 1; }
  if (ORX_SIGHT_SEEN != 64 || (ORX_SIGHT_SEEN & (ORX_VIEW_TILE_MASK | ORX_VIEW_PLAYER |
      ORX_VIEW_NPC | ORX_VIEW_ITEM | ORX_VIEW_ITEM_KIND)) != 0 || ORX_VIEW_MAX_RADIUS != 15) {
    printf("constants\n"); return 2;
  }
  if (strlen(orx_sight_build_id()) != 16) {
    printf("sight build id: %s\n", orx_sight_build_id()); return 3;
  }
  memset(&c, 0, sizeof c);
  c.width = 10; c.height = 8; c.despawn = ORX_DESPAWN_UNREACHABLE; c.max_ticks = 30;
  c.start_mode = ORX_START_TOGETHER; c.n_npcs = 4; c.npc_health = 3; c.npc_damage = 1;
  c.player_health = 10; c.player_damage = 2; c.player_armor = 1; c.autoreset = 1;
  bank = c; bank.n_layouts = 1;
  if (orx_validate_cfg(&c) != ORX_OK || orx_validate_cfg(&bank) != ORX_OK) {
    printf("valid cfg rejected: %s\n", orx_last_error()); return 4;
  }
  /* a state with every pointer orx_sight can read (never dereferenced here) */
  memset(&full, 0, sizeof full);
  full.p_x = i32; full.p_y = i32; full.p_layout = i16; full.bank_tiles = u8;

  refused("NULL cfg", sight(NULL, &full));
  refused("player 2", orx_sight(&c, &full, 2, 5, rows, cells, health, 1, NULL));
  refused("player -1", orx_sight(&c, &full, -1, 5, rows, NULL, NULL, 1, NULL));
  refused("radius 0", orx_sight(&c, &full, 0, 0, rows, cells, health, 1, NULL));
  refused("radius 16", orx_sight(&c, &full, 1, 16, NULL, cells, NULL, 1, NULL));
  refused("three NULL outputs", orx_sight(&c, &full, 0, 5, NULL, NULL, NULL, 1, NULL));
  refused("three NULL outputs on a bank", orx_sight(&bank, &full, 1, 15, NULL, NULL, NULL, 1, NULL));
  refused("misaligned rows",
          orx_sight(&c, &full, 0, 5, (uint32_t*)((uint8_t*)rows + 2), NULL, NULL, 1, NULL));
  refused("zero games", orx_sight(&c, &full, 0, 5, rows, cells, health, 0, NULL));
  refused("negative games", orx_sight(&c, &full, 0, 5, NULL, NULL, health, -5, NULL));
  refused("NULL state", sight(&c, NULL));
  refused("NULL state on a bank", sight(&bank, NULL));
#define ONE_NULL(cfg, field) \
  st = full; st.field = NULL; refused(#cfg " without " #field, sight(&cfg, &st))
  ONE_NULL(c, p_x);
  ONE_NULL(c, p_y);
  ONE_NULL(bank, p_layout);
  ONE_NULL(bank, bank_tiles);
#undef ONE_NULL
  c.width = 3;
  refused("bad cfg", sight(&c, &full));
  printf("orx_sight refusals: %d of %d\n", n_ok, n_all);
  return n_ok == n_all ? 0 : 6;
}
