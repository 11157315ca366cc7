/* Plain-C consumer of include/orx_npc_query.h next to include/orx.h: the header
 * compiles as C99 and orx_npc_options / orx_npc_seek link and refuse every bad
 * argument the header lists on the host, before any launch.  Built and run by
 * tests/test_npc_query.py (no GPU calls: every call here must be refused --
 * each passes a state that is complete but for the one pointer under test). */
#include <stdio.h>
#include <string.h>

#include "orx.h"
#include "orx_npc_query.h"

static int n_ok = 0, n_all = 0;

static void refused(const char* what, int r) {
  ++n_all;
  if (r == ORX_EINVAL && strlen(orx_last_error()) > 0) ++n_ok;
  else printf("%s: returned %d\n", what, r);
}

/* 16-byte aligned output rows of four lanes */
typedef union { uint8_t b[64]; int16_t h[32]; int32_t w[16]; int8_t c[64]; double align[8]; } row_t;
static row_t kind_buf, target_buf, amount_buf, dist_buf, move_buf;
static uint8_t where_buf[4];

static int options(const orx_cfg_t* c, const orx_state_t* st) {
  return orx_npc_options(c, st, kind_buf.b, target_buf.h, amount_buf.h, where_buf, 1, NULL);
}
static int seek(const orx_cfg_t* c, const orx_state_t* st, const uint16_t* pairs) {
  return orx_npc_seek(c, st, pairs, dist_buf.w, move_buf.c, target_buf.h, 1, NULL);
}

int main(void) {
  orx_cfg_t c, bank, dense, none, rpg;
  orx_state_t full, st;
  int32_t i32[16];
  uint16_t u16[16];
  int16_t i16[16];
  uint32_t u32[16];
  int8_t i8[16];
  uint8_t u8[256];
  uint8_t* kind = kind_buf.b;
  int16_t *target = target_buf.h, *amount = amount_buf.h;
  int32_t* dist = dist_buf.w;
  int8_t* move = move_buf.c;
  if (orx_abi_version() != ORX_ABI_VERSION || ORX_ABI_VERSION != 7) { printf("abi\n"); return 1; }
  if (ORX_NPC_DEPTH_GONE != 0 || ORX_NPC_DEPTH_WATCHED != 1 || ORX_NPC_DEPTH_UNWATCHED != 2 ||
      ORX_NPC_OUT_NONE != ORX_OUT_NONE || ORX_NPC_OUT_REST != ORX_OUT_REST ||
      ORX_NPC_OUT_BLOCKED != ORX_OUT_BLOCKED || ORX_NPC_OUT_STEP != ORX_OUT_STEP ||
      ORX_NPC_OUT_STAIRS != 4 || ORX_NPC_OUT_ATTACK_NPC != ORX_OUT_ATTACK_NPC ||
      ORX_NPC_OUT_ATTACK_PLAYER != ORX_OUT_ATTACK_PLAYER || ORX_NPC_OUT_FROZEN != 7 ||
      ORX_NPC_OUT_LETHAL != ORX_OUT_LETHAL || ORX_NPC_SEEK_P1 != 0 || ORX_NPC_SEEK_P2 != 1 ||
      ORX_NPC_SEEK_NEAREST != 2 || ORX_SEEK_COLS != 4 || ORX_MOVES_COLS != 8) {
    printf("constants\n"); return 2;
  }
  if (strlen(orx_npc_query_build_id()) != 16) {
    printf("npc query build id: %s\n", orx_npc_query_build_id()); return 3;
  }
  memset(&c, 0, sizeof c);
  c.width = 10; c.height = 8; c.despawn = ORX_DESPAWN_UNREACHABLE; c.max_ticks = 30;
  c.start_mode = ORX_START_TOGETHER; c.n_npcs = 4; c.npc_health = 3; c.npc_damage = 1;
  c.player_health = 10; c.player_damage = 2; c.player_armor = 1; c.autoreset = 1;
  bank = c; bank.n_layouts = 1;
  dense = c; dense.width = 16; dense.height = 16; dense.n_npcs = 40;
  none = c; none.n_npcs = 0;
  /* the flags are not restricted (a question, not a tick): the other refusals still hold */
  rpg = c; rpg.flags = ORX_EXT_CHARACTER; rpg.mana_max = 9;
  rpg.mana_regen = 1; rpg.mana_per_point = 1; rpg.xp_per_kill = 1; rpg.xp_per_level = 3;
  rpg.item_drop_pct = 50; rpg.item_bonus = 1; rpg.item_slots = 3; rpg.combat_cooldown = 3;
  if (orx_validate_cfg(&c) != ORX_OK || orx_validate_cfg(&bank) != ORX_OK ||
      orx_validate_cfg(&dense) != ORX_OK || orx_validate_cfg(&none) != ORX_OK ||
      orx_validate_cfg(&rpg) != ORX_OK) {
    printf("valid cfg rejected: %s\n", orx_last_error()); return 4;
  }
  /* a state with every pointer the queries can read (never dereferenced here) */
  memset(&full, 0, sizeof full);
  full.p_x = i32; full.p_y = i32; full.p_depth = i32; full.p_health = i32;
  full.st_x = i32; full.st_y = i32;
  full.npc_pos = u16; full.npc_health = i8; full.npc_alive = u32; full.npc_grid = u8;
  full.p_layout = i16; full.bank_tiles = u8;

  refused("options: NULL cfg", options(NULL, &full));
  refused("options: n_npcs == 0", options(&none, &full));
  refused("options: NULL kind",
          orx_npc_options(&c, &full, NULL, target, amount, where_buf, 1, NULL));
  refused("options: misaligned kind",
          orx_npc_options(&c, &full, kind + 4, NULL, NULL, NULL, 1, NULL));
  refused("options: misaligned target",
          orx_npc_options(&c, &full, kind, target + 4, NULL, NULL, 1, NULL));
  refused("options: misaligned amount",
          orx_npc_options(&c, &full, kind, NULL, amount + 1, NULL, 1, NULL));
  refused("options: zero games",
          orx_npc_options(&c, &full, kind, target, amount, where_buf, 0, NULL));
  refused("options: negative games", orx_npc_options(&c, &full, kind, NULL, NULL, NULL, -5, NULL));
  refused("options: NULL state", options(&c, NULL));
  refused("options: a character cfg, but a NULL kind",
          orx_npc_options(&rpg, &full, NULL, NULL, NULL, NULL, 1, NULL));
#define ONE_NULL(cfg, field) \
  st = full; st.field = NULL; refused("options: " #cfg " without " #field, options(&cfg, &st))
  ONE_NULL(c, p_x);
  ONE_NULL(c, p_y);
  ONE_NULL(c, p_depth);
  ONE_NULL(c, p_health);
  ONE_NULL(c, st_x);
  ONE_NULL(c, st_y);
  ONE_NULL(bank, p_layout);
  ONE_NULL(bank, bank_tiles);
  ONE_NULL(c, npc_pos);
  ONE_NULL(c, npc_health);
  ONE_NULL(c, npc_alive);
  ONE_NULL(dense, npc_grid);
#undef ONE_NULL

  refused("seek: NULL cfg", seek(NULL, &full, NULL));
  refused("seek: n_npcs == 0", seek(&none, &full, NULL));
  refused("seek: three NULL outputs", orx_npc_seek(&c, &full, NULL, NULL, NULL, NULL, 1, NULL));
  refused("seek: misaligned dist", orx_npc_seek(&c, &full, NULL, dist + 1, NULL, NULL, 1, NULL));
  refused("seek: misaligned move", orx_npc_seek(&c, &full, NULL, NULL, move + 2, NULL, 1, NULL));
  refused("seek: misaligned target",
          orx_npc_seek(&c, &full, NULL, NULL, NULL, target + 2, 1, NULL));
  refused("seek: zero games", orx_npc_seek(&c, &full, NULL, dist, move, target, 0, NULL));
  refused("seek: NULL state", seek(&c, NULL, NULL));
  refused("seek: a bank without pairs", seek(&bank, &full, NULL));
#define ONE_NULL(cfg, field) \
  st = full; st.field = NULL; refused("seek: " #cfg " without " #field, seek(&cfg, &st, u16))
  ONE_NULL(c, p_x);
  ONE_NULL(c, p_y);
  ONE_NULL(c, p_depth);
  ONE_NULL(c, st_x);
  ONE_NULL(c, st_y);
  ONE_NULL(bank, p_layout);
  ONE_NULL(bank, bank_tiles);
  ONE_NULL(c, npc_pos);
  ONE_NULL(c, npc_alive);
#undef ONE_NULL
  c.width = 3;
  refused("options: bad cfg", options(&c, &full));
  refused("seek: bad cfg", seek(&c, &full, NULL));
  printf("orx_npc_query refusals: %d of %d\n", n_ok, n_all);
  return n_ok == n_all ? 0 : 6;
}
