/* Plain-C consumer of include/orx_moves.h next to include/orx.h: the header
 * compiles as C99 and orx_moves links and refuses every bad argument its
 * header lists on the host, before any launch.  Built and run by
 * tests/test_moves.py (no GPU calls: every call here must be refused -- each
 * passes a state that is complete but for the one pointer under test). */
#include <stdio.h>
#include <string.h>

#include "orx.h"
#include "orx_moves.h"

static int n_ok = 0, n_all = 0;

static void refused(const char* what, int r) {
  ++n_all;
  if (r == ORX_EINVAL && strlen(orx_last_error()) > 0) ++n_ok;
  else printf("%s: returned %d\n", what, r);
}

/* 16-byte aligned output rows of one game */
static union { uint8_t b[16]; int16_t h[8]; double align[2]; } kind_buf, target_buf, amount_buf;

static int call(const orx_cfg_t* c, const orx_state_t* st) {
  return orx_moves(c, st, 0, kind_buf.b, target_buf.h, amount_buf.h, 1, NULL);
}

int main(void) {
  orx_cfg_t c, bank, dense, rpg;
  orx_state_t full, st;
  int32_t i32[16];
  uint16_t u16[16];
  int16_t i16[16];
  uint32_t u32[16];
  int8_t i8[16];
  uint8_t u8[256];
  uint8_t* kind = kind_buf.b;
  int16_t *target = target_buf.h, *amount = amount_buf.h;
  if (orx_abi_version() != ORX_ABI_VERSION) { printf("abi mismatch\n"); return 1; }
  if (ORX_MOVES_COLS != 8 || ORX_OUT_MASK != 7 || ORX_OUT_NONE != 0 || ORX_OUT_REST != 1 ||
      ORX_OUT_BLOCKED != 2 || ORX_OUT_STEP != 3 || ORX_OUT_DESCEND != 4 || ORX_OUT_ATTACK_NPC != 5 ||
      ORX_OUT_ATTACK_PLAYER != 6 || ORX_OUT_HEAL != 7 ||
      (ORX_OUT_MASK | ORX_OUT_LETHAL | ORX_OUT_ITEM | ORX_OUT_COOLDOWN) != 63) {
    printf("constants\n"); return 2;
  }
  if (strlen(orx_moves_build_id()) != 16) { printf("moves build id: %s\n", orx_moves_build_id()); return 3; }
  memset(&c, 0, sizeof c);
  c.width = 10; c.height = 8; c.despawn = ORX_DESPAWN_UNREACHABLE; c.max_ticks = 30;
  c.start_mode = ORX_START_TOGETHER; c.n_npcs = 4; c.npc_health = 3; c.npc_damage = 1;
  c.player_health = 10; c.player_damage = 2; c.player_armor = 1; c.autoreset = 1;
  bank = c; bank.n_layouts = 1;
  dense = c; dense.width = 16; dense.height = 16; dense.n_npcs = 40;
  rpg = c; rpg.flags = ORX_EXT_CHARACTER; rpg.mana_max = 9; rpg.mana_regen = 1;
  rpg.mana_per_point = 1; rpg.xp_per_kill = 1; rpg.xp_per_level = 3; rpg.item_drop_pct = 50;
  rpg.item_bonus = 1; rpg.item_slots = 3; rpg.combat_cooldown = 3;
  if (orx_validate_cfg(&c) != ORX_OK || orx_validate_cfg(&bank) != ORX_OK ||
      orx_validate_cfg(&dense) != ORX_OK || orx_validate_cfg(&rpg) != ORX_OK) {
    printf("valid cfg rejected: %s\n", orx_last_error()); return 4;
  }
  /* a state with every pointer orx_moves can read (never dereferenced here) */
  memset(&full, 0, sizeof full);
  full.p_x = i32; full.p_y = i32; full.p_depth = i32; full.p_health = i32;
  full.st_x = i32; full.st_y = i32;
  full.npc_pos = u16; full.npc_health = i8; full.npc_alive = u32; full.npc_grid = u8;
  full.p_layout = i16; full.bank_tiles = u8; full.p_rpg = i32;
  full.item_pos = u16; full.item_mask = u32;

  refused("NULL cfg", call(NULL, &full));
  refused("player 2", orx_moves(&c, &full, 2, kind, target, amount, 1, NULL));
  refused("player -1", orx_moves(&c, &full, -1, kind, target, amount, 1, NULL));
  refused("NULL kind", orx_moves(&c, &full, 0, NULL, target, amount, 1, NULL));
  refused("misaligned kind", orx_moves(&c, &full, 0, kind + 4, NULL, NULL, 1, NULL));
  refused("misaligned target", orx_moves(&c, &full, 0, kind, target + 4, NULL, 1, NULL));
  refused("misaligned amount", orx_moves(&c, &full, 0, kind, NULL, amount + 1, 1, NULL));
  refused("zero games", orx_moves(&c, &full, 0, kind, target, amount, 0, NULL));
  refused("negative games", orx_moves(&c, &full, 0, kind, NULL, NULL, -5, NULL));
  refused("NULL state", call(&c, NULL));
#define ONE_NULL(cfg, field) \
  st = full; st.field = NULL; refused(#cfg " without " #field, call(&cfg, &st))
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
  ONE_NULL(rpg, p_rpg);
  ONE_NULL(rpg, item_pos);
  ONE_NULL(rpg, item_mask);
  c.width = 3;
  refused("bad cfg", call(&c, &full));
  printf("orx_moves refusals: %d of %d\n", n_ok, n_all);
  return n_ok == n_all ? 0 : 6;
}
