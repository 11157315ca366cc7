/* Plain-C consumer of include/orx_path.h's orx_path_ticks: the header compiles
 * as C99 and the entry point links and refuses bad arguments on the host,
 * before any launch.  Built and run by tests/test_ticks.py (no GPU calls:
 * every call here must be refused). */
#include <stdio.h>
#include <string.h>

#include "orx.h"
#include "orx_path.h"

static int n_ok = 0, n_all = 0;

static void refused(const char* what, int r) {
  ++n_all;
  if (r == ORX_EINVAL && strlen(orx_last_error()) > 0) ++n_ok;
  else printf("%s: returned %d\n", what, r);
}

int main(void) {
  orx_cfg_t c, bank, npcs, wide, tall, rpg;
  orx_state_t st, full, fb, fn;
  uint8_t tiles[16];
  uint32_t planes[8];
  unsigned char raw[2][64];
  int32_t* ticks = (int32_t*)(((uintptr_t)raw[0] + 15) & ~(uintptr_t)15);
  uint16_t* window = (uint16_t*)(((uintptr_t)raw[1] + 15) & ~(uintptr_t)15);
  int8_t move[4];
  int32_t xs[2] = {1, 1};
  int16_t lay[2] = {0, 0};
  uint16_t pos[4] = {0, 0, 0, 0};
  int8_t hp[4] = {1, 1, 1, 1};
  uint32_t alive[1] = {3};
  if (orx_abi_version() != ORX_ABI_VERSION) { printf("abi mismatch\n"); return 1; }
  memset(&c, 0, sizeof c);
  memset(&st, 0, sizeof st);
  c.width = 10; c.height = 8; c.despawn = ORX_DESPAWN_UNREACHABLE; c.max_ticks = 30;
  c.start_mode = ORX_START_TOGETHER; c.n_npcs = 0; c.npc_health = 3; c.npc_damage = 1;
  c.player_health = 10; c.player_damage = 2; c.player_armor = 1; c.autoreset = 1;
  if (orx_validate_cfg(&c) != ORX_OK) { printf("valid cfg rejected: %s\n", orx_last_error()); return 4; }
  full = st;
  full.p_x = xs; full.p_y = xs; full.p_depth = xs; full.st_x = xs; full.st_y = xs;
  bank = c;
  bank.width = 4; bank.height = 4; bank.n_layouts = 1;
  if (orx_validate_cfg(&bank) != ORX_OK) { printf("valid bank cfg rejected: %s\n", orx_last_error()); return 5; }
  fb = full;
  fb.p_layout = lay; fb.bank_tiles = tiles;
  npcs = c;
  npcs.n_npcs = 2;
  if (orx_validate_cfg(&npcs) != ORX_OK) { printf("valid npc cfg rejected: %s\n", orx_last_error()); return 6; }
  fn = full;
  fn.npc_pos = pos; fn.npc_health = hp; fn.npc_alive = alive;
  wide = c;
  wide.width = 300; wide.height = 300;       /* W * H > 65536 */
  if (orx_validate_cfg(&wide) != ORX_OK) { printf("valid wide cfg rejected: %s\n", orx_last_error()); return 7; }
  tall = npcs;
  tall.width = 256; tall.height = 255; tall.n_npcs = 3;   /* W * H + 127 K reaches the sentinels */
  if (orx_validate_cfg(&tall) != ORX_OK) { printf("valid tall cfg rejected: %s\n", orx_last_error()); return 8; }
  rpg = c;
  rpg.flags = ORX_EXT_README_COMBAT;
  if (orx_validate_cfg(&rpg) != ORX_OK) { printf("valid rpg cfg rejected: %s\n", orx_last_error()); return 9; }

#define TICKS(cfg, s, p, pl, r, t, m, w, n) orx_path_ticks(cfg, s, p, pl, r, t, m, w, n, NULL)
  refused("player 2", TICKS(&c, &full, NULL, 2, 1, ticks, move, window, 1));
  refused("player -1", TICKS(&c, &full, NULL, -1, 1, ticks, move, window, 1));
  refused("no outputs", TICKS(&c, &full, NULL, 0, 1, NULL, NULL, NULL, 1));
  refused("radius 0 with a window", TICKS(&c, &full, NULL, 0, 0, ticks, move, window, 1));
  refused("radius 16 with a window",
          TICKS(&c, &full, NULL, 0, ORX_VIEW_MAX_RADIUS + 1, NULL, NULL, window, 1));
  refused("misaligned ticks",
          TICKS(&c, &full, NULL, 0, 1, (int32_t*)((unsigned char*)ticks + 2), move, window, 1));
  refused("misaligned window",
          TICKS(&c, &full, NULL, 0, 1, ticks, move, (uint16_t*)((unsigned char*)window + 1), 1));
  refused("misaligned planes",
          TICKS(&bank, &fb, (uint32_t*)((unsigned char*)planes + 2), 0, 1, ticks, move, window, 1));
  refused("zero games", TICKS(&c, &full, NULL, 0, 1, ticks, move, window, 0));
  refused("negative games", TICKS(&c, &full, NULL, 0, 1, ticks, move, window, -3));
  refused("NULL cfg", TICKS(NULL, &full, NULL, 0, 1, ticks, move, window, 1));
  c.width = 3;
  refused("bad cfg", TICKS(&c, &full, NULL, 0, 1, ticks, move, window, 1));
  c.width = 10;
  refused("W * H > 65536", TICKS(&wide, &full, NULL, 0, 1, ticks, move, NULL, 1));
  refused("bank without planes", TICKS(&bank, &fb, NULL, 0, 1, ticks, move, window, 1));
  fb.p_layout = NULL;
  refused("bank without p_layout", TICKS(&bank, &fb, planes, 0, 1, ticks, move, window, 1));
  fb.p_layout = lay;
  fb.bank_tiles = NULL;
  refused("bank without bank_tiles", TICKS(&bank, &fb, planes, 0, 1, ticks, move, window, 1));
  fb.bank_tiles = tiles;
  refused("a window whose values could reach the sentinels",
          TICKS(&tall, &fn, NULL, 0, 1, NULL, NULL, window, 1));
  refused("NULL state", TICKS(&c, NULL, NULL, 0, 1, ticks, move, window, 1));
  refused("NULL p_x", TICKS(&c, &st, NULL, 0, 1, ticks, move, window, 1));
  full.p_y = NULL;
  refused("NULL p_y", TICKS(&c, &full, NULL, 0, 1, ticks, move, window, 1));
  full.p_y = xs;
  full.p_depth = NULL;
  refused("NULL p_depth", TICKS(&c, &full, NULL, 0, 1, ticks, move, window, 1));
  full.p_depth = xs;
  full.st_x = NULL;
  refused("NULL st_x", TICKS(&c, &full, NULL, 0, 1, ticks, move, window, 1));
  full.st_x = xs;
  full.st_y = NULL;
  refused("NULL st_y", TICKS(&c, &full, NULL, 0, 1, ticks, move, window, 1));
  full.st_y = xs;
  refused("NPCs without npc_pos", TICKS(&npcs, &full, NULL, 0, 1, ticks, move, window, 1));
  fn.npc_alive = NULL;
  refused("NPCs without npc_alive", TICKS(&npcs, &fn, NULL, 0, 1, ticks, move, window, 1));
  fn.npc_alive = alive;
  fn.npc_health = NULL;
  refused("NPCs without npc_health", TICKS(&npcs, &fn, NULL, 0, 1, ticks, move, window, 1));
  fn.npc_health = hp;
  refused("a character flag without p_rpg", TICKS(&rpg, &full, NULL, 0, 1, ticks, move, window, 1));
  refused("move alone, no games", TICKS(&c, &full, NULL, 0, 99, NULL, move, NULL, 0));
  printf("orx_path_ticks refusals: %d of %d\n", n_ok, n_all);
  return n_ok == n_all ? 0 : 10;
}
