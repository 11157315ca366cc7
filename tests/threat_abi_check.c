/* Plain-C consumer of include/orx_path.h's danger-field entry point: the header
 * compiles as C99 and orx_path_threat links and refuses bad arguments on the
 * host, before any launch.  Built and run by tests/test_threat.py (no GPU
 * calls: every call here must be refused). */
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
  orx_cfg_t c, bank, npcs, wide;
  orx_state_t st, full, fb, fn;
  uint8_t tiles[16];
  uint16_t pairs[256];
  /* one row of each output, aligned for its vector store */
  unsigned char raw[5][64];
  int32_t* dist = (int32_t*)(((uintptr_t)raw[0] + 15) & ~(uintptr_t)15);
  int16_t* target = (int16_t*)(((uintptr_t)raw[1] + 15) & ~(uintptr_t)15);
  int8_t* move = (int8_t*)(((uintptr_t)raw[2] + 15) & ~(uintptr_t)15);
  int32_t* after = (int32_t*)(((uintptr_t)raw[3] + 15) & ~(uintptr_t)15);
  uint16_t* window = (uint16_t*)(((uintptr_t)raw[4] + 15) & ~(uintptr_t)15);
  int32_t xs[2] = {1, 1};
  int16_t lay[2] = {0, 0};
  uint16_t pos[2] = {0, 0};
  int8_t hp[2] = {1, 1};
  uint32_t alive[1] = {3};
  if (orx_abi_version() != ORX_ABI_VERSION) { printf("abi mismatch\n"); return 1; }
  if (ORX_THREAT_PLAYER != 0 || ORX_THREAT_NPC != 1 || ORX_THREAT_ANY != 2 ||
      ORX_THREAT_AFTER_COLS != 8 || ORX_SEEK_COLS != 4) { printf("constants\n"); return 2; }
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
  wide.width = 40000; wide.height = 26000;   /* W + H - 4 reaches the sentinels */
  if (orx_validate_cfg(&wide) != ORX_OK) { printf("valid wide cfg rejected: %s\n", orx_last_error()); return 7; }

#define THREAT(cfg, s, p, pl, r, d, m, t, a, w, n) \
  orx_path_threat(cfg, s, p, pl, r, d, m, t, a, w, n, NULL)
  refused("player 2", THREAT(&c, &full, NULL, 2, 1, dist, move, target, after, window, 1));
  refused("player -1", THREAT(&c, &full, NULL, -1, 1, dist, move, target, after, window, 1));
  refused("no outputs", THREAT(&c, &full, NULL, 0, 1, NULL, NULL, NULL, NULL, NULL, 1));
  refused("radius 0 with a window",
          THREAT(&c, &full, NULL, 0, 0, dist, move, target, after, window, 1));
  refused("radius 16 with a window",
          THREAT(&c, &full, NULL, 0, ORX_VIEW_MAX_RADIUS + 1, NULL, NULL, NULL, NULL, window, 1));
  refused("misaligned dist",
          THREAT(&c, &full, NULL, 0, 1, dist + 1, move, target, after, window, 1));
  refused("misaligned move",
          THREAT(&c, &full, NULL, 0, 1, dist, move + 1, target, after, window, 1));
  refused("misaligned target",
          THREAT(&c, &full, NULL, 0, 1, dist, move, target + 1, after, window, 1));
  refused("misaligned after",
          THREAT(&c, &full, NULL, 0, 1, dist, move, target, after + 2, window, 1));
  refused("misaligned window",
          THREAT(&c, &full, NULL, 0, 1, dist, move, target, after,
                 (uint16_t*)((unsigned char*)window + 1), 1));
  refused("zero games", THREAT(&c, &full, NULL, 0, 1, dist, move, target, after, window, 0));
  refused("negative games", THREAT(&c, &full, NULL, 0, 1, dist, move, target, after, window, -3));
  refused("NULL cfg", THREAT(NULL, &full, NULL, 0, 1, dist, move, target, after, window, 1));
  c.width = 3;
  refused("bad cfg", THREAT(&c, &full, NULL, 0, 1, dist, move, target, after, window, 1));
  c.width = 10;
  refused("bank without pairs",
          THREAT(&bank, &fb, NULL, 0, 1, dist, move, target, after, window, 1));
  fb.p_layout = NULL;
  refused("bank without p_layout",
          THREAT(&bank, &fb, pairs, 0, 1, dist, move, target, after, window, 1));
  fb.p_layout = lay;
  fb.bank_tiles = NULL;
  refused("bank without bank_tiles",
          THREAT(&bank, &fb, pairs, 0, 1, dist, move, target, after, window, 1));
  fb.bank_tiles = tiles;
  refused("NULL state", THREAT(&c, NULL, NULL, 0, 1, dist, move, target, after, window, 1));
  refused("NULL p_x", THREAT(&c, &st, NULL, 0, 1, dist, move, target, after, window, 1));
  full.p_y = NULL;
  refused("NULL p_y", THREAT(&c, &full, NULL, 0, 1, dist, move, target, after, window, 1));
  full.p_y = xs;
  full.p_depth = NULL;
  refused("NULL p_depth", THREAT(&c, &full, NULL, 0, 1, dist, move, target, after, window, 1));
  full.p_depth = xs;
  full.st_x = NULL;
  refused("NULL st_x", THREAT(&c, &full, NULL, 0, 1, dist, move, target, after, window, 1));
  full.st_x = xs;
  full.st_y = NULL;
  refused("NULL st_y", THREAT(&c, &full, NULL, 0, 1, dist, move, target, after, window, 1));
  full.st_y = xs;
  refused("NPCs without npc_pos",
          THREAT(&npcs, &full, NULL, 0, 1, dist, move, target, after, window, 1));
  fn.npc_alive = NULL;
  refused("NPCs without npc_alive",
          THREAT(&npcs, &fn, NULL, 0, 1, dist, move, target, after, window, 1));
  fn.npc_alive = alive;
  fn.npc_health = NULL;
  refused("NPCs without npc_health",
          THREAT(&npcs, &fn, NULL, 0, 1, dist, move, target, after, window, 1));
  fn.npc_health = hp;
  refused("a room too wide for a uint16 window",
          THREAT(&wide, &full, NULL, 0, 1, NULL, NULL, NULL, NULL, window, 1));
  printf("orx_path_threat refusals: %d of %d\n", n_ok, n_all);
  return n_ok == n_all ? 0 : 8;
}
