/* Plain-C consumer of include/orx_path.h's walking-distance entry points: the
 * header compiles as C99 and orx_path_rows / orx_path_seek link and refuse bad
 * arguments on the host, before any launch.  Built and run by
 * tests/test_seek.py (no GPU calls: every call here must be refused). */
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
  orx_cfg_t c, bank, npcs;
  orx_state_t st, full, fb;
  uint8_t tiles[16];
  int32_t lay32[1] = {0}, cell[1] = {5};
  uint16_t rows[16], pairs[256];
  /* one row of each output, aligned for its vector store */
  unsigned char raw[3][48];
  int32_t* dist = (int32_t*)(((uintptr_t)raw[0] + 15) & ~(uintptr_t)15);
  int16_t* target = (int16_t*)(((uintptr_t)raw[1] + 15) & ~(uintptr_t)15);
  int8_t* move = (int8_t*)(((uintptr_t)raw[2] + 15) & ~(uintptr_t)15);
  int32_t xs[2] = {1, 1};
  int16_t lay[2] = {0, 0};
  if (orx_abi_version() != ORX_ABI_VERSION) { printf("abi mismatch\n"); return 1; }
  if (ORX_SEEK_PLAYER != 0 || ORX_SEEK_NPC != 1 || ORX_SEEK_ITEM != 2 || ORX_SEEK_COLS != 4 ||
      ORX_SEEK_UNREACHABLE != -1 || ORX_SEEK_ABSENT != -2) { printf("constants\n"); return 2; }
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

  /* orx_path_rows */
  refused("rows: NULL cfg", orx_path_rows(NULL, tiles, lay32, cell, rows, 1, NULL));
  refused("rows: no layouts", orx_path_rows(&c, tiles, lay32, cell, rows, 1, NULL));
  refused("rows: NULL tiles", orx_path_rows(&bank, NULL, lay32, cell, rows, 1, NULL));
  refused("rows: NULL layout", orx_path_rows(&bank, tiles, NULL, cell, rows, 1, NULL));
  refused("rows: NULL cell", orx_path_rows(&bank, tiles, lay32, NULL, rows, 1, NULL));
  refused("rows: NULL rows", orx_path_rows(&bank, tiles, lay32, cell, NULL, 1, NULL));
  refused("rows: zero rows", orx_path_rows(&bank, tiles, lay32, cell, rows, 0, NULL));
  refused("rows: negative rows", orx_path_rows(&bank, tiles, lay32, cell, rows, -1, NULL));
  bank.width = 257; bank.height = 256;
  refused("rows: too many tiles", orx_path_rows(&bank, tiles, lay32, cell, rows, 1, NULL));
  bank.width = 0; bank.height = 4;
  refused("rows: zero width", orx_path_rows(&bank, tiles, lay32, cell, rows, 1, NULL));
  bank.width = 4;

  /* orx_path_seek */
  refused("seek: player 2", orx_path_seek(&c, &full, NULL, 2, dist, move, target, 1, NULL));
  refused("seek: player -1", orx_path_seek(&c, &full, NULL, -1, dist, move, target, 1, NULL));
  refused("seek: no outputs", orx_path_seek(&c, &full, NULL, 0, NULL, NULL, NULL, 1, NULL));
  refused("seek: zero games", orx_path_seek(&c, &full, NULL, 0, dist, move, target, 0, NULL));
  refused("seek: negative games",
          orx_path_seek(&c, &full, NULL, 0, dist, move, target, -3, NULL));
  refused("seek: misaligned dist",
          orx_path_seek(&c, &full, NULL, 0, dist + 1, move, target, 1, NULL));
  refused("seek: misaligned move",
          orx_path_seek(&c, &full, NULL, 0, dist, move + 1, target, 1, NULL));
  refused("seek: misaligned target",
          orx_path_seek(&c, &full, NULL, 0, dist, move, target + 1, 1, NULL));
  refused("seek: NULL state", orx_path_seek(&c, NULL, NULL, 0, dist, move, target, 1, NULL));
  refused("seek: NULL p_x", orx_path_seek(&c, &st, NULL, 0, dist, move, target, 1, NULL));
  full.p_depth = NULL;
  refused("seek: NULL p_depth", orx_path_seek(&c, &full, NULL, 0, dist, move, target, 1, NULL));
  full.p_depth = xs;
  full.st_x = NULL;
  refused("seek: NULL st_x", orx_path_seek(&c, &full, NULL, 0, dist, move, target, 1, NULL));
  full.st_x = xs;
  refused("seek: NPCs without npc_pos",
          orx_path_seek(&npcs, &full, NULL, 0, dist, move, target, 1, NULL));
  refused("seek: bank without pairs",
          orx_path_seek(&bank, &fb, NULL, 0, dist, move, target, 1, NULL));
  fb.p_layout = NULL;
  refused("seek: bank without p_layout",
          orx_path_seek(&bank, &fb, pairs, 0, dist, move, target, 1, NULL));
  fb.p_layout = lay;
  fb.bank_tiles = NULL;
  refused("seek: bank without bank_tiles",
          orx_path_seek(&bank, &fb, pairs, 0, dist, move, target, 1, NULL));
  c.width = 3;
  refused("seek: bad cfg", orx_path_seek(&c, &full, NULL, 0, dist, move, target, 1, NULL));
  printf("orx_path_seek refusals: %d of %d\n", n_ok, n_all);
  return n_ok == n_all ? 0 : 7;
}
