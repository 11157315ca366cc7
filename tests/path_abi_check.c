/* Plain-C consumer of include/orx_path.h next to include/orx.h: the header
 * compiles as C99 and both entry points link and refuse bad arguments on the
 * host, before any launch.  Built and run by tests/test_path.py (no GPU
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
  orx_cfg_t c, bank;
  orx_state_t st, full;
  uint8_t tiles[16];
  uint16_t field[16], window[9];
  int32_t dist[1];
  int8_t move[1];
  int32_t xs[2] = {1, 1};
  int16_t lay[2] = {0, 0};
  if (orx_abi_version() != ORX_ABI_VERSION) { printf("abi mismatch\n"); return 1; }
  if (ORX_PATH_WALL != 0xFFFF || ORX_PATH_UNREACHABLE != 0xFFFE) { printf("constants\n"); return 2; }
  if (strlen(orx_path_build_id()) != 16) { printf("path build id: %s\n", orx_path_build_id()); return 3; }
  memset(&c, 0, sizeof c);
  memset(&st, 0, sizeof st);
  c.width = 10; c.height = 8; c.despawn = ORX_DESPAWN_UNREACHABLE; c.max_ticks = 30;
  c.start_mode = ORX_START_TOGETHER; c.n_npcs = 0; c.npc_health = 3; c.npc_damage = 1;
  c.player_health = 10; c.player_damage = 2; c.player_armor = 1; c.autoreset = 1;
  if (orx_validate_cfg(&c) != ORX_OK) { printf("valid cfg rejected: %s\n", orx_last_error()); return 4; }
  full = st;
  full.p_x = xs; full.p_y = xs; full.st_x = xs; full.st_y = xs; full.p_layout = lay;
  bank = c;
  bank.width = 4; bank.height = 4; bank.n_layouts = 1;
  if (orx_validate_cfg(&bank) != ORX_OK) { printf("valid bank cfg rejected: %s\n", orx_last_error()); return 5; }

  /* orx_path_field */
  refused("field: NULL cfg", orx_path_field(NULL, tiles, field, NULL));
  refused("field: no layouts", orx_path_field(&c, tiles, field, NULL));
  refused("field: NULL tiles", orx_path_field(&bank, NULL, field, NULL));
  refused("field: NULL field", orx_path_field(&bank, tiles, NULL, NULL));
  bank.width = 257; bank.height = 256;
  refused("field: too many tiles", orx_path_field(&bank, tiles, field, NULL));
  bank.width = 0; bank.height = 4;
  refused("field: zero width", orx_path_field(&bank, tiles, field, NULL));
  bank.width = 4;

  /* orx_path_query */
  refused("query: player 2", orx_path_query(&c, &full, NULL, 2, 1, dist, move, window, 1, NULL));
  refused("query: radius 0", orx_path_query(&c, &full, NULL, 0, 0, dist, move, window, 1, NULL));
  refused("query: radius 16",
          orx_path_query(&c, &full, NULL, 0, ORX_VIEW_MAX_RADIUS + 1, dist, move, window, 1, NULL));
  refused("query: no outputs", orx_path_query(&c, &full, NULL, 0, 1, NULL, NULL, NULL, 1, NULL));
  refused("query: zero games", orx_path_query(&c, &full, NULL, 0, 1, dist, move, NULL, 0, NULL));
  refused("query: NULL state", orx_path_query(&c, NULL, NULL, 0, 1, dist, move, NULL, 1, NULL));
  refused("query: NULL p_x", orx_path_query(&c, &st, NULL, 0, 1, dist, move, NULL, 1, NULL));
  full.st_x = NULL;
  refused("query: NULL st_x", orx_path_query(&c, &full, NULL, 0, 1, dist, move, NULL, 1, NULL));
  full.st_x = xs;
  refused("query: bank without field",
          orx_path_query(&bank, &full, NULL, 0, 1, dist, move, NULL, 1, NULL));
  full.p_layout = NULL;
  refused("query: bank without p_layout",
          orx_path_query(&bank, &full, field, 0, 1, dist, move, NULL, 1, NULL));
  c.width = 3;
  refused("query: bad cfg", orx_path_query(&c, &full, NULL, 0, 1, dist, move, NULL, 1, NULL));
  printf("orx_path refusals: %d of %d\n", n_ok, n_all);
  return n_ok == n_all ? 0 : 6;
}
