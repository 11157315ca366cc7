/* Plain-C consumer of include/orx_view.h next to include/orx.h: the view's
 * header compiles as C99 and its entry point links and refuses bad arguments
 * on the host.  Built and run by tests/test_view.py (no GPU calls). */
#include <stdio.h>
#include <string.h>

#include "orx.h"
#include "orx_view.h"

int main(void) {
  orx_cfg_t c;
  orx_state_t st;
  uint8_t cells[9];
  int r;
  if (orx_abi_version() != ORX_ABI_VERSION) { printf("abi mismatch\n"); return 1; }
  memset(&c, 0, sizeof c);
  memset(&st, 0, sizeof st);
  c.width = 10; c.height = 8; c.despawn = ORX_DESPAWN_UNREACHABLE; c.max_ticks = 30;
  c.start_mode = ORX_START_TOGETHER; c.n_npcs = 4; c.npc_health = 3; c.npc_damage = 1;
  c.player_health = 10; c.player_damage = 2; c.player_armor = 1; c.autoreset = 1;
  if (orx_validate_cfg(&c) != ORX_OK) { printf("valid cfg rejected: %s\n", orx_last_error()); return 2; }
  if ((ORX_VIEW_PLAYER | ORX_VIEW_NPC | ORX_VIEW_ITEM | ORX_VIEW_ITEM_KIND | ORX_VIEW_TILE_MASK) != 63 ||
      ORX_VIEW_OUTSIDE != 0 || ORX_VIEW_MAX_RADIUS != 15) { printf("bit values\n"); return 3; }
  if (orx_view(&c, &st, 2, 1, cells, NULL, 1, NULL) != ORX_EINVAL) { printf("player 2 accepted\n"); return 4; }
  if (orx_view(&c, &st, 0, 0, cells, NULL, 1, NULL) != ORX_EINVAL) { printf("radius 0 accepted\n"); return 5; }
  if (orx_view(&c, &st, 0, ORX_VIEW_MAX_RADIUS + 1, cells, NULL, 1, NULL) != ORX_EINVAL) {
    printf("radius 16 accepted\n"); return 6;
  }
  if (orx_view(&c, &st, 0, 1, NULL, NULL, 1, NULL) != ORX_EINVAL) { printf("NULL cells accepted\n"); return 7; }
  if (orx_view(&c, &st, 0, 1, cells, NULL, 0, NULL) != ORX_EINVAL) { printf("zero games accepted\n"); return 8; }
  if (orx_view(&c, NULL, 0, 1, cells, NULL, 1, NULL) != ORX_EINVAL) { printf("NULL state accepted\n"); return 9; }
  c.width = 3;
  r = orx_view(&c, &st, 0, 1, cells, NULL, 1, NULL);
  if (r != ORX_EINVAL || strlen(orx_last_error()) == 0) { printf("bad cfg accepted\n"); return 10; }
  printf("orx_view refused: %d (%s)\n", r, orx_last_error());
  printf("sizeof(orx_cfg_t)=%zu\n", sizeof(orx_cfg_t));
  return 0;
}
