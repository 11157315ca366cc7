/* Plain-C consumer of include/orx_npc.h next to include/orx.h: the header
 * compiles as C99, the entry points link, orx_npc_max_events answers and
 * every refusal the header lists comes back from the host, before any device
 * call.  Built and run by tests/test_npc_given.py (no GPU calls: every step
 * call here must be refused; the pointers are host memory, never read). */
#include <stdio.h>
#include <string.h>

#include "orx.h"
#include "orx_npc.h"

static int n_ok = 0, n_all = 0;

/* r is ORX_EINVAL and the message names the reason (`needle`): the state
 * below is all NULL, so a call that got past its own check would be refused
 * for the state instead */
static void refused_for(const char* what, int r, const char* needle) {
  ++n_all;
  if (r == ORX_EINVAL && strstr(orx_last_error(), needle) != NULL) ++n_ok;
  else printf("%s: returned %d (%s)\n", what, r, orx_last_error());
}

static orx_state_t st;
static int8_t actions[2], table[255], act[2];
static int32_t obs[ORX_OBS_FIELDS], events[4 * 516], n_events[1], status[1];
static float reward[1];
static uint8_t done[1];

/* every entry point with this cfg and this table: each must refuse */
static void all_refuse(const char* what, const orx_cfg_t* c, const int8_t* moves,
                       const char* needle) {
  orx_env_step_args_t a;
  char name[128];
  memset(&a, 0, sizeof a);
  a.cfg = c; a.st = &st; a.actions = actions; a.action_bytes = 1; a.action_cols = 2;
  a.policy_p2 = ORX_POLICY_NONE; a.act = act; a.obs = obs; a.reward = reward; a.done = done;
  a.status = status; a.n_games = 1;
  snprintf(name, sizeof name, "%s: orx_npc_step", what);
  refused_for(name, orx_npc_step(c, &st, actions, moves, 1, 0, 0, NULL), needle);
  snprintf(name, sizeof name, "%s: orx_npc_step_events", what);
  refused_for(name, orx_npc_step_events(c, &st, actions, moves, events, n_events, 1, 0, 0, NULL),
              needle);
  snprintf(name, sizeof name, "%s: orx_npc_step_n", what);
  refused_for(name,
              orx_npc_step_n(c, &st, actions, moves, 1, NULL, ORX_OBS_INT32, 1, 0, 0, 1, NULL),
              needle);
  snprintf(name, sizeof name, "%s: orx_npc_env_step", what);
  refused_for(name, orx_npc_env_step(&a, moves), needle);
}

int main(void) {
  orx_cfg_t c, bad;
  orx_env_step_args_t a;
  int i;
  if (orx_abi_version() != ORX_ABI_VERSION) { printf("abi mismatch\n"); return 1; }
  if (strlen(orx_npc_build_id()) != 16) { printf("npc build id: %s\n", orx_npc_build_id()); return 2; }
  memset(&st, 0, sizeof st);   /* (never reached: every call is refused before the state) */
  for (i = 0; i < 255; ++i) table[i] = ORX_MOVE_STAY;
  actions[0] = actions[1] = ORX_MOVE_STAY;
  memset(&c, 0, sizeof c);
  c.width = 20; c.height = 20; c.despawn = ORX_DESPAWN_UNREACHABLE; c.max_ticks = 30;
  c.start_mode = ORX_START_TOGETHER; c.n_npcs = 8; c.npc_health = 3; c.npc_damage = 1;
  c.player_health = 10; c.player_damage = 2; c.player_armor = 1; c.autoreset = 1;
  if (orx_validate_cfg(&c) != ORX_OK) { printf("valid cfg rejected: %s\n", orx_last_error()); return 3; }

  /* orx_npc_max_events: 6 + 2 K or ORX_MAX_EVENTS, whatever npc_policy says */
  if (orx_npc_max_events(&c) != 22) { printf("max events K=8: %d\n", orx_npc_max_events(&c)); return 4; }
  bad = c; bad.npc_policy = ORX_NPC_CHASE;
  if (orx_npc_max_events(&bad) != 22) { printf("max events K=8 chase\n"); return 4; }
  bad = c; bad.n_npcs = 255;
  if (orx_npc_max_events(&bad) != 516) { printf("max events K=255: %d\n", orx_npc_max_events(&bad)); return 4; }
  bad = c; bad.n_npcs = 1;
  if (orx_npc_max_events(&bad) != ORX_MAX_EVENTS) { printf("max events K=1\n"); return 4; }

  bad = c; bad.n_npcs = 0;
  all_refuse("n_npcs 0", &bad, table, "n_npcs");
  refused_for("n_npcs 0: orx_npc_max_events", orx_npc_max_events(&bad), "n_npcs");
  bad = c; bad.flags = ORX_EXT_MANA; bad.mana_max = 9; bad.mana_regen = 1; bad.mana_per_point = 1;
  if (orx_validate_cfg(&bad) != ORX_OK) { printf("mana cfg rejected: %s\n", orx_last_error()); return 5; }
  all_refuse("flags outside the limit", &bad, table, "flags within");
  refused_for("flags outside the limit: orx_npc_max_events", orx_npc_max_events(&bad),
              "flags within");
  all_refuse("NULL table", &c, NULL, "npc_moves is NULL");
  bad = c; bad.width = 3;
  all_refuse("invalid cfg", &bad, table, "width and height");
  refused_for("invalid cfg: orx_npc_max_events", orx_npc_max_events(&bad), "width and height");
  all_refuse("NULL cfg", NULL, table, "cfg is NULL");
  bad = c; bad.npc_policy = 3;
  all_refuse("npc_policy 3", &bad, table, "npc_policy");

  /* stock-seed mode: orx_npc_step_n and orx_npc_env_step refuse it */
  bad = c; bad.rng = ORX_RNG_MT19937;
  if (orx_validate_cfg(&bad) != ORX_OK) { printf("stock cfg rejected: %s\n", orx_last_error()); return 6; }
  refused_for("stock-seed: orx_npc_step_n",
              orx_npc_step_n(&bad, &st, actions, table, 1, NULL, ORX_OBS_INT32, 1, 0, 0, 1, NULL),
              "stock-seed");
  memset(&a, 0, sizeof a);
  a.cfg = &bad; a.st = &st; a.actions = actions; a.action_bytes = 1; a.action_cols = 2;
  a.policy_p2 = ORX_POLICY_NONE; a.act = act; a.obs = obs; a.reward = reward; a.done = done;
  a.n_games = 1;
  refused_for("stock-seed: orx_npc_env_step", orx_npc_env_step(&a, table), "stock-seed");
  refused_for("NULL args", orx_npc_env_step(NULL, table), "args is NULL");
  printf("orx_npc refusals: %d of %d\n", n_ok, n_all);
  return n_ok == n_all ? 0 : 7;
}
