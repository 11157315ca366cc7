// plan_main.cpp -- prints the launch plan (optimax_rogue_amd/csrc/orx_plan.h)
// for the requests on its standard input, one per line, on a device of 1,024
// SIMDs and 160 KiB of LDS per workgroup (what the library assumes without a
// GPU).  Host code only: tests/test_plan.py builds it with g++, which proves
// the header needs no HIP, and compares the plans with orx_rollout_shape and
// with values derived by hand.
//
//   rollout  W H K flags n_layouts rng npc_policy  p1 p2 B trajectory compact concurrency [VAR=value ...]
//   step_n   W H K flags n_layouts rng npc_policy  B rows concurrency [VAR=value ...]
//   env_step W H K flags n_layouts rng npc_policy  B obs_aligned [VAR=value ...]
//
// A line may begin with two more words, the device's SIMD count and its LDS
// bytes per workgroup ("64 65536 rollout ..."): the plan on that device
// (tests/test_instance_sweep.py shows its requests' plans do not depend on it).
//
// The VAR=value words are the line's ORX_* environment.  Output per line:
//   form pm lanes nt threads blocks lds_bytes lds_n lds_bits lds_rows
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../optimax_rogue_amd/csrc/orx_plan.h"

using namespace orx_dev;

int main() {
  const Device default_dev{1024, 160 * 1024};
  const char* forms[] = {"moving", "mt", "paired", "one-lane", "replay", "generic"};
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    orx_cfg_t c{};
    Device dev = default_dev;
    if (!(in >> kind)) continue;
    if (kind[0] >= '0' && kind[0] <= '9') {  // the optional device: SIMDs, LDS bytes
      dev.simds = atoi(kind.c_str());
      if (!(in >> dev.lds_per_block >> kind) || dev.simds < 1) {
        fprintf(stderr, "bad device: %s\n", line.c_str());
        return 2;
      }
    }
    if (!(in >> c.width >> c.height >> c.n_npcs >> c.flags >> c.n_layouts >> c.rng >>
          c.npc_policy))
      continue;
    long long a[6] = {0, 0, 0, 0, 0, 0};
    const int n_args = kind == "rollout" ? 6 : kind == "step_n" ? 3 : kind == "env_step" ? 2 : -1;
    for (int i = 0; i < n_args; ++i) in >> a[i];
    if (n_args < 0 || !in) {
      fprintf(stderr, "bad request: %s\n", line.c_str());
      return 2;
    }
    std::vector<std::string> vars;
    for (std::string w; in >> w;) {
      const size_t eq = w.find('=');
      if (eq == std::string::npos) return 2;
      vars.push_back(w.substr(0, eq));
      setenv(vars.back().c_str(), w.c_str() + eq + 1, 1);
    }
    const Env env = read_env();
    for (const std::string& v : vars) unsetenv(v.c_str());
    Plan p;
    if (kind == "rollout")
      p = plan_rollout({&c, (int32_t)a[0], (int32_t)a[1], (uint32_t)a[2], a[3] != 0, a[4] != 0,
                        (uint32_t)a[5]}, env, dev);
    else if (kind == "step_n")
      p = plan_step_n(&c, (uint32_t)a[0], (int)a[1], (uint32_t)a[2], env, dev);
    else
      p = plan_env_step(&c, (uint32_t)a[0], a[1] != 0, env);
    printf("%s %d %u %d %u %u %u %u %u %d\n", forms[(int)p.form], p.pm, p.lanes, (int)p.nt,
           p.threads, p.blocks, p.lds_bytes, p.lds_n, p.lds_bits, (int)p.lds_rows);
  }
  return 0;
}
