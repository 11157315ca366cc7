"""CPU: the launch plan (optimax_rogue_amd/csrc/orx_plan.h) as plain C++.
tests/plan_main.cpp is built with g++ against orx_plan.h and include/orx.h
alone -- the compile proves the header needs no HIP -- and prints the plan of
each request for a device of 1,024 SIMDs and 160 KiB of LDS, what the library
assumes without a GPU.  Rollouts must agree with orx_rollout_shape (the cases
of test_abi.py's two shape tests, overrides included); the shapes no entry
point reports are pinned to values derived by hand from the rules."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("form", "pm", "lanes", "nt", "threads", "blocks", "lds_bytes", "lds_n", "lds_bits",
        "lds_rows")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan") / "plan_main"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "plan_main.cpp"), "-o", str(exe)], check=True)

    def run(requests):
        """requests: (kind, EnvConfig, n_layouts, args, env dict) -> one dict per request."""
        lines = []
        for kind, cfg, n_layouts, args, env in requests:
            c = cfg.to_c()
            words = [kind, c.width, c.height, c.n_npcs, c.flags, n_layouts, c.rng, c.npc_policy,
                     *args, *("%s=%s" % kv for kv in env.items())]
            lines.append(" ".join(str(w) for w in words))
        r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True,
                           text=True, env={k: v for k, v in os.environ.items()
                                           if not k.startswith("ORX_")})
        assert r.returncode == 0, r.stderr
        out = [dict(zip(KEYS, (w if i == 0 else int(w) for i, w in enumerate(l.split()))))
               for l in r.stdout.splitlines()]
        assert len(out) == len(requests)
        return out
    return run


def rollout_cases():
    """(cfg, B, p1, p2, trajectory, concurrency, n_layouts, env): every request of
    test_abi.py::test_rollout_shape_rules and ::test_rollout_shape_bank_lds."""
    from optimax_rogue_amd import EnvConfig as E
    c2, c3, c5 = E.c2(), E.c3(), E.c5()
    rpg = E(width=64, height=64, n_npcs=8, flags=4 | 8 | 16 | 32)
    small = E(width=12, height=10)
    rules = [(c5, 16384, 2, 2), (c2, 4096), (c5, 32768, 2, 2), (c5, 131072, 2, 2),
             (c3, 32768, 1, 1, 1, 2), (c3, 32768), (c3, 65536), (E(n_npcs=40), 4096),
             (c5, 16384, 2, 1), (c3, 32768, 1, 2, 1, 2),
             (E(width=20, height=20, flags=1, sep_period=3), 4096, 1, 2),
             (small, 4096, 2, 1, 1, 1, 4), (c3, 65536, 1, 2), (c2, 4096, 1, 1, 0),
             (rpg, 32768, 1, 1, 1, 2), (rpg, 4096), (c3, 32768, 1, 1, 1, 2, 16),
             (small, 4096, 2, 2, 1, 1, 4),
             (E(width=12, height=10, flags=1, sep_period=2), 4096, 2, 2, 1, 1, 4),
             (E(width=300, height=200), 4096, 2, 2), (c5, 65536, 2, 2, 1, 2),
             (c5, 131072, 2, 2, 1, 2), (c3, 65536, 1, 1, 1, 2)]
    defaults = (None, None, 1, 1, 1, 1, 0)
    cases = [r + defaults[len(r):] + ({},) for r in rules]
    bank = lambda n, env: (c3, 32768, 1, 1, 1, 2, n, env)
    cases += [bank(n, {}) for n in (16, 20, 24, 40, 41)]
    cases += [bank(n, {"ORX_REFUSE_LDS_RAISE": "1"}) for n in (16, 24)]
    cases += [bank(24, {"ORX_ROLLOUT_THREADS": "256"})]
    return cases


def test_rollout_plan_is_what_orx_rollout_shape_reports(plans, engine_lib, monkeypatch):
    from optimax_rogue_amd._lib import OrxRolloutShape
    cases = rollout_cases()
    got = plans([("rollout", cfg, n_layouts, (p1, p2, B, traj, 0, conc), env)
                 for cfg, B, p1, p2, traj, conc, n_layouts, env in cases])
    paired = 0
    for (cfg, B, p1, p2, traj, conc, n_layouts, env), p in zip(cases, got):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            c, out = cfg.to_c(), OrxRolloutShape()
            c.n_layouts = n_layouts
            assert engine_lib.orx_rollout_shape(ctypes.byref(c), p1, p2, B, traj, conc,
                                                ctypes.byref(out)) == 0
        assert (p["lanes"], 2 if p["form"] == "paired" else 1, p["nt"], p["threads"],
                p["lds_bytes"]) == (out.games_per_wave, out.lanes_per_game, out.nontemporal,
                                    out.threads_per_block, out.lds_bytes), (cfg, B, env, p)
        assert p["blocks"] == -(-B // (p["threads"] // 64 * p["lanes"]))
        paired += p["form"] == "paired"
    assert 0 < paired < len(cases)


def test_plans_no_entry_point_reports(plans):
    """C3 (64 x 64, 8 NPCs, no flags) at 1,024 SIMDs, by hand from the rules:
    paired waves hold 32 games once B * concurrency >= 2 * 1,024 * 32, at
    least 8; one-lane waves 64 once B >= 1,024 * 64, at least 16; a wave's row
    segment is a whole 128-B line (nontemporal stores) from 32 games up;
    workgroups = ceil(B / (threads / 64 * games per wave))."""
    from optimax_rogue_amd import EnvConfig
    c3 = EnvConfig.c3()
    chase = EnvConfig(width=64, height=64, n_npcs=8, npc_policy=2)
    one = {"ORX_REPLAY_PAIRED": "0"}
    got = plans([
        ("step_n", c3, 0, (65536, 1, 1), {}), ("step_n", c3, 0, (32768, 1, 2), {}),
        ("step_n", c3, 0, (4096, 1, 1), {}),
        ("step_n", c3, 0, (65536, 1, 1), one), ("step_n", c3, 0, (4096, 1, 1), one),
        ("env_step", c3, 0, (65536, 1), {}), ("env_step", c3, 0, (65536, 1), {"ORX_ENV_LANES": "32"}),
        ("env_step", c3, 0, (65536, 0), {}),
        ("env_step", c3, 0, (65536, 1), {"ORX_ENV_DIRECT_ROWS": "1"}),
        ("rollout", chase, 0, (1, 1, 4096, 1, 0, 1), {}),
        ("rollout", chase, 0, (1, 1, 4096, 1, 0, 1), {"ORX_MOV_LANES": "16"}),
        ("rollout", c3, 16, (1, 1, 32768, 1, 1, 2), {}),
        ("rollout", c3, 16, (1, 1, 32768, 1, 0, 2), {}),
    ])
    shape = lambda p: (p["form"], p["lanes"], p["threads"], p["blocks"])
    assert [shape(p) + (p["pm"], p["nt"]) for p in got[:3]] == [
        ("paired", 32, 256, 512, 6, 1), ("paired", 32, 256, 256, 6, 1),
        ("paired", 8, 256, 128, 6, 0)]                       # (partial lines: default-policy stores)
    assert [shape(p) for p in got[3:5]] == [("replay", 64, 256, 256), ("replay", 16, 256, 64)]
    assert [shape(p) + (p["lds_rows"],) for p in got[5:9]] == [
        ("generic", 64, 256, 256, 1), ("generic", 32, 256, 512, 1),
        ("generic", 64, 256, 256, 0), ("generic", 64, 256, 256, 0)]   # (direct rows)
    assert [shape(p) for p in got[9:11]] == [("moving", 64, 256, 16), ("moving", 16, 256, 64)]
    # compact rows have no bank instance of the buffer-store forms: the generic
    # one-lane form (PM 0, always nontemporal) with the tiles in LDS, at the
    # one-lane rule's 32 games per wave (32,768 >= 1,024 * 32); int32 rows pair
    assert shape(got[11]) + (got[11]["pm"], got[11]["nt"], got[11]["lds_bytes"]) == (
        "one-lane", 32, 256, 256, 0, 1, 65536)
    assert shape(got[12]) + (got[12]["pm"], got[12]["nt"]) == ("paired", 32, 256, 256, 1, 1)
