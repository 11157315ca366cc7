"""Times stock-seed mode (cfg.rng = ORX_RNG_MT19937), which bench.py does not
run: orx_reset, orx_policy + orx_step and orx_rollout(64).

    python tools/bench_stock.py [--games=65536] [--launches=200] [--lib=PATH]
                                [--out=profiles/game_record/bench_stock.jsonl]

Protocol.  Two configurations at --games games: the register-NPC one of the
stock tests (10 x 9, 4 NPCs, Unused despawn, max_ticks 30) and 128 x 128
without NPCs (the parity tests' ``stock_c5_stairs``); bots (1, 2).  Each shape
is warmed up (a reset, 8 policy + step pairs, one rollout), then every call is
timed --launches times (at least 200), each launch between two HIP events, and
the line quotes the median with the minimum and the 90th percentile.  --lib
loads another build of the library (an A/B against a parent's liborx.so).
One JSON line per configuration and call.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "stock_register": dict(width=10, height=9, n_npcs=4, despawn=2, max_ticks=30, rng=1),
    "stock_c5_stairs": dict(width=128, height=128, rng=1),
}
ROLLOUT_TICKS = 64


def timed(torch, fn, n):
    """microseconds of each of n launches of fn (one event pair per launch)"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) * 1e3 for a, b in ev)


def main():
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    B = int(opts.get("games", 65536))
    launches = max(200, int(opts.get("launches", 200)))
    if "lib" in opts:
        from optimax_rogue_amd import _lib
        _lib.LIB_PATH = os.path.abspath(opts["lib"])
    import torch
    from optimax_rogue_amd import EnvConfig
    from optimax_rogue_amd.engine import BatchedEngine
    dev = torch.device("cuda", 0)
    lines = []
    for name, cfg in CONFIGS.items():
        eng = BatchedEngine(EnvConfig.from_dict(cfg), B, seed=7, device=dev)

        def policy_step():
            eng.step(eng.policy(1, 2))

        calls = {"reset": eng.reset, "policy_step": policy_step,
                 "rollout64": lambda: eng.rollout(ROLLOUT_TICKS, 1, 2)}
        eng.reset()
        for _ in range(8):
            policy_step()
        eng.rollout(ROLLOUT_TICKS, 1, 2)
        torch.cuda.synchronize()
        for call, fn in calls.items():
            ts = timed(torch, fn, launches)
            rec = {"config": name, "games": B, "call": call, "launches": launches,
                   "median_us": round(ts[len(ts) // 2], 2), "min_us": round(ts[0], 2),
                   "p90_us": round(ts[int(len(ts) * 0.9)], 2)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del eng
        torch.cuda.empty_cache()
    if "out" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["out"])), exist_ok=True)
        with open(opts["out"], "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
