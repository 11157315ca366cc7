"""Times the tick with the NPCs' moves supplied by the caller (orx_npc_*,
include/orx_npc.h) beside the ticks of the built-in enemy AIs, on the C3 shape
(64 x 64, 8 NPCs, 65,536 games).

    python tools/bench_npc.py [--modes=given,random,chase] [--steps=512] [--ticks=128]
                              [--games=65536] [--lib=PATH] [--label=NAME] [--out=FILE.jsonl]

One process measures one library (--lib loads another build, e.g. a parent
commit's liborx.so, which has only the AI modes); run the builds alternately,
three processes each, and compare a build's lines with the other build's own
run-to-run spread.  One JSON line per measurement, each with the library's
build ids:

* ``vecenv_eager`` -- VecEnv.step through a ring of two output sets, player 2
  a RandomBot, --steps steps between two HIP events, the second-fastest of
  four blocks.  ``given``: cfg.npc_policy Stay and ``step(a, npc_moves=table[t
  % 64])`` with a uniform random int8 table resident on the device (what a
  policy for the NPCs would have written); ``random`` / ``chase``:
  cfg.npc_policy, no table.
* ``vecenv_graph`` -- the same step captured in a HIP graph (static action and
  table tensors), replayed --steps times.
* ``step_n`` -- orx_npc_step_n (given) or orx_step_n (the AIs) over --ticks
  ticks of a uniform random move log, no rows, the median of ten launches.

The given tick runs the AIs' resolution without an AI and reads 8 more bytes
per game, so it is expected to cost no more than the RANDOM tick.  --games=1024
makes the kernels negligible: ``vecenv_eager`` is then the host's cost per step
(the eager loop runs at the slower of the host and the kernel).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, RING = 8, 64


def timed_block(torch, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def main():
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    from optimax_rogue_amd import _lib
    if "lib" in opts:
        _lib.LIB_PATH = os.path.abspath(opts["lib"])
    import torch
    from optimax_rogue_amd import EnvConfig, VecEnv
    from optimax_rogue_amd.engine import BatchedEngine
    modes = opts.get("modes", "given,random,chase").split(",")
    steps, ticks = int(opts.get("steps", 512)), int(opts.get("ticks", 128))
    B = int(opts.get("games", 65536))
    dev = torch.device("cuda", 0)
    ids = {"label": opts.get("label", "tree"), "build_id": _lib.build_id(),
           "npc_build_id": _lib.part_id("npc"), "games": B, "n_npcs": K}
    gen = torch.Generator().manual_seed(7)
    acts = torch.randint(1, 6, (RING, B), generator=gen, dtype=torch.int8).to(dev)
    tables = torch.randint(1, 6, (RING, K, B), generator=gen, dtype=torch.int8).to(dev)
    lines = []

    def emit(rec):
        rec = dict(ids, **rec)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for mode in modes:
        given = mode == "given"
        pol = {"given": 0, "random": 1, "chase": 2}[mode]
        cfg = EnvConfig(64, 64, n_npcs=K, npc_policy=pol)
        mk = lambda ring: VecEnv(cfg, B, seed=3, opponent=1, check_actions=False, out_buffers=ring)
        # eager, through the ring
        env = mk(2)
        it = [0]

        def eager():
            t = it[0] = (it[0] + 1) % RING
            env.step(acts[t], npc_moves=tables[t]) if given else env.step(acts[t])
        for _ in range(32):
            eager()
        torch.cuda.synchronize()
        blocks = [timed_block(torch, eager, steps) for _ in range(4)]
        emit({"what": "vecenv_eager", "mode": mode, "steps": steps,
              "us_per_step": round(sorted(blocks)[1], 3),
              "us_blocks": [round(v, 3) for v in blocks]})
        # captured
        env = mk(1)
        sa, st = acts[0].clone(), tables[0].clone()
        step = (lambda: env.step(sa, npc_moves=st)) if given else (lambda: env.step(sa))
        step()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                step()
        torch.cuda.current_stream(dev).wait_stream(s)
        for _ in range(32):
            g.replay()
        torch.cuda.synchronize()
        blocks = [timed_block(torch, g.replay, steps) for _ in range(4)]
        emit({"what": "vecenv_graph", "mode": mode, "steps": steps,
              "us_per_step": round(sorted(blocks)[1], 3),
              "us_blocks": [round(v, 3) for v in blocks]})
        del env, g
        # the replay of a move log
        eng = BatchedEngine(cfg, B, seed=3, device=dev)
        log = torch.randint(1, 6, (ticks, B, 2), generator=gen, dtype=torch.int8).to(dev)
        tab = torch.randint(1, 6, (ticks, K, B), generator=gen, dtype=torch.int8).to(dev) \
            if given else None
        replay = lambda: eng.step_n(log, npc_moves=tab) if given else eng.step_n(log)
        replay()
        torch.cuda.synchronize()
        ts = sorted(timed_block(torch, replay, 1) for _ in range(10))
        emit({"what": "step_n", "mode": mode, "ticks": ticks, "us_per_launch": round(ts[5], 2),
              "us_min_max": [round(ts[0], 2), round(ts[-1], 2)]})
        del eng, log, tab
        torch.cuda.empty_cache()
    if "out" in opts:
        path = os.path.abspath(opts["out"])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
