"""Times the enemies' queries (orx_npc_options / orx_npc_seek,
include/orx_npc_query.h) and the closed loop they make possible, on the C3
shape (64 x 64, 8 NPCs, 65,536 games), beside the players' queries and the
built-in CHASE tick measured in the same process.

    python tools/bench_npc_query.py [--calls=512] [--games=65536] [--ticks=40]
                                    [--lib=PATH] [--label=NAME] [--out=FILE.jsonl]

One process measures one library (--lib loads another build, e.g. a parent
commit's liborx.so, which has only the yardsticks); run the builds
alternately and compare a build's lines with the other build's own run-to-run
spread.  The state is the one after --ticks ticks of RandomBot players and a
uniform random NPC table (Stay NPCs for a library without orx_npc_step).  One
JSON line per measurement, each with the library's build ids; a time is the
second-fastest of four blocks of --calls calls between two HIP events:

* ``query`` -- us per call of ``npc_options`` (all four outputs),
  ``npc_options_kind`` (kind and where only), ``npc_seek``, and of the
  yardsticks ``moves`` and ``seek`` for player 0, every one into preallocated
  outputs.  With each of the enemies' queries its algorithmic bytes (every
  state row it reads counted once per game, plus the rows written: K * B * 40 B
  for options) and the bytes/s they make of the time.
* ``graph`` -- us per replay of a captured tick: ``hunt`` is
  ``npc_hunt_moves`` -> a static table -> ``VecEnv.step(a, npc_moves=table)``;
  ``given`` the same step with a resident table (no queries); ``chase``
  ``VecEnv.step`` with cfg.npc_policy CHASE (the yardstick).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 8


def timed_block(torch, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def query_bytes(B, k):
    """name -> algorithmic bytes of one call (closed form, NPCs in registers)."""
    players = 2 * 4 * B                    # one int32 [2][B] row
    header = 3 * players + 2 * players     # p_x, p_y, p_depth; st_x, st_y
    npcs = 4 * B + 2 * k * B               # npc_alive, npc_pos
    options = header + players + npcs + k * B   # ... and p_health, npc_health
    return {"npc_options": options + k * B * 40 + B,
            "npc_options_kind": options + k * B * 8 + B,
            "npc_seek": header + npcs + k * B * (16 + 4 + 8)}


def main():
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    from optimax_rogue_amd import _lib
    if "lib" in opts:
        _lib.LIB_PATH = os.path.abspath(opts["lib"])
    import torch
    from optimax_rogue_amd import EnvConfig, VecEnv
    from optimax_rogue_amd.engine import BatchedEngine
    calls, ticks = int(opts.get("calls", 512)), int(opts.get("ticks", 40))
    B = int(opts.get("games", 65536))
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    has_query, has_given = hasattr(lib, "orx_npc_options"), hasattr(lib, "orx_npc_step")
    ids = {"label": opts.get("label", "tree"), "build_id": _lib.build_id(),
           "moves_build_id": _lib.part_id("moves"), "path_build_id": _lib.part_id("path"),
           "npc_query_build_id": _lib.part_id("npc_query"), "games": B, "n_npcs": K}
    gen = torch.Generator().manual_seed(7)
    lines = []

    def emit(rec):
        rec = dict(ids, **rec)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def measure(fn):
        for _ in range(32):
            fn()
        torch.cuda.synchronize()
        blocks = [timed_block(torch, fn, calls) for _ in range(4)]
        return round(sorted(blocks)[1], 3), [round(v, 3) for v in blocks]

    # -- the queries on one resident state ------------------------------------
    cfg = EnvConfig(64, 64, n_npcs=K)
    eng = BatchedEngine(cfg, B, seed=3, device=dev)
    for _ in range(ticks):
        a = torch.randint(1, 6, (B, 2), generator=gen, dtype=torch.int8).to(dev)
        if has_given:
            tab = torch.randint(1, 6, (K, B), generator=gen, dtype=torch.int8).to(dev)
            eng.step(a, npc_moves=tab)
        else:
            eng.step(a)
    queries = {"moves": (lambda out: eng.moves(0, out=out)),
               "seek": (lambda out: eng.seek(0, out=out))}
    if has_query:
        queries.update(npc_options=lambda out: eng.npc_options(out=out),
                       npc_seek=lambda out: eng.npc_seek(out=out))
    nbytes = query_bytes(B, K)
    for name, fn in queries.items():
        out = fn(None)
        us, blocks = measure(lambda: fn(out))
        rec = {"what": "query", "name": name, "calls": calls, "us_per_call": us,
               "us_blocks": blocks}
        if name in nbytes:
            rec.update(bytes=nbytes[name], gbytes_per_s=round(nbytes[name] / us / 1e3, 1))
        emit(rec)
    if has_query:
        us, blocks = measure(eng.npc_options_kind)   # (fresh outputs: two allocations per call)
        emit({"what": "query", "name": "npc_options_kind", "calls": calls, "us_per_call": us,
              "us_blocks": blocks, "bytes": nbytes["npc_options_kind"],
              "gbytes_per_s": round(nbytes["npc_options_kind"] / us / 1e3, 1)})
    del eng
    torch.cuda.empty_cache()

    # -- the captured tick -----------------------------------------------------
    acts = torch.randint(1, 6, (B,), generator=gen, dtype=torch.int8).to(dev)
    modes = ["chase"] + (["given"] if has_given else []) + (["hunt"] if has_query else [])
    for mode in modes:
        env = VecEnv(EnvConfig(64, 64, n_npcs=K, npc_policy=2 if mode == "chase" else 0), B,
                     seed=3, opponent=1, check_actions=False, out_buffers=1)
        table = torch.randint(1, 6, (K, B), generator=gen, dtype=torch.int8).to(dev)

        def step():
            if mode == "hunt":
                table.copy_(env.npc_hunt_moves())
            env.step(acts) if mode == "chase" else env.step(acts, npc_moves=table)
        step()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                step()
        torch.cuda.current_stream(dev).wait_stream(s)
        us, blocks = measure(g.replay)
        emit({"what": "graph", "mode": mode, "calls": calls, "us_per_step": us,
              "us_blocks": blocks})
        del env, g
        torch.cuda.empty_cache()
    if "out" in opts:
        path = os.path.abspath(opts["out"])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
