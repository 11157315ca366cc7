"""Times orx_path_ticks (BatchedEngine.path_ticks) beside orx_route (the same
search shape) and orx_path_query (the table lookup it replaces), by
tools/bench_route.py's protocol.

    python tools/bench_ticks.py [--games=65536,2097152] [--launches=40]
                                [--lib=/path/to/another/liborx.so]
                                [--out=profiles/ticks/bench_ticks.jsonl]

Shapes: DESIGN 7.11's -- 64 x 64, 8 NPCs, a bank of 8 connected layouts at wall
density 0.3 -- and C3's open room (64 x 64, 8 NPCs, no bank), after 16
RandomBot ticks, player 1 keeping its map at radius 5 for orx_route.  The
kernel is first checked equal to ``path.ticks`` at a small batch on both
shapes.  Then orx_path_ticks without and with a radius-5 window, orx_route and
orx_path_query alternate in one process, each block between two HIP events,
the median of four blocks.  The search's length comes from the reference's
answer: the mean of ``ticks`` is the mean number of steps of a search without a
window, and a game jumped when its answer passed a release, ``ticks > dist``
with the fight taken.  ``--lib`` times the calls an older library has (the
parent's: orx_route and orx_path_query) with this tree's Python, to show them
unchanged.  One JSON line per (shape, games).  Nothing here has a threshold:
the numbers are DESIGN 7.14's.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RADIUS = 5


def configs():
    from optimax_rogue_amd import DungeonBank, EnvConfig
    bank = DungeonBank.random(64, 64, 8, seed=3, wall_p=0.3, connected=True)
    return {"bank": EnvConfig(width=64, height=64, n_npcs=8, layouts=bank.layouts),
            "room": EnvConfig(width=64, height=64, n_npcs=8)}


def engine_at(torch, cfg, B, dev):
    from optimax_rogue_amd.engine import BatchedEngine
    eng = BatchedEngine(cfg, B, seed=3, device=dev)
    eng.explore(RADIUS)
    for _ in range(16):
        eng.step(eng.policy(1, 1))
        eng.explore(RADIUS)
    return eng


def check_kernel(torch, dev):
    import numpy as np
    from optimax_rogue_amd import path
    for cfg in configs().values():
        eng = engine_at(torch, cfg, 200, dev)
        snap = eng.snapshot()
        for p, radius in ((0, None), (0, RADIUS), (1, RADIUS)):
            want = path.ticks(snap, cfg, p, radius, bank=eng.bank)
            got = eng.path_ticks(player=p, radius=radius)
            for g, w in zip(got, want):
                assert np.array_equal(g.cpu().numpy(), w), "kernel != path.ticks"


def timed_block(torch, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def alternate(torch, fns, n):
    """The median-of-four block time of each of ``fns``, the blocks alternating."""
    for fn in fns + fns:   # warm-up
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(4):
        for ts, fn in zip(times, fns):
            ts.append(timed_block(torch, fn, max(1, n // 4)))
    return [sorted(ts)[1] for ts in times], times


def main():
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    if "lib" in opts:     # (before the package loads its own)
        from optimax_rogue_amd import _lib
        _lib.LIB_PATH = os.path.abspath(opts["lib"])
    import torch
    games = [int(v) for v in opts.get("games", "65536,2097152").split(",")]
    launches = max(4, int(opts.get("launches", 40)))
    out_path = opts.get("out")
    dev = torch.device("cuda", 0)
    has_ticks = "lib" not in opts
    if has_ticks:
        check_kernel(torch, dev)
    us = lambda s: round(s * 1e6, 2)
    lines = []
    for shape, cfg in configs().items():
        for B in games:
            eng = engine_at(torch, cfg, B, dev)
            n = launches if B <= (1 << 17) else max(8, launches // 4)
            r_outs, q_outs = eng.explore_route(), eng.path()
            rec = {"shape": shape, "games": B, "radius": RADIUS, "launches": n // 4 * 4,
                   "lib": opts.get("lib", "tree")}
            fns = [lambda: eng.explore_route(out=r_outs), lambda: eng.path(out=q_outs)]
            names = ["route_us", "path_query_us"]
            if has_ticks:
                t_outs, w_outs = eng.path_ticks(), eng.path_ticks(radius=RADIUS)
                t, d = t_outs[0], q_outs[0]
                fought = (t > d) & (d >= 0)
                rec.update(ticks_mean=round(float(t[t > 0].float().mean()), 2), ticks_max=int(t.max()),
                           dist_mean=round(float(d[d > 0].float().mean()), 2),
                           above_dist_share=round(float(fought.float().mean()), 4),
                           unreachable_share=round(float(((t < 0) & (d >= 0)).float().mean()), 4),
                           window_steps_max=int(w_outs[2].view(torch.int16).to(torch.int32)
                                                .clamp(min=0).max()))
                fns += [lambda: eng.path_ticks(out=t_outs),
                        lambda: eng.path_ticks(radius=RADIUS, out=w_outs), lambda: eng.rush_moves()]
                names += ["ticks_us", "ticks_window_us", "rush_moves_us"]
            meds, blocks = alternate(torch, fns, n)
            rec.update({k: us(v) for k, v in zip(names, meds)})
            rec.update({k + "_blocks": [us(t) for t in b] for k, b in zip(names, blocks)})
            if has_ticks:
                rec["ticks_over_route"] = round(meds[2] / meds[0], 2)
                rec["ns_per_game_step"] = round(meds[2] * 1e9 / B / max(rec["ticks_mean"], 1), 3)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del eng
            torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
