"""Times orx_route (BatchedEngine.explore_route) beside the unchanged
orx_explore_seek (explore_seek), by tools/bench_explore.py's protocol.

    python tools/bench_route.py [--games=65536,2097152] [--launches=40]
                                [--out=profiles/route/bench_route.jsonl]

Shape: orx_explore's -- 64 x 64, 8 NPCs, a bank of 8 connected
layouts at wall density 0.3, radius 5.  Two states per batch: after 16 RandomBot
ticks with the map updated after each (small maps, short walks), and after 256
more ticks in which player 1 follows ``explore_route_moves`` (large maps, long
walks: where a search costs most).  The kernel is first checked equal to
``route.route`` at a small batch in both kinds of state.  Then orx_route (with
the goal column -- each game's goal is the cell its player stood on eight ticks
earlier -- and without) and orx_explore_seek alternate in one process, each
block between two HIP events, the median of four blocks.  ``route_planes``'
one-off launch is timed once per engine.  One JSON line per (games, state).
Nothing here has a threshold: the numbers are DESIGN 7.11's.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RADIUS = 5
LAG = 8                    # the goal: where the player stood LAG ticks ago


def bank_config(n_npcs=8):
    from optimax_rogue_amd import DungeonBank, EnvConfig
    bank = DungeonBank.random(64, 64, 8, seed=3, wall_p=0.3, connected=True)
    return EnvConfig(width=64, height=64, n_npcs=n_npcs, layouts=bank.layouts)


class Run:
    """An engine whose player 1 keeps its map, and the ring of its last cells."""

    def __init__(self, torch, cfg, B, dev):
        from optimax_rogue_amd.engine import BatchedEngine
        self.t, self.eng = torch, BatchedEngine(cfg, B, seed=3, device=dev)
        self.H = int(cfg.height)
        self.ring = []
        self.eng.explore(RADIUS)
        self._push()

    def _push(self):
        e = self.eng
        self.ring = (self.ring + [e.p_x[0] * self.H + e.p_y[0]])[-(LAG + 1):]

    def tick(self, router: bool):
        e = self.eng
        a = e.policy(1, 1)
        if router:
            a[:, 0] = e.explore_route_moves()
        e.step(a)
        e.explore(RADIUS)
        self._push()

    def goal(self):
        return self.ring[0].to(self.t.int32).contiguous()


def check_kernel(torch, dev):
    """orx_route == route.route at a small batch, in both kinds of state."""
    import numpy as np
    from optimax_rogue_amd import route
    cfg = bank_config()
    run = Run(torch, cfg, 200, dev)
    for tick in range(16 + 48):
        run.tick(router=tick >= 16)
        if tick % 8 == 7:
            eng = run.eng
            memory, key = eng.explore_map(0)
            goal = run.goal()
            want = route.route(memory.view(torch.int32).cpu().numpy().view(np.uint32),
                               key.cpu().numpy(), eng.snapshot(), cfg, 0, goal=goal.cpu().numpy(),
                               bank=eng.bank)
            got = eng.explore_route(goal=goal)
            for g, w in zip(got, want):
                assert np.array_equal(g.cpu().numpy(), w), "kernel != route.route"
    assert (want[0][:, :3] > 0).any(axis=0).all()


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
    import torch
    from optimax_rogue_amd.engine import _ptr
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    games = [int(v) for v in opts.get("games", "65536,2097152").split(",")]
    launches = max(4, int(opts.get("launches", 40)))
    router_ticks = int(opts.get("router_ticks", 256))
    out_path = opts.get("out")
    dev = torch.device("cuda", 0)
    check_kernel(torch, dev)
    cfg = bank_config()
    us = lambda s: round(s * 1e6, 2)
    lines = []
    for B in games:
        run = Run(torch, cfg, B, dev)
        eng = run.eng
        torch.cuda.synchronize()
        planes_s = timed_block(torch, lambda: eng.route_planes, 1)     # (the one launch that packs them)
        eng.pair_field                                               # (the seek's table, before timing)
        n = launches if B <= (1 << 17) else max(8, launches // 4)
        for state, ticks, router in (("16 RandomBot ticks", 16, False),
                                     (f"{router_ticks} router ticks more", router_ticks, True)):
            for _ in range(ticks):
                run.tick(router)
            memory, key = eng.explore_map(0)
            goal = run.goal()
            r_outs, s_outs = eng.explore_route(goal=goal), eng.explore_seek()
            d = r_outs[0]
            rec = {"games": B, "state": state, "radius": RADIUS, "launches": n // 4 * 4,
                   "known_mean": round(float(key[:, 3].float().mean()), 1),
                   "frontier_dist_mean": round(float(d[:, 0][d[:, 0] > 0].float().mean()), 2),
                   "stairs_dist_mean": round(float(d[:, 1][d[:, 1] > 0].float().mean()), 2),
                   "goal_dist_mean": round(float(d[:, 2][d[:, 2] > 0].float().mean()), 2),
                   "dist_max": int(d.max()),
                   "stairs_known_share": round(float((d[:, 1] != -2).float().mean()), 3),
                   "stairs_longer_than_seek_share": round(float(
                       ((s_outs[0][:, 1] >= 0) & ((d[:, 1] > s_outs[0][:, 1]) | (d[:, 1] == -1)))
                       .float().mean()), 4),
                   "route_planes_us": us(planes_s)}

            def route(g, dist=r_outs[0], move=r_outs[1], target=r_outs[2]):
                return lambda: eng._call("orx_route", _ptr(eng.route_planes), 0, _ptr(memory), _ptr(key),
                                         _ptr(g), _ptr(dist), _ptr(move), _ptr(target), B, eng._stream())
            (with_goal, no_goal, move_only, seek), blocks = alternate(
                torch, [route(goal), route(None), route(None, dist=None, target=None),
                        lambda: eng.explore_seek(out=s_outs)], n)
            rec.update(route_goal_us=us(with_goal), route_us=us(no_goal), route_move_only_us=us(move_only),
                       seek_us=us(seek), route_over_seek=round(no_goal / seek, 2),
                       route_us_blocks=[us(t) for t in blocks[1]], seek_us_blocks=[us(t) for t in blocks[3]])
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del run, eng, memory, key, goal, r_outs, s_outs, d
        torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
