"""Times orx_path_query (BatchedEngine.path) against the best a user could do
on the device without it -- a pure-torch composition of the same outputs
(index arithmetic and gathers from the field tensor, no host sync) -- and
orx_path_field against the host's ``stair_field`` for the same bank.

    python tools/bench_path.py [--games=65536,2097152] [--radii=0,5,15]
                               [--launches=200] [--out=profiles/path/bench_path.jsonl]

Protocol.  Query: two configurations, the closed form (C3: 64 x 64, 8 NPCs)
and a 16-layout 64 x 64 bank (``DungeonBank.random(64, 64, 16, seed=0)``, no
NPCs), each after 16 RandomBot ticks; radius 0 stands for "no window".  The
torch composition is first checked against ``path.query`` at a small batch;
then the kernel and the composition are timed alternately in one process, each
block between two HIP events: the kernel over --launches launches in four
blocks, the composition over fewer (it takes tens of milliseconds per call at
2^21 games).  One JSON line per setting: both times (the second-fastest of the
four blocks), and for a window the kernel's written bytes B * V^2 * 2 over its
time, as a fraction of the 6.0-6.2 TB/s a plain-store stream reaches on this
GPU.  Below 64 MB of output a launch is not bandwidth-bound and the line says
so instead of quoting a fraction.
Field: the device field of a bank (one launch, HIP events, the median of
seven) beside the wall-clock of ``stair_field`` on the host, for the 16-layout
64 x 64 bank, a 64 x 64 serpentine (1,953 breadth-first levels) and two
256 x 256 layouts (the LDS limit).
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PLAIN_STORE_TBS = (6.0, 6.2)   # plain stores, one dword per lane, 256 B per wave-instruction
LAUNCH_FLOOR_BYTES = 64 << 20  # below this much output a launch is not bandwidth-bound
WALL, FAR = 0xFFFF, 0xFFFE


def torch_path(eng, player=0, radius=None):
    """(dist, move[, window]) composed from torch ops: int32 index math, one
    gather from the field for a bank; with a radius the five centre cells come
    out of the window."""
    import torch
    cfg, dev = eng.cfg, eng.device
    W, H = int(cfg.width), int(cfg.height)
    p = player
    px, py = eng.p_x[p], eng.p_y[p]
    field = eng.stair_field

    def value(x, y):
        g = (slice(None),) + (None,) * (x.dim() - 1)
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        if field is None:
            border = (x == 0) | (x == W - 1) | (y == 0) | (y == H - 1)
            v = torch.where(border, WALL, (x - eng.st_x[p][g]).abs() + (y - eng.st_y[p][g]).abs())
        else:
            idx = (eng.p_layout[p].long()[g] * (W * H)
                   + (x.clamp(0, W - 1) * H + y.clamp(0, H - 1)).long())
            v = field.view(torch.int16).reshape(-1)[idx].to(torch.int32) & 0xFFFF
        return torch.where(inside, v, WALL)

    if radius is None:
        own = value(px, py)
        nbr = (value(px, py - 1), value(px + 1, py), value(px, py + 1), value(px - 1, py))
        window = None
    else:
        R = int(radius)
        off = torch.arange(2 * R + 1, device=dev, dtype=torch.int32) - R
        win = value(px[:, None, None] + off[None, None, :], py[:, None, None] + off[None, :, None])
        own = win[:, R, R]
        nbr = (win[:, R - 1, R], win[:, R, R + 1], win[:, R + 1, R], win[:, R, R - 1])
        window = win.to(torch.int16).view(torch.uint16)
    dist = torch.where(own == FAR, -1, own)
    move = torch.full_like(own, 5)
    for code in (4, 3, 2, 1):
        move = torch.where(nbr[code - 1] == own - 1, code, move)
    move = torch.where((own == 0) | (own >= FAR), 5, move).to(torch.int8)
    return (dist, move) if window is None else (dist, move, window)


def bench_cfgs():
    from optimax_rogue_amd import DungeonBank, EnvConfig
    bank = DungeonBank.random(64, 64, 16, seed=0)
    return {"closed_form": EnvConfig.c3(),
            "bank16x64x64": EnvConfig(width=64, height=64, n_npcs=0, layouts=bank.layouts)}


def check_baseline(torch, dev):
    """torch_path == path.query == the kernel on small batches."""
    import numpy as np
    from optimax_rogue_amd import DungeonBank, EnvConfig
    from optimax_rogue_amd.engine import BatchedEngine
    from optimax_rogue_amd.path import query
    bank = DungeonBank.random(12, 10, 4, seed=1, wall_p=0.3, n_stairs=2).layouts
    for cfg in (EnvConfig(width=10, height=8, n_npcs=4, max_ticks=30),
                EnvConfig(width=12, height=10, n_npcs=6, layouts=bank)):
        eng = BatchedEngine(cfg, 200, seed=9, device=dev)
        for _ in range(20):
            eng.step(eng.policy(1, 1))
        snap = eng.snapshot()
        for radius in (None, 1, 5, 15):
            for player in (0, 1):
                want = query(snap, cfg, player, radius, bank=eng.bank)
                got = torch_path(eng, player, radius)
                ker = eng.path(player=player, radius=radius)
                for w, g, k in zip(want, got, ker):
                    assert np.array_equal(g.cpu().numpy(), w), "torch composition != path.query"
                    assert np.array_equal(k.cpu().numpy(), w), "orx_path_query != path.query"


def timed_block(torch, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def bench_field(torch, dev):
    """The device field beside the host's, per bank."""
    import ctypes
    import numpy as np
    import path_cases as pc
    from optimax_rogue_amd import DungeonBank, _lib
    from optimax_rogue_amd.config import OrxCfg
    from optimax_rogue_amd.path import stair_field
    lib = _lib.load()
    banks = {"bank16x64x64": DungeonBank.random(64, 64, 16, seed=0).layouts,
             "serpentine64x64": pc.serpentine()[None],
             "two256x256": np.array(pc.banks()["256x256"])}
    lines = []
    for name, layouts in banks.items():
        L, W, H = layouts.shape
        t0 = time.perf_counter()
        want = stair_field(layouts)
        host_s = time.perf_counter() - t0
        cfg = OrxCfg(width=W, height=H, n_layouts=L)
        tiles = torch.from_numpy(np.array(layouts).reshape(L, W * H)).to(dev)
        field = torch.empty((L, W, H), dtype=torch.uint16, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        go = lambda: _lib.check("orx_path_field", lib.orx_path_field(
            ctypes.byref(cfg), ctypes.c_void_p(tiles.data_ptr()),
            ctypes.c_void_p(field.data_ptr()), stream))
        go()
        torch.cuda.synchronize()
        assert np.array_equal(field.cpu().numpy(), want), "orx_path_field != stair_field"
        ts = sorted(timed_block(torch, go, 1) for _ in range(7))
        rec = {"field": name, "layouts": L, "width": W, "height": H,
               "levels": int(want[want < FAR].max()) + 1,
               "kernel_us": round(ts[3] * 1e6, 1), "kernel_us_min_max": [round(ts[0] * 1e6, 1),
                                                                         round(ts[-1] * 1e6, 1)],
               "host_stair_field_ms": round(host_s * 1e3, 2),
               "speedup": round(host_s / ts[3], 1)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    return lines


def main():
    import torch
    from optimax_rogue_amd.engine import BatchedEngine
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    games = [int(v) for v in opts.get("games", "65536,2097152").split(",")]
    radii = [int(v) or None for v in opts.get("radii", "0,5,15").split(",")]
    launches = max(4, int(opts.get("launches", 200)))
    out_path = opts.get("out")
    dev = torch.device("cuda", 0)
    check_baseline(torch, dev)
    lines = bench_field(torch, dev)
    for B in games:
        for name, cfg in bench_cfgs().items():
            eng = BatchedEngine(cfg, B, seed=3, device=dev)
            eng.rollout(16, 1, 1)
            eng.path()                                   # (the bank's field: once, untimed)
            for radius in radii:
                V = 2 * radius + 1 if radius else 0
                nbytes = B * V * V * 2
                out = [torch.empty(B, dtype=torch.int32, device=dev),
                       torch.empty(B, dtype=torch.int8, device=dev)]
                if radius:
                    out.append(torch.empty((B, V, V), dtype=torch.uint16, device=dev))
                out = tuple(out)
                kernel = lambda: eng.path(radius=radius, out=out)
                base = lambda: torch_path(eng, 0, radius)
                n_base = max(4, min(launches, int(2e9 // max(nbytes, 1))))
                for fn in (kernel, base, kernel, base):   # warm-up
                    fn()
                torch.cuda.synchronize()
                tk, tb = [], []
                for _ in range(4):                        # alternated blocks
                    tk.append(timed_block(torch, kernel, launches // 4))
                    tb.append(timed_block(torch, base, max(1, n_base // 4)))
                k_s, b_s = sorted(tk)[1], sorted(tb)[1]
                rec = {"config": name, "games": B, "radius": radius, "window_bytes": nbytes,
                       "launches": launches // 4 * 4, "kernel_us": round(k_s * 1e6, 2),
                       "kernel_us_blocks": [round(t * 1e6, 2) for t in tk],
                       "torch_us": round(b_s * 1e6, 2), "torch_launches": max(1, n_base // 4) * 4,
                       "speedup": round(b_s / k_s, 1)}
                if nbytes < LAUNCH_FLOOR_BYTES:
                    rec["note"] = ("%.1f MB of window: not bandwidth-bound, no bandwidth "
                                   "fraction quoted" % (nbytes / 1e6))
                else:
                    tbs = nbytes / k_s / 1e12
                    rec["written_TBps"] = round(tbs, 3)
                    rec["fraction_of_plain_store"] = [round(tbs / PLAIN_STORE_TBS[1], 3),
                                                      round(tbs / PLAIN_STORE_TBS[0], 3)]
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                del out
                torch.cuda.empty_cache()
            del eng
            torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
