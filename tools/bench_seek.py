"""Times orx_path_seek (BatchedEngine.seek) against the best a user could do on
the device without it -- a pure-torch composition of the same outputs from the
pair table tensor (index arithmetic and gathers, no host sync) -- and the table
build (orx_path_rows) against the host's ``pair_field``.

    python tools/bench_seek.py [--games=65536,2097152] [--launches=200]
                               [--per-thread=8,16,32,64,128]
                               [--out=profiles/seek/bench_seek.jsonl]

Protocol.  Query: two configurations with 8 NPCs, the closed form (C3: 64 x
64) and a 16-layout 64 x 64 bank (``DungeonBank.random(64, 64, 16, seed=0)``:
a 512 MiB table), each after 16 RandomBot ticks.  The torch composition is
first checked against ``path.seek`` and the kernel at a small batch; then the
kernel and the composition are timed alternately in one process, each block
between two HIP events: the kernel over --launches launches in four blocks,
the composition over fewer.  One JSON line per setting: both times (the
second-fastest of the four blocks) and the kernel's written bytes (28 per
game) over its time; a launch that writes less than 64 MB is not
bandwidth-bound and the line says so instead of quoting a fraction of the
6.0-6.2 TB/s a plain-store stream reaches on this GPU.
Table: orx_path_rows over every source of the bank (one launch, HIP events,
the median of five), its written bytes over its time, and for each
--per-thread value the same launch with that many plane entries per thread
(ORX_ROWS_PER_THREAD); beside it the wall-clock of ``path.pair_field`` on the
host for the bank's first two layouts, scaled to the bank, and the device rows
of those two layouts checked equal to it.
"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAIN_STORE_TBS = (6.0, 6.2)   # plain stores, one dword per lane, 256 B per wave-instruction
LAUNCH_FLOOR_BYTES = 64 << 20  # below this much output a launch is not bandwidth-bound
WALL, FAR = 0xFFFF, 0xFFFE
ROW_BYTES = 4 * (4 + 1 + 2)    # a game's dist, move and target rows


def torch_seek(eng, player=0):
    """(dist, move, target) composed from torch ops: index math, gathers from
    the table (or the closed form), an argmin per column, four more gathers for
    the move."""
    import torch
    cfg, dev = eng.cfg, eng.device
    W, H, K, B = int(cfg.width), int(cfg.height), int(cfg.n_npcs), eng.B
    p, q = player, 1 - player
    px, py, depth = eng.p_x[p].long(), eng.p_y[p].long(), eng.p_depth[p]
    pairs = eng.pair_field
    if pairs is not None:
        L, WH = len(eng.bank), W * H
        flat = pairs.view(torch.int16).reshape(-1)
        lay = eng.p_layout[p].long().clamp(0, L - 1)
        tiles = eng.bank_tiles.reshape(-1)
    else:
        sx, sy = eng.st_x[p].long(), eng.st_y[p].long()
    inside = lambda x, y: (x >= 0) & (x < W) & (y >= 0) & (y < H)
    cellof = lambda x, y: x.clamp(0, W - 1) * H + y.clamp(0, H - 1)

    def between(x, y, tx, ty):
        if pairs is not None:
            v = flat[(lay * WH + cellof(tx, ty)) * WH + cellof(x, y)].long() & 0xFFFF
        else:
            inner = lambda u, v: (u >= 1) & (u <= W - 2) & (v >= 1) & (v <= H - 2)
            mid = lambda s, a, b: ((a < s) & (s < b)) | ((b < s) & (s < a))
            detour = ((x == tx) & (sx == x) & mid(sy, y, ty)) | ((y == ty) & (sy == y) & mid(sx, x, tx))
            v = torch.where(inner(x, y) & inner(tx, ty),
                            (x - tx).abs() + (y - ty).abs() + 2 * detour.long(), WALL)
        return torch.where(inside(x, y) & inside(tx, ty), v, WALL)

    def is_stair(x, y):
        if pairs is not None:
            return inside(x, y) & (tiles[lay * WH + cellof(x, y)] == 3)
        return (x == sx) & (y == sy) & (x >= 1) & (x <= W - 2) & (y >= 1) & (y <= H - 2)

    here = inside(px, py)
    npc_depth = int(cfg.p1_depth) if int(cfg.start_mode) == 2 else 0
    on_npc_depth = here & (depth == npc_depth)
    columns = [((here & (eng.p_depth[q] == depth))[None], eng.p_x[q].long()[None],
                eng.p_y[q].long()[None], torch.tensor([q], device=dev))]
    slots = torch.arange(K, device=dev)
    if K > 0:
        bits = eng.npc_alive.reshape(-1, B)
        alive = ((bits[slots // 32] >> (slots % 32)[:, None]) & 1) == 1
        pos = eng.npc_pos[:K].long() & 0xFFFF
        columns.append((alive & on_npc_depth, pos & 0xFF, pos >> 8, slots))
        if eng.item_mask is not None:
            on = ((eng.item_mask[0][None] >> slots[:, None]) & 1) == 1
            ipos = eng.item_pos[:K].long() & 0xFFFF
            columns.append((on & on_npc_depth, ipos & 0xFF, ipos >> 8, slots))
    dist = torch.full((B, 4), -2, dtype=torch.int32, device=dev)
    move = torch.full((B, 4), 5, dtype=torch.int8, device=dev)
    target = torch.full((B, 4), -1, dtype=torch.int16, device=dev)
    for col, (present, tx, ty, ids) in enumerate(columns):
        v = between(px, py, tx, ty)
        v = torch.where(present, v.clamp(max=FAR), WALL)
        own, best = v.min(dim=0)          # (ties: checked against path.seek before timing)
        best = (v == own[None]).int().argmax(dim=0)
        bx, by = tx.gather(0, best[None])[0], ty.gather(0, best[None])[0]
        has = own != WALL
        mv = torch.full_like(own, 5)
        for code, dx, dy in ((4, -1, 0), (3, 0, 1), (2, 1, 0), (1, 0, -1)):
            x, y = px + dx, py + dy
            near = torch.where(is_stair(x, y) & ~((x == bx) & (y == by)), WALL,
                               between(x, y, bx, by))
            mv = torch.where(near == own - 1, code, mv)
        mv = torch.where((own == 0) | (own >= FAR), 5, mv)
        dist[:, col] = torch.where(has, torch.where(own == FAR, -1, own), -2).to(torch.int32)
        move[:, col] = torch.where(has, mv, 5).to(torch.int8)
        target[:, col] = torch.where(has, ids[best], -1).to(torch.int16)
    return dist, move, target


def bench_cfgs():
    from optimax_rogue_amd import DungeonBank, EnvConfig
    bank = DungeonBank.random(64, 64, 16, seed=0)
    return {"closed_form": EnvConfig.c3(),
            "bank16x64x64": EnvConfig(width=64, height=64, n_npcs=8, layouts=bank.layouts)}


def check_baseline(torch, dev):
    """torch_seek == path.seek == the kernel on small batches."""
    import numpy as np
    from optimax_rogue_amd import DungeonBank, EnvConfig
    from optimax_rogue_amd.engine import BatchedEngine
    from optimax_rogue_amd.enums import EXT_RPG
    from optimax_rogue_amd.path import seek
    bank = DungeonBank.random(12, 10, 4, seed=1, wall_p=0.3, n_stairs=2).layouts
    for cfg in (EnvConfig(width=10, height=8, n_npcs=4, max_ticks=30),
                EnvConfig(width=6, height=6, n_npcs=6, flags=EXT_RPG, item_drop_pct=100),
                EnvConfig(width=12, height=10, n_npcs=6, layouts=bank)):
        eng = BatchedEngine(cfg, 200, seed=9, device=dev)
        for _ in range(20):
            eng.step(eng.policy(1, 1))
        snap = eng.snapshot()
        for player in (0, 1):
            want = seek(snap, cfg, player, bank=eng.bank)
            got, ker = torch_seek(eng, player), eng.seek(player=player)
            for w, g, k in zip(want, got, ker):
                assert np.array_equal(g.cpu().numpy(), w), "torch composition != path.seek"
                assert np.array_equal(k.cpu().numpy(), w), "orx_path_seek != path.seek"


def timed_block(torch, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def bench_table(torch, dev, per_thread):
    """The device table of the 16 x 64 x 64 bank beside the host's."""
    import numpy as np
    from optimax_rogue_amd import DungeonBank, _lib
    from optimax_rogue_amd.config import OrxCfg
    from optimax_rogue_amd.path import pair_field
    lib = _lib.load()
    layouts = DungeonBank.random(64, 64, 16, seed=0).layouts
    L, W, H = layouts.shape
    WH, host_layouts = W * H, 2
    t0 = time.perf_counter()
    want = pair_field(layouts[:host_layouts])
    host_s = (time.perf_counter() - t0) * L / host_layouts
    cfg = OrxCfg(width=W, height=H, n_layouts=L)
    tiles = torch.from_numpy(np.array(layouts).reshape(L, WH)).to(dev)
    cells = torch.arange(L * WH, dtype=torch.int32, device=dev)
    lay, cell = (cells // WH).contiguous(), (cells % WH).contiguous()
    rows = torch.empty((L, WH, WH), dtype=torch.uint16, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    go = lambda: _lib.check("orx_path_rows", lib.orx_path_rows(
        ctypes.byref(cfg), p(tiles), p(lay), p(cell), p(rows), L * WH, stream))
    go()
    torch.cuda.synchronize()
    assert np.array_equal(rows[:host_layouts].cpu().numpy(), want), "orx_path_rows != pair_field"
    nbytes = 2 * L * WH * WH
    lines = []
    for per in [None] + list(per_thread):
        if per is None:
            os.environ.pop("ORX_ROWS_PER_THREAD", None)
        else:
            os.environ["ORX_ROWS_PER_THREAD"] = str(per)
        go()
        ts = sorted(timed_block(torch, go, 1) for _ in range(5))
        rec = {"table": "bank16x64x64", "rows": L * WH, "table_bytes": nbytes,
               "entries_per_thread": per or "default", "kernel_ms": round(ts[2] * 1e3, 3),
               "kernel_ms_min_max": [round(ts[0] * 1e3, 3), round(ts[-1] * 1e3, 3)],
               "written_TBps": round(nbytes / ts[2] / 1e12, 3),
               "fraction_of_plain_store": [round(nbytes / ts[2] / 1e12 / PLAIN_STORE_TBS[1], 3),
                                           round(nbytes / ts[2] / 1e12 / PLAIN_STORE_TBS[0], 3)],
               "host_pair_field_s": round(host_s, 2),
               "host_note": "pair_field on %d of %d layouts, scaled" % (host_layouts, L),
               "speedup": round(host_s / ts[2], 1)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    os.environ.pop("ORX_ROWS_PER_THREAD", None)
    return lines


def main():
    import torch
    from optimax_rogue_amd.engine import BatchedEngine
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    games = [int(v) for v in opts.get("games", "65536,2097152").split(",")]
    per_thread = [int(v) for v in opts.get("per-thread", "8,16,32,64,128").split(",") if v]
    launches = max(4, int(opts.get("launches", 200)))
    out_path = opts.get("out")
    dev = torch.device("cuda", 0)
    check_baseline(torch, dev)
    lines = bench_table(torch, dev, per_thread)
    for B in games:
        for name, cfg in bench_cfgs().items():
            eng = BatchedEngine(cfg, B, seed=3, device=dev)
            eng.rollout(16, 1, 1)
            eng.seek()                                   # (the bank's table: once, untimed)
            out = (torch.empty((B, 4), dtype=torch.int32, device=dev),
                   torch.empty((B, 4), dtype=torch.int8, device=dev),
                   torch.empty((B, 4), dtype=torch.int16, device=dev))
            kernel = lambda: eng.seek(out=out)
            base = lambda: torch_seek(eng, 0)
            for g, w in zip(kernel(), base()):
                assert torch.equal(g, w), "torch composition != orx_path_seek"
            n_base = max(4, min(launches, (1 << 23) // B))
            for fn in (kernel, base, kernel, base):   # warm-up
                fn()
            torch.cuda.synchronize()
            tk, tb = [], []
            for _ in range(4):                        # alternated blocks
                tk.append(timed_block(torch, kernel, launches // 4))
                tb.append(timed_block(torch, base, max(1, n_base // 4)))
            k_s, b_s = sorted(tk)[1], sorted(tb)[1]
            nbytes = B * ROW_BYTES
            rec = {"config": name, "games": B, "written_bytes": nbytes,
                   "launches": launches // 4 * 4, "kernel_us": round(k_s * 1e6, 2),
                   "kernel_us_blocks": [round(t * 1e6, 2) for t in tk],
                   "torch_us": round(b_s * 1e6, 2), "torch_launches": max(1, n_base // 4) * 4,
                   "speedup": round(b_s / k_s, 1)}
            if nbytes < LAUNCH_FLOOR_BYTES:
                rec["note"] = ("%.1f MB written: not bandwidth-bound, no bandwidth fraction "
                               "quoted" % (nbytes / 1e6))
            else:
                tbs = nbytes / k_s / 1e12
                rec["written_TBps"] = round(tbs, 3)
                rec["fraction_of_plain_store"] = [round(tbs / PLAIN_STORE_TBS[1], 3),
                                                  round(tbs / PLAIN_STORE_TBS[0], 3)]
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del eng, out
            torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
