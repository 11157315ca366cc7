"""Times orx_view (BatchedEngine.view) against the best a user could do on the
device without it: a pure-torch composition of the same window (gathers and
scatters over the engine's tensors, no host sync).

    python tools/bench_view.py [--games=65536,2097152] [--radii=5,15]
                               [--launches=200] [--out=profiles/view/bench_view.jsonl]

Protocol: C3 (64 x 64, 8 NPCs) after 16 RandomBot ticks; per (games, radius,
health) the torch composition is first checked against render_view at a small
batch, then the kernel and the composition are timed alternately in one
process, each block between two HIP events: the kernel over --launches
launches in four blocks, the composition over fewer (it takes tens of
milliseconds per call at 2^21 games).  One JSON line per setting: both times, the kernel's written
bytes B * V^2 * (1 or 2) over its time and that as a fraction of the 6.0-6.2
TB/s a plain-store stream reaches on this GPU.  At 65,536 games and radius 5
the output is 7.9 MB: the launch floor dominates there and the line says so
instead of quoting a bandwidth fraction.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAIN_STORE_TBS = (6.0, 6.2)   # plain stores, one dword per lane, 256 B per wave-instruction
LAUNCH_FLOOR_BYTES = 64 << 20  # below this much output a launch is not bandwidth-bound


def torch_view(eng, radius, player=0, health=False):
    """The same window composed from torch ops (int32 index math, one gather
    for a bank's tiles, one scatter per occupant kind)."""
    import torch
    from optimax_rogue_amd.enums import EXT_ITEMS
    from optimax_rogue_amd.view import npc_depth
    cfg, dev = eng.cfg, eng.device
    B, K, W, H, R = eng.B, eng.K, int(cfg.width), int(cfg.height), int(radius)
    V = 2 * R + 1
    p, q = player, 1 - player
    px, py, d = eng.p_x[p], eng.p_y[p], eng.p_depth[p]
    off = torch.arange(V, device=dev, dtype=torch.int32) - R
    x = px[:, None, None] + off[None, None, :]
    y = py[:, None, None] + off[None, :, None]
    inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    if eng.bank is None:
        tile = 1 + ((x == 0) | (x == W - 1) | (y == 0) | (y == H - 1)).to(torch.int32)
        tile = torch.where((x == eng.st_x[p][:, None, None]) & (y == eng.st_y[p][:, None, None]),
                           3, tile)   # (int32: a scalar does not promote it)
    else:
        idx = (eng.p_layout[p].long()[:, None, None] * (W * H)
               + (x.clamp(0, W - 1) * H + y.clamp(0, H - 1)).long())
        tile = eng.bank_tiles.reshape(-1)[idx] & 3
    # one spare byte at the end takes the scatters of occupants out of sight
    cells = torch.zeros(B * V * V + 1, dtype=torch.uint8, device=dev)
    cells[:-1] = torch.where(inside, tile, 0).to(torch.uint8).reshape(-1)
    hp = torch.zeros_like(cells) if health else None
    base = torch.arange(B, device=dev, dtype=torch.int64) * (V * V)

    def mark(games, ex, ey, bits, hval=None):
        i, j = ex - px + R, ey - py + R
        ok = games & (i >= 0) & (i < V) & (j >= 0) & (j < V) & (ex < W) & (ey < H)
        idx = torch.where(ok, base + (j * V + i), B * V * V).reshape(-1)
        cells[idx] = cells[idx] | torch.as_tensor(bits, device=dev).to(torch.uint8).expand(
            ok.shape).reshape(-1)
        if hp is not None and hval is not None:
            hp[idx] = hval.clamp(0, 255).to(torch.uint8).expand(ok.shape).reshape(-1)

    on = d == npc_depth(cfg)
    ks = torch.arange(max(K, 1), device=dev, dtype=torch.int32)[:, None]
    if K and int(cfg.flags) & EXT_ITEMS and eng.item_mask is not None:
        pos = eng.item_pos[:K].to(torch.int32) & 0xFFFF
        lies = ((eng.item_mask[0][None, :] >> ks[:K]) & 1) == 1
        kind = (eng.item_mask[1][None, :] >> ks[:K]) & 1
        mark(on[None, :] & lies, pos & 0xFF, pos >> 8, 16 + 32 * kind)
    if K:
        pos = eng.npc_pos[:K].to(torch.int32) & 0xFFFF
        alive = eng.npc_alive.reshape(-1, B)
        live = ((alive[(ks[:K, 0] // 32).long()] >> (ks[:K] % 32)) & 1) == 1
        mark(on[None, :] & live, pos & 0xFF, pos >> 8, 8, eng.npc_health[:K].to(torch.int32))
    mark(eng.p_depth[q] == d, eng.p_x[q], eng.p_y[q], 4, eng.p_health[q])
    cells = cells[:-1].reshape(B, V, V)
    return (cells, hp[:-1].reshape(B, V, V)) if health else cells


def check_baseline(torch, dev):
    """torch_view == render_view on small batches (plain, bank, dense, items)."""
    import numpy as np
    from optimax_rogue_amd import DungeonBank, EnvConfig
    from optimax_rogue_amd.engine import BatchedEngine
    from optimax_rogue_amd.view import render_view
    bank = DungeonBank.random(12, 10, 4, seed=1, n_stairs=2).layouts
    for cfg in (EnvConfig(width=10, height=8, n_npcs=4, max_ticks=30),
                EnvConfig(width=12, height=10, n_npcs=6, layouts=bank),
                EnvConfig(width=20, height=20, n_npcs=40),
                EnvConfig(width=10, height=8, n_npcs=4, flags=60, item_drop_pct=100)):
        eng = BatchedEngine(cfg, 200, seed=9, device=dev)
        for _ in range(20):
            eng.step(eng.policy(1, 1))
        snap = eng.snapshot()
        for radius in (1, 5, 15):
            for player in (0, 1):
                want = render_view(snap, cfg, player, radius, bank=eng.bank, health=True)
                got = torch_view(eng, radius, player, health=True)
                ker = eng.view(radius, player=player, health=True)
                for w, g, k in zip(want, got, ker):
                    assert np.array_equal(g.cpu().numpy(), w), "torch composition != render_view"
                    assert np.array_equal(k.cpu().numpy(), w), "orx_view != render_view"


def timed_block(torch, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def main():
    import torch
    from optimax_rogue_amd import EnvConfig
    from optimax_rogue_amd.engine import BatchedEngine
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    games = [int(v) for v in opts.get("games", "65536,2097152").split(",")]
    radii = [int(v) for v in opts.get("radii", "5,15").split(",")]
    launches = max(4, int(opts.get("launches", 200)))
    out_path = opts.get("out")
    dev = torch.device("cuda", 0)
    check_baseline(torch, dev)
    lines = []
    for B in games:
        eng = BatchedEngine(EnvConfig.c3(), B, seed=3, device=dev)
        eng.rollout(16, 1, 1)
        for radius in radii:
            V = 2 * radius + 1
            for health in (False, True):
                nbytes = B * V * V * (2 if health else 1)
                outs = [torch.empty((B, V, V), dtype=torch.uint8, device=dev)
                        for _ in range(2 if health else 1)]
                out = tuple(outs) if health else outs[0]
                kernel = lambda: eng.view(radius, health=health, out=out)
                base = lambda: torch_view(eng, radius, 0, health)
                n_base = max(2, min(launches // 4, int(2e9 // nbytes)))
                for fn in (kernel, base, kernel, base):   # warm-up
                    fn()
                torch.cuda.synchronize()
                tk, tb = [], []
                for _ in range(4):                        # alternated blocks
                    tk.append(timed_block(torch, kernel, launches // 4))
                    tb.append(timed_block(torch, base, max(1, n_base // 4)))
                k_s, b_s = sorted(tk)[1], sorted(tb)[1]
                rec = {"games": B, "radius": radius, "health": health, "bytes": nbytes,
                       "launches": launches // 4 * 4, "kernel_us": round(k_s * 1e6, 2),
                       "kernel_us_blocks": [round(t * 1e6, 2) for t in tk],
                       "torch_us": round(b_s * 1e6, 2), "torch_launches": max(1, n_base // 4) * 4,
                       "speedup": round(b_s / k_s, 1)}
                if nbytes < LAUNCH_FLOOR_BYTES:
                    rec["note"] = ("launch floor: %.1f MB of output, not bandwidth-bound; no "
                                   "bandwidth fraction quoted" % (nbytes / 1e6))
                else:
                    tbs = nbytes / k_s / 1e12
                    rec["written_TBps"] = round(tbs, 3)
                    rec["fraction_of_plain_store"] = [round(tbs / PLAIN_STORE_TBS[1], 3),
                                                      round(tbs / PLAIN_STORE_TBS[0], 3)]
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                del outs, out
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
