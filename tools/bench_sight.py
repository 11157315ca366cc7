"""Times orx_sight (BatchedEngine.sight, and the in-place masking seen_view
adds to view) against the best a user could do on the device without it: a
pure-torch composition of the same rule over orx_view's cells -- precomputed
index tables of every line's intermediate cells and of the neighbours toward
the viewer, two gathers, no host sync.

    python tools/bench_sight.py [--games=65536,2097152] [--radii=5,15]
                                [--launches=100] [--out=profiles/sight/bench_sight.jsonl]

Protocol: C3's shape (64 x 64, 8 NPCs) on a bank of 8 connected layouts at wall
density 0.3, after 16 RandomBot ticks.  The composition is first checked
against sight.visible at a small batch; then, per (games, radius) and for the
two outputs -- the row words alone, and the cells masked in place -- the kernel
and the composition are timed alternately in one process, each block between
two HIP events.  The cells are orx_view's output, written before the timed
blocks (a masked plane masks to itself, so every launch does the same work);
orx_view's own time at the same shape is measured beside it.  The composition
gathers B * V^2 * 2 * (R - 1) bytes: it runs in chunks of games that keep that
under 2 GiB.  One JSON line per setting.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GATHER_BYTES = 2 << 30     # the composition's largest intermediate


def tables(torch, dev, radius):
    from optimax_rogue_amd.sight import _tables
    lines, nbrs = _tables(radius)
    return (torch.from_numpy(lines).to(dev), torch.from_numpy(nbrs).to(dev),
            torch.arange(2 * radius + 1, device=dev, dtype=torch.int32))


def torch_sight(torch, cells, tabs, want_rows):
    """The rule composed from torch ops over windows of view codes: the row
    words (int32 [B, V]) or the masked cells (a new tensor)."""
    lines, nbrs, bits = tabs
    B, V = cells.shape[0], cells.shape[1]
    VV = V * V
    chunk = max(1, GATHER_BYTES // (VV * lines.shape[1] * lines.shape[2]))
    vis = torch.empty((B, VV), dtype=torch.bool, device=cells.device)
    for b0 in range(0, B, chunk):
        tile = cells[b0:b0 + chunk].reshape(-1, VV) & 3
        n = tile.shape[0]
        pad = torch.zeros((n, 1), dtype=torch.bool, device=cells.device)
        inside, opaque = tile != 0, tile == 2
        blocked = torch.cat([opaque, pad], 1)[:, lines.reshape(-1)].view(n, VV, 2, -1).any(3)
        clear = inside & ~blocked.all(2)
        floor = torch.cat([clear & ~opaque, pad], 1)
        vis[b0:b0 + chunk] = clear | (opaque & floor[:, nbrs.reshape(-1)].view(n, VV, 3).any(2))
    vis = vis.view(B, V, V)
    if want_rows:
        return (vis.to(torch.int32) << bits).sum(2, dtype=torch.int32)
    return torch.where(vis, cells | 64, 0).to(torch.uint8)


def bank_config(n_npcs=8):
    from optimax_rogue_amd import DungeonBank, EnvConfig
    bank = DungeonBank.random(64, 64, 8, seed=3, wall_p=0.3, connected=True)
    return EnvConfig(width=64, height=64, n_npcs=n_npcs, layouts=bank.layouts)


def check_baseline(torch, dev):
    """torch_sight == sight.visible == orx_sight at a small batch."""
    import numpy as np
    from optimax_rogue_amd import sight
    from optimax_rogue_amd.engine import BatchedEngine
    cfg = bank_config()
    eng = BatchedEngine(cfg, 200, seed=9, device=dev)
    eng.rollout(16, 1, 1)
    snap = eng.snapshot()
    for radius in (1, 5, 15):
        tabs = tables(torch, dev, radius)
        for player in (0, 1):
            vis = sight.visible(snap, cfg, player, radius, bank=eng.bank)
            cells = eng.view(radius, player=player)
            want = sight.apply(cells.cpu().numpy(), vis)
            rows = torch_sight(torch, cells, tabs, True).cpu().numpy().view(np.uint32)
            assert np.array_equal(rows, sight.pack_rows(vis)), "torch composition != visible"
            assert np.array_equal(torch_sight(torch, cells, tabs, False).cpu().numpy(), want)
            assert np.array_equal(eng.sight(radius, player=player).cpu().numpy(),
                                  sight.pack_rows(vis)), "orx_sight != visible"
            assert np.array_equal(eng.seen_view(radius, player=player).cpu().numpy(), want)
        assert vis.any() and (radius == 1 or not vis.all())


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
    from optimax_rogue_amd.engine import BatchedEngine, _ptr
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    games = [int(v) for v in opts.get("games", "65536,2097152").split(",")]
    radii = [int(v) for v in opts.get("radii", "5,15").split(",")]
    launches = max(4, int(opts.get("launches", 100)))
    out_path = opts.get("out")
    dev = torch.device("cuda", 0)
    check_baseline(torch, dev)
    cfg = bank_config()
    lines = []
    for B in games:
        eng = BatchedEngine(cfg, B, seed=3, device=dev)
        eng.rollout(16, 1, 1)
        for radius in radii:
            V = 2 * radius + 1
            tabs = tables(torch, dev, radius)
            cells = eng.view(radius)
            rows = torch.empty((B, V), dtype=torch.uint32, device=dev)
            masked = cells.clone()
            sight_cells = lambda: eng._call("orx_sight", 0, radius, None, _ptr(masked), None, B,
                                            eng._stream())
            view = lambda: eng.view(radius, out=masked)
            view()
            sight_cells()                 # (masked from here on: masking it again is the same work)
            t_view = sorted(timed_block(torch, view, launches // 4) for _ in range(4))[1]
            view()
            sight_cells()
            n_base = max(4, min(launches, int(4e9 // (B * V * V * 2 * max(radius - 1, 1)))))
            for mode, kernel, base in (
                    ("rows", lambda: eng.sight(radius, out=rows),
                     lambda: torch_sight(torch, cells, tabs, True)),
                    ("cells", sight_cells, lambda: torch_sight(torch, cells, tabs, False))):
                for fn in (kernel, base, kernel, base):   # warm-up
                    fn()
                torch.cuda.synchronize()
                tk, tb = [], []
                for _ in range(4):                        # alternated blocks
                    tk.append(timed_block(torch, kernel, launches // 4))
                    tb.append(timed_block(torch, base, max(1, n_base // 4)))
                k_s, b_s = sorted(tk)[1], sorted(tb)[1]
                rec = {"games": B, "radius": radius, "output": mode,
                       "launches": launches // 4 * 4, "kernel_us": round(k_s * 1e6, 2),
                       "kernel_us_blocks": [round(t * 1e6, 2) for t in tk],
                       "torch_us": round(b_s * 1e6, 2), "torch_launches": max(1, n_base // 4) * 4,
                       "speedup": round(b_s / k_s, 1), "orx_view_us": round(t_view * 1e6, 2),
                       "kernel_over_view": round(k_s / t_view, 2)}
                print(json.dumps(rec), flush=True)
                lines.append(rec)
            del cells, rows, masked
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
