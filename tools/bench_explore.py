"""Times orx_explore_update and orx_explore_seek (BatchedEngine.explore /
explore_seek) against the best a user could do on the device without them: a
pure-torch composition of the same rule -- a fog-of-war byte map [B, W, H], the
row words unpacked and scattered into it, and for the seek a masked min over
the gathered pair row -- with no host sync.

    python tools/bench_explore.py [--games=65536,2097152] [--radii=5,15]
                                  [--launches=40] [--out=profiles/explore/bench_explore.jsonl]

Protocol: orx_sight's shape (64 x 64, 8 NPCs, a bank of 8 connected layouts at
wall density 0.3).  The composition is first checked against explore.update /
explore.seek at a small batch over a run of ticks.  Then, per (games, radius),
the games play 16 RandomBot ticks with the map updated after each, and the
kernels and the composition are timed alternately in one process, each block
between two HIP events, in the state that follows: the update adds nothing new
(the steady state: a tick's gain is a few cells, and the kernel stores only
words that gain bits), with ``gained`` alone and with both planes rewritten in
place.  orx_sight (the row words) and orx_path_seek are timed beside them at
the same shape.  The composition's seek gathers B * W * H pair entries: it runs
in chunks of games.  One JSON line per setting; ``seek_whole_row_fraction`` is
games * (a pair row's W * H * 2 bytes) / time over the 8 TB/s peak: the share
of the peak the seek would run at if it streamed own's whole row, as its first
form did (the committed form reads only the targets' entries).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEEK_CHUNK = 32768         # games per chunk of the composition's seek
HBM_PEAK = 8.0e12          # bytes / s


def bank_config(n_npcs=8):
    from optimax_rogue_amd import DungeonBank, EnvConfig
    bank = DungeonBank.random(64, 64, 8, seed=3, wall_p=0.3, connected=True)
    return EnvConfig(width=64, height=64, n_npcs=n_npcs, layouts=bank.layouts)


class TorchMap:
    """The remembered map kept with torch ops: ``known`` uint8 [B, W, H] and
    ``key`` int32 [B, 4]."""

    def __init__(self, torch, eng):
        self.t, self.eng = torch, eng
        self.W, self.H = int(eng.cfg.width), int(eng.cfg.height)
        self.known = torch.zeros((eng.B, self.W, self.H), dtype=torch.uint8, device=eng.device)
        self.key = torch.full((eng.B, 4), -1, dtype=torch.int32, device=eng.device)

    def update(self, rows, radius, player=0):
        """rows: int32 [B, V] (orx_sight's words).  Returns gained."""
        t, e, W, H = self.t, self.eng, self.W, self.H
        B, V = rows.shape
        valid = (self.key[:, 3] >= 0) & (self.key[:, 0] == e.episode) \
            & (self.key[:, 1] == e.p_depth[player]) & (self.key[:, 2] <= e.tick)
        self.known *= valid.to(t.uint8)[:, None, None]
        off = t.arange(V, device=rows.device) - radius
        vis = ((rows[:, :, None] >> t.arange(V, device=rows.device, dtype=t.int32)) & 1).bool()
        x = e.p_x[player][:, None, None] + off[None, None, :]
        y = e.p_y[player][:, None, None] + off[None, :, None]
        seen = vis & (x >= 0) & (x < W) & (y >= 0) & (y < H)
        idx = (x.clamp(0, W - 1) * H + y.clamp(0, H - 1)).view(B, -1).to(t.int64)
        flat = self.known.view(B, -1)
        before = flat.sum(1, dtype=t.int32)
        flat.scatter_reduce_(1, idx, seen.view(B, -1).to(t.uint8), reduce="amax", include_self=True)
        after = flat.sum(1, dtype=t.int32)
        self.key = t.stack([e.episode, e.p_depth[player], e.tick, after], 1)
        return after - before

    def seek(self, pairs_i16, player=0):
        """(dist, move, target) int32 [B, 2], int32 [B, 2], int32 [B, 2] of the
        two columns, over chunks of games."""
        t, e, W, H = self.t, self.eng, self.W, self.H
        B, WH = e.B, W * H
        valid = (self.key[:, 3] >= 0) & (self.key[:, 0] == e.episode) \
            & (self.key[:, 1] == e.p_depth[player]) & (self.key[:, 2] <= e.tick)
        cell = t.arange(WH, device=e.device, dtype=t.int64)
        outs = []
        for b0 in range(0, B, SEEK_CHUNK):
            s = slice(b0, b0 + SEEK_CHUNK)
            lay = e.p_layout[player][s].to(t.int64)
            px, py = e.p_x[player][s].to(t.int64), e.p_y[player][s].to(t.int64)
            own = px * H + py
            k = self.known[s].bool()
            tiles = e.bank_tiles[lay].view(-1, W, H)
            un = ~k
            edge = t.zeros_like(k)
            edge[:, 1:, :] |= un[:, :-1, :]
            edge[:, :-1, :] |= un[:, 1:, :]
            edge[:, :, 1:] |= un[:, :, :-1]
            edge[:, :, :-1] |= un[:, :, 1:]
            row = pairs_i16[lay, own].to(t.int64) & 0xFFFF           # [n, WH]: own's row
            packed = (row.clamp(max=0xFFFE) << 16) | cell[None, :]
            none = 0xFFFFFFFF
            cols = []
            for mask in (k & (tiles == 1) & edge, k & (tiles == 3)):
                m = mask.view(-1, WH) & valid[s, None]
                cols.append(t.where(m, packed, none).min(1).values)
            best = t.stack(cols, 1)                                   # [n, 2]
            d, tc = best >> 16, (best & 0xFFFF).clamp(max=WH - 1)
            has, far = best != none, d == 0xFFFE
            dist = t.where(has, t.where(far, -1, d), -2)
            move = t.full_like(dist, 5)
            for code, dx, dy in ((4, -1, 0), (3, 0, 1), (2, 1, 0), (1, 0, -1)):
                nx, ny = (px + dx)[:, None], (py + dy)[:, None]
                inside = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
                nc = (nx.clamp(0, W - 1) * H + ny.clamp(0, H - 1)).expand(-1, 2)
                nd = pairs_i16[lay[:, None], tc, nc].to(t.int64) & 0xFFFF
                stair = (e.bank_tiles[lay[:, None], nc] == 3) & (nc != tc)
                ok = has & ~far & (d > 0) & inside & (nd == d - 1) & ~stair
                move = t.where(ok, code, move)
            outs.append((dist, move, t.where(has, tc, -1)))
        return tuple(t.cat([o[i] for o in outs]).to(t.int32) for i in range(3))


def as_i32(torch, rows):
    return rows.view(torch.int32)


def check_baseline(torch, dev):
    """The composition == explore.py == the kernels at a small batch, over ticks."""
    import numpy as np
    from optimax_rogue_amd import explore, sight
    from optimax_rogue_amd.engine import BatchedEngine
    cfg = bank_config()
    eng = BatchedEngine(cfg, 200, seed=9, device=dev)
    pairs = eng.pair_field.view(torch.int16)
    # (the host reference reads the bank's table: the device's, which the tests
    # hold equal to path.pair_field, spares a minute of breadth-first searches)
    eng.bank._pair_field = eng.pair_field.cpu().numpy()
    for radius in (5, 15):
        eng.explore_forget()
        tm = TorchMap(torch, eng)
        memory, key = explore.empty(200, 64, 64)
        for tick in range(12):
            eng.rollout(2, 2, 1)
            snap = eng.snapshot()
            rows = eng.sight(radius)
            want_g = explore.update(memory, key, snap, cfg, 0, radius,
                                    sight.pack_rows(sight.visible(snap, cfg, 0, radius, bank=eng.bank)))
            assert np.array_equal(tm.update(as_i32(torch, rows), radius).cpu().numpy(), want_g)
            assert np.array_equal(eng.explore(radius).cpu().numpy(), want_g), "kernel != explore.update"
            known = explore.unpack(memory, 64)
            assert np.array_equal(tm.known.bool().cpu().numpy(), known), "composition != explore.update"
            assert np.array_equal(tm.key.cpu().numpy(), key)
            want = explore.seek(memory, key, snap, cfg, 0, bank=eng.bank)
            got = eng.explore_seek()
            base = tm.seek(pairs)
            for i in range(3):
                assert np.array_equal(got[i].cpu().numpy(), want[i]), "kernel != explore.seek"
                assert np.array_equal(base[i].cpu().numpy(), want[i][:, :2]), \
                    "composition != explore.seek"
        assert (want[0][:, 0] > 0).any() and key[:, 3].min() > 0


def timed_block(torch, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def alternate(torch, kernel, base, n_kernel, n_base):
    for fn in (kernel, base, kernel, base):   # warm-up
        fn()
    torch.cuda.synchronize()
    tk, tb = [], []
    for _ in range(4):
        tk.append(timed_block(torch, kernel, max(1, n_kernel // 4)))
        tb.append(timed_block(torch, base, max(1, n_base // 4)))
    return sorted(tk)[1], sorted(tb)[1], tk


def main():
    import torch
    from optimax_rogue_amd.engine import BatchedEngine, _ptr
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    games = [int(v) for v in opts.get("games", "65536,2097152").split(",")]
    radii = [int(v) for v in opts.get("radii", "5,15").split(",")]
    launches = max(4, int(opts.get("launches", 40)))
    out_path = opts.get("out")
    dev = torch.device("cuda", 0)
    check_baseline(torch, dev)
    cfg = bank_config()
    lines = []
    for B in games:
        for radius in radii:
            eng = BatchedEngine(cfg, B, seed=3, device=dev)
            pairs = eng.pair_field.view(torch.int16)
            V = 2 * radius + 1
            tm = TorchMap(torch, eng)
            for _ in range(16):
                eng.rollout(1, 1, 1)
                rows = eng.sight(radius)
                eng.explore(radius)
                tm.update(as_i32(torch, rows), radius)
            rows32 = as_i32(torch, rows)
            memory, key = eng.explore_map(0)
            gained = torch.empty(B, dtype=torch.int32, device=dev)
            cells, hp = eng.view(radius, health=True)
            n_base = max(4, min(launches, (1 << 24) // B * 4))
            rec = {"games": B, "radius": radius, "launches": launches // 4 * 4,
                   "known_mean": round(float(key[:, 3].float().mean()), 1)}

            def update(c, h):
                return lambda: eng._call("orx_explore_update", 0, radius, _ptr(rows), _ptr(memory),
                                         _ptr(key), _ptr(gained), _ptr(c), _ptr(h), B, eng._stream())
            k, b, blocks = alternate(torch, update(None, None), lambda: tm.update(rows32, radius),
                                     launches, n_base)
            rec.update(update_us=round(k * 1e6, 2), update_us_blocks=[round(t * 1e6, 2) for t in blocks],
                       torch_update_us=round(b * 1e6, 2), update_speedup=round(b / k, 1))
            k, _, _ = alternate(torch, update(cells, hp), lambda: None, launches, 4)
            rec.update(update_planes_us=round(k * 1e6, 2))
            outs = eng.explore_seek()
            k, b, blocks = alternate(torch, lambda: eng.explore_seek(out=outs), lambda: tm.seek(pairs),
                                     launches, max(4, n_base // 4))
            rec.update(seek_us=round(k * 1e6, 2), seek_us_blocks=[round(t * 1e6, 2) for t in blocks],
                       torch_seek_us=round(b * 1e6, 2), seek_speedup=round(b / k, 1),
                       seek_pair_row_bytes=64 * 64 * 2,
                       seek_whole_row_fraction=round(B * 64 * 64 * 2 / k / HBM_PEAK, 3))
            srows = torch.empty((B, V), dtype=torch.uint32, device=dev)
            pouts = eng.seek()
            k, b, _ = alternate(torch, lambda: eng.sight(radius, out=srows),
                                lambda: eng.seek(out=pouts), launches, launches)
            rec.update(orx_sight_us=round(k * 1e6, 2), orx_path_seek_us=round(b * 1e6, 2))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del eng, tm, pairs, rows, rows32, cells, hp, srows, outs, pouts, memory, key, gained
            torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
