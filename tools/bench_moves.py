"""Times orx_moves (BatchedEngine.moves_kind / moves) against what a user
would write without it: a pure-torch composition of the same ``kind`` from the
engine's tensors (index arithmetic, broadcasts and gathers, no host sync).

    python tools/bench_moves.py [--games=65536,2097152] [--launches=200]
                                [--out=profiles/moves/bench_moves.jsonl]

Protocol.  Three configurations, each after 16 RandomBot ticks: C3 (the closed
form, 64 x 64, 8 NPCs), a 16-layout 64 x 64 bank with 8 NPCs
(``DungeonBank.random(64, 64, 16, seed=0)``) and dense NPCs (64 x 64, K = 40:
the occupancy grid).  The composition is first checked equal to
``moves.outcomes`` and to the kernel at a small batch and, at the timed batch,
equal to the kernel's ``kind``.  Then three things are timed alternately in one
process, each block between two HIP events: the kernel writing ``kind`` alone,
the kernel writing all three outputs (both into preallocated buffers through a
prebound ctypes call, so the host pays one call per launch), and the
composition.  One JSON line per setting: the times (the second-fastest of four
blocks), and the kernel's bytes -- what the algorithm has to move, computed
from the shapes by ``kernel_bytes`` below -- over its time, beside the
6.0-6.2 TB/s a plain-store stream reaches on this GPU.  A block of launches
between two events measures the device only while the queue stays full: at
65,536 games a launch is a few microseconds of device work, and the figure is
the launch rate the host and the command processor sustain, which the line
says (``bound``).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PLAIN_STORE_TBS = (6.0, 6.2)   # plain stores, one dword per lane, 256 B per wave-instruction
LAUNCH_FLOOR_BYTES = 64 << 20  # below this much traffic a launch is not bandwidth-bound


def kernel_bytes(cfg, n_games, full):
    """Bytes one orx_moves launch has to move: per game the eight player words
    it reads (x, y, depth, health of both), the staircase pair or the layout
    index, with up to 16 NPCs every slot's position and health and the alive
    word, above that four grid bytes (each its own 32-byte sector at best: the
    cells are a column apart), and the row(s) it writes.  Bank tiles are shared
    by all games (L2) and not counted."""
    K = int(cfg.n_npcs)
    per = 8 * 4 + (2 if cfg.layouts is not None else 8)
    if 0 < K <= 16:
        per += 3 * K + 4
    elif K > 16:
        per += 4 * 32
    per += 8 + (32 if full else 0)
    return per * n_games


def torch_kind(eng, player=0):
    """``kind`` uint8 [B, 8] composed from torch ops on the engine's tensors
    (configurations without the character mechanics)."""
    import torch
    cfg, dev = eng.cfg, eng.device
    W, H, K, B = int(cfg.width), int(cfg.height), int(cfg.n_npcs), eng.B
    p, q = player, 1 - player
    x, y, d = eng.p_x[p], eng.p_y[p], eng.p_depth[p]
    dxy = torch.tensor([[0, 1, 0, -1], [-1, 0, 1, 0]], dtype=torch.int32, device=dev)
    tx, ty = x[:, None] + dxy[0][None], y[:, None] + dxy[1][None]          # [B, 4]
    inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    cell = (tx.clamp(0, W - 1) * H + ty.clamp(0, H - 1)).long()
    if eng.bank is None:
        wall = (tx == 0) | (tx == W - 1) | (ty == 0) | (ty == H - 1)
        stair = ~wall & (tx == eng.st_x[p][:, None]) & (ty == eng.st_y[p][:, None])
    else:
        tile = eng.bank_tiles.reshape(-1)[eng.p_layout[p].long()[:, None] * (W * H) + cell]
        wall, stair = tile == 2, tile == 3
    blocked = ~inside | wall
    at_player = ~blocked & (eng.p_depth[q] == d)[:, None] & (tx == eng.p_x[q][:, None]) \
        & (ty == eng.p_y[q][:, None])
    atk = max(int(cfg.player_damage) - int(cfg.player_armor), 0)
    lethal_p = (eng.p_health[q] > 0) & (eng.p_health[q] <= atk)
    start_sep = int(cfg.start_mode) == 2
    on_depth = (d == (int(cfg.p1_depth) if start_sep else 0))[:, None]
    games = torch.arange(B, device=dev)
    if K == 0:
        at_npc = torch.zeros_like(blocked)
        nhp = torch.zeros_like(tx)
    elif eng.npc_grid is None:
        pos = eng.npc_pos[:K].to(torch.int32) & 0xFFFF                          # [K, B]
        alive = ((eng.npc_alive[None, :] >> torch.arange(K, device=dev)[:, None]) & 1) != 0
        key = tx | (ty << 8)
        match = alive[:, :, None] & (pos[:, :, None] == key[None]) & inside[None]   # [K, B, 4]
        at_npc = match.any(0) & on_depth
        slot = match.to(torch.uint8).argmax(0).long()                           # the first hit
        nhp = eng.npc_health[:K][slot, games[:, None]].to(torch.int32)
    else:
        g = eng.npc_grid.reshape(-1)[games[:, None] * (W * H) + cell].to(torch.int32)
        slot = (g - 1).clamp(min=0).long()
        rows = eng.npc_alive.reshape(-1, B)
        bit = (rows[slot >> 5, games[:, None]] >> (slot & 31).to(torch.int32)) & 1
        at_npc = inside & (g > 0) & (bit != 0) & on_depth
        nhp = eng.npc_health[:K][slot, games[:, None]].to(torch.int32)
    at_npc = at_npc & ~blocked & ~at_player
    lethal_n = (nhp > 0) & (nhp <= atk)
    k4 = torch.where(blocked, 2,
                     torch.where(at_player, 6 + 8 * lethal_p[:, None].to(torch.int32),
                                 torch.where(at_npc, 5 + 8 * lethal_n.to(torch.int32),
                                             torch.where(stair, 4, 3))))
    kind = torch.zeros((B, 8), dtype=torch.uint8, device=dev)
    kind[:, 1:5] = k4.to(torch.uint8)
    kind[:, 5] = 1
    return kind


def bench_cfgs():
    from optimax_rogue_amd import DungeonBank, EnvConfig
    bank = DungeonBank.random(64, 64, 16, seed=0)
    return {"c3_closed_form": EnvConfig.c3(),
            "bank16x64x64_k8": EnvConfig(width=64, height=64, n_npcs=8, layouts=bank.layouts),
            "dense_k40": EnvConfig(width=64, height=64, n_npcs=40)}


def check_baseline(torch, dev):
    """torch_kind == moves.outcomes == the kernel on small batches."""
    import numpy as np
    from optimax_rogue_amd import DungeonBank, EnvConfig
    from optimax_rogue_amd.engine import BatchedEngine
    from optimax_rogue_amd.moves import outcomes
    bank = DungeonBank.random(12, 12, 4, seed=5, wall_p=0.25, n_stairs=2).layouts
    seen = 0
    for cfg in (EnvConfig(width=8, height=8, n_npcs=4), EnvConfig(width=6, height=6, n_npcs=6),
                EnvConfig(width=8, height=8, n_npcs=4, start_mode=2, p1_depth=1, p2_depth=0),
                EnvConfig(width=12, height=12, n_npcs=4, layouts=bank),
                EnvConfig(width=16, height=16, n_npcs=40)):
        eng = BatchedEngine(cfg, 2000, seed=9, device=dev)
        eng.rollout(12, 1, 1)
        snap = eng.snapshot()
        for player in (0, 1):
            want = outcomes(cfg, snap, player)[0]
            assert np.array_equal(torch_kind(eng, player).cpu().numpy(), want), \
                "torch composition != moves.outcomes"
            assert np.array_equal(eng.moves_kind(player).cpu().numpy(), want), \
                "orx_moves != moves.outcomes"
            seen |= int(np.bitwise_or.reduce(1 << (want & 7), axis=None))
    assert seen & 0x7E == 0x7E, "a checked outcome never occurred"


def timed_block(torch, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def launcher(eng, kind, target=None, amount=None):
    """A zero-argument orx_moves launch for player 0 with its C arguments
    bound once."""
    import ctypes
    from optimax_rogue_amd import _lib
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    fn = eng.lib.orx_moves
    args = (eng._pcfg, eng._pst, 0, ptr(kind), ptr(target), ptr(amount), eng.B, eng._stream())

    def launch():
        code = fn(*args)
        if code:
            _lib.check("orx_moves", code)
    return launch


def main():
    import torch
    from optimax_rogue_amd.engine import BatchedEngine
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    games = [int(v) for v in opts.get("games", "65536,2097152").split(",")]
    launches = max(4, int(opts.get("launches", 200)))
    out_path = opts.get("out")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    check_baseline(torch, dev)
    lines = []
    for B in games:
        for name, cfg in bench_cfgs().items():
            eng = BatchedEngine(cfg, B, seed=3, device=dev)
            eng.rollout(16, 1, 1)
            kind = torch.empty((B, 8), dtype=torch.uint8, device=dev)
            target = torch.empty((B, 8), dtype=torch.int16, device=dev)
            amount = torch.empty((B, 8), dtype=torch.int16, device=dev)
            k_only, k_full = launcher(eng, kind), launcher(eng, kind, target, amount)
            base = lambda: torch_kind(eng, 0)
            k_full()
            assert torch.equal(kind, base()), "torch composition != orx_moves at the timed batch"
            assert torch.equal(kind, eng.moves_kind(0))
            n_base = max(4, min(launches, (1 << 24) // B * 4))
            for fn in (k_only, k_full, base) * 2:        # warm-up
                fn()
            torch.cuda.synchronize()
            t1, t3, tb = [], [], []
            for _ in range(4):                           # alternated blocks
                t1.append(timed_block(torch, k_only, launches // 4))
                t3.append(timed_block(torch, k_full, launches // 4))
                tb.append(timed_block(torch, base, max(1, n_base // 4)))
            s1, s3, sb = sorted(t1)[1], sorted(t3)[1], sorted(tb)[1]
            rec = {"config": name, "games": B, "launches": launches // 4 * 4,
                   "kind_us": round(s1 * 1e6, 2), "kind_us_blocks": [round(t * 1e6, 2) for t in t1],
                   "full_us": round(s3 * 1e6, 2), "full_us_blocks": [round(t * 1e6, 2) for t in t3],
                   "torch_us": round(sb * 1e6, 2), "torch_launches": max(1, n_base // 4) * 4,
                   "speedup_kind": round(sb / s1, 1), "speedup_full": round(sb / s3, 1)}
            for tag, full, s in (("kind", False, s1), ("full", True, s3)):
                nbytes = kernel_bytes(cfg, B, full)
                rec[tag + "_bytes"] = nbytes
                rec[tag + "_TBps"] = round(nbytes / s / 1e12, 3)
                rec[tag + "_fraction_of_plain_store"] = [
                    round(nbytes / s / 1e12 / PLAIN_STORE_TBS[1], 3),
                    round(nbytes / s / 1e12 / PLAIN_STORE_TBS[0], 3)]
            rec["bound"] = ("launch rate: %.1f MB per launch is not bandwidth-bound"
                            % (rec["full_bytes"] / 1e6)
                            if rec["full_bytes"] < LAUNCH_FLOOR_BYTES else "device time")
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del eng, kind, target, amount
            torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
