"""Times orx_path_threat (BatchedEngine.threat) in the forms a learner calls --
all rows without a window, with a radius-5 window, the flee move alone -- beside
the unchanged orx_path_seek on the same states.

    python tools/bench_threat.py [--games=65536,2097152] [--launches=200] [--radius=5]
                                 [--out=profiles/threat/bench_threat.jsonl]

Protocol.  tools/bench_seek.py's two configurations with 8 NPCs, the closed
form (C3: 64 x 64) and a 16-layout 64 x 64 bank (``DungeonBank.random(64, 64,
16, seed=0)``: a 512 MiB table), and the closed form with 64 NPCs (the long
per-lane loop of dense NPCs), each after 16 RandomBot ticks.  The kernel is
first checked equal to ``path.threat`` on small batches; then the four forms
are timed alternately in one process, each block between two HIP events, over
--launches launches in four blocks.  One JSON line per setting: every form's
time (the second-fastest of its four blocks) with all four blocks beside it,
and for the window form its written bytes over its time; a launch that writes
less than 64 MB is not bandwidth-bound and the line says so instead of quoting
a fraction of the 6.0-6.2 TB/s a plain-store stream reaches on this GPU.
Recorded, not gated.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAIN_STORE_TBS = (6.0, 6.2)   # plain stores, one dword per lane, 256 B per wave-instruction
LAUNCH_FLOOR_BYTES = 64 << 20  # below this much output a launch is not bandwidth-bound
ROW_BYTES = 4 * (4 + 1 + 2 + 8)  # a game's dist, move, target and after rows


def bench_cfgs():
    from optimax_rogue_amd import DungeonBank, EnvConfig
    bank = DungeonBank.random(64, 64, 16, seed=0)
    c3 = EnvConfig.c3()
    dense = EnvConfig.from_dict(dict(c3.to_dict(), n_npcs=64))
    return {"closed_form": c3,
            "bank16x64x64": EnvConfig(width=64, height=64, n_npcs=8, layouts=bank.layouts),
            "closed_form_k64": dense}


def check_kernel(torch, dev, radius):
    """orx_path_threat == path.threat on small batches, every output."""
    import numpy as np
    from optimax_rogue_amd import DungeonBank, EnvConfig
    from optimax_rogue_amd.engine import BatchedEngine
    from optimax_rogue_amd.path import threat
    bank = DungeonBank.random(12, 10, 4, seed=1, wall_p=0.3, n_stairs=2).layouts
    for cfg in (EnvConfig(width=10, height=8, n_npcs=4, max_ticks=30),
                EnvConfig(width=20, height=20, n_npcs=40),
                EnvConfig(width=12, height=10, n_npcs=6, layouts=bank)):
        eng = BatchedEngine(cfg, 200, seed=9, device=dev)
        for _ in range(20):
            eng.step(eng.policy(1, 1))
        snap = eng.snapshot()
        for player in (0, 1):
            want = threat(snap, cfg, player, radius, bank=eng.bank)
            for w, g in zip(want, eng.threat(player=player, radius=radius)):
                assert np.array_equal(g.cpu().numpy(), w), "orx_path_threat != path.threat"
            assert np.array_equal(eng.flee_moves(player).cpu().numpy(), want[1][:, 2])


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
    launches = max(4, int(opts.get("launches", 200)))
    radius = int(opts.get("radius", 5))
    out_path = opts.get("out")
    dev = torch.device("cuda", 0)
    check_kernel(torch, dev, radius)
    V = 2 * radius + 1
    lines = []
    for B in games:
        for name, cfg in bench_cfgs().items():
            eng = BatchedEngine(cfg, B, seed=3, device=dev)
            eng.rollout(16, 1, 1)
            eng.seek()                                   # (the bank's table: once, untimed)
            i32, i8, i16 = torch.int32, torch.int8, torch.int16
            rows = tuple(torch.empty((B, n), dtype=dt, device=dev)
                         for dt, n in ((i32, 4), (i8, 4), (i16, 4), (i32, 8)))
            window = torch.empty((B, V, V), dtype=torch.uint16, device=dev)
            seek_out = tuple(torch.empty((B, 4), dtype=dt, device=dev) for dt in (i32, i8, i16))
            pairs, stream = _ptr(eng.pair_field), eng._stream()
            forms = {
                "threat": lambda: eng.threat(out=rows),
                "threat_window": lambda: eng.threat(radius=radius, out=rows + (window,)),
                "move_alone": lambda: eng._call("orx_path_threat", pairs, 0, 0, None,
                                                _ptr(rows[1]), None, None, None, B, stream),
                "seek": lambda: eng.seek(out=seek_out),
            }
            for fn in list(forms.values()) * 2:          # warm-up
                fn()
            torch.cuda.synchronize()
            blocks = {k: [] for k in forms}
            for _ in range(4):                           # alternated blocks
                for k, fn in forms.items():
                    blocks[k].append(timed_block(torch, fn, launches // 4))
            rec = {"config": name, "games": B, "npcs": int(cfg.n_npcs), "radius": radius,
                   "launches": launches // 4 * 4}
            for k, ts in blocks.items():
                rec[k + "_us"] = round(sorted(ts)[1] * 1e6, 2)
                rec[k + "_us_blocks"] = [round(t * 1e6, 2) for t in ts]
            nbytes = B * (ROW_BYTES + 2 * V * V)
            rec["threat_window_written_bytes"] = nbytes
            if nbytes < LAUNCH_FLOOR_BYTES:
                rec["note"] = ("%.1f MB written with the window: not bandwidth-bound, no "
                               "bandwidth fraction quoted" % (nbytes / 1e6))
            else:
                tbs = nbytes / sorted(blocks["threat_window"])[1] / 1e12
                rec["threat_window_written_TBps"] = round(tbs, 3)
                rec["fraction_of_plain_store"] = [round(tbs / PLAIN_STORE_TBS[1], 3),
                                                  round(tbs / PLAIN_STORE_TBS[0], 3)]
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del eng, rows, window, seek_out, forms
            torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
