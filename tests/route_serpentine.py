"""The largest grid orx_route takes with a bank: B = 2 on a fully known 256 x
256 serpentine corridor (route_cases.serpentine), the player at one end, the
goal -- the staircase -- at the other; the second game's map is empty.  The
expected distance is the construction's, not the reference's.  Run by
tests/test_gpu_route.py in a process of its own, under a time limit.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import route_cases as rc
    from optimax_rogue_amd import DungeonBank, EnvConfig, explore
    from optimax_rogue_amd.engine import BatchedEngine, _ptr
    W = H = 256
    lay, start, end, moves = rc.serpentine(W, H)
    assert moves == 127 * 253 + 126 * 2
    bank = DungeonBank(lay[None])
    cfg = EnvConfig(width=W, height=H, n_npcs=0, layouts=bank.layouts)
    B = 2
    eng = BatchedEngine(cfg, B, seed=1)
    eng.p_x[0, :], eng.p_y[0, :] = start
    eng.p_layout[:] = 0
    snap = eng.snapshot()
    known = np.zeros((B, W, H), bool)
    known[0] = True
    memory = torch.from_numpy(explore.pack(known).view(np.int32)).to(eng.device)
    key = torch.from_numpy(np.stack([snap["episode"], snap["p_depth"][0], snap["tick"],
                                     known.sum(axis=(1, 2))], axis=1).astype(np.int32)).to(eng.device)
    cell = end[0] * H + end[1]
    goal = torch.full((B,), cell, dtype=torch.int32, device=eng.device)
    dist, move, target = (torch.full((B, 4), 77, dtype=dt, device=eng.device)
                          for dt in (torch.int32, torch.int8, torch.int32))
    eng._call("orx_route", _ptr(eng.route_planes), 0, _ptr(memory), _ptr(key), _ptr(goal),
              _ptr(dist), _ptr(move), _ptr(target), B, eng._stream())
    torch.cuda.synchronize(eng.device)
    got = [t.cpu().numpy().tolist() for t in (dist, move, target)]
    want = [[[-2, moves, moves, -2], [-2, -2, -1, -2]], [[5, 2, 2, 5], [5, 5, 5, 5]],
            [[-1, cell, cell, -1], [-1, -1, cell, -1]]]
    if got != want:
        print("serpentine 256 x 256: got", got, "want", want)
        return 1
    print("serpentine 256 x 256: ok,", moves, "moves")
    return 0


if __name__ == "__main__":
    sys.exit(main())
