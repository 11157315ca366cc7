"""GPU: orx_route over the query sweep's draws (tests/query_sweep.py) -- the
fuzz's whole configuration space: grid shapes, banks and the empty room, both
start modes, stock seeding, 0-255 NPCs, moving NPCs, every extension flag --
with the remembered maps built by ``explore`` over the draw's bot ticks, a
radius per player.  Batches of 1, 63, 257 and 1000 games (the draw's own where
the reference's boolean arrays stay small); on the final state, for both
players, the kernel's rows equal ``route.route`` exactly, into poison-guarded
buffers under both poisons, in full and with the draw's NULL outputs, and the
state and the maps are as they were.
"""
import numpy as np
import pytest

import explore_cases as ec
import query_sweep as qs
import route_cases as rc
from guarded import POISONS, Guarded

pytestmark = pytest.mark.gpu

N_CASES = min(qs.N_CASES, 48)
SIZES = (1, 63, 257, 1000)
CELLS = 1 << 21                     # B * W * H of the reference's arrays, at most


def batch(d):
    """The case's batch: SIZES in turn, the largest whose arrays stay small."""
    want = SIZES[d.case % len(SIZES)]
    fits = [b for b in SIZES if b <= want and b * d.cfg["width"] * d.cfg["height"] <= CELLS]
    return fits[-1] if fits else 1


CASES = [qs.draw(c) for c in range(N_CASES)]


def test_the_draws_cover_the_configurations():
    """Conditions on the draws themselves (no GPU work): every batch size, with
    and without a bank, stock seeding, Separated starts."""
    assert {batch(d) for d in CASES} == set(SIZES)
    assert any(d.layouts is not None for d in CASES) and any(d.layouts is None for d in CASES)
    assert any(d.cfg.get("rng") == 1 for d in CASES)
    assert any(d.cfg.get("start_mode") == 2 for d in CASES)
    assert all(d.cfg["width"] * d.cfg["height"] <= 65536 for d in CASES)


def host(t):
    import torch
    if t.dtype == torch.uint32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    return t.cpu().numpy()


@pytest.mark.parametrize("case", range(N_CASES))
def test_route_equals_its_reference(case):
    import torch
    from optimax_rogue_amd import explore, route
    from optimax_rogue_amd.engine import BatchedEngine, _ptr
    d = CASES[case]
    B = batch(d)
    msg = qs.where(d) + f" (route sweep B={B})"
    cfg = qs.env_config(d)
    eng = BatchedEngine(cfg, B, seed=d.seed, game_offset=d.off, device=torch.device("cuda", 0))
    W, H = int(cfg.width), int(cfg.height)
    for tick in range(d.ticks + 1):
        if tick:
            eng.step(eng.policy(*d.pol))
        for p in (0, 1):
            eng.explore(d.radius[p], player=p)
    snap = eng.snapshot()
    rs = np.random.RandomState(qs.QBASE + case)
    i32, i8 = torch.int32, torch.int8
    for p in (0, 1):
        memory, key = (host(t) for t in eng.explore_map(p))
        tiles = ec.tiles_of(cfg, snap, p, eng.bank)
        goal, _ = rc.draw_goals(rs, tiles, explore.unpack(memory, W), H)
        goal_t = torch.from_numpy(goal).to(eng.device)
        want = route.route(memory, key, snap, cfg, p, goal=goal, bank=eng.bank)
        for poison in POISONS:
            for mask in (7, d.seek_mask[p]):
                outs = [Guarded(eng.device, dt, (B, 4), poison) if mask >> j & 1 else None
                        for j, dt in enumerate((i32, i8, i32))]
                m_t, k_t = eng.explore_map(p)
                eng._call("orx_route", _ptr(eng.route_planes), p, _ptr(m_t), _ptr(k_t), _ptr(goal_t),
                          *(None if g is None else _ptr(g.out) for g in outs), B, eng._stream())
                for g, w, nm in zip(outs, want, ("dist", "move", "target")):
                    if g is not None:
                        g.check(w, f"{msg} player {p} outputs {mask} {nm} poison {poison:#x}")
        for t, a in zip(eng.explore_map(p), (memory, key)):
            assert np.array_equal(host(t), a), (msg, "map changed")
    after = eng.snapshot()
    for k in snap:
        assert np.array_equal(snap[k], after[k]), (msg, "state changed", k)
    assert eng._pair_field is None
