"""GPU: orx_sight over the query sweep's draws (tests/query_sweep.py): the
fuzz's whole configuration space, a radius of 1..15 per player, batches of 1,
63, 257, 1000 and 1531 games, on the engine's state after the draw's bot ticks
(made as tests/test_gpu_query_sweep.py makes it).

Per case and player: the row words, the masked cells and the masked health
plane equal the numpy reference of that snapshot exactly, written into
poison-guarded buffers under both poisons (the planes hold orx_view's output
first); on alternate cases the rows start 4 bytes and the planes 1 byte past a
16-byte boundary.  The coverage conditions tests/test_sight.py asserts on the
oracle's states are asserted again on the engine's.
"""
import numpy as np
import pytest

import query_sweep as qs
import sight_cases as sc
from guarded import POISONS, Guarded
from test_gpu_query_sweep import engine_state

pytestmark = pytest.mark.gpu

CASES = [qs.draw(c) for c in range(qs.N_CASES)]
TALLIES = {}               # case -> (tally of the engine's state, asymmetric games at R = 15)


def run_case(d, guarded=True):
    import torch
    from optimax_rogue_amd import sight, view
    from optimax_rogue_amd.engine import _ptr
    eng, cfg, snap = engine_state(d)
    msg, B, odd = qs.where(d), eng.B, d.case % 2
    tallies = []
    for p in (0, 1):
        R = d.radius[p]
        V = 2 * R + 1
        cells, hp = view.render_view(snap, cfg, p, R, bank=eng.bank, health=True)
        vis = sight.visible_of(cells)
        tallies.append(sc.tally(cells, vis))
        want = (sight.pack_rows(vis),) + sight.apply(cells, vis, hp)
        for poison in POISONS if guarded else ():
            gr = Guarded(eng.device, torch.uint32, (B, V), poison, 4 * odd)
            gc = Guarded(eng.device, torch.uint8, (B, V, V), poison, odd)
            gh = Guarded(eng.device, torch.uint8, (B, V, V), poison, odd)
            eng.view(R, player=p, health=True, out=(gc.out, gh.out))
            eng._call("orx_sight", p, R, _ptr(gr.out), _ptr(gc.out), _ptr(gh.out), B,
                      eng._stream())
            for g, w, nm in zip((gr, gc, gh), want, ("rows", "cells", "health")):
                g.check(w, f"{msg} sight R={R} player {p} {nm} poison {poison:#x}")
    a, b = eng.sees_other(15, 0), eng.sees_other(15, 1)
    for p, got in ((0, a), (1, b)):
        vis = sight.visible(snap, cfg, p, 15, bank=eng.bank)
        assert np.array_equal(got.cpu().numpy(), sc.sees_other(snap, vis, p, 15)), msg
    after = eng.snapshot()
    for k in snap:
        assert np.array_equal(snap[k], after[k]), (msg, "state changed", k)
    total = sc.add_up(tallies)
    total["banks"] = int(d.layouts is not None)
    return total, int((a != b).sum())


@pytest.mark.parametrize("case", range(qs.N_CASES))
def test_sight_equals_its_reference(case):
    TALLIES[case] = run_case(CASES[case])


def test_engine_states_cover_sight():
    """test_sight.py's sweep conditions on what the ENGINE's states gave (a
    case that did not run in this process is run here, unguarded)."""
    if qs.N_CASES < 96:
        pytest.skip("the coverage conditions are those of the whole sweep")
    for d in CASES:
        if d.case not in TALLIES:
            TALLIES[d.case] = run_case(d, guarded=False)
    total = sc.add_up(t for t, _ in TALLIES.values())
    print("engine sight coverage:", total)
    assert total["banks"] >= 10, total
    for k in ("player_seen", "player_unseen", "npc_seen", "npc_unseen"):
        assert total[k] > 0, total
    assert sum(n for _, n in TALLIES.values()) == 0
