"""GPU: orx_path_ticks over the query sweep's 96 draws (tests/query_sweep.py,
unmodified): the fuzz's whole configuration space -- grid shapes, both despawn
rules, start depths, banks, 0-255 NPCs of 1 to 127 health, player damage and
armor on both sides of a == 0, stock seeding, every extension flag (the
character flags take the damage from p_rpg), moving NPCs -- at the draws'
batches of 1, 63, 257, 1000 and 1531 games and their radii of 1..15.

Per case, on the engine's state after the draw's bot ticks, for both players:
every output equals ``path.ticks`` of that snapshot exactly, in full (with a
window where the draw asks the path query for one) and with the NULL outputs
the draw's seek mask names; the outputs are views into poisoned buffers
(tests/guarded.py), run under two poison bytes, the window on alternate cases
at an offset that is no multiple of 16; ``ticks >= dist``; and the state is left
untouched.  No case is skipped: the query needs no pair table.
"""
import numpy as np
import pytest

import query_sweep as qs
from guarded import POISONS, Guarded

pytestmark = pytest.mark.gpu

CASES = [qs.draw(c) for c in range(qs.N_CASES)]
NAMES = ("ticks", "move", "window")


def engine_state(d):
    import torch
    from optimax_rogue_amd.engine import BatchedEngine
    cfg = qs.env_config(d)
    eng = BatchedEngine(cfg, d.B, seed=d.seed, game_offset=d.off, device=torch.device("cuda", 0))
    if d.ticks:
        eng.rollout(d.ticks, *d.pol)
    return eng, cfg, eng.snapshot()


def check_ticks(d, eng, want, p, poison, msg):
    import torch
    from optimax_rogue_amd.engine import _ptr
    B, R = eng.B, d.radius[p]
    V = 2 * R + 1
    dts = (torch.int32, torch.int8, torch.uint16)
    shapes = ((B,), (B,), (B, V, V))
    G = lambda j: Guarded(eng.device, dts[j], shapes[j], poison, 2 * (d.case % 2) if j == 2 else 0)

    def checked(outs, what):
        for g, w, nm in zip(outs, want, NAMES):
            if g is not None:
                g.check(w, f"{msg} ticks {what} player {p} {nm} poison {poison:#x}")

    # in full, through the engine's method
    outs = [G(j) for j in range(3 if d.window[p] else 2)]
    got = eng.path_ticks(p, R if d.window[p] else None, out=tuple(g.out for g in outs))
    assert all(x is g.out for x, g in zip(got, outs))
    checked(outs, f"R={R if d.window[p] else None}")
    # the draw's NULL outputs: seek's mask (bits ticks, move, window; never 0)
    m = d.seek_mask[p]
    outs = [G(j) if m >> j & 1 else None for j in range(3)]
    eng._call("orx_path_ticks", _ptr(eng.route_planes), p, R,
              *(None if g is None else _ptr(g.out) for g in outs), B, eng._stream())
    checked(outs, f"R={R} outputs {m:#x}")


@pytest.mark.parametrize("case", range(qs.N_CASES))
def test_ticks_equals_its_reference(case):
    from optimax_rogue_amd import path
    d = CASES[case]
    msg = qs.where(d)
    eng, cfg, snap = engine_state(d)
    for p in (0, 1):
        want = path.ticks(snap, cfg, p, d.radius[p], bank=eng.bank)
        dist = path.query(snap, cfg, p, bank=eng.bank)[0]
        assert ((want[0] >= dist) | (want[0] == -1)).all(), msg
        assert (want[0][dist < 0] == -1).all(), msg
        for poison in POISONS:
            check_ticks(d, eng, want, p, poison, msg)
    after = eng.snapshot()
    assert after.keys() == snap.keys(), msg
    for k in snap:
        assert np.array_equal(snap[k], after[k]), (msg, "state changed", k)


def test_the_sweep_is_not_one_kind_of_case():
    assert sum(d.layouts is not None for d in CASES) >= 10
    assert sum(d.cfg["n_npcs"] > 64 for d in CASES) >= 1 and any(d.cfg["n_npcs"] == 0 for d in CASES)
    assert sum(d.cfg["n_npcs"] > 16 for d in CASES) >= 10
    assert sum(d.cfg["player_damage"] <= d.cfg["player_armor"] for d in CASES) >= 5    # a == 0
    assert sum(bool(d.cfg["flags"] & 124) for d in CASES) >= 10                        # p_rpg's damage
    assert {True, False} <= {w for d in CASES for w in d.window}
