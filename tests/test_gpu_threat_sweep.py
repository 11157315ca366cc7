"""GPU: orx_path_threat over the query sweep's 96 draws (tests/query_sweep.py,
unmodified): the fuzz's whole configuration space -- grid shapes, both despawn
rules, start depths, banks, 0-255 NPCs, stock seeding, every extension flag,
moving NPCs -- at the draws' batches of 1, 63, 257, 1000 and 1531 games and
their radii of 1..15.

Per case, on the engine's state after the draw's bot ticks, for both players:
every output equals ``path.threat`` of that snapshot exactly, in full (with a
window where the draw asks the path query for one) and with the NULL outputs
the draw's masks name; the outputs are views into poisoned buffers
(tests/guarded.py), run under two poison bytes, the window on alternate cases
at an offset that is no multiple of 16; and the state is left untouched.  A
bank whose pair table exceeds ``PAIR_TABLE_MAX`` is skipped, as the sweep skips
``seek`` there, under its cap ``MAX_UNSEEKABLE``.
"""
import numpy as np
import pytest

import query_sweep as qs
from guarded import POISONS, Guarded

pytestmark = pytest.mark.gpu

CASES = [qs.draw(c) for c in range(qs.N_CASES)]
NAMES = ("dist", "move", "target", "after", "window")


def engine_state(d):
    import torch
    from optimax_rogue_amd.engine import BatchedEngine
    cfg = qs.env_config(d)
    eng = BatchedEngine(cfg, d.B, seed=d.seed, game_offset=d.off, device=torch.device("cuda", 0))
    if d.ticks:
        eng.rollout(d.ticks, *d.pol)
    return eng, cfg, eng.snapshot()


def check_threat(d, eng, want, p, poison, msg):
    import torch
    from optimax_rogue_amd.engine import _ptr
    B, R = eng.B, d.radius[p]
    V = 2 * R + 1
    dts = (torch.int32, torch.int8, torch.int16, torch.int32, torch.uint16)
    shapes = ((B, 4), (B, 4), (B, 4), (B, 8), (B, V, V))
    G = lambda j: Guarded(eng.device, dts[j], shapes[j], poison, 2 * (d.case % 2) if j == 4 else 0)

    def checked(outs, what):
        for g, w, nm in zip(outs, want, NAMES):
            if g is not None:
                g.check(w, f"{msg} threat {what} player {p} {nm} poison {poison:#x}")

    # in full, through the engine's method
    outs = [G(j) for j in range(5 if d.window[p] else 4)]
    got = eng.threat(p, R if d.window[p] else None, out=tuple(g.out for g in outs))
    assert all(x is g.out for x, g in zip(got, outs))
    checked(outs, f"R={R if d.window[p] else None}")
    # the draw's NULL outputs: seek's mask for dist, move and target, the view's
    # health draw for after, and the window always (every case runs that kernel too)
    m = d.seek_mask[p] | (8 if d.health[p] else 0) | 16
    outs = [G(j) if m >> j & 1 else None for j in range(5)]
    eng._call("orx_path_threat", _ptr(eng.pair_field), p, R,
              *(None if g is None else _ptr(g.out) for g in outs), B, eng._stream())
    checked(outs, f"R={R} outputs {m:#x}")


@pytest.mark.parametrize("case", range(qs.N_CASES))
def test_threat_equals_its_reference(case):
    from optimax_rogue_amd import path
    d = CASES[case]
    if not d.seekable:
        pytest.skip(f"the pair table needs {d.pair_bytes} bytes, above PAIR_TABLE_MAX")
    msg = qs.where(d)
    eng, cfg, snap = engine_state(d)
    for p in (0, 1):
        want = path.threat(snap, cfg, p, d.radius[p], bank=eng.bank)
        for poison in POISONS:
            check_threat(d, eng, want, p, poison, msg)
    after = eng.snapshot()
    assert after.keys() == snap.keys(), msg
    for k in snap:
        assert np.array_equal(snap[k], after[k]), (msg, "state changed", k)


def test_the_sweep_skips_few():
    skipped = sum(not d.seekable for d in CASES)
    assert skipped <= qs.MAX_UNSEEKABLE * len(CASES), skipped
    # and what runs is not one kind of answer: both kernels, banks and rooms, dense NPCs
    ran = [d for d in CASES if d.seekable]
    assert sum(d.layouts is not None for d in ran) >= 10
    assert sum(d.cfg["n_npcs"] > 16 for d in ran) >= 10 and any(d.cfg["n_npcs"] == 0 for d in ran)
    assert {True, False} <= {w for d in ran for w in d.window}
