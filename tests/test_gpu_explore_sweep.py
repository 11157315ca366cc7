"""GPU: orx_explore_update / orx_explore_seek over the query sweep's draws
(tests/query_sweep.py): the fuzz's whole configuration space, a radius of 1..15
per player, batches of 1, 63, 257, 1000 and 1531 games, on the engine's state
after the draw's bot ticks (made as tests/test_gpu_query_sweep.py makes it) and
after each of a few more ticks.

Per case, tick and player: the map, the key, ``gained``, the remembered planes
and the seek's three rows equal the numpy reference (``optimax_rogue_amd.
explore``) exactly; the kernel works on its own map from tick to tick, in
poison-guarded buffers whose guards are checked every tick; on alternate cases
the words start 4 bytes, the planes 1 byte and the rows 16 bytes past a 16-byte
boundary.  The seek is skipped where the draw's pair table is too large
(``seekable``), as the other seeks are.
"""
import numpy as np
import pytest

import query_sweep as qs
from guarded import POISONS, Guarded
from test_gpu_explore import poisoned, upload
from test_gpu_query_sweep import engine_state

pytestmark = pytest.mark.gpu

CASES = [qs.draw(c) for c in range(qs.N_CASES)]
TICKS = 3                  # map updates per case, an engine tick between two
KEYS = ("gained", "cleared", "frontier", "stairs", "absent", "seeks")
TALLIES = {}               # case -> its counts


def run_case(case):
    import torch
    from optimax_rogue_amd import explore, sight, view
    from optimax_rogue_amd.engine import _ptr
    d = CASES[case]
    TALLY = {k: 0 for k in KEYS}
    eng, cfg, snap = engine_state(d)
    msg, B, odd = qs.where(d), eng.B, d.case % 2
    W, H = int(cfg.width), int(cfg.height)
    seekable = d.seekable and W * H <= 65536
    poison = POISONS[(d.case // 2) % 2]
    G = lambda dt, shape, skew: Guarded(eng.device, dt, shape, poison, skew)
    host = [explore.empty(B, W, H) for _ in (0, 1)]
    dev = []
    for p in (0, 1):
        gm, gk = G(torch.uint32, host[p][0].shape, 4 * odd), G(torch.int32, (B, 4), 16 * odd)
        upload(gm, host[p][0]), upload(gk, host[p][1])
        dev.append((gm, gk))
    for tick in range(TICKS):
        if tick:
            eng.rollout(1, *d.pol)
            snap = eng.snapshot()
        for p in (0, 1):
            R = d.radius[p]
            V = 2 * R + 1
            what = f"{msg} explore tick {tick} R={R} player {p}"
            memory, key = host[p]
            gm, gk = dev[p]
            TALLY["cleared"] += int((~explore.valid(key, snap, p) & (key[:, 3] >= 0)).sum())
            cells, hp = view.render_view(snap, cfg, p, R, bank=eng.bank, health=True)
            rows = sight.pack_rows(sight.visible_of(cells))
            want_g = explore.update(memory, key, snap, cfg, p, R, rows, cells, hp)
            gg, gc, gh = G(torch.int32, (B,), 4 * odd), G(torch.uint8, (B, V, V), odd), \
                G(torch.uint8, (B, V, V), odd)
            got_rows = eng.sight(R, player=p)
            assert np.array_equal(got_rows.view(torch.int32).cpu().numpy().view(np.uint32), rows), what
            eng.view(R, player=p, health=True, out=(gc.out, gh.out))
            with_h = d.health[p]
            eng._call("orx_explore_update", p, R, _ptr(got_rows), _ptr(gm.out), _ptr(gk.out),
                      _ptr(gg.out), _ptr(gc.out), _ptr(gh.out) if with_h else None, B, eng._stream())
            gm.check(memory, what + " memory")
            gk.check(key, what + " key")
            gg.check(want_g, what + " gained")
            gc.check(cells, what + " cells")
            if with_h:
                gh.check(hp, what + " health")
            TALLY["gained"] += int(want_g.sum())
            if not seekable:
                continue
            want = explore.seek(memory, key, snap, cfg, p, bank=eng.bank)
            mask = d.seek_mask[p]
            outs = [G(dt, (B, 4), skew) for dt, skew in
                    ((torch.int32, 16 * odd), (torch.int8, 4 * odd), (torch.int32, 16 * odd))]
            eng._call("orx_explore_seek", _ptr(eng.pair_field), p, _ptr(gm.out), _ptr(gk.out),
                      *(_ptr(g.out) if mask >> k & 1 else None for k, g in enumerate(outs)), B,
                      eng._stream())
            for k, (g, w, nm) in enumerate(zip(outs, want, ("dist", "move", "target"))):
                g.check(w if mask >> k & 1 else poisoned((B, 4), w.dtype, poison), f"{what} seek {nm}")
            gm.check(memory, what + " memory after the seek")
            TALLY["frontier"] += int((want[0][:, 0] > 0).sum())
            TALLY["stairs"] += int((want[0][:, 1] > 0).sum())
            TALLY["absent"] += int((want[0][:, :2] == -2).sum())
            TALLY["seeks"] += 1
    after = eng.snapshot()
    for k in snap:
        assert np.array_equal(snap[k], after[k]), (msg, "state changed", k)
    return TALLY


@pytest.mark.parametrize("case", range(qs.N_CASES))
def test_explore_equals_its_reference(case):
    TALLIES[case] = run_case(case)


def test_the_sweep_covers_the_map():
    """Conditions on what the sweep's states gave: maps gain cells and are
    cleared, both columns find targets and lack them (a case that did not run
    in this process is run here)."""
    for case in range(qs.N_CASES):
        if case not in TALLIES:
            TALLIES[case] = run_case(case)
    total = {k: sum(t[k] for t in TALLIES.values()) for k in KEYS}
    print("explore sweep coverage:", total)
    assert all(total[k] > 0 for k in KEYS), total
