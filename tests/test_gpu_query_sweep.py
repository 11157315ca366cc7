"""GPU: the six query kernels -- orx_view, orx_path_query (with
orx_path_field), orx_path_seek (with orx_path_rows), orx_moves,
orx_npc_options, orx_npc_seek -- over the query sweep's draws
(tests/query_sweep.py): the fuzz's whole configuration space, a radius of
1..15 per player, every optional output asked for or not, batches of 1, 63,
257, 1000 and 1531 games (the lone game, the wave's and the 256-thread
workgroup's tails, several workgroups of every window size).

Per case, on the engine's state after the draw's bot ticks, for both players:
  * every output equals the numpy reference of that snapshot exactly (dtype
    and shape too) -- the references are held to the oracle's tick, the
    reference-schema restatements and Dijkstra by tests/test_query_sweep.py;
  * the outputs are views into buffers filled with a poison byte: the bytes
    before and after them stay poison, and no cell is left unwritten (every
    call runs with two poison bytes, so a cell that was skipped differs from
    the reference under one of them); view's cells and path's window start,
    on alternate cases, at an offset that is no multiple of 16 (stream_out's
    element path);
  * the queries leave the state untouched;
  * without moving NPCs, one drawn (player, move) is then played and the tick
    is what ``moves`` predicted (moves_cases.compare_move).
All values are integers: every comparison is exact.
"""
import numpy as np
import pytest

import moves_cases as mc
import query_sweep as qs
from guarded import POISONS, Guarded, same

pytestmark = pytest.mark.gpu

CASES = [qs.draw(c) for c in range(qs.N_CASES)]
TALLIES = {}               # case -> query_sweep.tally of the engine's state


def engine_state(d):
    """(engine, cfg, snapshot) of the case after its bot ticks."""
    import torch
    from optimax_rogue_amd.engine import BatchedEngine
    cfg = qs.env_config(d)
    eng = BatchedEngine(cfg, d.B, seed=d.seed, game_offset=d.off, device=torch.device("cuda", 0))
    if d.ticks:
        eng.rollout(d.ticks, *d.pol)
    return eng, cfg, eng.snapshot()


def check_queries(d, eng, refs, poison, msg):
    """Every query into guarded outputs filled with ``poison``."""
    import torch
    from optimax_rogue_amd.engine import _ptr
    from optimax_rogue_amd.moves import MOVES_COLS
    from optimax_rogue_amd.path import SEEK_COLS
    dev, B, K = eng.device, eng.B, eng.K
    u8, i8, i16, u16, i32 = torch.uint8, torch.int8, torch.int16, torch.uint16, torch.int32
    G = lambda dt, shape, skew=0: Guarded(dev, dt, shape, poison, skew)
    ptr = lambda g: None if g is None else _ptr(g.out)
    odd = d.case % 2          # alternate cases: an offset that is no multiple of 16

    def checked(outs, wants, names, what):
        for g, w, nm in zip(outs, wants, names):
            if g is not None:
                g.check(w, f"{msg} {what} {nm} poison {poison:#x}")

    for p in (0, 1):
        R = d.radius[p]
        V = 2 * R + 1
        # orx_view: cells, and the health plane where the case asks for it
        outs = [G(u8, (B, V, V), 2 * odd)] + ([G(u8, (B, V, V), 6 * odd)] if d.health[p] else [])
        got = eng.view(R, player=p, health=d.health[p],
                       out=tuple(g.out for g in outs) if d.health[p] else outs[0].out)
        assert (got[0] if d.health[p] else got) is outs[0].out
        checked(outs, refs["view", p], ("cells", "health"), f"view R={R} player {p}")
        # orx_path_query: dist, move, and the window where the case asks for it
        outs = [G(i32, (B,)), G(i8, (B,))] + ([G(u16, (B, V, V), 2 * odd)] if d.window[p] else [])
        eng.path(p, R if d.window[p] else None, out=tuple(g.out for g in outs))
        checked(outs, refs["path", p], ("dist", "move", "window"), f"path R={R} player {p}")
        # orx_moves: in full, the kind alone, and with the case's NULL outputs
        shape = (B, MOVES_COLS)
        outs = [G(u8, shape), G(i16, shape), G(i16, shape)]
        eng.moves(p, out=tuple(g.out for g in outs))
        names = ("kind", "target", "amount")
        checked(outs, refs["moves", p], names, f"moves player {p}")
        same(eng.moves_kind(p), refs["moves", p][0], f"{msg} moves_kind player {p}")
        m = d.moves_mask[p]
        outs = [G(u8, shape), G(i16, shape) if m & 1 else None, G(i16, shape) if m & 2 else None]
        eng._call("orx_moves", p, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), B, eng._stream())
        checked(outs, refs["moves", p], names, f"moves (outputs {m}) player {p}")
        # orx_path_seek: in full, and with the case's NULL outputs
        if d.seekable:
            shape = (B, SEEK_COLS)
            names = ("dist", "move", "target")
            outs = [G(i32, shape), G(i8, shape), G(i16, shape)]
            eng.seek(p, out=tuple(g.out for g in outs))
            checked(outs, refs["seek", p], names, f"seek player {p}")
            m = d.seek_mask[p]
            outs = [G(dt, shape) if m >> j & 1 else None for j, dt in enumerate((i32, i8, i16))]
            eng._call("orx_path_seek", _ptr(eng.pair_field), p, ptr(outs[0]), ptr(outs[1]),
                      ptr(outs[2]), B, eng._stream())
            checked(outs, refs["seek", p], names, f"seek (outputs {m}) player {p}")
    if not K:
        return
    # orx_npc_options: in full, kind and where alone, and with the case's NULL outputs
    shape = (K, B, MOVES_COLS)
    names = ("kind", "target", "amount", "where")
    outs = [G(u8, shape), G(i16, shape), G(i16, shape), G(u8, (B,))]
    eng.npc_options(out=tuple(g.out for g in outs))
    checked(outs, refs["npc_options"], names, "npc_options")
    kind, where = eng.npc_options_kind()
    same(kind, refs["npc_options"][0], f"{msg} npc_options_kind kind")
    same(where, refs["npc_options"][3], f"{msg} npc_options_kind where")
    m = d.npc_mask
    outs = [G(u8, shape), G(i16, shape) if m & 1 else None, G(i16, shape) if m & 2 else None,
            G(u8, (B,)) if m & 4 else None]
    eng._call("orx_npc_options", ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), B,
              eng._stream())
    checked(outs, refs["npc_options"], names, f"npc_options (outputs {m})")
    if d.seekable:
        shape = (K, B, SEEK_COLS)
        names = ("dist", "move", "target")
        outs = [G(i32, shape), G(i8, shape), G(i16, shape)]
        eng.npc_seek(out=tuple(g.out for g in outs))
        checked(outs, refs["npc_seek"], names, "npc_seek")
        m = d.seek_mask[1]
        outs = [G(dt, shape) if m >> j & 1 else None for j, dt in enumerate((i32, i8, i16))]
        eng._call("orx_npc_seek", _ptr(eng.pair_field), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                  B, eng._stream())
        checked(outs, refs["npc_seek"], names, f"npc_seek (outputs {m})")


@pytest.mark.parametrize("case", range(qs.N_CASES))
def test_queries_equal_their_references(case):
    import torch
    from optimax_rogue_amd import moves as mv
    d = CASES[case]
    msg = qs.where(d)
    eng, cfg, snap = engine_state(d)
    grid = eng.npc_grid.clone() if eng.K > 16 else None
    refs = qs.references(d, cfg, snap, eng.bank)
    TALLIES[case] = qs.tally(d, cfg, snap, refs)
    for poison in POISONS:
        check_queries(d, eng, refs, poison, msg)
    # the queries left the state as it was
    after = eng.snapshot()
    assert after.keys() == snap.keys(), msg
    for k in snap:
        assert np.array_equal(snap[k], after[k]), (msg, "state changed", k)
    if grid is not None:
        assert torch.equal(eng.npc_grid, grid), (msg, "npc_grid changed")
    if d.moving:
        return
    # prediction equals play: one drawn (player, move) against the engine's own tick
    rs = np.random.RandomState(qs.QBASE + case)
    p, m = int(rs.randint(0, 2)), int(rs.randint(1, mv.move_count(cfg) + 1))
    pred = tuple(t.cpu().numpy() for t in eng.moves(p))
    actions = torch.from_numpy(mc.actions_for(eng.B, p, m)).to(eng.device)
    _, ev, nev = eng.step(actions, events=True)
    try:
        mc.compare_move(cfg, snap, pred, p, m, eng.snapshot(), ev.cpu().numpy(), nev.cpu().numpy())
    except AssertionError as e:
        raise AssertionError(f"{msg} player {p} move {m}: {e}") from e


def test_engine_states_cover_the_queries():
    """query_sweep.check_coverage on what the ENGINE's states gave (those of
    the cases above; a case that did not run in this process is run here)."""
    if qs.N_CASES < 96:
        pytest.skip("the coverage conditions are those of the whole sweep")
    for d in CASES:
        if d.case not in TALLIES:
            eng, cfg, snap = engine_state(d)
            TALLIES[d.case] = qs.tally(d, cfg, snap, qs.references(d, cfg, snap, eng.bank))
    total = qs.add_up(TALLIES[d.case] for d in CASES)
    print("engine coverage:", total)
    qs.check_coverage(total)
