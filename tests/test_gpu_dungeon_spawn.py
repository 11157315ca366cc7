"""GPU: orx_dungeon_spawn / orx_dungeon_stairs (stairs_kernel) against the
oracle's world, generation 1 included, against the engine's own descents, at
request counts off a block multiple into guarded buffers, and its refusals
(dungeon_cases.py; test_dungeon_spawn.py holds the oracle's side)."""
import ctypes

import numpy as np
import pytest

import dungeon_cases as dc
from guarded import POISONS, Guarded

pytestmark = pytest.mark.gpu
EINVAL = -22


def _engine(case, n=dc.B, offset=dc.OFFSET, cfg=None):
    import torch
    from optimax_rogue_amd import EnvConfig
    from optimax_rogue_amd.engine import BatchedEngine
    return BatchedEngine(EnvConfig.from_dict(case.cfg if cfg is None else cfg,
                                             layouts=dc.layouts_of(case)), n, seed=case.seed,
                         game_offset=offset, device=torch.device("cuda", 0))


@pytest.fixture(scope="module")
def runs(oracle_lib):
    return {c.name: dc.run(oracle_lib, c) for c in dc.CASES}


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_world_vs_oracle(case, runs):
    """Every dungeon of every followed game's world at every tick, with the
    generation the players' depths give it: staircase and layout (-1 without a
    bank) as the oracle holds them."""
    ticks, _ = runs[case.name]
    rows = np.concatenate([r for _, _, _, r in ticks])
    tick_of = np.concatenate([np.full(len(r), t) for t, _, _, r in ticks])
    assert (rows[:, 3] == 1).any() == (case.cfg["despawn"] == dc.UNUSED)
    got = _engine(case).dungeon_stairs(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3])
    bad = np.flatnonzero((got != rows[:, 4:7]).any(axis=1))
    assert not len(bad), (case.name, "tick", tick_of[bad[:3]], "(game, episode, depth, gen, sx, "
                          "sy, layout)", rows[bad[:3]], "got", got[bad[:3]])


@pytest.mark.parametrize("case", [c for c in dc.CASES if c.cfg["despawn"] == dc.UNUSED],
                         ids=lambda c: c.name)
def test_generation_one(case, runs):
    """The staircase (and layout) a player lands on when it enters a depth the
    other player has passed through is generation 1's, and generation 0's
    answer differs from it in at least one such descent."""
    ticks, tr = runs[case.name]
    assert tr.gen1
    g1 = np.array(tr.gen1)
    t, g, p, nd = g1[:, 0], g1[:, 1], g1[:, 2], g1[:, 3]
    state = lambda f: np.array([ticks[a][2][f][b][c] for a, b, c in zip(t, p, g)], np.int64)
    ep = np.array([ticks[a][2]["episode"][c] for a, c in zip(t, g)], np.int64)
    landed = np.stack([state("st_x"), state("st_y"),
                       state("p_layout") if case.bank else np.full(len(g1), -1)], 1)
    eng = _engine(case)
    one = eng.dungeon_stairs(g, ep, nd, np.ones(len(g1), np.int64))
    zero = eng.dungeon_stairs(g, ep, nd, np.zeros(len(g1), np.int64))
    bad = np.flatnonzero((one != landed).any(axis=1))
    assert not len(bad), (case.name, g1[bad[:3]], landed[bad[:3]], one[bad[:3]])
    assert (zero != landed).any(axis=1).any(), case.name


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_engines_own_descents(case):
    """Every descent orx_step_events records (an ORX_EV_POSITION of a player
    onto a deeper depth) in a game the tracker follows lands on the other
    player's staircase where that player stands on the depth, else on the
    staircase dungeon_stairs names for its (game, episode, depth, generation)
    -- also where both players descend in one tick; and where one does, a
    dungeon is recorded as made (ORX_EV_DUNGEON) exactly when the rule above
    ``descend`` says so."""
    eng = _engine(case)
    tr = dc.Tracker(case.cfg, dc.B)
    start = dc.starts(case.cfg)
    unused = case.cfg["despawn"] == dc.UNUSED
    prev = eng.snapshot()
    req, want, checked_made, two = [], [], 0, 0
    for t in range(dc.TICKS):
        _, ev, nev = eng.step(eng.policy(*case.bots), events=True)
        ev, nev = ev.cpu().numpy(), nev.cpu().numpy()
        s = eng.snapshot()
        tr.see(t, prev, s)
        for g in range(dc.B):
            if s["episode"][g] != prev["episode"][g] or tr.unknown[g]:
                continue
            recs = [tuple(int(v) for v in r) for r in ev[g, : nev[g]]]
            down = [r for r in recs if r[0] == 3 and r[1] in (1, 2)
                    and r[2] > prev["p_depth"][r[1] - 1][g]]
            made = [r[2] for r in recs if r[0] == 4]
            assert len(down) == sum(s["p_depth"][p][g] > prev["p_depth"][p][g] for p in (0, 1))
            if len(down) == 2:
                # both descend: whatever order they moved in, each stands in the
                # dungeon of the generation the tracker holds for its depth
                for r in down:
                    p, nd = r[1] - 1, r[2]
                    req.append((g, int(s["episode"][g]), nd, tr.gen(g, nd)))
                    want.append((int(s["st_x"][p][g]), int(s["st_y"][p][g]),
                                 int(s["p_layout"][p][g]) if case.bank else -1))
                two += 1
            if len(down) != 1:
                continue
            p, nd = down[0][1] - 1, down[0][2]
            od = int(prev["p_depth"][1 - p][g])
            present = od == nd if unused else start[1 - p] <= nd <= od
            assert made == ([] if present else [nd]), (case.name, t, g, recs)
            checked_made += 1
            landed = (int(s["st_x"][p][g]), int(s["st_y"][p][g]),
                      int(s["p_layout"][p][g]) if case.bank else -1)
            if od == nd:
                theirs = (int(prev["st_x"][1 - p][g]), int(prev["st_y"][1 - p][g]),
                          int(prev["p_layout"][1 - p][g]) if case.bank else -1)
                assert landed == theirs, (case.name, t, g)
                continue
            req.append((g, int(s["episode"][g]), nd, tr.gen(g, nd)))
            want.append(landed)
        prev = s
    req, want = np.array(req), np.array(want)
    assert len(req) > dc.B // 4 and checked_made >= len(req) - 2 * two
    # ticks in which both players descend, checked (the oracle's runs hold 13 to
    # 3,001 of them; none where a RandomBot leads on 12 x 10)
    assert two >= (0 if case.name == "unreachable_bank1_12x10" else 10), two
    got = eng.dungeon_stairs(req[:, 0], req[:, 1], req[:, 2], req[:, 3])
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (case.name, req[bad[:3]], want[bad[:3]], got[bad[:3]])


def _spawn(eng, n, tensors, layout=True, entry="orx_dungeon_spawn", seed=None, cfg=None):
    """The entry point on raw pointers: (games, episodes, depths, gens, sx, sy,
    layout) tensors or None each; its return code."""
    import torch
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    g, e, d, gn, sx, sy, lay = tensors
    pcfg = ctypes.byref(eng._ccfg if cfg is None else cfg)
    seed = eng.seed if seed is None else seed
    with torch.cuda.device(eng.device):
        if entry == "orx_dungeon_stairs":
            return eng.lib.orx_dungeon_stairs(pcfg, ptr(g), ptr(e), ptr(d), ptr(gn), ptr(sx),
                                              ptr(sy), n, seed, eng._stream())
        return eng.lib.orx_dungeon_spawn(pcfg, ctypes.byref(eng._st), ptr(g), ptr(e), ptr(d),
                                         ptr(gn), ptr(sx), ptr(sy), ptr(lay) if layout else None,
                                         n, seed, eng._stream())


def _requests(case, n, offset):
    """n requests over 499 distinct (game, episode, depth, generation) keys in
    a scrambled order, and their reference rows."""
    rs = np.random.RandomState(n)
    keys = np.stack([rs.randint(0, 1 << 20, 499) + offset, rs.randint(0, 40, 499),
                     rs.randint(0, 300, 499), rs.randint(0, 2, 499)], 1)
    req = keys[(np.arange(n) * 7919 + n) % 499]
    return req, dc.ref_rows(case, *req.T)


SHAPES = (1, 255, 256, 257, 100003)


@pytest.mark.parametrize("name", ["unused_sep_9x7", "unused_sep_bank6_12x10"])
@pytest.mark.parametrize("n", SHAPES)
def test_shapes_guarded(name, n):
    """n off a block multiple and past one block, a game offset, a NULL layout
    with a bank, orx_dungeon_stairs without one: outputs in guarded buffers
    under both poisons, against oracle/pyref.py's spawn_dungeon."""
    import torch
    case = dc.CASE[name]
    eng = _engine(case, n=1, offset=77)
    dev = eng.device
    req, want = _requests(case, n, 77)
    ins = [torch.from_numpy(np.ascontiguousarray(req[:, j]).astype(np.int32)).to(dev)
           for j in range(4)]
    for poison in POISONS:
        for layout in (True, False):
            outs = [Guarded(dev, torch.int32, (n,), poison, skew=4 * (j + 1)) for j in range(3)]
            entry = "orx_dungeon_spawn" if case.bank or layout else "orx_dungeon_stairs"
            code = _spawn(eng, n, ins + [o.out for o in outs], layout=layout, entry=entry)
            assert code == 0, eng.lib.orx_last_error().decode()
            where = f"{name} n={n} poison {poison:#x} layout {layout}"
            outs[0].check(want[:, 0], where + " sx")
            outs[1].check(want[:, 1], where + " sy")
            outs[2].check(want[:, 2] if layout else np.full(n, poison * 0x01010101, np.uint32)
                          .view(np.int32), where + " layout")
    torch.cuda.synchronize()


def test_refusals():
    """Stock-seed mode, a bank through orx_dungeon_stairs, NULL pointers and
    n < 0 are refused; n == 0 is ORX_OK and writes nothing."""
    import torch
    from optimax_rogue_amd import EnvConfig
    plain, bank = dc.CASE["unused_sep_9x7"], dc.CASE["unused_sep_bank6_12x10"]
    eng, eng_bank = _engine(plain, n=1), _engine(bank, n=1)
    dev = eng.device
    n = 8
    ins = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4)]
    outs = [Guarded(dev, torch.int32, (n,), POISONS[0]) for _ in range(3)]
    args = ins + [o.out for o in outs]
    untouched = np.full(n, POISONS[0] * 0x01010101, np.uint32).view(np.int32)

    def refused(code, what):
        assert code == EINVAL, (what, code)
        assert eng.lib.orx_last_error(), what
        for o in outs:
            o.check(untouched, what)

    stock = EnvConfig.from_dict(dict(plain.cfg, rng=1)).to_c()
    refused(_spawn(eng, n, args, cfg=stock), "stock-seed mode")
    refused(_spawn(eng, n, args, entry="orx_dungeon_stairs", cfg=stock), "stock-seed stairs")
    refused(_spawn(eng_bank, n, args, entry="orx_dungeon_stairs"), "a bank through stairs")
    for j in range(6):   # (layout may be NULL)
        holed = list(args)
        holed[j] = None
        refused(_spawn(eng, n, holed), f"pointer {j} NULL")
        refused(_spawn(eng_bank, n, holed), f"pointer {j} NULL with a bank")
    refused(_spawn(eng, -1, args), "n < 0")
    refused(_spawn(eng, -1, args, entry="orx_dungeon_stairs"), "n < 0 stairs")
    for e, entry in ((eng, "orx_dungeon_spawn"), (eng, "orx_dungeon_stairs"),
                     (eng_bank, "orx_dungeon_spawn")):
        assert _spawn(e, 0, args, entry=entry) == 0
        assert _spawn(e, 0, [None] * 7, entry=entry) == 0
    torch.cuda.synchronize()
    for o in outs:
        o.check(untouched, "n == 0")
