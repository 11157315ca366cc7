"""GPU: the enemies' queries (include/orx_npc_query.h: orx_npc_options,
orx_npc_seek and the Python layers above them) -- against the numpy reference
(optimax_rogue_amd/npc_query.py, itself pinned on the CPU by
tests/test_npc_query.py), against the engine's own given-move tick, and in a
closed loop.  All values are integers: every comparison is exact."""
import numpy as np
import pytest

from npc_given_cases import BASE_CFG, bank
from npc_query_cases import ABSENT, env_config, hand_seek, hand_states

pytestmark = pytest.mark.gpu

B301 = 301   # two workgroups per slot, a partial wave, an odd row stride
SEP = dict(BASE_CFG, start_mode=2, p1_depth=2, p2_depth=1, max_ticks=60)
CFGS = {
    "k1_5x4": dict(BASE_CFG, width=5, height=4, n_npcs=1),
    "k6": dict(BASE_CFG),
    "k16": dict(BASE_CFG, n_npcs=16),                                  # the last register form
    "k17": dict(BASE_CFG, width=12, height=12, n_npcs=17),             # the first dense one
    "k33": dict(BASE_CFG, width=12, height=12, n_npcs=33),             # two alive words
    "k40": dict(BASE_CFG, width=12, height=12, n_npcs=40, npc_health=2),
    "bank": dict(BASE_CFG, width=9, height=8, n_npcs=5),
    "unwatched": dict(SEP, despawn=1),   # player 1 leaves depth 2, player 2 is above it
    "gone": dict(SEP, despawn=2),
    "stock": dict(BASE_CFG, rng=1),
}


def _layouts(name):
    return bank(9, 8, 3, 307) if name == "bank" else None


def _engine(cfg, n_games, seed, layouts=None):
    import torch
    from optimax_rogue_amd.engine import BatchedEngine
    return BatchedEngine(env_config(cfg, layouts), n_games, seed=seed,
                         device=torch.device("cuda", 0))


def _random_play(eng, ticks, gen):
    """``ticks`` steps of random player actions and a random NPC table."""
    import torch
    for _ in range(ticks):
        a = torch.randint(1, 6, (eng.B, 2), generator=gen, dtype=torch.int8).to(eng.device)
        tab = torch.randint(1, 6, (eng.K, eng.B), generator=gen, dtype=torch.int8).to(eng.device)
        eng.step(a, npc_moves=tab)


def _check_against_reference(eng, what, outs=None, seek_outs=None):
    """Every output of both queries on the engine's resident state equals the
    numpy reference on its snapshot, bit for bit; returns (kind, where)."""
    from optimax_rogue_amd import npc_query
    snap = eng.snapshot()
    want = npc_query.options(snap, eng.cfg, eng.bank)
    got = eng.npc_options(out=outs)
    if outs is not None:
        assert all(g is o for g, o in zip(got, outs))
    for g, w, nm in zip(got, want, ("kind", "target", "amount", "where")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, nm)
        assert np.array_equal(g, w), (what, nm, np.argwhere(g != w)[:5])
    want_seek = npc_query.seek(snap, eng.cfg, eng.bank)
    got_seek = eng.npc_seek(out=seek_outs)
    for g, w, nm in zip(got_seek, want_seek, ("dist", "move", "target")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, nm)
        assert np.array_equal(g, w), (what, nm, np.argwhere(g != w)[:5])
    # the optional outputs NULL: the same kind, nothing else written
    kind, where = eng.npc_options_kind()
    assert np.array_equal(kind.cpu().numpy(), want[0]), what
    assert np.array_equal(where.cpu().numpy(), want[3]), what
    import torch
    from optimax_rogue_amd.engine import _ptr
    bare = torch.full_like(kind, 0xEE)
    eng._call("orx_npc_options", _ptr(bare), None, None, None, eng.B, eng._stream())
    assert torch.equal(bare, kind), what
    move = torch.full_like(got_seek[1], 0x6E)
    eng._call("orx_npc_seek", _ptr(eng.pair_field), None, _ptr(move), None, eng.B, eng._stream())
    assert torch.equal(move, got_seek[1]), what
    # the Python layers on top: torch ops equal their numpy twins
    assert np.array_equal(eng.npc_action_mask().cpu().numpy(),
                          npc_query.action_mask(want[0], want[3])), what
    assert np.array_equal(eng.npc_hunt_moves().cpu().numpy(),
                          npc_query.hunt_moves(want[0], want_seek[1], want_seek[2])), what
    return want[0], want[3]


# -- 6. kernel == numpy reference, bit for bit ------------------------------------
@pytest.mark.parametrize("name", list(CFGS))
def test_kernels_equal_the_reference(name):
    """Snapshots after 0, 7 and 40 ticks of random play with random tables, at
    B = 1, 65 and 301; fresh outputs, an ``out=`` reuse, and the optional
    outputs NULL."""
    import torch
    from optimax_rogue_amd import enums as E
    cfg, lay = CFGS[name], _layouts(name)
    seen_kinds, seen_where = set(), set()
    for B in (1, 65, B301):
        eng = _engine(cfg, B, 5100 + B, layouts=lay)
        gen = torch.Generator().manual_seed(5200 + B)
        outs = seek_outs = None
        for more in (0, 7, 33):
            _random_play(eng, more, gen)
            kind, where = _check_against_reference(eng, (name, B, more), outs, seek_outs)
            if outs is None:   # the next snapshot reuses these
                outs, seek_outs = eng.npc_options(), eng.npc_seek()
                for t in outs + seek_outs:
                    t.fill_(0x5A)
            seen_kinds |= set(np.unique(kind & E.NPC_OUT_MASK).tolist())
            seen_where |= set(np.unique(where).tolist())
    if name in ("k6", "k16", "k40", "bank", "stock"):
        assert {E.NPC_OUT_REST, E.NPC_OUT_BLOCKED, E.NPC_OUT_STEP, E.NPC_OUT_FROZEN,
                E.NPC_OUT_ATTACK_NPC} <= seen_kinds, (name, seen_kinds)
    if name in ("unwatched", "gone"):
        other = E.NPC_DEPTH_UNWATCHED if name == "unwatched" else E.NPC_DEPTH_GONE
        assert {E.NPC_DEPTH_WATCHED, other} <= seen_where, (name, seen_where)


@pytest.mark.parametrize("name", ("room", "unwatched", "gone"))
def test_hand_built_states_through_load_snapshot(name):
    """The hand-built states of tests/npc_query_cases.py (one per row of the
    header's rule table), loaded into an engine: the kernels give the
    expectations written from the header, and the reference."""
    case = hand_states()[name]
    B = len(case["where"])
    eng = _engine(case["cfg"], B, 1)
    eng.load_snapshot(case["snap"])
    kind, target, amount, where = (t.cpu().numpy() for t in eng.npc_options())
    assert list(where) == case["where"]
    for (b, k, m), want in case["expect"].items():
        got = (int(kind[k, b, m]), int(target[k, b, m]), int(amount[k, b, m]))
        assert got == want, (name, b, k, m, got, want)
    dist, move, tgt = (t.cpu().numpy() for t in eng.npc_seek())
    for (nm, b, k), want in hand_seek().items():
        if nm == name:
            got = tuple((int(dist[k, b, c]), int(move[k, b, c]), int(tgt[k, b, c]))
                        for c in range(3))
            assert got == want, (name, b, k, got, want)
    assert (int(dist[0, 0, 3]), int(move[0, 0, 3]), int(tgt[0, 0, 3])) == ABSENT
    _check_against_reference(eng, name)


# -- 7. query == engine ------------------------------------------------------------
@pytest.mark.parametrize("name", ("k6", "k30"))
def test_prediction_is_what_the_engine_plays(name):
    """301 games; for each move every game picks a live slot, one snapshot is
    reloaded and stepped with the players on Stay and a table that is all Stay
    but for that byte: the event records (move, attack with its target, death)
    and the health taken equal the prediction."""
    import torch
    from optimax_rogue_amd import enums as E
    cfg = CFGS["k6"] if name == "k6" else dict(BASE_CFG, width=12, height=12, n_npcs=30,
                                               npc_health=1)
    K = cfg["n_npcs"]
    eng = _engine(cfg, B301, 5300)
    gen = torch.Generator().manual_seed(5301)
    _random_play(eng, 6, gen)
    snap = eng.snapshot()
    nd = 0
    alive = E.npc_alive_bits(snap["npc_alive"], K)                     # [K, B]
    playing = (snap["status"] == 1) & alive.any(axis=0)
    rs = np.random.RandomState(5302)
    stay = torch.full((B301, 2), 5, dtype=torch.int8, device=eng.device)
    seen = {}
    for m in range(1, 6):
        eng.load_snapshot(snap)
        kind, target, amount, _ = (t.cpu().numpy() for t in eng.npc_options())
        # a live slot per game (slot 0 where there is none: its byte is not looked at)
        pick = np.array([rs.choice(np.flatnonzero(alive[:, b])) if alive[:, b].any() else 0
                         for b in range(B301)])
        tab = np.full((K, B301), 5, np.int8)
        tab[pick, np.arange(B301)] = m
        _, ev, nev = eng.step(stay, events=True,
                              npc_moves=torch.from_numpy(tab).to(eng.device))
        ev, nev = ev.cpu().numpy(), nev.cpu().numpy()
        post = eng.snapshot()
        post_alive = E.npc_alive_bits(post["npc_alive"], K)
        for b in np.flatnonzero(playing):
            k = int(pick[b])
            iden = 3 + k
            kd, tg, am = int(kind[k, b, m]), int(target[k, b, m]), int(amount[k, b, m])
            out, lethal = kd & E.NPC_OUT_MASK, bool(kd & E.NPC_OUT_LETHAL)
            x, y = int(snap["npc_pos"][k, b]) & 0xFF, int(snap["npc_pos"][k, b]) >> 8
            dx, dy = {1: (0, -1), 2: (1, 0), 3: (0, 1), 4: (-1, 0), 5: (0, 0)}[m]
            want = []
            if out == E.NPC_OUT_STEP:
                want = [(E.EV_POSITION, iden, nd, (x + dx) | (y + dy) << 16)]
            elif out == E.NPC_OUT_STAIRS:
                want = [(E.EV_DEATH, iden, 0, 0)]
            elif out in (E.NPC_OUT_ATTACK_NPC, E.NPC_OUT_ATTACK_PLAYER):
                want = [(E.EV_COMBAT, iden, tg, int(E.CombatFlag.Block))]
                if lethal and tg >= 3:
                    want.append((E.EV_DEATH, tg, 0, 0))
                if tg >= 3:
                    before = int(snap["npc_health"][tg - 3, b])
                    assert lethal == (am >= before > 0)
                    if lethal:
                        assert not post_alive[tg - 3, b]
                    else:
                        assert int(post["npc_health"][tg - 3, b]) == before - am
                else:
                    before = int(snap["p_health"][tg - 1, b])
                    assert int(post["p_health"][tg - 1, b]) == before - am
                    assert lethal == (am >= before > 0)
            else:
                assert out in (E.NPC_OUT_REST, E.NPC_OUT_FROZEN, E.NPC_OUT_BLOCKED), (m, b, out)
                assert (out == E.NPC_OUT_REST) == (m == 5)
            got = [tuple(int(v) for v in r) for r in ev[b, : nev[b]]]
            assert got == want, (name, m, b, k, E.NPC_OUT_NAMES[out], got, want)
            assert bool(post_alive[k, b]) == (out != E.NPC_OUT_STAIRS)
            nm = E.NPC_OUT_NAMES[out]
            seen[nm] = seen.get(nm, 0) + 1
            if lethal:
                seen["LETHAL"] = seen.get("LETHAL", 0) + 1
    need = {"REST", "STEP", "BLOCKED", "ATTACK_NPC", "ATTACK_PLAYER"}
    assert need <= set(seen) and playing.sum() > 200, (name, seen)
    if name == "k30":   # (crowded, health 1: every hit on an NPC kills)
        assert {"LETHAL", "STAIRS", "FROZEN"} <= set(seen), seen


# -- 8. the mask is the engine's -----------------------------------------------------
@pytest.mark.parametrize("name", ("k6", "k17", "bank"))
def test_masked_table_plays_the_same_game(name):
    """Two engines with one seed, 40 ticks of a random table and random player
    actions: one plays the table, the other the table with every byte the
    mask refuses replaced by Stay.  Their states are equal after every tick."""
    import torch
    from golden_util import compare_state
    cfg, lay = CFGS[name], _layouts(name)
    a, b = _engine(cfg, B301, 5400, layouts=lay), _engine(cfg, B301, 5400, layouts=lay)
    K = a.K
    gen = torch.Generator().manual_seed(5401)
    refused = 0
    for t in range(40):
        act = torch.randint(1, 6, (B301, 2), generator=gen, dtype=torch.int8).to(a.device)
        tab = torch.randint(1, 6, (K, B301), generator=gen, dtype=torch.int8).to(a.device)
        mask = b.npc_action_mask()
        allowed = torch.gather(mask, 2, (tab.to(torch.int64) - 1).unsqueeze(2)).squeeze(2)
        refused += int((~allowed).sum())
        a.step(act, npc_moves=tab)
        b.step(act, npc_moves=torch.where(allowed, tab, torch.full_like(tab, 5)))
        sa, sb = a.snapshot(), b.snapshot()
        compare_state(sa, sb, K, f"{name} t={t + 1}")
        compare_state(sb, sa, K, f"{name} t={t + 1}")
    assert refused > 1000, refused


# -- 9. pursuit round a wall ---------------------------------------------------------
def _wall_layout():
    """9 x 8: a Wall border, a wall down column 4 with its gap at the bottom
    row, the staircase in the top left corner."""
    t = np.ones((9, 8), np.uint8)
    t[[0, -1], :] = 2
    t[:, [0, -1]] = 2
    t[4, 1:6] = 2
    t[1, 1] = 3
    return t[None]


def _wall_state(npcs):
    """Player 1 at (6, 2) behind the wall, player 2 beyond it at (7, 1), both
    with health 100; ``npcs``: (x, y) per slot, health 3."""
    K = len(npcs)
    snap = {f: np.zeros((2, 1), np.int32) for f in ("p_depth", "p_layout")}
    snap["p_x"], snap["p_y"] = np.array([[6], [7]], np.int32), np.array([[2], [1]], np.int32)
    snap["p_health"] = np.full((2, 1), 100, np.int32)
    snap["st_x"] = snap["st_y"] = np.ones((2, 1), np.int32)
    snap["npc_pos"] = np.array([[x | y << 8] for x, y in npcs], np.uint16)
    snap["npc_health"] = np.full((K, 1), 3, np.int8)
    snap["npc_alive"] = np.array([(1 << K) - 1], np.uint32)
    snap["status"], snap["tick"] = np.ones(1, np.int32), np.ones(1, np.int32)
    return snap


def test_pursuit_walks_round_a_wall():
    """Under ``npc_hunt_moves`` the walking distance to player 1 drops by
    exactly 1 per tick until it is 1, then player 1 loses npc_damage -
    npc_armor per tick; the built-in CHASE on the same state stops at the
    wall; a second NPC standing in the corridor is never attacked."""
    import torch
    cfg = dict(BASE_CFG, width=9, height=8, n_npcs=1, max_ticks=200, npc_damage=3, npc_armor=1)
    lay = _wall_layout()
    eng = _engine(cfg, 1, 5500, layouts=lay)
    eng.load_snapshot(_wall_state([(2, 2)]))
    stay = torch.full((1, 2), 5, dtype=torch.int8, device=eng.device)
    dists, healths = [], []
    for t in range(16):
        dists.append(int(eng.npc_seek()[0][0, 0, 0]))
        healths.append(int(eng.p_health[0, 0]))
        eng.step(stay, npc_moves=eng.npc_hunt_moves())
    # (2, 2) -> (2, 6) -> (6, 6) -> (6, 3): 12 moves from the player's cell
    assert dists[:12] == list(range(12, 0, -1)) and set(dists[12:]) == {1}, dists
    assert healths[:12] == [100] * 12, healths
    assert [healths[i] - healths[i + 1] for i in range(11, 15)] == [2] * 4, healths
    assert int(eng.p_health[1, 0]) == 100 and int(eng.status[0]) == 1

    chase = _engine(dict(cfg, npc_policy=2), 1, 5500, layouts=lay)
    chase.load_snapshot(_wall_state([(2, 2)]))
    for t in range(16):
        chase.step(stay)
    assert int(chase.npc_seek()[0][0, 0, 0]) > 1 and int(chase.p_health[0, 0]) == 100
    assert int(chase.npc_pos[0, 0]) == 3 | 2 << 8   # (it stands at the wall)

    # a fellow NPC in the gap of the wall: both hunt -- nobody hits the other, the
    # first arrives; then it holds still -- the second waits behind it
    for hold in (False, True):
        two = _engine(dict(cfg, n_npcs=2), 1, 5500, layouts=lay)
        two.load_snapshot(_wall_state([(2, 2), (4, 6)]))
        for t in range(16):
            table = two.npc_hunt_moves()
            if hold:
                table[1] = 5
            _, ev, nev = two.step(stay, events=True, npc_moves=table)
            for r in ev[0, : int(nev[0])].tolist():
                assert not (r[0] == 1 and r[2] >= 3), (hold, t, r)
        assert two.npc_health[:2, 0].tolist() == [3, 3]
        assert (int(two.p_health[0, 0]) < 100) == (not hold)


# -- 10. closed loop in a graph -------------------------------------------------------
@pytest.mark.parametrize("name", ("k6", "bank"))
def test_closed_loop_in_a_graph(name):
    """``npc_hunt_moves`` -> a static table -> ``VecEnv.step(a, npc_moves=
    table)`` captured once and replayed 20 times equals the eager loop."""
    import torch
    from optimax_rogue_amd import VecEnv
    cfg = env_config(CFGS[name], _layouts(name))
    T, seed = 20, 5600
    mk = lambda **kw: VecEnv(cfg, B301, seed=seed, opponent=1, check_actions=False, **kw)
    eager, graphed = mk(), mk(out_buffers=1)
    dev = eager.device
    gen = torch.Generator().manual_seed(5601)
    a = torch.randint(1, 6, (T + 1, B301), generator=gen, dtype=torch.int64).to(dev)
    outs = []
    for t in range(T + 1):
        outs.append([v.clone() for v in eager.step(a[t], npc_moves=eager.npc_hunt_moves())])
    sa = a[0].clone()
    table = graphed.npc_hunt_moves().clone()   # (also builds a bank's pair table)
    first = graphed.step(sa, npc_moves=table)  # (settles the host-side launch blocks)
    for got, want in zip(first, outs[0]):
        assert torch.equal(got, want)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            table.copy_(graphed.npc_hunt_moves())
            obs, reward, done, status = graphed.step(sa, npc_moves=table)
    torch.cuda.current_stream(dev).wait_stream(s)
    for t in range(1, T + 1):
        sa.copy_(a[t])
        g.replay()
        torch.cuda.synchronize(dev)
        for got, want in zip((obs, reward, done, status), outs[t]):
            assert torch.equal(got, want), (name, t)
    from golden_util import compare_state
    compare_state(graphed.engine.snapshot(), eager.engine.snapshot(), cfg.n_npcs, name)


def test_python_layers_refuse_what_the_kernels_would_not_survive():
    import torch
    eng = _engine(CFGS["k6"], 8, 1)
    kind, target, amount, where = eng.npc_options()
    for bad in ((kind, target, amount), (kind, target, amount, where[:4]),
                (kind.to(torch.int16), target, amount, where),
                (kind[:, :4], target, amount, where), (kind, target, target, where),
                (kind.cpu(), target, amount, where)):
        with pytest.raises(ValueError):
            eng.npc_options(out=bad)
    dist, move, tgt = eng.npc_seek()
    for bad in ((dist, move), (dist.to(torch.int64), move, tgt), (dist[:3], move, tgt)):
        with pytest.raises(ValueError):
            eng.npc_seek(out=bad)
    none = _engine(dict(CFGS["k6"], n_npcs=0), 8, 1)
    for fn in (none.npc_options, none.npc_seek, none.npc_action_mask, none.npc_hunt_moves):
        with pytest.raises(ValueError):
            fn()
