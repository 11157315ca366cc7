"""Generates the given-NPC-move fixtures in tests/golden/given/ from the
REFERENCE updater (include/orx_npc.h: the tick with the NPCs' moves supplied
by the caller).

Run in the build container only (it needs /root/reference, as make_golden.py):

    python tests/golden/make_given.py [case ...]

It imports make_golden as a module and builds the same harness around the
unmodified reference.  Only the updater's enemy-AI hook
``Updater.decide_npc_move`` (updater.py:165-178) is replaced: ``GivenUpdater``
applies the engine's three guards (an NPC on a depth without a dungeon stays;
an NPC on a depth where a player stands next to a staircase tile stays; a move
into a blocked cell becomes Stay) and then returns ``table[t][ent.iden -
3][g]`` -- t the step of the run (autoreset steps count), g the game.  The
reference's ``update`` does everything else: the shuffles, handle_move, the
death sweep.  ``table`` is uniform over Move 1..5 from a seeded numpy
Generator and is stored with the usual fixture arrays as ``npc_moves`` int8
[T][K][G].  The fixtures' cfg keeps ``npc_policy`` 0: the entry points do not
read it.

The fixtures go to tests/golden/given/, not tests/golden/ (golden_util's
case_names() lists that directory for the existing parametrised tests).  They
are written as zip archives with a fixed timestamp, so a rerun reproduces them
byte for byte.
"""
from __future__ import annotations

import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

OUT = os.path.join(HERE, "given")

CASES = {
    # register NPCs (K <= 8), keyed mode
    "given_regs_8x8": dict(cfg=dict(width=8, height=8, n_npcs=6, max_ticks=50), seed=81,
                           games=14, ticks=160, table_seed=1081),
    # dense NPCs (the occupancy-grid form)
    "given_dense_12x12": dict(cfg=dict(width=12, height=12, n_npcs=30, npc_health=2,
                                       max_ticks=50), seed=82, games=12, ticks=130,
                              table_seed=1082),
    # an explicit-grid bank: interior walls, open borders
    "given_bank_9x8": dict(cfg=dict(width=9, height=8, n_npcs=6, max_ticks=50,
                                    layouts=mg.make_layouts(9, 8, 4, 106, open_border=True)),
                           seed=83, games=14, ticks=160, table_seed=1083),
    # stock-seed mode: nothing is drawn between the two shuffles
    "given_stock_8x8": dict(cfg=dict(rng=1, width=8, height=8, n_npcs=6, max_ticks=50,
                                     policy=(1, 2)), seed=8400, games=14, ticks=160,
                            table_seed=1084),
}


def next_to_stairs(R, dung, p):
    for m in (R.moves.Move.Up, R.moves.Move.Right, R.moves.Move.Down, R.moves.Move.Left):
        x, y = R.updater.calculate_pos(p.x, p.y, m)
        if 0 <= x < dung.width and 0 <= y < dung.height \
                and dung.tiles[x, y] == R.world.Tile.StaircaseDown:
            return True
    return False


def given_harness(table, first_gid):
    """make_golden.Harness whose updater's decide_npc_move reads ``table``."""

    class GivenHarness(mg.Harness):
        def __init__(self, R, cfg, seed, game_id):
            super().__init__(R, cfg, seed, game_id)
            harness = self
            Move = R.moves.Move
            self.t = 0
            self.g = game_id - first_gid
            self.stair_deaths = 0

            class GivenUpdater(R.updater.Updater):
                """The reference's Updater with only its enemy-AI hook
                overridden: the guards, then the table."""

                def decide_npc_move(self, game_state, ent, result):
                    if ent.depth not in game_state.world.dungeons:
                        return Move.Stay
                    dung = game_state.world.get_at_depth(ent.depth)
                    players = [p for p in (game_state.player_1, game_state.player_2)
                               if p.depth == ent.depth]
                    if any(next_to_stairs(R, dung, p) for p in players):
                        return Move.Stay
                    move = Move(int(table[harness.t, ent.iden - 3, harness.g]))
                    if dung.is_blocked(*R.updater.calculate_pos(ent.x, ent.y, move)):
                        return Move.Stay
                    return move

            old = self.updater
            self.updater = GivenUpdater(old.dgen, old.despawn_strat, old.max_ticks)

        def step(self, acts):
            before = {e.iden: e for e in self.gs.entities}
            try:
                events = super().step(acts)
            finally:
                self.t += 1
            # an NPC removed with health left died on a staircase (updater.py:263-270)
            self.stair_deaths += sum(1 for ty, i, _, _ in events
                                     if ty == 2 and i >= 3 and before[i].health > 0)
            return events

    return GivenHarness


def tally(events):
    out = {}
    for t_, i_, a_, b_ in events.tolist():
        who = "npc" if i_ >= 3 else "player"
        if t_ == 1:
            k = f"{who}->{'npc' if a_ >= 3 else 'player'}:" \
                f"{['', 'Block', 'Ambush', 'Flee', 'Parry'][b_]}"
        elif t_ == 3:
            k = f"{who} move"
        elif t_ == 2:
            k = "npc death"
        else:
            k = f"type{t_}"
        out[k] = out.get(k, 0) + 1
    return dict(sorted(out.items()))


def covers(tl, stair_deaths):
    """The condition on a fixture: at least one of each thing a given move can do."""
    need = ["npc move", "npc->npc:Block", "npc->npc:Ambush", "npc->npc:Flee"]
    return (all(tl.get(k, 0) > 0 for k in need) and stair_deaths > 0
            and any(tl.get(f"npc->player:{f}", 0) for f in ("Block", "Ambush", "Flee"))
            and any(tl.get(f"player->npc:{f}", 0) for f in ("Block", "Ambush", "Flee")))


def write_npz(path, arrays):
    """np.savez_compressed with a fixed timestamp per member (reproducible bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[name]), allow_pickle=False)


def run_case(R, name, spec):
    cfg = dict(mg.DEFAULT_CFG)
    cfg.update(spec["cfg"])
    T, G, K = spec["ticks"], spec["games"], cfg["n_npcs"]
    table = np.random.default_rng(spec["table_seed"]).integers(1, 6, size=(T, K, G),
                                                               dtype=np.int8)
    made = []
    cls = given_harness(table, spec.get("offset", 0))

    class Tracked(cls):
        def __init__(self, *a):
            super().__init__(*a)
            made.append(self)

    saved = mg.Harness, mg.HERE
    with tempfile.TemporaryDirectory() as tmp:
        mg.Harness, mg.HERE = Tracked, tmp
        try:
            mg.run_case(R, name, {k: v for k, v in spec.items() if k != "table_seed"})
        finally:
            mg.Harness, mg.HERE = saved
        z = np.load(os.path.join(tmp, f"{name}.npz"))
        arrays = {k: z[k] for k in z.files}
    arrays["npc_moves"] = table
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.npz")
    write_npz(path, arrays)
    tl = tally(arrays["events"])
    deaths = sum(h.stair_deaths for h in made)
    ok = covers(tl, deaths)
    print(f"    {tl}, npc staircase deaths={deaths}, bytes={os.path.getsize(path)}, "
          f"covers={'yes' if ok else 'NO'}")
    return ok


def main():
    R = mg.import_reference()
    only = sys.argv[1:]
    ok = True
    for name, spec in CASES.items():
        if not only or name in only:
            ok = run_case(R, name, spec) and ok
    if not ok:
        raise SystemExit("a fixture misses one of the events it must hold: choose other seeds")


if __name__ == "__main__":
    main()
