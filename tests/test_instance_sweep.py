"""CPU: the ledger of rollout and replay kernel instances (instance_sweep.py)
against the macro text of orx_engine.hip, its requests against the launch plan
(tests/plan_main.cpp, built as test_plan.py builds it) on three devices, and
each request's run on the oracle against the list of things the instance
exists for.  test_gpu_instance_sweep.py then runs every request on the GPU."""
import os
import re

import pytest

import instance_sweep as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICES = ((1024, 160 * 1024), (64, 64 * 1024), (4096, 160 * 1024))


# -- the macro text ---------------------------------------------------------
def _macros():
    """name -> (parameters, body) of every ORX_*_LIST* macro of orx_engine.hip."""
    text = open(os.path.join(ROOT, "optimax_rogue_amd", "csrc", "orx_engine.hip")).read()
    text = text.replace("\\\n", " ")
    out = {}
    for m in re.finditer(r"^#define (ORX_\w*LIST\w*)\(([^)]*)\)(.*)$", text, re.M):
        out[m.group(1)] = ([p.strip() for p in m.group(2).split(",")], m.group(3))
    return out


def _expand(macros, name, args):
    """The argument tuples a list macro passes to X, in order."""
    params, body = macros[name]
    assert len(params) == len(args), (name, args)
    bind = dict(zip(params, args))
    out = []
    for m in re.finditer(r"(\w+)\(([^()]*)\)", body):
        call = [bind.get(a.strip(), a.strip()) for a in m.group(2).split(",")]
        if bind.get(m.group(1)) == "X":
            out.append(tuple(call))
        else:
            assert m.group(1) in macros, (name, m.group(1))
            out += _expand(macros, m.group(1), call)
    return out


def _value(word):
    return {"true": True, "false": False, "kDense": sw.DENSE, "kStreamAux": True,
            "kPartialAux": False}.get(word, None if not word.isdigit() else int(word))


def _list(macros, name, *args):
    out = [tuple(_value(w) for w in t) for t in _expand(macros, name, ("X",) + args)]
    assert all(v is not None for t in out for v in t), (name, out)
    return tuple(out)


def test_lists_are_the_macros():
    """The hand-written lists are what the X-macro lists expand to, in order
    (the dispatch and the explicit instantiations both come from them), and
    the counts are the ones DESIGN.md states."""
    m = _macros()
    assert sw.PAIR_LIST == _list(m, "ORX_PAIR_LIST")
    assert sw.PAIR_LIST_L == sum((_list(m, "ORX_PAIR_LIST_L", n) for n in ("0", "8", "16")), ())
    assert sw.ROLLOUT_LIST == _list(m, "ORX_ROLLOUT_LIST")
    assert sw.NG_LIST == _list(m, "ORX_NG_LIST")
    assert sw.MOV_ROLLOUT_LIST == _list(m, "ORX_MOV_ROLLOUT_LIST")
    assert sw.REPLAY_LIST == _list(m, "ORX_REPLAY_LIST")
    assert [len(l) for l in (sw.PAIR_LIST, sw.PAIR_LIST_L, sw.ROLLOUT_LIST, sw.NG_LIST,
                             sw.MOV_ROLLOUT_LIST, sw.REPLAY_LIST)] == [72, 12, 64, 8, 12, 18]
    led = sw.ledger()
    assert len(led) == len(set(led)) == 186
    # the host side passes exactly these lists to its dispatch macros
    text = open(os.path.join(ROOT, "optimax_rogue_amd", "csrc", "orx_engine.hip")).read()
    for use in ("ORX_PAIR_LIST(ORX_PAIR)", "ORX_ROLLOUT_LIST(ORX_ROLLOUT_AC)",
                "ORX_MOV_ROLLOUT_LIST(ORX_MOV_ROLLOUT)", "ORX_NG_LIST(ORX_MT_ROLLOUT)",
                "ORX_PAIR_LIST_L(ORX_PAIR_LOG, 0) ORX_PAIR_LIST_L(ORX_PAIR_LOG, 8)",
                "ORX_PAIR_LIST_L(ORX_PAIR_LOG, 16)", "ORX_REPLAY_LIST(ORX_REPLAY)"):
        assert use in text, use


def test_traced_names_are_the_ledger():
    """profiles/instances/kernel_names.txt: the rollout and replay kernel names
    of one kernel trace of test_gpu_instance_sweep.py on an MI355X, as the
    trace spells them (the store policy by value: ORX_STREAM_AUX = 2, partial
    lines 0; kDense = 256).  The one check that does not go through
    instance_of: the set is the ledger, and every instance ran at least one
    request's three launches (the second column is its launch count)."""
    path = os.path.join(ROOT, "profiles", "instances", "kernel_names.txt")
    got = dict(l.rstrip("\n").split("\t") for l in open(path))

    def traced(inst):
        name = sw.instance_name(inst)
        for a, b in (("kStreamAux", "2"), ("kPartialAux", "0"), ("kDense", "256")):
            name = name.replace(a, b)
        return name
    assert set(got) == {traced(i) for i in sw.ledger()}
    assert all(int(n) >= sw.N_LAUNCHES for n in got.values())


# -- the plans ----------------------------------------------------------------
@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """device -> one plan (a dict) per request."""
    exe = sw.build_plan_main(tmp_path_factory.mktemp("plan"))
    return {dev: sw.plans_of(exe, sw.REQUESTS, dev) for dev in (None,) + DEVICES}


def test_every_instance_has_a_request(plans):
    """Each request's plan names the instance it was written for; together they
    name every listed instance, and none names a tuple outside the lists (that
    would be a launch ending in ORX_EIO)."""
    got = [sw.instance_of(p, r.cfg, r) for r, p in zip(sw.REQUESTS, plans[DEVICES[0]])]
    for i, (r, inst) in enumerate(zip(sw.REQUESTS, got)):
        assert inst == r.want, "%s: the plan names %s" % (
            sw.request_id(i), inst and sw.instance_name(inst))
    led = set(sw.ledger())
    assert not set(got) - led, sorted(sw.instance_name(i) for i in set(got) - led)
    missing = [sw.instance_name(i) for i in sw.ledger() if i not in set(got)]
    assert not missing, "no request reaches: " + ", ".join(missing)


def test_generic_instances_have_all_three_requests():
    """A generic instance's writer reads the format at run time: no rows,
    int32 rows without the actions, and compact rows with them."""
    for inst in sw.ledger():
        if inst[0] != sw.ROLLOUT or inst[1][1] != 0:
            continue
        forms = {(r.fmt, r.act) for r in sw.REQUESTS if r.want == inst}
        assert forms == {(None, False), ("int32", False), ("compact", True)}, sw.instance_name(inst)


def test_overrides_pin_the_plan(plans):
    """ORX_ROLLOUT_LANES on every paired, one-lane and replay request, and the
    plan is then the same on every device (and without one named)."""
    for i, r in enumerate(sw.REQUESTS):
        if r.want[0] != sw.LANE:
            assert "ORX_ROLLOUT_LANES" in r.env, sw.request_id(i)
        for dev in DEVICES:
            assert plans[dev][i] == plans[None][i], (sw.request_id(i), dev)
        p = plans[None][i]
        assert p["lds_bytes"] <= 64 * 1024            # (no LDS limit raise anywhere)
        assert p["blocks"] == -(-sw.B // (p["threads"] // 64 * p["lanes"]))


def test_requests_are_small_and_distinct():
    assert len({(r.seed, r.offset) for r in sw.REQUESTS}) == len(sw.REQUESTS)
    for r in sw.REQUESTS:
        assert (r.cfg["width"], r.cfg["height"], r.cfg["max_ticks"]) == (12, 10, 24)
        assert r.offset > 0 and r.bank in (0, 3, 4, 5, 6)
        if r.bank:
            lay = sw.bank_layouts(r.bank)
            assert ((lay == 3).sum(axis=(1, 2)) >= 2).all()
            assert ((lay[:, 1:-1, 1:-1] == 2).sum(axis=(1, 2)) >= 3).all()
            assert (lay == 1).sum(axis=(1, 2)).min() >= r.cfg["n_npcs"] + 2
    mov = {r.cfg["npc_policy"] for r in sw.REQUESTS if r.cfg.get("npc_policy")}
    assert mov == {1, 2}
    for pm, bots in ((4, (1, 2)), (5, (2, 1))):
        assert {r.bots for r in sw.REQUESTS if r.want[0] == sw.PAIR and r.want[1][1] == pm} == {bots}


@pytest.mark.parametrize("i", range(len(sw.REQUESTS)), ids=sw.request_id)
def test_oracle_run_contains_what_the_instance_is_for(i, oracle_lib):
    """A condition on the inputs: the oracle's run of the request ends episodes
    by max_ticks and by a win, restarts one inside a launch, descends, and --
    by the instance -- hits an NPC, takes separation damage, picks up an item
    and gains a level, and uses two layouts."""
    r = sw.REQUESTS[i]
    _, seen = sw.run_oracle(oracle_lib, r, witness=True)
    want = sw.wanted_witnesses(r)
    assert want <= seen, "%s lacks %s" % (sw.request_id(i), sorted(want - seen))
