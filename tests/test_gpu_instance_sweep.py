"""GPU: every rollout and replay kernel instance against the oracle, one small
case per request of instance_sweep.py (test_instance_sweep.py shows on the CPU
that the requests reach every instance of the lists, on any device, and that
each run contains what its instance exists for).  257 games on a 12 x 10 grid,
three launches of 20 ticks at max_ticks 24: every tick's rows and actions and
the state after each launch, bit-exact (all of it is integer)."""
import numpy as np
import pytest

import instance_sweep as sw
from golden_util import compare_state


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return sw.plans_of(sw.build_plan_main(tmp_path_factory.mktemp("plan")), sw.REQUESTS)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(sw.REQUESTS)), ids=sw.request_id)
def test_instance_vs_oracle(i, plans, oracle_lib, monkeypatch):
    import torch
    from optimax_rogue_amd import EnvConfig
    from optimax_rogue_amd.engine import BatchedEngine, decode_compact, obs_rows
    from optimax_rogue_amd.enums import OBS_COMPACT, OBS_INT32
    r, plan, where = sw.REQUESTS[i], plans[i], sw.request_id(i)
    assert sw.instance_of(plan, r.cfg, r) == r.want, where
    for k in sw.PLAN_OVERRIDES:
        monkeypatch.delenv(k, raising=False)
    for k, v in r.env.items():
        monkeypatch.setenv(k, v)
    dev = torch.device("cuda", 0)
    layouts = sw.layouts_of(r)

    ora = sw.new_oracle(oracle_lib, r)
    eng = BatchedEngine(EnvConfig.from_dict(r.cfg, layouts=layouts), sw.B, seed=r.seed,
                        game_offset=r.offset, device=dev)

    def same_state(what):
        got, want = eng.snapshot(), ora_state[0]
        compare_state(got, want, ora.K, f"{where} {what}")
        compare_state(want, got, ora.K, f"{where} {what} (oracle against engine)")

    ora_state = [ora.export()]
    same_state("reset")

    # the launch is the one the plan names (orx_rollout_shape has no row format)
    if r.kind == "rollout" and r.fmt != "compact":
        shape = eng.rollout_shape(*r.bots, trajectory=r.fmt is not None and r.act)
        assert shape == dict(games_per_wave=plan["lanes"],
                             lanes_per_game=2 if plan["form"] == "paired" else 1,
                             nontemporal=bool(plan["nt"]), threads_per_block=plan["threads"],
                             lds_bytes=plan["lds_bytes"]), (where, plan)

    fmt = OBS_COMPACT if r.fmt == "compact" else OBS_INT32
    n = sw.N_TICKS
    obs = act = None
    if r.fmt is not None:
        obs = torch.full((n, obs_rows(fmt), sw.B), -7, dtype=torch.int32, device=dev)
    if r.kind == "rollout" and r.act:
        act = torch.full((n, sw.B, 2), -7, dtype=torch.int8, device=dev)
    for c, (want_act, want_obs, state) in enumerate(sw.run_oracle(oracle_lib, r)):
        if r.kind == "rollout":
            eng.rollout(n, *r.bots, obs=obs, act=act, obs_format=fmt)
        else:
            eng.step_n(torch.from_numpy(want_act).to(dev).contiguous(), obs=obs, obs_format=fmt)
        if obs is not None:
            got = (decode_compact(obs) if r.fmt == "compact" else obs).cpu().numpy()
            bad = np.argwhere(got != want_obs)
            assert not len(bad), f"{where} launch {c}: rows differ at [tick, field, game] {bad[:5]}"
        if act is not None:
            bad = np.argwhere(act.cpu().numpy() != want_act)
            assert not len(bad), f"{where} launch {c}: actions differ at [tick, game, player] {bad[:5]}"
        ora_state[0] = state
        same_state(f"after launch {c}")
    torch.cuda.synchronize()
