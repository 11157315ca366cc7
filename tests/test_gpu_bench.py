"""GPU: a plain `bench.py` run and its `--dump-outputs` files.  The plain line
carries the headline alone (no extras, no CPU baseline), and the files hold
what the last timed step wrote: the same launches issued here in-process
(same seed, shards, warmup + steps) give the same rows, sums and returns."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_step(tmp_path):
    import torch
    from optimax_rogue_amd import EnvConfig
    from optimax_rogue_amd.engine import StreamShardedEngine
    B, T, steps, warmup = 4099, 128, 3, 1      # odd batch: unequal stream shards
    out = str(tmp_path / "dump")
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--batch", str(B), "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", out],
                       env=env, capture_output=True, text=True, timeout=110, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(B * T * 1e3 / line["ms_per_step"])
    assert line["extras"] is None and line["cpu_baseline"] is None
    got = {n[:-4]: np.load(os.path.join(out, n)) for n in os.listdir(out)}
    assert sorted(got) == ["act", "episode_returns", "game_ids", "obs", "obs_sum"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    # the same launches in this process
    dev = torch.device("cuda", 0)
    eng = StreamShardedEngine(EnvConfig.c3(), B, seed=3, device=dev, n_streams=2)
    obs, act = eng.trajectory_buffers(T)
    launch = eng.rollout_launcher(T, 1, 1, obs=obs, act=act)
    eng.fork()
    for _ in range(warmup + steps):
        launch()
    eng.join()
    torch.cuda.synchronize()
    want_obs = torch.cat(obs, dim=2).cpu().numpy()
    want_act = torch.cat(act, dim=1).cpu().numpy()
    ids = got["game_ids"].astype(np.int64)
    assert len(ids) == 2048 and len(np.unique(ids)) == 2048 and ids.min() >= 0 and ids.max() < B
    assert np.array_equal(got["obs"], want_obs[:, :, ids])
    assert np.array_equal(got["act"], want_act[:, ids, :])
    assert np.array_equal(got["obs_sum"], want_obs.astype(np.int64).sum(axis=2))
    assert np.array_equal(got["episode_returns"], eng.episode_returns().cpu().numpy())
    from optimax_rogue_amd import OBS_FIELDS
    assert got["obs"][:, OBS_FIELDS.index("tick")].max() >= T   # (the rows are not blank)
