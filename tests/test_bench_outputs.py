"""bench.py: a plain run times the headline only (the sub-records and the CPU baseline are behind --full), and --dump-outputs
writes the state the timed launches leave -- the same arrays a batch stepped the same way in this process reads back."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from conftest import load_topology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_full_and_dump_options():
    a = bench.parse_args([])
    assert not a.full and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out", "--only", "headline"])
    assert a.full and a.dump_outputs == "out"
    with pytest.raises(SystemExit) as e:     # a sub-record alone has no headline outputs to write
        bench.parse_args(["--only", "phy", "--dump-outputs", "out"])
    assert e.value.code == 2


@pytest.mark.gpu
def test_plain_run_dumps_the_state_of_the_timed_batch(tmp_path):
    B, chunk, steps, warm = 1024, 100, 3, 1
    env_vars = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", str(B), "--chunk", str(chunk),
                        "--steps", str(steps), "--warmup", str(warm), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, env=env_vars, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warm
    assert "sub_records" not in d and "cpu_baseline" not in d
    assert d["ms_per_step"] > 0 and abs(d["ms_per_step"] * steps - d["timed_region_s"] * 1e3) < 1e-6 * d["ms_per_step"] * steps
    dump = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert all(a.dtype in (np.float32, np.float64) for a in dump.values())
    assert sum(a.nbytes for a in dump.values()) <= 64 << 20

    # the same batch, stepped the same way in this process (the library only: no torch here)
    from optical_rl_gym_amd import BatchedRMSAEnv
    from optical_rl_gym_amd.batched import COUNTER_NAMES
    env = BatchedRMSAEnv(load_topology(bench.TOPOLOGY), B, **bench.ENV_KW, seed=10, stats_level="full")
    for _ in range(warm + steps):
        env.run("sap_ff", chunk, auto_reset=True)
    c = env.counters()
    assert np.array_equal(dump["env_index"], np.arange(B))
    assert np.array_equal(dump["counters"], np.stack([c[k] for k in COUNTER_NAMES], axis=1).astype(np.float64))
    assert np.array_equal(dump["current_time"], env.current_time())
    req = env.requests()
    assert np.array_equal(dump["pending_request"], np.stack([req[k].astype(np.float64) for k in req.dtype.names], axis=1))
    assert np.array_equal(dump["num_running"], env.num_running().astype(np.float64))
    assert np.array_equal(dump["episodes_done"], env.episodes_done().astype(np.float64))
    gs = env.graph_stats()
    assert np.array_equal(dump["graph_stats"], np.stack([gs[k] for k in ("throughput", "compactness", "last_update")], axis=1))
    red = env.reduce_counters()[1]
    assert np.array_equal(dump["reduced_counters"], red.astype(np.float64))
    assert red[0] == B * (chunk * (steps + warm) + 1) == d["blocking"]["services_processed"]
    s = dump["sample_env_index"].astype(np.int64)
    assert len(s) == 256 and len(np.unique(s)) == 256
    assert np.array_equal(dump["sample_available_slots"], env.available_slots()[s].astype(np.float32))
    ls = env.link_stats()
    assert np.array_equal(dump["sample_link_stats"][..., 0], ls["utilization"][s])
    assert np.array_equal(dump["sample_link_stats"][..., 2], ls["compactness"][s])
    env.close()
