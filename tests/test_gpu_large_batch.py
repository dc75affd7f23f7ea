"""Full-size batches of BASELINE.json on the device, held to the oracle on sampled environments:
the north-star batch (65 536 environments, four-environments-per-wave kernel picked by AUTO) and the topology groups of
configs[4] (NSFNET / JPN12 / US14) at 32 768 environments each, the per-GPU batch of that configuration."""
import numpy as np
import pytest

from conftest import load_topology, oracle_env_from_kwargs
from gpu_support import decisions_match, device_log_fixture, drive, oracle_run, rmsa_env, same_bytes, snapshot, state_matches  # noqa: F401

pytestmark = pytest.mark.gpu


def _check_samples(env, name, kw, policy, warm, n, tr, samples):
    """the sampled environments after `warm` steps and n more (tr: the outputs of the n) against the oracle"""
    snap = snapshot(env, save_state=False)
    for i in samples:
        (_, want), final = oracle_run(name, tuple(sorted(kw.items())), kw["seed"] + i, policy, (warm, n))
        decisions_match(tr, i, want, ("act_path", "act_slot", "accepted"), i)
        state_matches(snap, i, final, i)


def test_north_star_batch_65536(device_log_in_oracle):
    """B = 65 536 on NSFNET-320 (the batch BASELINE.json's north_star quotes its target on, bench.py's headline): AUTO must
    pick the four-environments-per-wave kernel; a long launch (ticket queue over 16 384 quads), short launches (static
    striding) and a long launch with outputs; 12 sampled environments -- first / last of the batch, of a quad, of the
    resident set -- bit-exact against the oracle on decisions, occupancy, clock, counters and link statistics."""
    name = "nsfnet_chen_5-paths_6-modulations"
    kw = dict(num_spectrum_resources=320, load=50, mean_service_holding_time=25, episode_length=1000, seed=10)
    B = 65536
    env = rmsa_env(name, B, **kw)
    env.run("sap_ff", 150)
    # (150 steps, full statistics, no per-step link outputs: the instantiation that defers the links' float64 updates)
    assert env.last_kernel().startswith("orlg_rmsa_group_kernel<5,2,false,true>"), env.last_kernel()
    for _ in range(2):
        env.run("sap_ff", 3)
    tr = env.run("sap_ff", 120, outputs=("act_path", "act_slot", "accepted"))
    cnt = env.counters()
    assert np.all(cnt["services_processed"] == 277)
    assert np.array_equal(cnt["services_accepted"] >= tr["accepted"].sum(axis=0), np.ones(B, bool))
    samples = (0, 1, 2, 3, 4, 11263, 11264, 16383, 32768, 50001, 65532, 65535)
    _check_samples(env, name, kw, "sap_ff", 156, 120, tr, samples)
    red, _ = env.reduce_counters()
    assert red["num_envs"] == B and red["services_processed"] == 277 * B
    assert red["services_accepted"] == int(cnt["services_accepted"].sum())
    env.close()


@pytest.mark.parametrize("name", ["nsfnet_chen_5-paths_6-modulations", "jpn12_5-paths_6-modulations", "us14_3-paths_6-modulations"])
def test_mixed_topology_groups_32768(name, device_log_in_oracle):
    """The three topology groups of BASELINE configs[4] (JPN12 stands in for "JPN48": SURVEY 0.7) at that configuration's
    per-GPU batch, 262 144 / 8 = 32 768 environments, on the kernel AUTO picks for it (four environments per wave); sampled
    environments -- first / last of the batch, of a quad, of the resident set, of the ticket queue -- against the oracle."""
    kw = dict(num_spectrum_resources=320, load=50, mean_service_holding_time=25, episode_length=1000, seed=10)
    B = 32768
    env = rmsa_env(name, B, **kw)
    env.run("sap_ff", 200)
    tr = env.run("sap_ff", 150, outputs=("act_path", "act_slot", "accepted"))
    assert env.last_kernel().startswith("orlg_rmsa_group_kernel"), env.last_kernel()
    _check_samples(env, name, kw, "sap_ff", 200, 150, tr, (0, 3, 4, 4095, 4096, 11263, 11264, 16384, 20001, 32764, 32767))
    red, _ = env.reduce_counters()
    assert red["num_envs"] == B and red["services_processed"] == 351 * B
    env.close()


@pytest.mark.parametrize("B,n,outs", [(20004, 400, ("act_path", "act_slot", "accepted", "done")), (65536, 1000, ("accepted",))])
def test_tickets_in_chunks_of_steps(device_log_in_oracle, B, n, outs):
    """Long launches of batches beyond one round of resident waves hand a quad's launch out in CHUNKS of steps (the work queue of
    orlg_rmsa_group_kernel: ticket = (quad, chunk); the wave that draws a chunk waits for the quad's previous chunk to be
    published -- agent-scope release / acquire, the two waves may sit on different XCDs).  B = 20 004 (5 001 quads on 3 072 wave
    slots: every wave hands quads over, under the uneven load of a last partial round; a partial last quad), three launches of
    400 steps with per-step outputs (and the headline's batch, B = 65 536, three launches of 1000 steps), against the same launches with whole-launch tickets (ORLG_NO_CHUNKS): outputs at their
    step's row, counters, link statistics and the saved state byte for byte; forced to 7 chunks as well; spot checks against
    the oracle."""
    nsfnet = load_topology("nsfnet_chen_5-paths_6-modulations")
    kw = dict(num_spectrum_resources=320, load=50, mean_service_holding_time=25, episode_length=300, seed=901)
    run = lambda env_vars: drive(lambda: rmsa_env(nsfnet, B, "group", **kw), (n,) * 3, outs, env_vars=env_vars, policy="sap_ff")
    ref = run({"ORLG_NO_CHUNKS": "1"})
    assert ref["said"][-1].endswith("chunks=1"), ref["said"][-1]
    for env_vars in ({}, {"ORLG_GROUP_CHUNKS": "7"}):
        got = run(env_vars)
        assert not got["said"][-1].endswith("chunks=1"), got["said"][-1]
        same_bytes(got["tr"], ref["tr"], (env_vars, "outputs"))
        same_bytes(got["snap"], ref["snap"], (env_vars, "state"))
    for i in (0, 4999, 12345, B - 1):
        o = oracle_env_from_kwargs(nsfnet, kw, seed=901 + i)
        tr = o.run("sap_ff", 3 * n, reset_on_done=True)
        assert np.array_equal(ref["tr"]["accepted"][:, i], tr["accepted"]), i
        o.close()
