"""Checkpoint / resume of the batched state (orlg_save_state / orlg_load_state): a restored batch continues bit for bit.  Then
what both kinds of handle share on the host -- reseed, set_stream, save / load, the reductions -- with one body for both."""
import numpy as np
import pytest

from conftest import load_golden, load_phy_tables, load_topology, oracle_env_from_kwargs, phy_oracle_from_kwargs
from gpu_support import device_log_fixture, phy_env, rmsa_env, same_bytes, snapshot  # noqa: F401

pytestmark = pytest.mark.gpu


def test_rmsa_save_load_resume(nsfnet):
    kw = dict(num_spectrum_resources=320, load=50, mean_service_holding_time=25, episode_length=100, seed=3)
    outs = ("act_path", "act_slot", "accepted", "arrival", "network_compactness")
    a = rmsa_env(nsfnet, 40, **kw)
    a.run("sap_ff", 170, auto_reset=True)
    snap = a.save_state()
    want = a.run("sap_ff", 130, auto_reset=True, outputs=outs)
    a.load_state(snap)                                     # rewind the same handle
    again = a.run("sap_ff", 130, auto_reset=True, outputs=outs)
    b = rmsa_env(nsfnet, 40, **dict(kw, seed=999))       # and restore into a fresh one
    b.load_state(snap)
    other = b.run("sap_ff", 130, auto_reset=True, outputs=outs)
    same_bytes(want, again, "rewound")
    same_bytes(want, other, "restored")
    # (read-backs: b was created on another seed; save_state byte for byte after a load is test_gpu_many_links' checkpoint test)
    same_bytes(snapshot(a, save_state=False), snapshot(b, save_state=False), "state")
    a.close(); b.close()


def test_phy_save_load_resume():
    z, meta = load_golden("phy_us14_s10_bmfa_defrag_cut")
    topo, tables = load_topology(meta["topology"]), load_phy_tables(meta["tables"])
    kw = dict(meta["env_kwargs"], grooming=True)
    outs = ("act_path", "channels", "channels_used", "accepted", "number_cuts_total", "defrag_counters")
    a = phy_env(topo, tables, kw, 6)
    a.run("bmfa", 140, auto_reset=True)
    snap = a.save_state()
    want = a.run("bmfa", 90, auto_reset=True, outputs=outs)
    b = phy_env(topo, tables, dict(kw, seed=77), 6)
    b.load_state(snap)
    other = b.run("bmfa", 90, auto_reset=True, outputs=outs)
    same_bytes(want, other, "restored")
    # (read-backs, not save_state: the QoT-aware blob also carries never-written slots)
    same_bytes(snapshot(a, save_state=False), snapshot(b, save_state=False), "state")
    assert a.channel_state(3) == b.channel_state(3)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ both kinds of handle
# B = 4; RMSA on NSFNET-320, the QoT-aware handle on US14 (the network the suite has QoT tables for)
B = 4
RMSA_KW = dict(num_spectrum_resources=320, load=50, mean_service_holding_time=25, episode_length=1000)
PHY_KW = dict(episode_length=200, grooming=True, load=1400, mean_service_holding_time=25)
POLICY = {"rmsa": "sap_ff", "phy": "sapff"}
OUTS = ("act_path", "accepted", "arrival", "holding")


def make(kind, nsfnet, seed=3, batch=B, **extra):
    if kind == "rmsa":
        return rmsa_env(nsfnet, batch, **dict(RMSA_KW, seed=seed), **extra)
    return phy_env(load_topology("us14_3-paths_6-modulations"), load_phy_tables("us14_k3"), dict(PHY_KW, seed=seed), batch, **extra)


def state(env):
    """counters, clock and occupancy: what a reseed with a full reset brings back to a fresh handle's"""
    return {k: v for k, v in snapshot(env, save_state=False).items() if k.split(".")[0] in ("counters", "current_time", "occupancy")}


@pytest.mark.parametrize("kind", ["rmsa", "phy"])
def test_reseed_and_full_reset_equal_a_fresh_handle(nsfnet, kind):
    env = make(kind, nsfnet, seed=3)
    env.run(POLICY[kind], 20)
    env.reseed(77)
    env.reset(only_episode_counters=False)
    env.run(POLICY[kind], 50)
    fresh = make(kind, nsfnet, seed=77)
    fresh.run(POLICY[kind], 50)
    same_bytes(state(env), state(fresh))
    env.close(); fresh.close()


@pytest.mark.parametrize("kind", ["rmsa", "phy"])
def test_a_new_stream_between_launches_changes_nothing(nsfnet, kind):
    env, straight = make(kind, nsfnet), make(kind, nsfnet)
    env.run(POLICY[kind], 10)
    env.set_stream(None)          # the handle drops its stream and creates another
    env.run(POLICY[kind], 40)
    straight.run(POLICY[kind], 50)
    same_bytes(state(env), state(straight))
    env.close(); straight.close()


@pytest.mark.parametrize("traced", [False, True])
@pytest.mark.parametrize("kind", ["rmsa", "phy"])
def test_load_state_rewinds_the_handle(nsfnet, kind, traced):
    """save_state, 30 steps, load_state, 30 steps: the second 30 are the first 30 -- also for a handle that replays a trace, whose
    position comes back with the state."""
    from optical_rl_gym_amd import record_trace
    env = make(kind, nsfnet)
    if traced:
        trace = record_trace(env, POLICY[kind], 80, outputs=OUTS)
        env.close()
        if kind == "rmsa":
            env = rmsa_env(nsfnet, B, trace=trace, num_spectrum_resources=320, episode_length=1000)
        else:
            env = phy_env(load_topology("us14_3-paths_6-modulations"), load_phy_tables("us14_k3"),
                                dict(episode_length=200, grooming=True), B, trace=trace)
    env.run(POLICY[kind], 10)
    position = env.trace_position
    assert position == (11 if traced else 0)
    snap = env.save_state()
    first = env.run(POLICY[kind], 30, outputs=OUTS)
    after = state(env)
    assert env.trace_position == (41 if traced else 0)
    env.load_state(snap)
    assert env.trace_position == position
    again = env.run(POLICY[kind], 30, outputs=OUTS)
    same_bytes(first, again, "outputs")
    same_bytes(after, state(env))
    env.close()


@pytest.mark.parametrize("kind", ["rmsa", "phy"])
def test_reductions_equal_the_sums_of_the_counters(nsfnet, kind):
    """reduce_counters is the sum of get_counters over the batch; reduce_counters(by_group=True) with two groups the sum per group."""
    from optical_rl_gym_amd.batched import COUNTER_NAMES
    groups = np.array([0, 1, 1, 0], np.int32)
    env = make(kind, nsfnet, groups=groups, num_groups=2)
    env.run(POLICY[kind], 50)
    per_env = env.counters()
    _, total = env.reduce_counters()
    grouped = env.reduce_counters(by_group=True)
    assert grouped.shape == (2, 16)
    for i, name in enumerate(COUNTER_NAMES):
        assert total[i] == per_env[name].sum(), name
        for g in range(2):
            assert grouped[g, i] == per_env[name][groups == g].sum(), (name, g)
    assert total[9] == B and list(grouped[:, 9]) == [2, 2]
    env.close()


@pytest.mark.parametrize("kind", ["rmsa", "phy"])
def test_shared_read_backs_equal_the_oracle(nsfnet, kind, device_log_in_oracle):
    """What the handle base reads back for both kinds -- pending requests, counters, time, services in progress, traffic, trace
    length, last kernel, device -- after 20 steps of a device policy on 3 environments, against one oracle per environment."""
    batch, seed, n = 3, 3, 20
    env = make(kind, nsfnet, seed=seed, batch=batch)
    env.run(POLICY[kind], n)
    req, cnt, now, nrun = env.requests(), env.counters(), env.current_time(), env.num_running()
    assert req.shape == now.shape == nrun.shape == (batch,)
    for i in range(batch):
        if kind == "rmsa":
            o = oracle_env_from_kwargs(nsfnet, RMSA_KW, seed=seed + i)
        else:
            o = phy_oracle_from_kwargs(load_topology("us14_3-paths_6-modulations"), load_phy_tables("us14_k3"), PHY_KW, seed=seed + i)
        o.run(POLICY[kind], n)
        r = o.request()
        assert (req[i]["service_id"], req[i]["src"], req[i]["dst"], req[i]["bit_rate"]) == (r.service_id, r.src, r.dst, r.bit_rate), i
        assert (req[i]["arrival_time"], req[i]["holding_time"]) == (r.arrival_time, r.holding_time), i
        oc = o.counters()
        assert set(oc) == set(cnt)
        for name in oc:
            assert cnt[name][i] == oc[name], (name, i)
        assert now[i] == o.current_time() and nrun[i] == o.num_running(), i
        o.close()
    # the constructor's rates (optical_network_env.py:127-129, rmsa_env.py:646-651), one group
    kw = RMSA_KW if kind == "rmsa" else PHY_KW
    holding = kw["mean_service_holding_time"]
    arrival_lambda, holding_lambda, group = env.traffic_rates()
    assert arrival_lambda.tolist() == [1 / (1 / float(kw["load"] / float(holding)))] * batch
    assert holding_lambda.tolist() == [1 / holding] * batch and group.tolist() == [0] * batch
    assert env.trace_length == 0
    assert env.last_kernel()
    assert env.device == 0
    env.close()
