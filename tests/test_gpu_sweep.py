"""Load sweeps in one handle (include/orlg.h orlg_traffic): environments with their own arrival and holding rates, counters
per group.  Every environment of a mixed handle is held to what a handle (or the oracle, or the reference's trace) of ITS load
and seed gives: bit for bit against the oracle (device log in the oracle, as tests/test_gpu_rmsa.py), decisions and counters
exactly and times to rtol 1e-12 against the reference's traces (as tests/test_gpu_phy.py)."""
import numpy as np
import pytest

from conftest import deeprmsa_to_rmsa_kwargs, load_golden, load_phy_tables, load_topology, oracle_env_from_kwargs
from gpu_support import (PHY_CONTINUOUS_OUTS as COUTS, RMSA_OUTS, device_log_fixture, everything_matches_oracle,  # noqa: F401
                         one_step_launches, phy_env, phy_matches_oracle, phy_matches_reference, rmsa_env, same_bytes, snapshot, step_kernel as step_kernel_both, tooling_env)

pytestmark = pytest.mark.gpu

PHY_OUTS = ("act_path", "n_channels", "channels", "channels_used", "accepted", "done", "request", "arrival", "holding",
            "number_cuts_total", "rss_total_metric", "defrag_counters")
RMSA_KW = dict(num_spectrum_resources=320, mean_service_holding_time=25, episode_length=200)
# 4 loads x 8 seeds: 2 Erlang leaves steps without a release, 400 Erlang blocks on NSFNET-320
SWEEP_LOADS, SWEEP_SEEDS = (2.0, 50.0, 120.0, 400.0), 8


def rmsa_sweep(topo, loads=SWEEP_LOADS, seeds_per_load=SWEEP_SEEDS, seed=10, **extra):
    from optical_rl_gym_amd import make_sweep
    return make_sweep("rmsa", topo, loads=loads, seeds_per_load=seeds_per_load, seed=seed, **dict(RMSA_KW, **extra))


# ------------------------------------------------------------------------------------------------ 2. against the oracle: RMSA
@pytest.mark.parametrize("policy", ["sap_ff", "llp_ff"])
@pytest.mark.parametrize("kernel,mode", [("wave", "long"), ("group", "long"), ("wave", "steps"), ("group", "steps"),
                                         ("group", "chunks")])
def test_rmsa_sweep_vs_oracle(nsfnet, device_log_in_oracle, kernel, policy, mode):
    """4 loads x 8 seeds, every float bit-exact: long launches (the deferred link statistics and the release summaries),
    one launch per step (the release queue stays in HBM) and long launches cut into forced chunks."""
    n = 700 if mode != "steps" else 90
    with tooling_env(**({"ORLG_GROUP_CHUNKS": "3"} if mode == "chunks" else {})):
        env = rmsa_sweep(nsfnet, step_kernel=kernel)
        assert env.batch_size == 32 and env.num_groups == 4
        tr = env.run(policy, n, outputs=RMSA_OUTS, auto_reset=True) if mode != "steps" else \
            one_step_launches(env, policy, n, RMSA_OUTS, auto_reset=True)
        if mode == "chunks":
            assert "chunks=3" in env.last_kernel(), env.last_kernel()
        if mode == "steps" and kernel == "group" and policy == "sap_ff":
            assert ",true>" in env.last_kernel(), env.last_kernel()   # the instantiation with the queue in HBM
    state = snapshot(env, save_state=False)
    for i in range(env.batch_size):
        kw = dict(RMSA_KW, load=float(env.loads[i]), seed=10 + i % SWEEP_SEEDS)
        everything_matches_oracle(nsfnet, kw, tr, i, state, policy, n, True)
    if mode == "long":
        g = env.groups
        assert tr["accepted"][:, g == 3].mean() < 0.999, "the highest load must block"
        assert tr["accepted"][:, g == 0].all(), "the lowest load must not"
    env.close()


def test_rmsa_sweep_continuous_bit_rates_vs_oracle(nsfnet, device_log_in_oracle, step_kernel_both):
    kwx = dict(bit_rate_selection="continuous", bit_rate_lower_bound=25, bit_rate_higher_bound=100)
    env = rmsa_sweep(nsfnet, step_kernel=step_kernel_both, **kwx)
    tr = env.run("sap_ff", 500, outputs=RMSA_OUTS, auto_reset=True)
    state = snapshot(env, save_state=False)
    for i in range(env.batch_size):
        everything_matches_oracle(nsfnet, dict(RMSA_KW, load=float(env.loads[i]), seed=10 + i % SWEEP_SEEDS, **kwx), tr, i, state, "sap_ff", 500, True)
    env.close()


def test_deeprmsa_sweep_external_actions_vs_oracle(nsfnet, device_log_in_oracle, step_kernel_both):
    """DeepRMSA with external actions, one launch per step, 4 loads x 8 seeds."""
    from optical_rl_gym_amd import make_sweep
    loads = (20.0, 100.0, 250.0, 600.0)
    dkw = dict(j=1, num_spectrum_resources=100, episode_length=100)
    env = make_sweep("deeprmsa", nsfnet, loads=loads, seeds_per_load=8, seed=7, mean_service_holding_time=25.0,
                     step_kernel=step_kernel_both, **dkw)
    B, n = env.batch_size, 150
    rng = np.random.default_rng(11)
    actions = rng.integers(0, nsfnet.k_paths, (n, B)).astype(np.int32)
    outs = ("act_path", "act_slot", "accepted", "reward", "done", "arrival", "holding")
    tr = one_step_launches(env, "deeprmsa_external", n, outs, actions=actions, auto_reset=True)
    obs, cnt = env.observation(), env.counters()
    for i in range(B):
        ld = loads[i // 8]
        kw, j = deeprmsa_to_rmsa_kwargs(dict(dkw, mean_service_holding_time=25.0, mean_service_inter_arrival_time=25.0 / ld, seed=7 + i % 8))
        o = oracle_env_from_kwargs(nsfnet, kw, j=j, reward_mode=1)
        ot = o.run("deeprmsa_external", n, reset_on_done=True, actions=np.ascontiguousarray(actions[:, i]))
        for f in outs:
            assert np.array_equal(tr[f][:, i], ot[f]), (f, i)
        assert np.array_equal(obs[i], o.observation()), i
        for name, v in o.counters().items():
            assert cnt[name][i] == v, (name, i)
        o.close()
    env.close()


# ------------------------------------------------------------------------------------------------ 1. + 2. QoT-aware
def run_mixed_phy(cases, copies, extra_envs, device_policy=None):
    """One handle: `copies` environments per fixture of `cases` (its seed and load), then extra_envs = [(load, seed)].  Every
    environment is held to the oracle at its load; the fixture environments also to their traces."""
    metas = [load_golden(c) for c in cases]
    meta0 = metas[0][1]
    topo, tables = load_topology(meta0["topology"]), load_phy_tables(meta0["tables"])
    base = {k: v for k, v in meta0["env_kwargs"].items() if k not in ("load", "seed")}
    for _, m in metas:
        assert {k: v for k, v in m["env_kwargs"].items() if k not in ("load", "seed")} == base, "fixtures must differ in load and seed only"
        assert m["policy"] == meta0["policy"] and m["topology"] == meta0["topology"] and m["tables"] == meta0["tables"]
    policy = device_policy or meta0["policy"]
    envs = []   # (load, seed, fixture or None, steps)
    for z, m in metas:
        for _ in range(copies):
            envs.append((m["env_kwargs"]["load"], m["env_kwargs"]["seed"], z, m["steps"]))
    envs += [(ld, sd, None, 0) for ld, sd in extra_envs]
    loads, seeds = [e[0] for e in envs], [e[1] for e in envs]
    n = max(e[3] for e in envs)
    groups = [sorted(set(loads)).index(ld) for ld in loads]
    env = phy_env(topo, tables, base, len(envs), load=loads, seeds=seeds, groups=groups)
    tr = env.run(policy, n, outputs=PHY_OUTS, auto_reset=True)
    state = snapshot(env, save_state=False)
    for i, (ld, sd, z, steps) in enumerate(envs):
        phy_matches_oracle(topo, tables, dict(base, load=ld, seed=sd), env, tr, i, state, policy, n)
        if z is not None:
            phy_matches_reference(z, tr, i, steps)
    env.close()


def test_phy_mixed_handle_vs_reference_traces_bmfa(device_log_in_oracle):
    """Seeds 10 / 11 / 12 at loads 1400 / 2400 / 4000 in ONE handle, each environment against ITS trace of the reference
    for the trace's own step count (longer traces are continued while shorter ones are no longer compared)."""
    run_mixed_phy(["phy_us14_s10_bmfa", "phy_us14_s11_bmfa_load2400", "phy_us14_s12_bmfa_load4000"], 3, [])


def test_phy_mixed_handle_vs_reference_traces_sapff(device_log_in_oracle):
    run_mixed_phy(["phy_us14_s10_sapff", "phy_us14_s14_sapff_load4000"], 3, [])


@pytest.mark.parametrize("case", ["phy_us14_s10_bmfa_defrag_cut", "phy_us14_s16_sapff_defrag_load3000"])
def test_phy_mixed_handle_defragmentation_fixture(case, device_log_in_oracle):
    """The defragmentation traces, each in a mixed handle of its own policy next to environments at other loads."""
    run_mixed_phy([case], 2, [(900.0, 3), (2000.0, 4), (3600.0, 5), (1400.0, 6), (3000.0, 7), (200.0, 8)])


@pytest.mark.parametrize("policy,extra", [("bmfa", {}), ("bmfa_rss", {}), ("sapff", {}),
                                          ("bmfa", dict(defrag_period=10, number_moves=10, metric="cut")),
                                          ("bmfa_rss", dict(defrag_period=10, number_moves=10, metric="rss")),
                                          ("sapff", dict(defrag_period=10, number_moves=10, metric="cut")),
                                          ("bmfa", dict(grooming=True)), ("bmfa", dict(gn=True)),
                                          ("bmfa", dict(narrow=True)), ("sapff", dict(narrow=True, defrag_period=10, number_moves=10)),
                                          ("sapff", dict(gn=True, defrag_period=10, number_moves=10, metric="rss"))])
def test_phy_sweep_vs_oracle(policy, extra, device_log_in_oracle):
    """4 loads x 8 seeds on US14, one policy per family, plain / defragmentation in both metrics / GN gate / grooming.  30
    Erlang leaves steps without a release.  The 268 channels of US14 take thousands of steps to fill; the `narrow` cases
    run 32 channels (number_spectrum_channels=10, s band 12), where 2400 and 4000 Erlang block within the run."""
    from optical_rl_gym_amd import gn_gate_parameters, traffic
    topo, tables = load_topology("us14_3-paths_6-modulations"), load_phy_tables("us14_k3")
    extra = dict(extra)
    if extra.pop("gn", False):
        extra["gn_gate"] = gn_gate_parameters(topo)
    narrow = extra.pop("narrow", False)
    if narrow:
        extra.update(number_spectrum_channels=10, number_spectrum_channels_s_band=12)
        tables = (tables[0], np.ascontiguousarray(tables[1][:, :32]), np.ascontiguousarray(tables[2][:, :32]))
    base = dict(dict(mean_service_holding_time=25, episode_length=150, grooming=False), **extra)
    loads = (30.0, 1400.0, 2400.0, 4000.0)
    load, seeds, group = traffic.load_sweep(loads, 8, seed=10)
    env = phy_env(topo, tables, base, load.size, load=load, seeds=seeds, groups=group)
    n = 400
    tr = env.run(policy, n, outputs=PHY_OUTS, auto_reset=True)
    state = snapshot(env, save_state=False)
    for i in range(load.size):
        phy_matches_oracle(topo, tables, dict(base, load=float(load[i]), seed=int(seeds[i])), env, tr, i, state, policy, n)
    if "gn_gate" not in extra:   # (the GN gate refuses services whatever the load)
        assert tr["accepted"][:, group == 0].all(), "the lowest load must not block"
    if narrow:
        assert tr["accepted"][:, group == 3].mean() < 0.95, "the highest load must block"
    env.close()


def continuous_state_slices(env, topo, queue_capacity):
    """save_state of a continuous QoT-aware handle cut into one byte string per environment.  The blob is the concatenation of
    [B][...] arrays (orlg_phy_api.hip phy_state_parts: occupancy, release times, service records, MT19937, scalars,
    channel_state lists and their lengths, the three arrival rings, the float64 shares of lists and services) and a 16-byte
    tag; the size of a service record follows from the blob's size."""
    B, Q = env.batch_size, queue_capacity
    lists = topo.num_nodes * topo.num_nodes * topo.k_paths
    cs = env.L.orlg_phy_channel_state_capacity(env.h)
    blob = env.save_state()
    per_env = [topo.num_links * env.words_per_link * 8, Q * 8, None, 624 * 4, 224, lists * cs * 4, lists, 64 * 8, 64 * 8, 64 * 4,
               lists * cs * 16, Q * 14 * 8]
    rest = blob.size - 16 - B * sum(x for x in per_env if x is not None)
    assert rest > 0 and rest % (B * Q) == 0, (blob.size, rest)
    per_env[2] = rest // B
    out, off = [b""] * B, 0
    for x in per_env:
        for i in range(B):
            out[i] += blob[off + i * x:off + (i + 1) * x].tobytes()
        off += B * x
    assert off + 16 == blob.size
    return out


def test_phy_continuous_mixed_handle_device_against_device():
    """Continuous bit rates have no oracle: a mixed continuous handle holds the fixture's seed at the fixture's load and at a
    second load; each environment equals the same seed on a UNIFORM continuous handle of its load -- device against device:
    every per-step output and every environment's slice of save_state byte for byte."""
    z, meta = load_golden("cont_us14_s20_sapff")
    topo, tables = load_topology(meta["topology"]), load_phy_tables(meta["tables"])
    kw = dict(meta["env_kwargs"])
    ld0, sd, n = kw.pop("load"), kw.pop("seed"), meta["steps"]
    ld1 = 2.5 * ld0
    loads, seeds = [ld0, ld1, ld0, ld1, ld1, ld0], [sd, sd, sd + 1, sd + 1, sd, sd]
    cap = dict(queue_capacity=2048, channel_state_capacity=32)   # the same capacities on every handle
    mixed = phy_env(topo, tables, dict(kw, load=loads), 6, seeds=seeds, **cap)
    tm = mixed.run(meta["policy"], n, outputs=COUTS, auto_reset=True)
    sm = continuous_state_slices(mixed, topo, cap["queue_capacity"])
    assert np.array_equal(tm["act_path"][:, 0], z["act_path"][:n]) and np.array_equal(tm["accepted"][:, 0], z["accepted"][:n])
    np.testing.assert_allclose(tm["arrival"][:, 0], z["arrival"][:n], rtol=1e-12, atol=0)
    for ld in (ld0, ld1):
        idx = [i for i in range(6) if loads[i] == ld]
        uni = phy_env(topo, tables, dict(kw, load=ld), len(idx), seeds=[seeds[i] for i in idx], **cap)
        tu = uni.run(meta["policy"], n, outputs=COUTS, auto_reset=True)
        same_bytes({f: tm[f][:, idx] for f in COUTS}, tu, ld)
        for get in ("counters", "current_time", "num_running", "available_channels", "requests", "episode_stats"):
            x, y = getattr(mixed, get)(), getattr(uni, get)()
            if isinstance(x, dict):
                assert all(np.array_equal(x[k][idx], y[k]) for k in x), (get, ld)
            else:
                assert np.array_equal(x[idx], y), (get, ld)
        su = continuous_state_slices(uni, topo, cap["queue_capacity"])
        for q, i in enumerate(idx):
            assert mixed.channel_state(i) == uni.channel_state(q), (i, ld)
            assert sm[i] == su[q], (i, ld)
        uni.close()
    mixed.close()


# ------------------------------------------------------------------------------------------------ 3. a uniform array is the scalar
@pytest.mark.parametrize("kernel", ["wave", "group"])
def test_uniform_array_is_the_scalar_rmsa(nsfnet, kernel):
    B = 24
    a = rmsa_env(nsfnet, B, kernel, load=50, seed=3, **RMSA_KW)
    b = rmsa_env(nsfnet, B, kernel, load=np.full(B, 50.0), seed=3, **RMSA_KW)
    assert np.array_equal(a.traffic_rates()[0], b.traffic_rates()[0]) and np.array_equal(a.traffic_rates()[1], b.traffic_rates()[1])
    ta = a.run("sap_ff", 1000, outputs=RMSA_OUTS, auto_reset=True)
    tb = b.run("sap_ff", 1000, outputs=RMSA_OUTS, auto_reset=True)
    same_bytes(ta, tb, "outputs")
    same_bytes(snapshot(a), snapshot(b), "state")
    a.close(); b.close()


def test_uniform_array_is_the_scalar_phy():
    topo, tables = load_topology("us14_3-paths_6-modulations"), load_phy_tables("us14_k3")
    kw = dict(mean_service_holding_time=25, episode_length=200, seed=10, defrag_period=10, number_moves=10)
    a = phy_env(topo, tables, kw, 8, load=50)
    b = phy_env(topo, tables, kw, 8, load=np.full(8, 50.0))
    ta = a.run("bmfa", 1000, outputs=PHY_OUTS, auto_reset=True)
    tb = b.run("bmfa", 1000, outputs=PHY_OUTS, auto_reset=True)
    same_bytes(ta, tb, "outputs")
    same_bytes(snapshot(a), snapshot(b), "state")
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 4. the kernels continue each other
def test_mixed_loads_kernels_continue_each_other_and_checkpoint(nsfnet):
    """wave -> group -> wave on a sweep equals wave alone, byte for byte on save_state; a checkpoint taken mid-run and loaded
    into a fresh sweep handle continues identically; resets and a reseed keep every environment's rates."""
    def sweep(kernel):
        return rmsa_sweep(nsfnet, step_kernel=kernel)
    ref, a = sweep("wave"), sweep("wave")
    ref.run("sap_ff", 900, auto_reset=True)
    a.run("sap_ff", 300, auto_reset=True)
    mid = a.save_state()
    g = sweep("group")
    g.load_state(mid)
    g.run("sap_ff", 300, auto_reset=True)
    a.load_state(g.save_state())
    a.run("sap_ff", 300, auto_reset=True)
    assert a.save_state().tobytes() == ref.save_state().tobytes()
    fresh = sweep("group")
    fresh.load_state(mid)
    fresh.run("sap_ff", 600, auto_reset=True)
    assert fresh.save_state().tobytes() == ref.save_state().tobytes()
    # the rates are configuration: a reseed and both resets keep them
    rates = fresh.traffic_rates()
    fresh.reset(only_episode_counters=False); fresh.reseed(seed=99); fresh.reset(only_episode_counters=True)
    assert all(np.array_equal(x, y) for x, y in zip(rates, fresh.traffic_rates()))
    # after a reseed and a full reset every environment draws with ITS rates again: from the second request on (the pending one
    # stays through a reseed) the handle equals a fresh sweep of the new seeds
    other = rmsa_sweep(nsfnet, step_kernel="group", seed=99)
    chk = sweep("wave")
    chk.reseed(seeds=np.tile(np.arange(SWEEP_SEEDS, dtype=np.uint64) + np.uint64(99), len(SWEEP_LOADS)))
    chk.reset(only_episode_counters=False)
    t1 = chk.run("sap_ff", 200, outputs=("arrival", "holding"))
    t2 = other.run("sap_ff", 200, outputs=("arrival", "holding"))
    same_bytes(t1, t2, "after the reseed")
    for e in (ref, a, g, fresh, other, chk):
        e.close()


# ------------------------------------------------------------------------------------------------ 5. grouped reduction
def numpy_group_by(counters, episodes_done, groups, G):
    out = np.zeros((G, 16), np.int64)
    cols = ("services_processed", "services_accepted", "episode_services_processed", "episode_services_accepted",
            "bit_rate_requested", "bit_rate_provisioned", "episode_bit_rate_requested", "episode_bit_rate_provisioned")
    for q, name in enumerate(cols):
        np.add.at(out[:, q], groups, counters[name])
    np.add.at(out[:, 8], groups, episodes_done)
    np.add.at(out[:, 9], groups, 1)
    np.add.at(out[:, 10], groups, (counters["services_processed"] - counters["services_accepted"]) ** 2)
    np.add.at(out[:, 11], groups, (counters["episode_services_processed"] - counters["episode_services_accepted"]) ** 2)
    return out


@pytest.mark.parametrize("B,G,steps", [(4, 1, 300), (20004, 7, 300), (262144, 256, 3)])
def test_grouped_reduction_rmsa(nsfnet, B, G, steps):
    from optical_rl_gym_amd import BatchedRMSAEnv
    rng = np.random.default_rng(B)
    if G == 7:      # unequal sizes, scrambled order
        groups = rng.choice(7, B, p=[0.3, 0.05, 0.2, 0.01, 0.14, 0.2, 0.1]).astype(np.int32)
    else:
        groups = rng.integers(0, G, B).astype(np.int32)
    loads = 20.0 + 10.0 * (groups % 9)
    kw = dict(RMSA_KW, episode_length=100, stats_level="counters" if B > 100000 else "full")
    env = BatchedRMSAEnv(nsfnet, B, load=loads, seed=1, groups=groups if G > 1 else None, num_groups=G if G > 1 else None, **kw)
    env.run("sap_ff", steps, auto_reset=True)
    got = env.reduce_counters(by_group=True)
    assert got.shape == (G, 16) and got.dtype == np.int64
    want = numpy_group_by(env.counters(), env.episodes_done(), groups if G > 1 else np.zeros(B, np.int64), G)
    assert np.array_equal(got, want)
    _, total = env.reduce_counters()
    assert np.array_equal(got[:, :10].sum(axis=0), total[:10]) and not got[:, 12:].any()
    env.close()


@pytest.mark.parametrize("B,G", [(4, 1), (1000, 7)])
def test_grouped_reduction_phy(B, G):
    topo, tables = load_topology("us14_3-paths_6-modulations"), load_phy_tables("us14_k3")
    rng = np.random.default_rng(B)
    groups = rng.integers(0, G, B).astype(np.int32)
    loads = 1200.0 + 80.0 * groups
    env = phy_env(topo, tables, dict(mean_service_holding_time=25, episode_length=60, seed=2), B, load=loads,
                  groups=groups if G > 1 else None)
    env.run("sapff", 200, auto_reset=True)
    got = env.reduce_counters(by_group=True)
    want = numpy_group_by(env.counters(), env.episode_stats()["episodes_done"], groups, G)
    assert want[:, 8].sum() > 0 and np.array_equal(got, want)
    assert np.array_equal(got[:, :10].sum(axis=0), env.reduce_counters()[1][:10])
    env.close()


def test_grouped_reduction_reports_an_overflowed_queue(nsfnet):
    """The construction of tests/test_gpu_errors.py: a queue of 64 slots under 150 Erlang.  A reported error code."""
    from optical_rl_gym_amd import BatchedRMSAEnv, OrlgError
    kw = dict(num_spectrum_resources=320, mean_service_holding_time=25, episode_length=1000, seed=1)
    env = BatchedRMSAEnv(nsfnet, 16, load=np.full(16, 150.0), groups=np.arange(16) % 2, queue_capacity=64, **kw)
    env.run("sap_ff", 3000)
    with pytest.raises(OrlgError) as ei:
        env.reduce_counters(by_group=True)
    assert ei.value.code == -4 and "queue" in str(ei.value)
    env.close()


# ------------------------------------------------------------------------------------------------ 6. sizing
def test_capacities_come_from_the_largest_load(nsfnet):
    from optical_rl_gym_amd import BatchedRMSAEnv, OrlgError
    loads = np.repeat(np.arange(50.0, 401.0, 50.0), 4)
    kw = dict(num_spectrum_resources=320, mean_service_holding_time=25, episode_length=1000, seed=1)
    env = BatchedRMSAEnv(nsfnet, loads.size, load=loads, queue_capacity=0, **kw)
    env.run("sap_ff", 2000, auto_reset=True)
    env.reduce_counters()            # raises ORLG_ERR_QUEUE_FULL if a queue overflowed
    env.reduce_counters(by_group=True)
    # what queue_capacity = 0 picks for 50 Erlang alone (mean + 10 sigma = 120 -> 128 slots) is too small for the sweep
    small = BatchedRMSAEnv(nsfnet, loads.size, load=loads, queue_capacity=128, **kw)
    small.run("sap_ff", 2000, auto_reset=True)
    with pytest.raises(OrlgError) as ei:
        small.reduce_counters()
    assert ei.value.code == -4
    env.close(); small.close()


# ------------------------------------------------------------------------------------------------ 7. Monitor tree
@pytest.mark.parametrize("kind", ["rmsa", "phy"])
def test_monitor_tree_on_the_device(kind, nsfnet, tmp_path):
    """3 loads x 4 seeds x 2 episodes: one file per load in the reference's tree, values = the per-environment info arrays."""
    from optical_rl_gym_amd import evaluate_heuristic_batched, evaluate_phy_heuristic_batched, make_sweep
    from optical_rl_gym_amd.monitor import PHY_INFO_KEYWORDS, RMSA_INFO_KEYWORDS
    if kind == "rmsa":
        loads, L = [100.0, 250.0, 400.0], 120
        env = make_sweep("rmsa", nsfnet, loads=loads, seeds_per_load=4, seed=5, **dict(RMSA_KW, episode_length=L))
        r, l, info, by = evaluate_heuristic_batched(env, "sap_ff", 2, monitor_dir=str(tmp_path), monitor_name="sapff", by_group=True)
        keys = RMSA_INFO_KEYWORDS
    else:
        topo, tables = load_topology("us14_3-paths_6-modulations"), load_phy_tables("us14_k3")
        loads, L = [1200.0, 2400.0, 4000.0], 100
        env = make_sweep("phy", topo, loads=loads, seeds_per_load=4, seed=5, modulation_level=tables[1],
                         connections_detail=tables[0], gsnr=tables[2], mean_service_holding_time=25, episode_length=L)
        r, l, info, by = evaluate_phy_heuristic_batched(env, "bmfa", 2, monitor_dir=str(tmp_path), monitor_name="sapff", by_group=True)
        keys = PHY_INFO_KEYWORDS
    assert r.shape == (2, 12) and np.array_equal(by["load"], loads) and np.array_equal(by["num_envs"], [4, 4, 4])
    for g, ld in enumerate(loads):
        path = tmp_path / f"logs_{ld:g}_{L}" / "sapff.monitor.csv"
        lines = path.read_text().splitlines()
        assert lines[0].startswith("#{") and lines[1] == "r,l,t," + ",".join(keys) and len(lines) == 2 + 2 * 4
        for ep in range(2):
            for q in range(4):
                cells = lines[2 + ep * 4 + q].split(",")
                i = g * 4 + q
                assert float(cells[0]) == r[ep, i] and int(cells[1]) == l[ep, i]
                for c, k in zip(cells[3:], keys):
                    assert float(c) == float(info[k][ep, i]), (k, ep, i)
        # the summary from the grouped reduction is the statistic of the per-environment rates
        for ep in range(2):
            rates = info["episode_service_blocking_rate"][ep, g * 4:(g + 1) * 4]
            assert by["episode_service_blocking_rate"][ep, g] == pytest.approx(rates.mean(), rel=1e-12, abs=1e-15)
            assert by["episode_service_blocking_rate_stderr"][ep, g] == pytest.approx(rates.std(ddof=1) / 2.0, rel=1e-9, abs=1e-12)
    env.close()
