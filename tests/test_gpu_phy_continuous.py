"""GPU parity of the QoT-aware (PhyRMSA) path with bit_rate_selection="continuous" (phy_rmsa_env.py:37-42, 114-134,
979-984): rng.randint bit rates and float64 channel shares.  The CPU oracle has no continuous mode, so the device is held to
the reference's own traces (tests/golden/make_golden_phy_continuous.py) in every environment of a batch, and to itself
(split launches, checkpoints, the GN-gate instantiation with a gate that passes everything)."""
import numpy as np
import pytest

from conftest import load_golden, load_phy_tables, load_topology
from gpu_support import PHY_CONTINUOUS_OUTS as OUTS, check_state, check_trace, phy_env as make_env, same_bytes, snapshot

pytestmark = pytest.mark.gpu

CASES = ["cont_us14_s20_sapff", "cont_us14_s21_bmff", "cont_us14_s22_sapbm", "cont_us14_s23_faff",
         "cont_us14_s24_bmfa", "cont_us14_s25_bmfa_groom", "cont_us14_s26_bmfa_rss_groom",
         "cont_us14_s27_sapbm_100_600", "cont_us14_s28_faff_rss_100_600",
         "cont_us14_s29_sapff_100_600_load20000", "cont_jpn12_s30_bmff"]
def same_state(a, b, envs):
    """Two handles hold the same simulation (the saved state also carries never-written, uninitialised slots)."""
    same_bytes(snapshot(a, save_state=False), snapshot(b, save_state=False), "state")
    for i in envs:
        assert a.channel_state(i) == b.channel_state(i), i


@pytest.mark.parametrize("case", CASES)
def test_phy_continuous_policy_vs_reference(case):
    """Every environment of the batch seeded with the fixture's seed: each one is the reference's trace, bit for bit in the
    decisions, the float64 shares and the counters (time-derived floats to rtol 1e-12: the device's log)."""
    z, meta = load_golden(case)
    topo, tables = load_topology(meta["topology"]), load_phy_tables(meta["tables"])
    kw, policy, n = meta["env_kwargs"], meta["policy"], meta["steps"]
    assert kw["bit_rate_selection"] == "continuous"
    batch = 8
    env = make_env(topo, tables, kw, batch, seeds=[kw["seed"]] * batch)
    assert env.continuous and env.requests()["bit_rate"][0] == z["bit_rate"][0]
    assert env.node_vectors   # (the continuous instantiations keep the cut metric's node-degree vectors on chip)
    # the first n - 1 steps in one launch (the last one is not the end of an episode: its info ratios are checked) ...
    tr = env.run(policy, n - 1, outputs=OUTS, auto_reset=True)
    assert env.last_kernel().startswith(f"orlg_phy_kernel<{env.words_per_link},false,false,"), env.last_kernel()
    assert env.last_kernel().split(" ")[0].endswith(",true>"), env.last_kernel()
    for i in range(batch):
        check_trace(topo, tables, tr, i, z, 0, n - 1)
        check_state(env, i, z, n - 2)
    # ... and the last one in a launch of its own
    tr = env.run(policy, 1, outputs=OUTS, auto_reset=True)
    av = env.available_channels()
    fin = np.unpackbits(z["final_available_channels"], axis=1, bitorder="little")[:, :env.num_channels]
    for i in range(batch):
        check_trace(topo, tables, tr, i, z, n - 1, n)
        check_state(env, i, z, n - 1)
        assert np.array_equal(av[i], fin), i
    assert env.episode_stats()["queue_overflow"].max() == 0
    if "load20000" in case:
        assert z["services_accepted"][-1] < n   # the fixture blocks
    env.close()


def test_phy_continuous_work_queue_more_envs_than_resident_waves():
    """B = 9000 > resident waves: the long launches draw environments from the work queue.  Every environment runs the
    fixture's seed; sampled ones (across the static / ticket boundary) are held to the reference."""
    case = "cont_us14_s25_bmfa_groom"
    z, meta = load_golden(case)
    topo, tables = load_topology(meta["topology"]), load_phy_tables(meta["tables"])
    kw, policy, n = meta["env_kwargs"], meta["policy"], 300
    B = 9000
    env = make_env(topo, tables, kw, B, seeds=[kw["seed"]] * B)
    tr = env.run(policy, n, outputs=OUTS, auto_reset=True)
    av = env.available_channels()
    for i in (0, 4095, 4096, 8191, 8192, 8999):
        check_trace(topo, tables, tr, i, z, 0, n)
        check_state(env, i, z, n - 1)
    # every environment made the same decisions
    assert np.all(tr["act_path"] == tr["act_path"][:, :1]) and np.all(tr["channels_used_f64"] == tr["channels_used_f64"][:, :1])
    assert np.all(av == av[:1])
    env.close()


def test_phy_continuous_view_reproduces_reference():
    """orlg.make("PhyRMSA-v0", bit_rate_selection="continuous"): the Python heuristics on the view's float channel_state
    tuples drive the float64 external actions and reproduce the reference's trace."""
    import optical_rl_gym_amd as pkg
    for case, heuristic, n in (("cont_us14_s20_sapff", "sapff_rmsa", 200),
                               ("cont_us14_s27_sapbm_100_600", "phy_aware_sapbm_rmsa", 120)):
        z, meta = load_golden(case)
        pairs, mod, gsnr = load_phy_tables(meta["tables"])
        env = pkg.make("PhyRMSA-v0", topology=load_topology(meta["topology"]), modulation_level=mod,
                       connections_detail=pairs, gsnr=gsnr, **meta["env_kwargs"])
        fn = getattr(pkg, heuristic)
        virtual = 0
        for t in range(n):
            s = env.current_service
            assert (s.source_id, s.destination_id, s.bit_rate) == (z["src_id"][t], z["dst_id"][t], z["bit_rate"][t]), t
            a = fn(env)
            assert a[0] == z["act_path"][t] and len(a[1]) == z["n_channels"][t], t
            assert [c[0] for c in a[1]] == z["channels"][t][:len(a[1])].tolist()
            assert [float(c[1]) for c in a[1]] == z["ch_used"][t][:len(a[1])].tolist(), t
            assert [float(c[2]) for c in a[1]] == z["ch_free"][t][:len(a[1])].tolist(), t
            virtual += a[0] >= 20
            obs, reward, done, truncated, info = env.step(a)
            assert reward == z["reward"][t] and done == bool(z["done"][t])
            assert info["number_cuts_total"] == z["number_cuts_total"][t]
            assert info["bit_rate_blocking_rate"] == z["bit_rate_blocking_rate"][t]
            assert info["physical_paths"] == z["physical_paths"][t]
            if done:
                env.reset()
        assert virtual > 10
        # the float tuples of channel_state (continuous shares are not whole hundredths)
        st = env._batched.channel_state(0)
        shares = [x[1] for lst in st.values() for x in lst]
        assert shares and all(isinstance(x, float) for x in shares)
        env.close()


def test_phy_continuous_split_launches_and_checkpoint():
    """300 + 300 steps equal 600 steps; a save_state -> fresh handle -> load_state resume is byte-identical; a state of the
    other bit-rate mode is refused."""
    from optical_rl_gym_amd import OrlgError
    z, meta = load_golden("cont_us14_s22_sapbm")
    topo, tables = load_topology(meta["topology"]), load_phy_tables(meta["tables"])
    kw, policy = meta["env_kwargs"], meta["policy"]
    whole = make_env(topo, tables, kw, 16)
    tw = whole.run(policy, 600, outputs=OUTS, auto_reset=True)
    a = make_env(topo, tables, kw, 16)
    t1 = a.run(policy, 300, outputs=OUTS, auto_reset=True)
    snap = a.save_state()
    t2 = a.run(policy, 300, outputs=OUTS, auto_reset=True)
    same_bytes({f: np.concatenate([t1[f], t2[f]]) for f in OUTS}, tw, "split launches")
    same_state(a, whole, range(16))
    b = make_env(topo, tables, kw, 16, seeds=np.arange(16) + 999)
    b.load_state(snap)
    t3 = b.run(policy, 300, outputs=OUTS, auto_reset=True)
    same_bytes(t3, t2, "resumed")
    assert b.save_state().tobytes() == a.save_state().tobytes()
    assert b.channel_state(3) == a.channel_state(3)
    # across modes: refused either way
    d = make_env(topo, tables, dict(kw, bit_rate_selection="discrete"), 16)
    assert not d.continuous and d.last_kernel().startswith("orlg_phy_kernel<5,false,false,-1>")
    with pytest.raises(OrlgError) as ei:
        d.load_state(snap)
    assert ei.value.code == -1
    with pytest.raises(OrlgError) as ei:
        b.load_state(d.save_state())
    assert ei.value.code == -1
    # the refused loads left b alone
    assert b.save_state().tobytes() == a.save_state().tobytes()
    for e in (whole, a, b, d):
        e.close()


def test_phy_continuous_gn_gate_passing_everything_equals_plain():
    """No reference for the gate: with thresholds every channel passes, the GN instantiation's trace equals the plain
    continuous one byte for byte, and so does the simulation it leaves."""
    from optical_rl_gym_amd import gn_gate_parameters
    z, meta = load_golden("cont_us14_s27_sapbm_100_600")
    topo, tables = load_topology(meta["topology"]), load_phy_tables(meta["tables"])
    kw, policy = meta["env_kwargs"], meta["policy"]
    gate = dict(gn_gate_parameters(topo), thresholds_db=np.full(31, -1e300))
    plain = make_env(topo, tables, kw, 64)
    gated = make_env(topo, tables, kw, 64, gn_gate=gate)
    tp = plain.run(policy, 400, outputs=OUTS, auto_reset=True)
    tg = gated.run(policy, 400, outputs=OUTS + ("gn_gsnr_db",), auto_reset=True)
    assert gated.last_kernel().startswith("orlg_phy_kernel<5,false,true,4,true>"), gated.last_kernel()
    for f in OUTS:
        assert np.array_equal(tp[f], tg[f]), f
    same_state(plain, gated, range(64))
    assert np.isfinite(tg["gn_gsnr_db"]).mean() > 0.2   # the gate ran
    plain.close(); gated.close()


def test_phy_continuous_gn_gate_batch_4096():
    """B = 4096 with real thresholds: every environment finishes, provisions no more than it was asked for, and every
    accepted physical service's last checked channel reached the threshold of its level."""
    from optical_rl_gym_amd import gn_gate_parameters
    topo, tables = load_topology("us14_3-paths_6-modulations"), load_phy_tables("us14_k3")
    gate = gn_gate_parameters(topo)
    kw = dict(load=1400, mean_service_holding_time=25, episode_length=200, seed=10, grooming=True, gn_gate=gate,
              bit_rate_selection="continuous", bit_rate_lower_bound=100, bit_rate_higher_bound=600)
    n, B = 320, 4096
    env = make_env(topo, tables, kw, B)
    tr = env.run("bmfa", n, outputs=("act_path", "n_channels", "channels", "accepted", "gn_gsnr_db", "request"), auto_reset=True)
    cnt = env.counters()
    assert np.all(cnt["services_processed"] == n + 1)
    assert np.all(cnt["bit_rate_provisioned"] <= cnt["bit_rate_requested"])
    assert np.all((tr["request"][..., 3] >= 100) & (tr["request"][..., 3] <= 600))
    pairs, mod, _ = tables
    rows = topo.pair_table_rows(pairs)
    thr = np.asarray(gate["thresholds_db"])
    phys = (tr["accepted"] == 1) & (tr["act_path"] >= 0) & (tr["act_path"] < 10)
    ts, es = np.nonzero(phys)
    assert ts.size > 1000
    last = tr["channels"][ts, es, tr["n_channels"][ts, es] - 1]
    row = rows[tr["request"][ts, es, 1] * topo.num_nodes + tr["request"][ts, es, 2]]
    lvl = mod[row, last, tr["act_path"][ts, es]]
    assert np.all(tr["gn_gsnr_db"][ts, es] >= thr[lvl - 1])
    blocked_by_gate = (tr["accepted"] == 0) & (tr["act_path"] >= 0) & (tr["act_path"] < 10)
    assert blocked_by_gate.sum() > 0
    assert env.episode_stats()["queue_overflow"].max() == 0
    env.close()
