"""GN-model GSNR admission check inside the step of the slot-based environments (``include/orlg.h`` ``orlg_rmsa_gn_gate``,
DESIGN 2.20) on the device, held to the CPU gated oracle of ``gn_gate_reference.py``: decisions, requests, counters and occupancy
exact, the GSNR the check compared to rtol 1e-9 (the tolerance of the QoT-aware gate, DESIGN 2.8: the device sums the interferers
by a wave reduction, the oracle one after the other), NaN exactly where the oracle ran no check."""
import ctypes as C

import numpy as np
import pytest

import gn_gate_reference as ref
from conftest import deeprmsa_to_rmsa_kwargs, load_topology
from gpu_support import device_log_in_oracle, kernel_name, rmsa_env, snapshot, state_matches

pytestmark = pytest.mark.gpu

RTOL = 1e-9
OUTS = ("act_path", "act_slot", "accepted", "done", "request", "reward", "gn_gsnr_db")


def _gsnr_matches(dev, want, what):
    assert np.array_equal(np.isnan(dev), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.allclose(dev[ok], want[ok], rtol=RTOL, atol=0), (what, float(np.max(np.abs(dev[ok] / want[ok] - 1))))


def _steps_match(tr, i, want, what, rows=slice(None)):
    """per-step outputs of environment i against the gated oracle's arrays"""
    for name in ("act_path", "act_slot", "accepted", "done", "request"):
        assert np.array_equal(tr[name][:, i], want[name][rows]), (what, name)
    _gsnr_matches(tr["gn_gsnr_db"][:, i], want["gsnr"][rows], what)


def _state(env):
    """the read-backs state_matches compares, fetched once per handle"""
    return snapshot(env, save_state=False)


def _concat(a, b):
    return {k: np.concatenate([a[k], b[k]]) for k in a}


def _gated_env(case, B, stats_level="full", seeds=None, **over):
    c = ref.CASES[case]
    topo = load_topology(c["topology"])
    kw = ref.case_kwargs(case, **over)
    if seeds is not None:
        kw.pop("seed")
    return rmsa_env(topo, B, gn_gate=ref.case_gate(topo), stats_level=stats_level, seeds=seeds, **kw), topo, c


@pytest.mark.parametrize("case", list(ref.CASES))
def test_case_against_the_gated_oracle(case):
    """B = 8 environments on the case's seed: 599 steps in one launch, one more in its own."""
    B = 8
    env, topo, c = _gated_env(case, B, seeds=[ref.CASES[case]["seed"]] * B)
    tr = _concat(env.run(c["policy"], ref.N_STEPS - 1, outputs=OUTS, auto_reset=True),
                 env.run(c["policy"], 1, outputs=OUTS, auto_reset=True))
    W = env.words_per_link
    assert env.last_kernel().startswith(kernel_name("wave", W, "full", gn=True)), env.last_kernel()
    want, final, fig = ref.run_case(case)
    assert int(np.isfinite(tr["gn_gsnr_db"][:, 0]).sum()) == fig["checks"]
    state = _state(env)
    for i in range(B):
        _steps_match(tr, i, want, (case, i))
        state_matches(state, i, final, (case, i))
    env.close()


def test_statistics_levels_decide_alike():
    case = "nsfnet_s320_l150_sapff"
    want, final, _ = ref.run_case(case)
    for level, stats in enumerate(("counters", "network", "full")):
        env, topo, c = _gated_env(case, 2, stats_level=stats, seeds=[ref.CASES[case]["seed"]] * 2)
        tr = env.run(c["policy"], ref.N_STEPS, outputs=OUTS, auto_reset=True)
        assert env.last_kernel().startswith(kernel_name("wave", env.words_per_link, level, gn=True)), env.last_kernel()
        state = _state(env)
        for i in range(2):
            _steps_match(tr, i, want, (stats, i))
            state_matches(state, i, final, (stats, i))
        env.close()


def test_agent_driven_deeprmsa():
    """BatchedDeepRMSAEnv, j = 1, NSFNET S = 320, 150 launches of one step: environment 0 takes the oracle's
    deeprmsa_sap_ff action, environment 1 the same but an action out of range every fifth step."""
    from optical_rl_gym_amd import BatchedDeepRMSAEnv
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    dkw = dict(mean_service_holding_time=25.0, mean_service_inter_arrival_time=25.0 / 150, num_spectrum_resources=320,
               episode_length=ref.EPISODE_LENGTH, seed=21, j=1)
    okw, j = deeprmsa_to_rmsa_kwargs(dkw)
    gate = ref.case_gate(topo)
    B, n = 2, 150
    env = BatchedDeepRMSAEnv(topo, B, gn_gate=gate, seeds=[21] * B, **{k: v for k, v in dkw.items() if k != "seed"})
    K = topo.k_paths
    with device_log_in_oracle():
        gos = [ref.GatedOracle(topo, okw, gate, seed=21, j=j, reward_mode=1) for _ in range(B)]
        for t in range(n):
            acts = [go.o.policy("deeprmsa_sap_ff")[0] for go in gos]
            if t % 5 == 4:
                acts[1] = K * j + (t % 3)   # out of range: a rejection, no check
            rows = [go.step(*go.resolve_deeprmsa(a)) for go, a in zip(gos, acts)]
            tr = env.run("deeprmsa_external", 1, actions=np.array(acts, np.int32), outputs=OUTS, auto_reset=True)
            assert env.last_kernel().startswith(kernel_name("wave", env.words_per_link, "full", gn=True)), env.last_kernel()
            for i, row in enumerate(rows):
                want = {k: np.array([v]) for k, v in row.items()}
                _steps_match(tr, i, want, (t, i))
                assert tr["reward"][0, i] == row["reward"], (t, i)
                if t % 5 == 4 and i == 1:
                    assert np.isnan(tr["gn_gsnr_db"][0, i]) and not tr["accepted"][0, i]
    assert all(go.checks > 50 and go.rejects > 0 for go in gos), [(go.checks, go.rejects) for go in gos]
    for i, go in enumerate(gos):
        assert np.array_equal(env.available_slots()[i], go.o.available_slots()), i
        go.close()
    env.close()


def test_external_actions_occupied_and_out_of_range():
    """policy "external" / "path_ff_external": an occupied window and an action out of range give NaN and run no check; a free
    window is checked whoever proposed it."""
    case = "nsfnet_s320_l150_sapff"
    env, topo, c = _gated_env(case, 2, seeds=[11, 11])
    K, S = topo.k_paths, c["S"]
    n = 150
    occupied = checked = 0
    with device_log_in_oracle():
        gos = [ref.GatedOracle(topo, ref.case_kwargs(case), ref.case_gate(topo), seed=11) for _ in range(2)]
        for t in range(n):
            acts = []
            for i, go in enumerate(gos):
                p, s = go.propose("sap_ff")
                if i == 1 and t % 3 == 1 and p < K:   # an occupied window of the proposed path, if it has one
                    nsl = go.o.number_slots(p)
                    busy = [q for q in range(S) if not go.o.is_path_free(p, q, nsl)]
                    if busy:
                        s = busy[len(busy) // 2]
                        occupied += 1
                elif i == 1 and t % 3 == 2:           # out of range, in either component
                    p, s = (K, S) if t % 2 else (p, S + 3)
                acts.append((p, s))
            rows = [go.step(p, s) for go, (p, s) in zip(gos, acts)]
            tr = env.run("external", 1, actions=np.array(acts, np.int32), outputs=OUTS, auto_reset=True)
            for i, row in enumerate(rows):
                _steps_match(tr, i, {k: np.array([v]) for k, v in row.items()}, (t, i))
                checked += int(np.isfinite(row["gsnr"]))
                if i == 1 and t % 3 == 2:   # out of range: no check ran
                    assert np.isnan(tr["gn_gsnr_db"][0, i]) and not tr["accepted"][0, i]
        # PathOnlyFirstFitAction on the same handles: the path from the caller, the slot by first fit, then the check
        for t in range(20):
            paths = [go.propose("sap_ff")[0] for go in gos]
            rows = []
            for go, p in zip(gos, paths):
                s = S
                if p < K:
                    nsl = go.o.number_slots(p)
                    s = next(q for q in range(S - nsl) if go.o.is_path_free(p, q, nsl))
                rows.append(go.step(p, s))
            tr = env.run("path_ff_external", 1, actions=np.array(paths, np.int32), outputs=OUTS, auto_reset=True)
            for i, row in enumerate(rows):
                _steps_match(tr, i, {k: np.array([v]) for k, v in row.items()}, ("path_ff", t, i))
    assert occupied > 20 and checked > 100 and gos[1].rejects > 0
    for i, go in enumerate(gos):
        assert np.array_equal(env.available_slots()[i], go.o.available_slots()), i
        go.close()
    env.close()


def test_work_queue_beyond_the_resident_waves():
    """B = 4200, more environments than the device keeps waves resident (4096): the first wave of environments is taken
    statically, the rest by ticket; six environments across that boundary against their own gated oracles."""
    case = "nsfnet_s320_l50_sapff"
    B, n = 4200, 200
    env, topo, c = _gated_env(case, B)   # environment i: seed 10 + i
    tr = env.run(c["policy"], n, outputs=OUTS, auto_reset=True)
    assert env.last_kernel().startswith("orlg_rmsa_kernel<5,2,false,true>"), env.last_kernel()
    state = _state(env)
    for i in (0, 4095, 4096, 4097, 4150, 4199):
        want, final, fig = ref.run_case(case, seed=c["seed"] + i, n_steps=n)
        assert fig["checks"] > 0
        _steps_match(tr, i, want, i)
        state_matches(state, i, final, i)
    env.close()


def test_a_gate_that_passes_everything_is_the_ungated_kernel():
    """Thresholds at -1e9: every per-step output and the saved state byte-identical to a handle without a gate on the same seeds
    (the yardstick is the existing kernel); a snapshot crosses between the two handles and both continue alike."""
    from optical_rl_gym_amd import BatchedRMSAEnv
    case = "nsfnet_s320_l150_sapff"
    c = ref.CASES[case]
    topo = load_topology(c["topology"])
    kw = ref.case_kwargs(case)
    outs = ("act_path", "act_slot", "accepted", "done", "reward", "request", "arrival", "holding", "network_compactness",
            "network_compactness_difference", "avg_link_compactness", "avg_link_utilization")
    B = 16
    gated = BatchedRMSAEnv(topo, B, gn_gate=ref.case_gate(topo, thresholds_db=[-1e9] * 6), **kw)
    plain = BatchedRMSAEnv(topo, B, **kw)

    def both(policy, n, **k):
        a = gated.run(policy, n, outputs=outs + ("gn_gsnr_db",), auto_reset=True, **k)
        b = plain.run(policy, n, outputs=outs, auto_reset=True, **k)
        assert gated.last_kernel().startswith("orlg_rmsa_kernel<5,2,false,true>"), gated.last_kernel()
        assert ",false,true>" not in plain.last_kernel(), plain.last_kernel()
        for name in outs:
            assert a[name].tobytes() == b[name].tobytes(), (policy, n, name)
        assert np.array_equal(np.isfinite(a["gn_gsnr_db"]), a["act_path"] < topo.k_paths)   # every proposal was checked, and passed
        assert np.array_equal(a["accepted"] != 0, a["act_path"] < topo.k_paths)
        assert gated.save_state().tobytes() == plain.save_state().tobytes(), (policy, n)

    both("sap_ff", 300)
    both("llp_ff", 40)
    both("sap_ff", 1)
    # the gate is configuration, not state: snapshots cross
    sg, sp = gated.save_state(), plain.save_state()
    assert sg.size == sp.size
    both("sap_ff", 50)
    later = gated.save_state()
    gated.load_state(sp)
    plain.load_state(sg)
    both("sap_ff", 50)
    assert gated.save_state().tobytes() == later.tobytes()
    # a handle without a gate asked for the output: no check ran
    r = plain.run("sap_ff", 2, outputs=("gn_gsnr_db", "accepted"))
    assert np.isnan(r["gn_gsnr_db"]).all() and r["gn_gsnr_db"].shape == (2, B)
    gated.close()
    plain.close()


def test_refusals():
    from optical_rl_gym_amd import BatchedRMSAEnv, OrlgError, _lib
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    kw = dict(num_spectrum_resources=100, load=20, mean_service_holding_time=25, seed=1)
    g = ref.case_gate(topo)
    with pytest.raises(ValueError, match="group"):
        BatchedRMSAEnv(topo, 4, gn_gate=g, step_kernel="group", **kw)
    with pytest.raises(ValueError, match="thresholds_db has 3 entries"):
        BatchedRMSAEnv(topo, 4, gn_gate=dict(g, thresholds_db=g["thresholds_db"][:3]), **kw)

    # the library's own refusals (a caller of the C ABI)
    def gate_struct(d):
        gg, keep = _lib.RmsaGnGate(), []
        for name in ("launch_power_density_w_hz", "frequency_start_hz", "slot_width_hz", "attenuation_normalized", "noise_figure"):
            setattr(gg, name, float(d[name]))
        for name, dt in (("link_num_spans", np.int32), ("link_span_length_km", np.float64), ("thresholds_db", np.float64)):
            a = np.ascontiguousarray(d[name], dt)
            keep.append(a)
            setattr(gg, name, a.ctypes.data_as(C.c_void_p))
        gg.num_thresholds = len(d["thresholds_db"])
        return gg, keep

    grp = BatchedRMSAEnv(topo, 4, step_kernel="group", **kw)
    gg, keep = gate_struct(g)
    assert grp.L.orlg_set_gn_gate(grp.h, C.byref(gg)) == -1
    assert b"GROUP" in grp.L.orlg_last_error()
    grp.run("sap_ff", 5)
    assert grp.last_kernel().startswith("orlg_rmsa_group_kernel"), grp.last_kernel()
    grp.close()
    env = BatchedRMSAEnv(topo, 4, **kw)
    for bad, word in ((dict(g, thresholds_db=g["thresholds_db"][:3]), b"spectral efficiency"),
                      (dict(g, noise_figure=float("nan")), b"noise_figure"), (dict(g, slot_width_hz=0.0), b"slot_width_hz"),
                      (dict(g, launch_power_density_w_hz=-1.0), b"launch_power_density_w_hz")):
        gg, keep = gate_struct(bad)
        assert env.L.orlg_set_gn_gate(env.h, C.byref(gg)) == -1 and word in env.L.orlg_last_error(), word
    # a refused gate leaves the handle without one; a set gate can be taken off again
    r = env.run("sap_ff", 3, outputs=("gn_gsnr_db",))
    assert np.isnan(r["gn_gsnr_db"]).all() and "false,true>" not in env.last_kernel()
    gg, keep = gate_struct(g)
    _lib.check(env.L.orlg_set_gn_gate(env.h, C.byref(gg)))
    r = env.run("sap_ff", 3, outputs=("gn_gsnr_db",))
    assert np.isfinite(r["gn_gsnr_db"]).any() and env.last_kernel().startswith("orlg_rmsa_kernel<2,2,false,true>")
    _lib.check(env.L.orlg_set_gn_gate(env.h, None))
    env.run("sap_ff", 3)
    assert "false,true>" not in env.last_kernel()
    with pytest.raises(OrlgError):
        _lib.check(env.L.orlg_set_gn_gate(None, None))
    env.close()


def test_views_forward_the_gate():
    from optical_rl_gym_amd import DeepRMSAEnv, RMSAEnv, shortest_available_path_first_fit
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    g = ref.case_gate(topo)
    env = RMSAEnv(topology=topo, num_spectrum_resources=100, load=20, mean_service_holding_time=25, seed=13, gn_gate=g)
    seen = []
    for _ in range(30):
        _, _, _, info = env.step(shortest_available_path_first_fit(env))
        seen.append(info["gn_gsnr_db"])
    assert np.isfinite(seen).any()
    env.close()
    env = RMSAEnv(topology=topo, num_spectrum_resources=100, load=20, mean_service_holding_time=25, seed=13)
    assert "gn_gsnr_db" not in env.step(shortest_available_path_first_fit(env))[3]
    env.close()
    env = DeepRMSAEnv(topology=topo, num_spectrum_resources=100, seed=13, gn_gate=g)
    assert "gn_gsnr_db" in env.step(0)[3]
    env.close()
