"""A GN-model admission check that protects the running lightpaths (``include/orlg.h`` ``orlg_set_gn_protect``) on
the device, held to the CPU protecting oracle of ``gn_protect_reference.py``: decisions, requests, counters, occupancy and clock
exact; ``gn_gsnr_db`` to rtol 1e-9 (the tolerance of the gate); ``gn_neighbour_margin_db`` to atol = 1e-9 x the largest
|GSNR| the oracle computed in the case -- the same tolerance carried to a difference of a GSNR and a threshold --; NaN exactly
where the oracle ran no check.  Every test here needs ``orlg_set_gn_protect``."""
import ctypes as C

import numpy as np
import pytest

import gn_protect_reference as pref
from conftest import deeprmsa_to_rmsa_kwargs, load_topology
from gpu_support import device_log_in_oracle, rmsa_env, snapshot, state_matches

pytestmark = pytest.mark.gpu

RTOL = 1e-9
OUTS = ("act_path", "act_slot", "accepted", "done", "request", "reward", "gn_gsnr_db", "gn_neighbour_margin_db")


def protect_name(W, level, cause=False):
    """what last_kernel() starts with on a protecting handle (csrc/orlg_variants.h orlg_kernel_name)"""
    return f"orlg_rmsa_kernel<{W},{level},false,true,{'true' if cause else 'false'},false,false,false,true>"


def _same_nan(dev, want, what):
    assert np.array_equal(np.isnan(dev), np.isnan(want)), (what, np.flatnonzero(np.isnan(dev) != np.isnan(want))[:6])
    return ~np.isnan(want)


def _steps_match(tr, i, want, atol, what, rows=slice(None), pairs=None):
    """per-step outputs of environment i against the protecting oracle's arrays; atol: of the margin -- None: the (device, oracle)
    margins go to `pairs`, for a caller whose oracle is still running (_margins_match)"""
    for name in ("act_path", "act_slot", "accepted", "done", "request"):
        assert np.array_equal(tr[name][:, i], want[name][rows]), (what, name)
    dev, ref = tr["gn_gsnr_db"][:, i], want["gsnr"][rows]
    ok = _same_nan(dev, ref, (what, "gsnr"))
    assert np.allclose(dev[ok], ref[ok], rtol=RTOL, atol=0), (what, float(np.max(np.abs(dev[ok] / ref[ok] - 1))))
    dev, ref = tr["gn_neighbour_margin_db"][:, i], want["margin"][rows]
    ok = _same_nan(dev, ref, (what, "margin"))
    if atol is None:
        pairs.extend(zip(dev[ok], ref[ok]))
    else:
        assert np.allclose(dev[ok], ref[ok], rtol=0, atol=atol), (what, float(np.max(np.abs(dev[ok] - ref[ok]))), atol)


def _margins_match(pairs, oracles):
    """the margins collected over a step-by-step run, to 1e-9 x the largest |GSNR| its oracles computed"""
    d = np.array(pairs)
    atol = RTOL * max(po.max_abs_gsnr for po in oracles)
    assert len(d) and np.allclose(d[:, 0], d[:, 1], rtol=0, atol=atol), (float(np.max(np.abs(d[:, 0] - d[:, 1]))), atol)


def _concat(a, b):
    return {k: np.concatenate([a[k], b[k]]) for k in a}


def _env(case, B, protect=True, stats_level="full", seeds=None, gate_over=None, **over):
    c = pref.CASES[case]
    topo = load_topology(c["topology"])
    kw = pref.case_kwargs(case, **over)
    if seeds is not None:
        kw.pop("seed")
    gate = None if protect is None else pref.case_gate(topo, protect=protect, **(gate_over or {}))
    return rmsa_env(topo, B, gn_gate=gate, stats_level=stats_level, seeds=seeds, **kw), topo, c


def _rows(row):
    return {k: np.array([v]) for k, v in row.items()}


@pytest.mark.parametrize("case", list(pref.CASES))
def test_case_against_the_protecting_oracle(case):
    """B = 8 environments on the case's seed + 0 .. 7: 599 steps in one launch, one more in its own."""
    env, topo, c = _env(case, pref.B)
    assert env.gn_protect
    tr = _concat(env.run(c["policy"], pref.N_STEPS - 1, outputs=OUTS, auto_reset=True),
                 env.run(c["policy"], 1, outputs=OUTS, auto_reset=True))
    assert env.last_kernel().startswith(protect_name(env.words_per_link, 2)), env.last_kernel()
    state = snapshot(env, save_state=False)
    for i, (want, final, fig) in enumerate(pref.run_batch(case)):
        assert int(np.isfinite(tr["gn_neighbour_margin_db"][:, i]).sum()) == fig["n_checks"]
        _steps_match(tr, i, want, RTOL * fig["max_abs_gsnr"], (case, i))
        state_matches(state, i, final, (case, i))
    env.close()


def test_statistics_levels_decide_alike():
    case = "nsfnet_s320_l150_sapff"
    want, final, fig = pref.run_case(case)
    for level, stats in enumerate(("counters", "network", "full")):
        env, topo, c = _env(case, 2, stats_level=stats, seeds=[pref.CASES[case]["seed"]] * 2)
        tr = env.run(c["policy"], pref.N_STEPS, outputs=OUTS, auto_reset=True)
        assert env.last_kernel().startswith(protect_name(env.words_per_link, level)), env.last_kernel()
        state = snapshot(env, save_state=False)
        for i in range(2):
            _steps_match(tr, i, want, RTOL * fig["max_abs_gsnr"], (stats, i))
            state_matches(state, i, final, (stats, i))
        env.close()


@pytest.mark.parametrize("case", ["nsfnet_s320_l150_llpff", "ring34_s100_l60_sapff"])
def test_block_cause_is_gn_exactly_on_the_steps_either_check_refused(case):
    from optical_rl_gym_amd import _lib
    GN = _lib.BLOCK_CAUSES.index("gn")
    env, topo, c = _env(case, pref.B)
    n = 300
    tr = env.run(c["policy"], n, outputs=OUTS + ("block_cause",), cause_counts=True, auto_reset=True)
    assert env.last_kernel().startswith(protect_name(env.words_per_link, 2, cause=True)), env.last_kernel()
    refused = (tr["accepted"] == 0) & np.isfinite(tr["gn_gsnr_db"])
    assert np.array_equal(tr["block_cause"] == GN, refused)
    assert np.array_equal((tr["block_cause"] == 0), tr["accepted"] != 0)
    counts = tr["block_cause_counts"]
    assert counts.shape == (pref.B, _lib.NUM_CAUSES) and (counts.sum(axis=1) == n).all() and (counts[:, 7] == 0).all()
    assert np.array_equal(counts[:, GN], refused.sum(axis=0))
    for i, (want, final, fig) in enumerate(pref.run_batch(case, n_steps=n)):
        _steps_match(tr, i, want, RTOL * fig["max_abs_gsnr"], (case, i))
    # both kinds of refusal occur: by the neighbour check (a margin below zero) and by the candidate's own check (no margin)
    assert (refused & (tr["gn_neighbour_margin_db"] < 0)).any() and (refused & np.isnan(tr["gn_neighbour_margin_db"])).any()
    env.close()


@pytest.mark.parametrize("case", pref.SAP_GN_CASES)
def test_sap_ff_gn_goes_on_after_either_refusal(case):
    env, topo, c = _env(case, pref.B)
    tr = env.run("sap_ff_gn", pref.N_STEPS, outputs=OUTS, auto_reset=True)
    assert env.last_kernel().startswith(protect_name(env.words_per_link, 2)), env.last_kernel()
    state = snapshot(env, save_state=False)
    later = 0
    for i, (want, final, fig) in enumerate(pref.run_batch(case, policy="sap_ff_gn")):
        _steps_match(tr, i, want, RTOL * fig["max_abs_gsnr"], (case, i))
        state_matches(state, i, final, (case, i))
        later += fig["later_taken"]
    assert later >= 5
    env.close()


def test_agent_driven_deeprmsa_and_path_first_fit():
    """BatchedDeepRMSAEnv, j = 1, NSFNET S = 320: 150 launches of one step -- environment 0 takes the oracle's deeprmsa_sap_ff
    action, environment 1 the same but an action out of range every fifth step --, then 40 launches of path_ff_external."""
    from optical_rl_gym_amd import BatchedDeepRMSAEnv
    topo = load_topology(pref.NSF)
    dkw = dict(mean_service_holding_time=25.0, mean_service_inter_arrival_time=25.0 / 150, num_spectrum_resources=320,
               episode_length=pref.EPISODE_LENGTH, seed=21, j=1)
    okw, j = deeprmsa_to_rmsa_kwargs(dkw)
    gate = pref.case_gate(topo)
    B, n = 2, 150
    env = BatchedDeepRMSAEnv(topo, B, gn_gate=gate, seeds=[21] * B, **{k: v for k, v in dkw.items() if k != "seed"})
    K, S = topo.k_paths, 320
    pairs = []
    with device_log_in_oracle():
        pos = [pref.ProtectingOracle(topo, okw, gate, seed=21, j=j, reward_mode=1) for _ in range(B)]
        for t in range(n):
            acts = [po.o.policy("deeprmsa_sap_ff")[0] for po in pos]
            if t % 5 == 4:
                acts[1] = K * j + (t % 3)   # out of range: a rejection, no check
            rows = [po.step(*po.resolve_deeprmsa(a)) for po, a in zip(pos, acts)]
            tr = env.run("deeprmsa_external", 1, actions=np.array(acts, np.int32), outputs=OUTS, auto_reset=True)
            assert env.last_kernel().startswith(protect_name(env.words_per_link, 2)), env.last_kernel()
            for i, row in enumerate(rows):
                _steps_match(tr, i, _rows(row), None, (t, i), pairs=pairs)
                assert tr["reward"][0, i] == row["reward"], (t, i)
                if t % 5 == 4 and i == 1:
                    assert np.isnan(tr["gn_gsnr_db"][0, i]) and np.isnan(tr["gn_neighbour_margin_db"][0, i]) and not tr["accepted"][0, i]
        for t in range(40):   # PathOnlyFirstFitAction: the path from the caller, the slot by first fit, then both checks
            paths = [po.propose("sap_ff")[0] for po in pos]
            rows = []
            for po, p in zip(pos, paths):
                s = S
                if p < K:
                    nsl = po.o.number_slots(p)
                    s = next(q for q in range(S - nsl) if po.o.is_path_free(p, q, nsl))
                rows.append(po.step(p, s))
            tr = env.run("path_ff_external", 1, actions=np.array(paths, np.int32), outputs=OUTS, auto_reset=True)
            for i, row in enumerate(rows):
                _steps_match(tr, i, _rows(row), None, ("path_ff", t, i), pairs=pairs)
    _margins_match(pairs, pos)
    assert all(po.n_checks > 50 and po.n_rejects > 0 for po in pos), [po.figures() for po in pos]
    for i, po in enumerate(pos):
        assert np.array_equal(env.available_slots()[i], po.o.available_slots()), i
        po.close()
    env.close()


def test_external_actions_occupied_and_out_of_range():
    """policy "external": an occupied window and an action out of range give NaN in both outputs and run no check."""
    case = "nsfnet_s320_l150_sapff"
    seed = pref.CASES[case]["seed"]
    env, topo, c = _env(case, 2, seeds=[seed, seed])
    K, S = topo.k_paths, c["S"]
    occupied = outside = 0
    pairs = []
    with device_log_in_oracle():
        pos = [pref.ProtectingOracle(topo, pref.case_kwargs(case), pref.case_gate(topo), seed=seed) for _ in range(2)]
        for t in range(150):
            acts = []
            for i, po in enumerate(pos):
                p, s = po.propose("sap_ff")
                if i == 1 and t % 3 == 1 and p < K:   # an occupied window of the proposed path, if it has one
                    nsl = po.o.number_slots(p)
                    busy = [q for q in range(S) if not po.o.is_path_free(p, q, nsl)]
                    if busy:
                        s = busy[len(busy) // 2]
                        occupied += 1
                elif i == 1 and t % 3 == 2:           # out of range, in either component
                    p, s = (K, S) if t % 2 else (p, S + 3)
                    outside += 1
                acts.append((p, s))
            rows = [po.step(p, s) for po, (p, s) in zip(pos, acts)]
            tr = env.run("external", 1, actions=np.array(acts, np.int32), outputs=OUTS, auto_reset=True)
            for i, row in enumerate(rows):
                _steps_match(tr, i, _rows(row), None, (t, i), pairs=pairs)
            if t % 3:
                if np.isnan(rows[1]["gsnr"]):
                    assert np.isnan(tr["gn_gsnr_db"][0, 1]) and np.isnan(tr["gn_neighbour_margin_db"][0, 1]) and not tr["accepted"][0, 1]
    _margins_match(pairs, pos)
    # (environment 1 provisions a third of its requests and stays lightly loaded: both checks run there, the refusals of the
    # neighbour check are environment 0's, which follows sap_ff)
    assert occupied > 20 and outside > 40 and pos[1].n_checks > 0 and pos[0].n_rejects > 0
    for i, po in enumerate(pos):
        assert np.array_equal(env.available_slots()[i], po.o.available_slots()), i
        po.close()
    env.close()


def test_a_launch_continued_with_the_ring_head_wrapped():
    """Two calls of 300 steps on a release queue of 80 slots: each call releases more services than the ring holds, so the second
    starts with the head wrapped, and the neighbour check walks the ring across its end."""
    case = "nsfnet_s320_l50_sapff"
    env, topo, c = _env(case, pref.B, queue_capacity=80)
    a = env.run(c["policy"], 300, outputs=OUTS, auto_reset=True)
    released = a["accepted"].sum(axis=0) - env.num_running()
    assert (released > 80).all(), released
    tr = _concat(a, env.run(c["policy"], 300, outputs=OUTS, auto_reset=True))
    assert ((tr["accepted"].sum(axis=0) - env.num_running()) - released > 80).all()
    state = snapshot(env, save_state=False)
    for i, (want, final, fig) in enumerate(pref.run_batch(case)):
        _steps_match(tr, i, want, RTOL * fig["max_abs_gsnr"], (case, i))
        state_matches(state, i, final, (case, i))
    env.close()


def test_work_queue_beyond_the_resident_waves():
    """B = 4200, more environments than the device keeps waves resident (4096): the first wave of environments is taken
    statically, the rest by ticket; six environments across that boundary against their own protecting oracles."""
    case = "nsfnet_s320_l50_sapff"
    B, n = 4200, 200
    env, topo, c = _env(case, B)   # environment i: seed 2 + i
    tr = env.run(c["policy"], n, outputs=OUTS, auto_reset=True)
    assert env.last_kernel().startswith(protect_name(5, 2)), env.last_kernel()
    state = snapshot(env, save_state=False)
    for i in (0, 4095, 4096, 4097, 4150, 4199):
        want, final, fig = pref.run_case(case, seed=c["seed"] + i, n_steps=n)
        assert fig["n_checks"] > 0
        _steps_match(tr, i, want, RTOL * fig["max_abs_gsnr"], i)
        state_matches(state, i, final, i)
    env.close()


def test_protection_that_refuses_nothing_is_the_gated_kernel():
    """At 0 dBm per 50 GHz nothing is refused on NSFNET: the protecting handle is byte-identical in state and outputs to the gated
    handle on the same seeds, and the second check ran.  Snapshots cross all three kinds of handle."""
    case = "nsfnet_s320_l150_sapff"
    outs = ("act_path", "act_slot", "accepted", "done", "reward", "request", "arrival", "holding", "network_compactness",
            "network_compactness_difference", "avg_link_compactness", "avg_link_utilization", "gn_gsnr_db")
    B = 16
    over = dict(launch_power_dbm_per_50ghz=0.0)
    prot, topo, c = _env(case, B, gate_over=over)
    gated, _, _ = _env(case, B, protect=False, gate_over=over)
    plain, _, _ = _env(case, B, protect=None)
    assert prot.gn_protect and not gated.gn_protect and not plain.gn_protect

    def both(policy, n):
        a = prot.run(policy, n, outputs=outs + ("gn_neighbour_margin_db",), auto_reset=True)
        b = gated.run(policy, n, outputs=outs + ("gn_neighbour_margin_db",), auto_reset=True)
        assert prot.last_kernel().startswith(protect_name(5, 2)), prot.last_kernel()
        assert gated.last_kernel().startswith("orlg_rmsa_kernel<5,2,false,true>"), gated.last_kernel()
        for name in outs:
            assert a[name].tobytes() == b[name].tobytes(), (policy, n, name)
        assert np.isnan(b["gn_neighbour_margin_db"]).all()          # a handle that does not protect: no second check
        m = a["gn_neighbour_margin_db"]
        assert not (m < 0).any() and not (np.isfinite(m) & ~np.isfinite(a["gn_gsnr_db"])).any()
        assert prot.save_state().tobytes() == gated.save_state().tobytes(), (policy, n)
        return m

    assert np.isfinite(both("sap_ff", 300)).mean() > 0.5
    both("llp_ff", 40)
    both("sap_ff_gn", 40)
    both("sap_ff", 1)
    # protection is configuration, not state: snapshots cross all three kinds of handle
    for policy, n in (("sap_ff", 300), ("llp_ff", 40), ("sap_ff", 40), ("sap_ff", 1)):   # (sap_ff_gn is sap_ff where nothing is refused)
        plain.run(policy, n, auto_reset=True)
    assert plain.save_state().tobytes() == prot.save_state().tobytes()
    sp, sg, su = prot.save_state(), gated.save_state(), plain.save_state()
    assert sp.size == sg.size == su.size
    both("sap_ff", 50)
    later = prot.save_state()
    prot.load_state(su); gated.load_state(sp); plain.load_state(sg)
    both("sap_ff", 50)
    plain.run("sap_ff", 50, auto_reset=True)
    assert prot.save_state().tobytes() == later.tobytes() == plain.save_state().tobytes()
    r = plain.run("sap_ff", 2, outputs=("gn_neighbour_margin_db", "accepted"))
    assert np.isnan(r["gn_neighbour_margin_db"]).all() and r["gn_neighbour_margin_db"].shape == (2, B)
    for e in (prot, gated, plain):
        e.close()


def test_a_snapshot_of_an_unprotecting_handle_is_loaded_and_nothing_is_torn_down():
    """A state the gated handle built at +6 dBm: loaded into a protecting handle, every service stays, the next request is the
    same, and a step whose neighbour margin is below zero is a refusal."""
    case = "nsfnet_s320_l150_sapff"
    prot, topo, c = _env(case, 4)
    gated, _, _ = _env(case, 4, protect=False)
    gated.run("sap_ff", 300, auto_reset=True)
    prot.load_state(gated.save_state())
    assert np.array_equal(prot.num_running(), gated.num_running()) and np.array_equal(prot.occupancy_words(), gated.occupancy_words())
    a = prot.run("sap_ff", 100, outputs=OUTS, auto_reset=True)
    b = gated.run("sap_ff", 1, outputs=OUTS[:-1], auto_reset=True)
    assert np.array_equal(a["request"][0], b["request"][0])
    below = a["gn_neighbour_margin_db"] < 0
    assert below.any() and not a["accepted"][below].any()
    assert a["accepted"][np.isfinite(a["gn_neighbour_margin_db"]) & ~below].all()
    prot.close(); gated.close()


def test_c_level_refusals():
    from optical_rl_gym_amd import BatchedRMSAEnv, OrlgError, _lib
    topo = load_topology(pref.NSF)
    kw = dict(num_spectrum_resources=100, load=20, mean_service_holding_time=25, seed=1)
    B = 4
    env = BatchedRMSAEnv(topo, B, **kw)
    L = env.L
    # no gate: the setter refuses, and the step's margin is all NaN
    assert L.orlg_set_gn_protect(env.h, 1) == -1 and b"gn_gate" in L.orlg_last_error()
    assert L.orlg_set_gn_protect(None, 1) == -1
    r = env.run("sap_ff", 3, outputs=("gn_neighbour_margin_db", "gn_gsnr_db"))
    assert np.isnan(r["gn_neighbour_margin_db"]).all() and np.isnan(r["gn_gsnr_db"]).all()
    env.close()
    g = pref.case_gate(topo, protect=False)
    env = BatchedRMSAEnv(topo, B, gn_gate=g, **kw)
    _lib.check(L.orlg_set_gn_protect(env.h, 1))
    env.run("sap_ff", 5)
    assert env.last_kernel().startswith(protect_name(2, 2)), env.last_kernel()
    # the three entries that know the candidate's own check only name the limit
    m, f = np.zeros((B, topo.k_paths), np.uint8), np.zeros((B, topo.k_paths))
    assert L.orlg_gn_action_masks(env.h, m.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), None, None) == -1
    assert b"protects its running lightpaths" in L.orlg_last_error()
    s16 = np.zeros((B, topo.k_paths), np.int16)
    assert L.orlg_gn_path_windows(env.h, 0, s16.ctypes.data_as(C.c_void_p), None, None) == -1
    assert b"protects its running lightpaths" in L.orlg_last_error()
    io = _lib.StepIO()
    assert L.orlg_step_rule_gn(env.h, _lib.POLICIES["sap_ff"], 3, 0, 2, None, 0, C.byref(io), None) == -1
    assert b"protects its running lightpaths" in L.orlg_last_error()
    # every pointer of the new entry may be NULL; a new gate keeps the protection, no gate clears it
    _lib.check(L.orlg_step_gn_protect(env.h, _lib.POLICIES["sap_ff"], 2, None, 0, None, None, None))
    gg = _lib.RmsaGnGate()
    for name in ("launch_power_density_w_hz", "frequency_start_hz", "slot_width_hz", "attenuation_normalized", "noise_figure"):
        setattr(gg, name, float(g[name]))
    keep = [np.ascontiguousarray(g["link_num_spans"], np.int32), np.ascontiguousarray(g["link_span_length_km"], np.float64),
            np.ascontiguousarray(g["thresholds_db"], np.float64)]
    gg.link_num_spans, gg.link_span_length_km, gg.thresholds_db = (a.ctypes.data_as(C.c_void_p) for a in keep)
    gg.num_thresholds = len(keep[2])
    _lib.check(L.orlg_set_gn_gate(env.h, C.byref(gg)))
    env.run("sap_ff", 2)
    assert env.last_kernel().startswith(protect_name(2, 2)), env.last_kernel()
    _lib.check(L.orlg_set_gn_protect(env.h, 0))
    env.run("sap_ff", 2)
    assert env.last_kernel().startswith("orlg_rmsa_kernel<2,2,false,true>") and not env.last_kernel().startswith(protect_name(2, 2))
    _lib.check(L.orlg_gn_action_masks(env.h, m.ctypes.data_as(C.c_void_p), None, None, None))   # served again
    _lib.check(L.orlg_set_gn_protect(env.h, 1))
    _lib.check(L.orlg_set_gn_gate(env.h, None))
    env.run("sap_ff", 2)
    assert "false,true" not in env.last_kernel().split(" ")[0], env.last_kernel()
    _lib.check(L.orlg_set_gn_gate(env.h, C.byref(gg)))   # a gate after none: not protecting
    env.run("sap_ff", 2)
    assert env.last_kernel().startswith("orlg_rmsa_kernel<2,2,false,true>") and not env.last_kernel().startswith(protect_name(2, 2))
    with pytest.raises(OrlgError):
        _lib.check(L.orlg_set_gn_protect(None, 0))
    env.close()


def test_views_forward_the_protection():
    from optical_rl_gym_amd import DeepRMSAEnv, RMSAEnv, shortest_available_path_first_fit
    topo = load_topology(pref.NSF)
    g = pref.case_gate(topo)
    env = RMSAEnv(topology=topo, num_spectrum_resources=100, load=20, mean_service_holding_time=25, seed=13, gn_gate=g)
    seen = []
    for _ in range(60):
        _, _, _, info = env.step(shortest_available_path_first_fit(env))
        seen.append((info["gn_gsnr_db"], info["gn_neighbour_margin_db"]))
    seen = np.array(seen)
    assert np.isfinite(seen[:, 1]).any() and not (np.isfinite(seen[:, 1]) & np.isnan(seen[:, 0])).any()
    with pytest.raises(ValueError, match="protects its running lightpaths"):
        env._batched.action_masks("path_ff_gn")
    env.close()
    env = RMSAEnv(topology=topo, num_spectrum_resources=100, load=20, mean_service_holding_time=25, seed=13,
                  gn_gate=pref.case_gate(topo, protect=False))
    info = env.step(shortest_available_path_first_fit(env))[3]
    assert "gn_gsnr_db" in info and "gn_neighbour_margin_db" not in info
    env.close()
    env = DeepRMSAEnv(topology=topo, num_spectrum_resources=100, seed=13, gn_gate=g)
    info = env.step(0)[3]
    assert "gn_gsnr_db" in info and "gn_neighbour_margin_db" in info
    env.close()
