"""Assignment rules behind the GN-model admission check on the device (``orlg_step_rule_gn`` / ``run(..., gn_rule=)``,
``orlg_gn_path_windows`` / ``path_rule_windows``), held to the CPU reference of ``gn_rules_reference.py``: decisions,
windows and masks exact, GSNR to rtol 1e-9 (the tolerance ``test_gpu_rmsa_gn_gate.py`` uses for the same arithmetic) with NaN in
the same places; to the gated step itself bit for bit; and to each other across launch shapes, batch sizes, buffers and views.
The conditions these comparisons rest on (margins to the thresholds, refusals, later paths, windows other than first fit) are
held by ``test_gn_rules_args.py`` on the oracle alone, for the cases of ``gn_rules_reference.GPU_CASES``."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import gn_gate_reference as ref
import gn_rules_reference as gref
from conftest import load_topology
from gpu_support import COMPACTNESS, RMSA_OUTS, against_oracle, rmsa_env, same_bytes, snapshot, state_matches, topology

pytestmark = pytest.mark.gpu

RTOL = 1e-9
B = gref.B
OUTS = RMSA_OUTS + ("gn_gsnr_db",)
NSFNET = "nsfnet_chen_5-paths_6-modulations"
GN_CAUSE = 6   # ORLG_CAUSE_GN


def _gsnr_matches(dev, want, what):
    assert np.array_equal(np.isnan(dev), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.allclose(dev[ok], want[ok], rtol=RTOL, atol=0), (what, float(np.max(np.abs(dev[ok] / want[ok] - 1))))


def _setup(name, batch=B, gated=True, gate_over=None, **over):
    """(handle, topology, keyword arguments, case) of a name of GPU_CASES"""
    c = gref.GPU_CASES[name]
    case = gref.gpu_case(name)
    topo, kw, _ = ref.resolve_case(case, "unused")
    kw.update(over)
    gate = ref.case_gate(topo, **dict(dict(c["gate"]), **(gate_over or {}))) if gated else None
    return rmsa_env(topo, batch, gn_gate=gate, **kw), topo, kw, c


def _reference(name, **kw):
    c = gref.GPU_CASES[name]
    return gref.run_batch(gref.gpu_case(name), c["route"], c["rule"], c["mode"], n_steps=c["n"], gate_items=c["gate"], **kw)


def _policy(c):
    return gref.policy_name(c["route"], c["rule"])


def _decisions_match(tr, runs, what):
    for i, (want, _, _) in enumerate(runs):
        for f in ("act_path", "act_slot", "accepted", "done", "request"):
            assert np.array_equal(tr[f][:, i], want[f]), (what, f, i, np.flatnonzero(np.atleast_2d(tr[f][:, i] != want[f]).T.any(axis=1))[:4])
        _gsnr_matches(tr["gn_gsnr_db"][:, i], want["gsnr"], (what, i))


# ---------------------------------------------------------------------------------------- 1. one launch against the reference
LEVELS = [(name, "full") for name in sorted(gref.GPU_CASES)] + [
    (name, level) for name in sorted(gref.GPU_CASES) if gref.GPU_CASES[name]["levels"] for level in ("counters", "network")]


@pytest.mark.parametrize("name,level", LEVELS)
def test_one_launch_against_the_reference(name, level):
    """Decisions and GSNR per step for every environment; occupancy, counters, clock and (level full) link statistics of the first
    and the last environment against the oracle driven through `external` with the admitted actions."""
    env, topo, kw, c = _setup(name, stats_level=level)
    runs = _reference(name)
    tr = env.run(_policy(c), c["n"], outputs=OUTS, auto_reset=True, gn_rule=c["mode"])
    said = env.last_kernel()
    snap = snapshot(env)
    env.close()
    cut = ",true" if c["rule"] == "min_cut" else ""
    assert said.startswith("orlg_rmsa_kernel<%d,%d,false,true,false,true%s>" % (c["W"], ("counters", "network", "full").index(level), cut)), said
    _decisions_match(tr, runs, name)
    for i, (_, final, _) in enumerate(runs):
        state_matches(snap, i, final, (name, i), link_stats=False)
    K, S = topo.k_paths, kw["num_spectrum_resources"]
    acc = tr["accepted"] != 0
    actions = np.stack([np.where(acc, tr["act_path"], K), np.where(acc, tr["act_slot"], S)], axis=-1).astype(np.int32)
    fields = ("accepted", "arrival", "holding") + (COMPACTNESS if level != "counters" else ())
    against_oracle(topo, kw, dict(tr=tr, snap=snap), "external", c["n"], (0, B - 1), level, actions=actions, fields=fields)


# ---------------------------------------------------------------------------------------- 2. launch shapes; the query per step
@pytest.mark.parametrize("name", sorted(gref.GPU_CASES))
def test_every_launch_shape_has_the_same_bits(name):
    """One launch of N steps, N launches of one step, a 7 / N - 7 split: the same outputs and the same saved state.  Before every
    one-step launch the query of the case's rule equals the reference's rows: windows and admitted exact, GSNR to rtol 1e-9."""
    c = gref.GPU_CASES[name]
    n, policy = c["n"], _policy(c)
    runs = _reference(name)
    env, topo, kw, _ = _setup(name)
    one = env.run(policy, n, outputs=OUTS, auto_reset=True, gn_rule=c["mode"])
    state = env.save_state()
    env.close()
    env, _, _, _ = _setup(name)
    steps = []
    for t in range(n):
        slots, gsnr, adm = env.path_rule_windows(c["rule"])
        for i, (want, _, _) in enumerate(runs):
            assert np.array_equal(slots[i], want["q_slots"][t]) and np.array_equal(adm[i], want["q_admitted"][t]), (name, t, i)
            _gsnr_matches(gsnr[i], want["q_gsnr"][t], (name, "query", t, i))
        steps.append(env.run(policy, 1, outputs=OUTS, auto_reset=True, gn_rule=c["mode"]))
    for k in OUTS:
        assert np.concatenate([s[k] for s in steps]).tobytes() == one[k].tobytes(), (name, k)
    assert env.save_state().tobytes() == state.tobytes()
    env.close()
    env, _, _, _ = _setup(name)
    parts = [env.run(policy, m, outputs=OUTS, auto_reset=True, gn_rule=c["mode"]) for m in (7, n - 7)]
    for k in OUTS:
        assert np.concatenate([s[k] for s in parts]).tobytes() == one[k].tobytes(), (name, k)
    assert env.save_state().tobytes() == state.tobytes()
    env.close()


# ---------------------------------------------------------------------------------------- 3. the agent's path
@pytest.mark.parametrize("name,rule", gref.PATH_CASES)
def test_the_agents_path_under_check(name, rule):
    """path_<rule>_external with random paths -1 .. k + 1 (k and the values on both sides of the range are rejections)."""
    env, topo, kw, _ = _setup(name)
    n, paths = gref.PATH_STEPS, gref.path_actions(topo.k_paths)
    assert {-1, topo.k_paths, topo.k_paths + 1} <= set(paths.ravel().tolist())
    runs = gref.run_path_case(name, rule)
    policy = gref.policy_name("path", rule)
    steps = [env.run(policy, 1, actions=paths[t], outputs=OUTS, auto_reset=True, gn_rule="check") for t in range(n)]
    tr = {k: np.concatenate([s[k] for s in steps]) for k in OUTS}
    snap = snapshot(env, save_state=False)
    env.close()
    _decisions_match(tr, runs, (name, rule))
    out_of_range = (paths < 0) | (paths >= topo.k_paths)
    assert (tr["act_path"][out_of_range] == topo.k_paths).all() and np.isnan(tr["gn_gsnr_db"][out_of_range]).all()
    refused = ~np.isnan(tr["gn_gsnr_db"]) & (tr["accepted"] == 0)
    assert refused.sum() > 0 and (tr["accepted"] != 0).sum() > 0
    for i, (_, final, _) in enumerate(runs):
        state_matches(snap, i, final, (name, rule, i), link_stats=False)


# ---------------------------------------------------------------------------------------- 4. the blocking cause
@pytest.mark.parametrize("name", sorted(gref.GPU_CASES))
def test_block_cause(name):
    """block_cause == GN exactly where the GSNR is not NaN and the step is not accepted; every cause_counts row sums to the
    launch's steps; the classifier changes no other output and no state."""
    c = gref.GPU_CASES[name]
    env, topo, kw, _ = _setup(name)
    plain = env.run(_policy(c), c["n"], outputs=OUTS, auto_reset=True, gn_rule=c["mode"])
    state = env.save_state()
    env.close()
    env, _, _, _ = _setup(name)
    tr = env.run(_policy(c), c["n"], outputs=OUTS + ("block_cause",), auto_reset=True, cause_counts=True, gn_rule=c["mode"])
    cut = ",true" if c["rule"] == "min_cut" else ""
    assert env.last_kernel().startswith("orlg_rmsa_kernel<%d,2,false,true,true,true%s>" % (c["W"], cut)), env.last_kernel()
    for k in OUTS:
        assert tr[k].tobytes() == plain[k].tobytes(), (name, k)
    assert env.save_state().tobytes() == state.tobytes()
    env.close()
    cause, counts = tr["block_cause"], tr["block_cause_counts"]
    gn = ~np.isnan(tr["gn_gsnr_db"]) & (tr["accepted"] == 0)
    assert np.array_equal(cause == GN_CAUSE, gn) and gn.sum() >= 10
    assert np.array_equal(cause == 0, tr["accepted"] != 0)
    assert (counts.sum(axis=1) == c["n"]).all()
    for code in range(8):
        assert np.array_equal(counts[:, code], (cause == code).sum(axis=0)), code


# ---------------------------------------------------------------------------------------- 5. a gate that passes everything
@pytest.mark.parametrize("name,policy,mode", [
    ("w5_l150_sap_best_next", "sap_bf", "next_path"), ("w5_l150_sap_best_next", "llp_lf", "check"), ("w5_l50_sap_mincut_next", "sap_mc", "next_path"),
    ("w5_l50_sap_mincut_next", "min_cut", "check"), ("w2_sap_last_check", "sp_ef", "check"), ("w1_sap_last_check", "sap_ff_full", "next_path")])
def test_a_gate_that_passes_everything(name, policy, mode):
    """At 0 dBm per 50 GHz the gate refuses nothing: run(name, gn_rule=) on the gated handle is run(name) on a handle without a
    gate from the same seed, byte for byte -- decisions and saved state; the snapshots cross between the two."""
    a, _, _, _ = _setup(name, gate_over=dict(launch_power_dbm_per_50ghz=0.0))
    b, _, _, _ = _setup(name, gated=False)
    outs = RMSA_OUTS
    for n in (1, 150, 1):
        ra, rb = a.run(policy, n, outputs=outs + ("gn_gsnr_db",), auto_reset=True, gn_rule=mode), b.run(policy, n, outputs=outs, auto_reset=True)
        for k in outs:
            assert ra[k].tobytes() == rb[k].tobytes(), (n, k)
        assert not ((ra["accepted"] == 0) & ~np.isnan(ra["gn_gsnr_db"])).any()
        assert a.save_state().tobytes() == b.save_state().tobytes(), n
    sa = a.save_state()
    ra = a.run(policy, 20, outputs=outs, auto_reset=True, gn_rule=mode)
    b.load_state(sa)
    rb = b.run(policy, 20, outputs=outs, auto_reset=True)
    sb = b.save_state()
    a.load_state(sb)
    for k in outs:
        assert ra[k].tobytes() == rb[k].tobytes(), k
    assert a.save_state().tobytes() == sb.tobytes()
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------- 6. the query is the step
@pytest.mark.parametrize("name", ["w5_l150_sap_best_next", "w2_sap_last_check", "ring36_w8_check", "w1_sap_last_check"])
def test_the_query_is_the_step_bit_for_bit(name):
    """From one saved state (B = 32, after 120 steps): path_<rule>_external on every path in turn accepts exactly where
    `admitted` says so, at the query's slot, with the bytes of the query's GSNR; "first" is action_masks("path_ff_gn") byte for
    byte; under next_path a step accepts iff an admitted column is set and shows the first such column."""
    c = gref.GPU_CASES[name]
    batch = 32
    env, topo, kw, _ = _setup(name, batch=batch)
    K, S = topo.k_paths, kw["num_spectrum_resources"]
    env.run("sap_ff", 120, auto_reset=True)
    state = env.save_state()
    refused = accepted = 0
    for rule in gref.RULES[1:]:
        env.load_state(state)
        slots, gsnr, adm = env.path_rule_windows(rule)
        assert slots.dtype == np.int16 and gsnr.dtype == np.float64 and adm.dtype == np.uint8 and slots.shape == gsnr.shape == adm.shape == (batch, K)
        assert np.array_equal(np.isnan(gsnr), slots == S) and not adm[slots == S].any()
        for p in range(K):
            env.load_state(state)
            r = env.run(gref.policy_name("path", rule), 1, actions=np.full(batch, p, np.int32), outputs=("act_path", "act_slot", "accepted", "gn_gsnr_db"),
                        gn_rule="check")
            assert np.array_equal(r["accepted"][0], adm[:, p]), (rule, p)
            assert np.array_equal(r["act_slot"][0], slots[:, p]), (rule, p)
            assert np.array_equal(r["act_path"][0], np.where(slots[:, p] < S, p, K)), (rule, p)
            assert np.ascontiguousarray(r["gn_gsnr_db"][0]).tobytes() == np.ascontiguousarray(gsnr[:, p]).tobytes(), (rule, p)
        refused += int(((slots < S) & (adm == 0)).sum())
        accepted += int(adm.sum())
        # next_path on route sap: accepts iff a column is set, the first such column; refused: the first path with a window
        env.load_state(state)
        r = env.run(gref.policy_name("sap", rule), 1, outputs=("act_path", "act_slot", "accepted", "gn_gsnr_db"), gn_rule="next_path")
        acc = r["accepted"][0] != 0
        assert np.array_equal(acc, adm.any(axis=1)), rule
        has = (slots < S).any(axis=1)
        shown = np.where(acc, adm.argmax(axis=1), np.where(has, (slots < S).argmax(axis=1), K))
        assert np.array_equal(r["act_path"][0], shown), rule
        rows = np.flatnonzero(has)
        assert np.array_equal(r["act_slot"][0][rows], slots[rows, shown[rows]]), rule
        assert r["gn_gsnr_db"][0][rows].tobytes() == gsnr[rows, shown[rows]].tobytes(), rule
        assert np.isnan(r["gn_gsnr_db"][0][~has]).all() and (r["act_slot"][0][~has] == S).all(), rule
    assert refused > 0 and accepted > 0
    env.load_state(state)
    slots, gsnr, adm = env.path_rule_windows("first")
    mask, mg = env.action_masks("path_ff_gn", gsnr_out=True)
    assert adm.tobytes() == np.ascontiguousarray(mask[:, :K]).tobytes() and gsnr.tobytes() == mg.tobytes()
    assert np.array_equal(slots == S, np.isnan(mg))
    assert env.save_state().tobytes() == state.tobytes()   # the queries read state only
    env.close()


# ---------------------------------------------------------------------------------------- 7. beyond the resident waves
def test_beyond_the_resident_waves():
    """B = 4200, across the boundary between the environments taken statically and by ticket: its first environments have the
    bytes of the B = 4 run, and environments on both sides of the boundary agree with the reference."""
    name, n = "w5_l150_sap_best_next", 100
    c = gref.GPU_CASES[name]
    small, _, kw, _ = _setup(name)
    big, _, _, _ = _setup(name, batch=4200)
    a = small.run(_policy(c), n, outputs=OUTS, auto_reset=True, gn_rule=c["mode"])
    b = big.run(_policy(c), n, outputs=OUTS, auto_reset=True, gn_rule=c["mode"])
    assert big.last_kernel().startswith("orlg_rmsa_kernel<5,2,false,true,false,true>"), big.last_kernel()
    for k in OUTS:
        assert np.ascontiguousarray(b[k][:, :B]).tobytes() == a[k].tobytes(), k
    for i in (4095, 4096, 4199):
        want, _, _ = gref.run_case(gref.gpu_case(name), c["route"], c["rule"], c["mode"], seed=kw["seed"] + i, n_steps=n, gate_items=c["gate"])
        for f in ("act_path", "act_slot", "accepted", "done"):
            assert np.array_equal(b[f][:, i], want[f]), (f, i)
        _gsnr_matches(b["gn_gsnr_db"][:, i], want["gsnr"], i)
    for x, y in zip(small.path_rule_windows(c["rule"]), big.path_rule_windows(c["rule"])):
        assert np.ascontiguousarray(y[:B]).tobytes() == x.tobytes()
    small.close()
    big.close()


# ---------------------------------------------------------------------------------------- 8. kernel selection
def test_kernel_selection():
    """A new launch names a new instantiation; an old name on the same handle, and a handle without a gate, launch what they
    launched."""
    env, topo, kw, _ = _setup("w5_l150_sap_best_next")
    first = lambda: env.last_kernel().split(" ")[0]
    for policy, mode, want in (("sap_bf", "check", "false,true,false,true>"), ("sap_bf", "next_path", "false,true,false,true>"),
                               ("llp_ef", "check", "false,true,false,true>"), ("sap_mc", "next_path", "false,true,false,true,true>"),
                               ("min_cut", "check", "false,true,false,true,true>")):
        env.run(policy, 3, gn_rule=mode)
        assert first() == "orlg_rmsa_kernel<5,2," + want, (policy, mode, first())
        env.run(policy, 20, gn_rule=mode, cause_counts=True)
        assert first() == "orlg_rmsa_kernel<5,2," + want.replace("true,false,true", "true,true,true", 1), (policy, mode, first())
    for policy in ("sap_ff", "sap_ff_gn", "llp_ff"):
        env.run(policy, 3)
        assert first() == "orlg_rmsa_kernel<5,2,false,true>", (policy, first())
    env.run("sap_ff", 3, cause_counts=True)
    assert first() == "orlg_rmsa_kernel<5,2,false,true,true>", first()
    env.path_rule_windows("best")
    env.close()
    env, _, _, _ = _setup("w5_l150_sap_best_next", gated=False)
    for policy, want in (("sap_ff", "orlg_rmsa_kernel_ff<5,2>"), ("sap_bf", "orlg_rmsa_kernel<5,2,false,false,false,true>"),
                         ("sap_mc", "orlg_rmsa_kernel<5,2,false,false,false,true,true>")):
        env.run(policy, 3)
        assert first() == want, (policy, first())
    env.close()


# ---------------------------------------------------------------------------------------- 9. the library's own refusals
def test_refusals_of_the_library():
    from optical_rl_gym_amd import OrlgError, _lib
    SP, SAP, LLP, PATH, CUTS = 0, 1, 2, 6, _lib.ROUTE_FEWEST_CUTS
    MC, MU, ANY = _lib.RULE_FEWEST_CUTS, _lib.RULE_MOST_USED, _lib.ROUTE_BEST_WINDOW
    env, topo, kw, _ = _setup("w2_sap_last_check")
    env.run("sap_lf", 40, auto_reset=True, gn_rule="check")
    before = snapshot(env)
    io = _lib.StepIO()
    call = lambda e, route, rule, mode, n=1, actions=None: e.L.orlg_step_rule_gn(e.h, route, rule, mode, n, actions, 1, C.byref(io), None)
    err = lambda e: e.L.orlg_last_error()
    for route in (-1, 3, 4, 5, 7, 8, 9, 99):
        assert call(env, route, 3, 0) == -1 and b"needs a route" in err(env), route
    for rule in (-1, 5, 6, 99, 101):
        assert call(env, SAP, rule, 0) == -1 and b"needs a rule" in err(env), rule
    assert call(env, SAP, 0, 0) == -1 and b"ORLG_ASSIGN_FIRST" in err(env)
    for mode in (-1, 2, 99):
        assert call(env, SAP, 3, mode) == -1 and b"gn_mode" in err(env), mode
    for route in (SP, LLP, PATH, CUTS):
        assert call(env, route, MC if route == CUTS else 3, 1) == -1 and b"NEXT_PATH" in err(env), route
    for rule in (1, 2, 3, 4):
        assert call(env, CUTS, rule, 0) == -1 and b"ORLG_RULE_FEWEST_CUTS" in err(env), rule
    assert call(env, SAP, MU, 0) == -1 and b"MOST_USED" in err(env)
    assert call(env, ANY, 3, 0) == -1 and b"BEST_WINDOW" in err(env)
    assert call(env, PATH, 3, 0) == -1 and b"action array" in err(env)          # the agent's path needs its actions
    assert call(env, SAP, 3, 0, n=0) == -1 and b"n_steps" in err(env)
    out = np.zeros((B, topo.k_paths), np.int16)
    ptr = out.ctypes.data_as(C.c_void_p)
    for rule in (-1, 5, 99, 100, 101):
        assert env.L.orlg_gn_path_windows(env.h, rule, ptr, None, None) == -1 and b"unknown rule" in err(env), rule
    assert env.L.orlg_gn_path_windows(env.h, 3, None, None, None) == -1 and b"null argument" in err(env)
    # the entries that refused a gated handle before still do, in the library and in Python
    d = _lib.StepDiag(None, None, None)
    assert env.L.orlg_step_assign(env.h, SAP, 3, 1, None, 1, C.byref(io), C.byref(d)) == -1 and b"gn_gate" in err(env)
    assert env.L.orlg_step_min_cut(env.h, SAP, 1, None, 1, C.byref(io), C.byref(d)) == -1 and b"gn_gate" in err(env)
    assert env.L.orlg_step_window(env.h, SAP, 3, 1, None, 1, C.byref(io), C.byref(d)) == -1 and b"gn_gate" in err(env)
    for policy in ("sap_bf", "sap_mc", "sap_mu"):
        with pytest.raises(ValueError, match="gn_gate"):
            env.run(policy, 1)
    same_bytes(snapshot(env), before, "refusals on a gated handle")
    assert env.L.orlg_gn_path_windows(env.h, 3, ptr, None, None) == 0 and (out <= kw["num_spectrum_resources"]).all()   # one buffer alone
    env.run("sap_lf", 3, gn_rule="next_path")   # the handle goes on
    env.close()
    env, _, _, _ = _setup("w2_sap_last_check", gated=False)
    env.run("sap_lf", 40, auto_reset=True)
    before = snapshot(env)
    for mode in (0, 1):
        assert call(env, SAP, 3, mode) == -1 and b"no gn_gate" in err(env)
    assert env.L.orlg_gn_path_windows(env.h, 3, ptr, None, None) == -1 and b"gn_gate" in err(env)
    with pytest.raises(ValueError, match="gn_gate"):
        env.run("sap_lf", 1, gn_rule="check")
    with pytest.raises(OrlgError):
        _lib.check(call(env, SAP, 3, 0))
    same_bytes(snapshot(env), before, "refusals on a handle without a gate")
    env.close()


# ---------------------------------------------------------------------------------------- 10. views and callbacks
def test_views_and_callbacks_against_the_batched_trace():
    from optical_rl_gym_amd import RMSAEnv, assignment_heuristic, evaluate_heuristic_batched, min_cut_heuristic
    topo = load_topology(NSFNET)
    gate = ref.case_gate(topo)
    kw = dict(num_spectrum_resources=320, load=150, mean_service_holding_time=25, seed=11, episode_length=200)
    cases = ((assignment_heuristic("sap", "best", gn="next_path"), "sap_bf", "next_path"),
             (assignment_heuristic("llp", "last", gn="check"), "llp_lf", "check"),
             (min_cut_heuristic("sap", gn="next_path"), "sap_mc", "next_path"),
             (min_cut_heuristic("min_cut", gn="check"), "min_cut", "check"))
    for heuristic, policy, mode in cases:
        view, dev = RMSAEnv(topology=topo, gn_gate=gate, **kw), rmsa_env(topo, 1, gn_gate=gate, **kw)
        refused = 0
        for t in range(150):
            p, s = heuristic(view)
            _, _, done, info = view.step((p, s))
            r = dev.run(policy, 1, outputs=("act_path", "act_slot", "accepted", "done", "gn_gsnr_db"), gn_rule=mode)
            assert (p, s) == (int(r["act_path"][0, 0]), int(r["act_slot"][0, 0])), (policy, mode, t)
            assert view._last_served.accepted == bool(r["accepted"][0, 0]) and done == bool(r["done"][0, 0]), (policy, mode, t)
            assert np.array([info["gn_gsnr_db"]]).tobytes() == r["gn_gsnr_db"][0].tobytes(), (policy, mode, t)
            refused += int(not r["accepted"][0, 0] and not np.isnan(r["gn_gsnr_db"][0, 0]))
        assert refused > 0, (policy, mode)
        assert np.array_equal(view._batched.occupancy_words(), dev.occupancy_words())
        view.close()
        dev.close()
    # evaluate_heuristic_batched forwards the keyword
    a, b = (rmsa_env(topo, 4, gn_gate=gate, **dict(kw, episode_length=50)) for _ in range(2))
    rewards, lengths, _ = evaluate_heuristic_batched(a, "sap_bf", n_eval_episodes=2, gn_rule="next_path")
    assert rewards.shape == (2, 4) and (lengths == 49).all() and (rewards > 0).all()
    want = []
    for _ in range(2):
        b.reset(only_episode_counters=True)
        want.append(b.run("sap_bf", 49, outputs=("reward",), gn_rule="next_path")["reward"].sum(axis=0))
    assert np.array_equal(rewards, np.stack(want))
    with pytest.raises(ValueError, match="gn_gate"):
        evaluate_heuristic_batched(a, "sap_bf", n_eval_episodes=1)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------- 11. buffers
def test_buffers_pageable_pinned_device():
    """The query into pageable, pinned and device (torch) buffers: the same bytes.  In a child process: torch has to create its
    HIP context before the library does."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys
        import numpy as np, torch
        torch.zeros(1, device="cuda")
        sys.path[:0] = [%r, %r]
        import gn_gate_reference as ref
        from conftest import load_topology
        from optical_rl_gym_amd import BatchedRMSAEnv
        case = "nsfnet_s320_l150_sapff"
        topo = load_topology(ref.CASES[case]["topology"])
        env = BatchedRMSAEnv(topo, 64, gn_gate=ref.case_gate(topo), **ref.case_kwargs(case))
        env.run("sap_bf", 150, auto_reset=True, gn_rule="next_path")
        shape = (64, topo.k_paths)
        for rule in ("first", "best", "min_cut"):
            s, g, a = env.path_rule_windows(rule)
            assert 0 < a.mean() < 1 and np.isfinite(g).any() and ((s < 320) & (a == 0)).any()
            hs, hg, ha = np.full(shape, 9, np.int16), np.full(shape, 7.0), np.full(shape, 9, np.uint8)
            r = env.path_rule_windows(rule, slots_out=hs, gsnr_out=hg, admitted_out=ha)
            assert r[0] is hs and r[1] is hg and r[2] is ha
            assert hs.tobytes() == s.tobytes() and hg.tobytes() == g.tobytes() and ha.tobytes() == a.tobytes()
            ps, pg, pa = (torch.full(shape, 9, dtype=dt).pin_memory() for dt in (torch.int16, torch.float64, torch.uint8))
            env.path_rule_windows(rule, slots_out=ps, gsnr_out=pg, admitted_out=pa)
            env.synchronize()
            assert ps.numpy().tobytes() == s.tobytes() and pg.numpy().tobytes() == g.tobytes() and pa.numpy().tobytes() == a.tobytes()
            ds, dg, da = (torch.full(shape, 9, dtype=dt, device="cuda") for dt in (torch.int16, torch.float64, torch.uint8))
            torch.cuda.synchronize()
            env.path_rule_windows(rule, slots_out=ds, gsnr_out=dg, admitted_out=da)
            env.synchronize()
            assert ds.cpu().numpy().tobytes() == s.tobytes() and dg.cpu().numpy().tobytes() == g.tobytes() and da.cpu().numpy().tobytes() == a.tobytes()
            # mixed: device slots, pageable GSNR, pinned admitted
            ds.fill_(9); hg[:] = 7.0; pa.fill_(9); torch.cuda.synchronize()
            env.path_rule_windows(rule, slots_out=ds, gsnr_out=hg, admitted_out=pa)
            env.synchronize()
            assert ds.cpu().numpy().tobytes() == s.tobytes() and hg.tobytes() == g.tobytes() and pa.numpy().tobytes() == a.tobytes()
        env.close()
        print("gn rule buffers ok")
    """) % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "gn rule buffers ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
