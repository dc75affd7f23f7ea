"""The GN gate's rule launches (``run(..., gn_rule=)``, ``path_rule_windows``) and its protection of the running
lightpaths (``protect_running=True``) at every shape: above eight candidate paths at one to six words per link (the
six grids of ``gpu_support.MANY_PATHS``), with continuous bit rates (up to 256 rate indices in the queue descriptors the checks
decode), with per-environment loads and on a replayed trace.  Every batch is held to its CPU oracle as the modules of the shipped
topologies hold theirs (``test_gpu_gn_protect.py``, ``test_gpu_gn_rules.py``): decisions, requests, counters, occupancy and clock
exact, ``gn_gsnr_db`` to rtol 1e-9, ``gn_neighbour_margin_db`` to atol = 1e-9 x the largest |GSNR| of the batch, NaN in the same
places.  ``test_gn_shapes_args.py`` pins from the oracles alone what each batch exercises."""
import numpy as np
import pytest

import gn_gate_reference as ref
import gn_protect_reference as pref
import gn_rules_reference as gref
import gn_shapes_reference as sh
from gpu_support import MANY_PATHS, kernel_name, rmsa_env, same_bytes, snapshot, state_matches, topology

pytestmark = pytest.mark.gpu

RTOL = 1e-9
P_OUTS = ("act_path", "act_slot", "accepted", "done", "request", "reward", "gn_gsnr_db", "gn_neighbour_margin_db")
G_OUTS = P_OUTS[:-1]
N = sh.N_STEPS


def protect_name(W, level=2, cause=False):
    """what last_kernel() starts with on a protecting handle (csrc/orlg_variants.h orlg_kernel_name)"""
    return f"orlg_rmsa_kernel<{W},{level},false,true,{'true' if cause else 'false'},false,false,false,true>"


def rule_name(W, cut, cause=False):
    return "orlg_rmsa_kernel<%d,2,false,true,%s,true%s>" % (W, "true" if cause else "false", ",true" if cut else "")


def _kernel(env):
    return env.last_kernel().split()[0]


def _close(dev, want, what, rtol=RTOL, atol=0.0):
    assert np.array_equal(np.isnan(dev), np.isnan(want)), (what, np.flatnonzero(np.isnan(dev) != np.isnan(want))[:6])
    ok = ~np.isnan(want)
    assert np.allclose(dev[ok], want[ok], rtol=rtol, atol=atol), (what, float(np.max(np.abs(dev[ok] - want[ok]))), rtol, atol)


def _steps_match(tr, i, want, what, margin_atol=None):
    """per-step outputs of environment i against an oracle's arrays; margin_atol: the protecting oracle's margin too"""
    for name in ("act_path", "act_slot", "accepted", "done", "request"):
        differ = tr[name][:, i] != want[name]
        bad = np.flatnonzero(differ.reshape(len(differ), -1).any(axis=1))
        assert bad.size == 0, (what, name, "first at step", int(bad[0]), tr[name][bad[0], i], want[name][bad[0]])
    _close(tr["gn_gsnr_db"][:, i], want["gsnr"], (what, "gsnr"))
    if margin_atol is not None:
        _close(tr["gn_neighbour_margin_db"][:, i], want["margin"], (what, "margin"), rtol=0, atol=margin_atol)


def _batch_matches(tr, state, runs, what, protect):
    atol = RTOL * max(fig["max_abs_gsnr"] for _, _, fig in runs) if protect else None
    for i, (want, final, fig) in enumerate(runs):
        _steps_match(tr, i, want, (what, i), atol)
        if protect:
            assert int(np.isfinite(tr["gn_neighbour_margin_db"][:, i]).sum()) == fig["n_checks"], (what, i)
        state_matches(state, i, final, (what, i), link_stats=False)


def _handle(topo, kw, seeds, protect, **over):
    dev_kw = {k: v for k, v in kw.items() if k != "seed"}
    gate = pref.case_gate(topo, protect=True) if protect else ref.case_gate(topo)
    return rmsa_env(topo, len(seeds), gn_gate=gate, seeds=list(seeds), **dict(dev_kw, **over))


# ---------------------------------------------------------------------------------------- 1. protection, many paths
@pytest.mark.parametrize("name,policy", sh.PROTECT_BATCHES)
def test_protecting_batch_against_the_oracle(name, policy, tmp_path):
    """Eight environments (seeds 3 .. 10), 149 steps in one launch and one more in its own, against ProtectingOracle.  Above eight
    paths sap_ff_gn runs the general policy loop, which starts over behind a path either check refused (idp0 = sap.from) and
    reports the first candidate -- its GSNR and its margin -- when the paths end."""
    topo, kw, runs = sh.protect_batch(name, policy, tmp_path)
    env = _handle(topo, kw, sh.protect_seeds(name, policy), True)
    assert env.gn_protect and env.words_per_link == MANY_PATHS[name]["W"]
    a, b = (env.run(policy, n, outputs=P_OUTS, auto_reset=True) for n in (N - 1, 1))
    tr = {k: np.concatenate([a[k], b[k]]) for k in a}
    assert _kernel(env) == protect_name(MANY_PATHS[name]["W"]), env.last_kernel()
    _batch_matches(tr, snapshot(env, save_state=False), runs, (name, policy), True)
    env.close()


def test_protecting_block_cause(tmp_path):
    """k = 21, W = 3, sap_ff_gn with cause_counts: block_cause is GN exactly on the steps that either check refused."""
    from optical_rl_gym_amd import _lib
    GN = _lib.BLOCK_CAUSES.index("gn")
    topo, kw, runs = sh.protect_batch(sh.K21, "sap_ff_gn", tmp_path)
    env = _handle(topo, kw, sh.protect_seeds(sh.K21, "sap_ff_gn"), True)
    tr = env.run("sap_ff_gn", N, outputs=P_OUTS + ("block_cause",), cause_counts=True, auto_reset=True)
    assert _kernel(env) == protect_name(3, cause=True), env.last_kernel()
    _batch_matches(tr, snapshot(env, save_state=False), runs, "cause", True)
    refused = (tr["accepted"] == 0) & np.isfinite(tr["gn_gsnr_db"])
    assert np.array_equal(tr["block_cause"] == GN, refused) and np.array_equal(tr["block_cause"] == 0, tr["accepted"] != 0)
    want = np.stack([(w["accepted"] == 0) & np.isfinite(w["gsnr"]) for w, _, _ in runs], axis=1)
    assert np.array_equal(refused, want)
    counts = tr["block_cause_counts"]
    assert (counts.sum(axis=1) == N).all() and np.array_equal(counts[:, GN], refused.sum(axis=0))
    assert (refused & (tr["gn_neighbour_margin_db"] < 0)).any() and (refused & np.isnan(tr["gn_neighbour_margin_db"])).any()
    env.close()


@pytest.mark.parametrize("name", [sh.K32, sh.K10])
def test_protecting_one_step_launches_equal_one_launch(name, tmp_path):
    """sap_ff_gn as 150 launches of one step and as one launch of 150: the same bytes in every output and in the saved state (the
    retry state of a step does not outlive it)."""
    topo, kw, runs = sh.protect_batch(name, "sap_ff_gn", tmp_path)
    seeds = sh.protect_seeds(name, "sap_ff_gn")
    env = _handle(topo, kw, seeds, True)
    one = env.run("sap_ff_gn", N, outputs=P_OUTS, auto_reset=True)
    whole = snapshot(env)
    env.close()
    env = _handle(topo, kw, seeds, True)
    steps = [env.run("sap_ff_gn", 1, outputs=P_OUTS, auto_reset=True) for _ in range(N)]
    same_bytes(one, {k: np.concatenate([s[k] for s in steps]) for k in P_OUTS}, "outputs")
    same_bytes(whole, snapshot(env), "state")
    env.close()
    _batch_matches(one, whole, runs, name, True)


# ---------------------------------------------------------------------------------------- 2. rule launches, many paths
@pytest.mark.parametrize("name,route,rule,mode", sh.RULE_BATCHES)
def test_rule_batch_against_the_reference(name, route, rule, mode, tmp_path):
    """One launch against gn_rules_reference: decisions and GSNR per step, occupancy, counters and clock.  On the shapes of
    QUERY_SHAPES the run is repeated as launches of one step with path_rule_windows(rule) before each: slots and admitted exact,
    GSNR to rtol 1e-9, the step's own decision the row's entry, and the same bytes as the one launch."""
    topo, kw, runs = sh.rule_batch(name, route, rule, mode, tmp_path)
    batch, n = sh.rule_size(name, route, rule, mode)
    c = MANY_PATHS[name]
    K, S, policy = c["k"], c["S"], gref.policy_name(route, rule)
    seeds = range(kw["seed"], kw["seed"] + batch)
    env = _handle(topo, kw, seeds, False)
    tr = env.run(policy, n, outputs=G_OUTS, auto_reset=True, gn_rule=mode)
    assert _kernel(env) == rule_name(c["W"], rule == "min_cut"), env.last_kernel()
    state = snapshot(env)
    env.close()
    _batch_matches(tr, state, runs, (name, route, rule, mode), False)
    if name not in sh.QUERY_SHAPES:
        return
    env = _handle(topo, kw, seeds, False)
    steps = []
    for t in range(n):
        slots, gsnr, adm = env.path_rule_windows(rule)
        for i, (want, _, _) in enumerate(runs):
            assert np.array_equal(slots[i], want["q_slots"][t]) and np.array_equal(adm[i], want["q_admitted"][t]), (name, t, i, slots[i], want["q_slots"][t])
            _close(gsnr[i], want["q_gsnr"][t], (name, "query", t, i))
        r = env.run(policy, 1, outputs=G_OUTS, auto_reset=True, gn_rule=mode)
        # the step is the row: its path's entry of `admitted`, at the row's slot, with the bytes of the row's GSNR
        p, rows = r["act_path"][0], np.arange(batch)
        shown = p < K
        assert np.array_equal(r["accepted"][0][shown] != 0, adm[rows[shown], p[shown]] != 0), (name, t)
        assert np.array_equal(r["act_slot"][0][shown], slots[rows[shown], p[shown]]), (name, t)
        assert r["gn_gsnr_db"][0][shown].tobytes() == gsnr[rows[shown], p[shown]].tobytes(), (name, t)
        assert not r["accepted"][0][~shown].any() and np.isnan(r["gn_gsnr_db"][0][~shown]).all(), (name, t)
        if mode == "next_path":   # accepts iff a column is admitted: the first such; refused: the first path with a window
            acc = adm.any(axis=1)
            has = (slots < S).any(axis=1)
            want_p = np.where(acc, adm.argmax(axis=1), np.where(has, (slots < S).argmax(axis=1), K))
            assert np.array_equal(p, want_p) and np.array_equal(r["accepted"][0] != 0, acc), (name, t)
        steps.append(r)
    same_bytes({k: tr[k] for k in G_OUTS}, {k: np.concatenate([s[k] for s in steps]) for k in G_OUTS}, "outputs")
    assert env.save_state().tobytes() == state["state"].tobytes()
    env.close()


@pytest.mark.parametrize("name", sh.SHAPES)
def test_the_query_of_rule_first(name, tmp_path):
    """path_rule_windows("first") above eight paths reads the candidates W lanes apart (LS = W in orlg_gn_rule_kernels.hip; the other
    rules scan eight paths per pass): before each of 150 one-step launches of llp_lf under check, slots and admitted exact, GSNR
    to rtol 1e-9, and admitted / GSNR the bytes of action_masks("path_ff_gn", gsnr_out=True)."""
    topo, kw, runs = sh.first_query_batch(name, tmp_path)
    c = MANY_PATHS[name]
    K = c["k"]
    env = _handle(topo, kw, range(kw["seed"], kw["seed"] + sh.RULE_B), False)
    steps = []
    for t in range(N):
        slots, gsnr, adm = env.path_rule_windows("first")
        mask, mg = env.action_masks("path_ff_gn", gsnr_out=True)
        assert adm.tobytes() == np.ascontiguousarray(mask[:, :K]).tobytes() and gsnr.tobytes() == mg.tobytes(), (name, t)
        for i, (want, _) in enumerate(runs):
            assert np.array_equal(slots[i], want["f_slots"][t]) and np.array_equal(adm[i], want["f_admitted"][t]), (name, t, i, slots[i], want["f_slots"][t])
            _close(gsnr[i], want["f_gsnr"][t], (name, "first", t, i))
        steps.append(env.run("llp_lf", 1, outputs=G_OUTS, auto_reset=True, gn_rule="check"))
    assert _kernel(env) == rule_name(c["W"], False), env.last_kernel()
    tr = {k: np.concatenate([s[k] for s in steps]) for k in G_OUTS}
    state = snapshot(env, save_state=False)
    for i, (want, final) in enumerate(runs):
        _steps_match(tr, i, want, (name, i))
        state_matches(state, i, final, (name, i), link_stats=False)
    env.close()


@pytest.mark.parametrize("name,rule", sh.PATH_CASES)
def test_the_agents_path_on_the_high_paths(name, rule, tmp_path):
    """path_<rule>_external under gn_rule="check", 150 launches of one step: more than half the given paths lie in 8 .. K - 1 (the
    path column of external_actions(kind="high_paths")), K among them; accepted and refused steps on those paths."""
    topo, kw, paths, runs = sh.path_batch(name, rule, tmp_path)
    c = MANY_PATHS[name]
    K, B = c["k"], sh.RULE_B
    assert ((paths >= 8) & (paths < K)).mean() > 0.5 and (paths == K).any()
    env = _handle(topo, kw, range(kw["seed"], kw["seed"] + B), False)
    policy = gref.policy_name("path", rule)
    steps = [env.run(policy, 1, actions=paths[t], outputs=G_OUTS, auto_reset=True, gn_rule="check") for t in range(N)]
    assert _kernel(env) == rule_name(c["W"], rule == "min_cut"), env.last_kernel()
    tr = {k: np.concatenate([s[k] for s in steps]) for k in G_OUTS}
    _batch_matches(tr, snapshot(env, save_state=False), runs, (name, rule), False)
    high = (tr["act_path"] >= 8) & (tr["act_path"] < K)
    refused = np.isfinite(tr["gn_gsnr_db"]) & (tr["accepted"] == 0)
    print(name, rule, "accepted on a path >= 8:", int((high & (tr["accepted"] != 0)).sum()), "refused there:", int((high & refused).sum()))
    assert (high & (tr["accepted"] != 0)).sum() >= 10 and (high & refused).sum() >= 1
    assert (tr["act_path"][paths == K] == K).all() and np.isnan(tr["gn_gsnr_db"][paths == K]).all()
    env.close()


# ---------------------------------------------------------------------------------------- 3. every instantiation of a word count
LEVELS = ("counters", "network", "full")


@pytest.mark.parametrize("name", sh.SHAPES)
def test_every_instantiation_of_the_word_count(name, tmp_path):
    """The statistics levels and the blocking-cause classifier are template arguments too: per word count six protecting
    instantiations (sap_ff_gn) and twelve gated rule instantiations (sap_bf and sap_mc under next_path), each named by
    last_kernel() and held to the batch's oracle on decisions, GSNR, margin, counters, occupancy and clock."""
    W = MANY_PATHS[name]["W"]
    topo, kw, runs = sh.protect_batch(name, "sap_ff_gn", tmp_path)
    said = set()
    for level, stats in enumerate(LEVELS):
        for cause in (False, True):
            env = _handle(topo, kw, sh.protect_seeds(name, "sap_ff_gn"), True, stats_level=stats)
            tr = env.run("sap_ff_gn", N, outputs=P_OUTS, cause_counts=cause, auto_reset=True)
            assert _kernel(env) == protect_name(W, level, cause), env.last_kernel()
            said.add(_kernel(env))
            _batch_matches(tr, snapshot(env, save_state=False), runs, (name, stats, cause), True)
            env.close()
    for rule in ("best", "min_cut"):
        topo, kw, runs = sh.rule_batch(name, "sap", rule, "next_path", tmp_path)
        batch, n = sh.rule_size(name, "sap", rule, "next_path")
        for level, stats in enumerate(LEVELS):
            for cause in (False, True):
                env = _handle(topo, kw, range(kw["seed"], kw["seed"] + batch), False, stats_level=stats)
                tr = env.run(gref.policy_name("sap", rule), n, outputs=G_OUTS, cause_counts=cause, auto_reset=True, gn_rule="next_path")
                assert _kernel(env) == rule_name(W, rule == "min_cut", cause).replace(f"<{W},2,", f"<{W},{level},"), env.last_kernel()
                said.add(_kernel(env))
                _batch_matches(tr, snapshot(env, save_state=False), runs, (name, rule, stats, cause), False)
                env.close()
    assert len(said) == 18, sorted(said)


# ---------------------------------------------------------------------------------------- 4. continuous rates
def test_continuous_rates_on_a_protecting_handle():
    """Rates 100 .. 350: a running service's width comes from nslots[rate index x stride + SE] with up to 251 indices, in the
    own check and in the victims' checks."""
    topo, kw = sh.continuous_case()
    runs = sh.continuous_protect_runs()
    env = _handle(topo, kw, range(kw["seed"], kw["seed"] + sh.CONT_B), True)
    tr = env.run(sh.CONT_POLICY, sh.CONT_STEPS, outputs=P_OUTS, auto_reset=True)
    assert _kernel(env) == protect_name(5), env.last_kernel()
    _batch_matches(tr, snapshot(env, save_state=False), runs, "continuous", True)
    assert len(np.unique(tr["request"][..., 3][tr["accepted"] != 0])) >= 50
    env.close()


def test_continuous_rates_on_a_gated_handle():
    """The gated step against GatedOracle (300 steps); then, on a fresh handle after 200 steps of sap_ff, before each of 100 steps the path_ff_gn mask with
    its GSNR row against gn_candidates_reference and path_rule_windows("best") against gn_rules_reference, the step itself one
    sap_bf launch under gn_rule="next_path"."""
    topo, kw = sh.continuous_case()
    seeds = range(kw["seed"], kw["seed"] + sh.CONT_B)
    env = _handle(topo, kw, seeds, False)
    tr = env.run(sh.CONT_POLICY, sh.CONT_STEPS, outputs=G_OUTS, auto_reset=True)
    assert _kernel(env) == kernel_name("wave", 5, "full", gn=True), env.last_kernel()
    _batch_matches(tr, snapshot(env, save_state=False), sh.continuous_gated_runs(), "continuous gated", False)
    env.close()
    env = _handle(topo, kw, seeds, False)
    runs = [sh.continuous_query_run(s) for s in seeds]
    env.run(sh.CONT_POLICY, sh.CONT_WARMUP, auto_reset=True)
    K, steps = topo.k_paths, []
    for t in range(sh.CONT_QUERY_STEPS):
        mask, mg = env.action_masks("path_ff_gn", gsnr_out=True)
        slots, gsnr, adm = env.path_rule_windows("best")
        for i, (want, _) in enumerate(runs):
            assert np.array_equal(mask[i, :K], want["path_ff_gn"][t]), (t, i)
            _close(mg[i], want["path_ff_gsnr"][t], ("mask", t, i))
            assert np.array_equal(slots[i], want["q_slots"][t]) and np.array_equal(adm[i], want["q_admitted"][t]), (t, i)
            _close(gsnr[i], want["q_gsnr"][t], ("query", t, i))
        steps.append(env.run("sap_bf", 1, outputs=G_OUTS, auto_reset=True, gn_rule="next_path"))
    assert _kernel(env) == rule_name(5, False), env.last_kernel()
    tr = {k: np.concatenate([s[k] for s in steps]) for k in G_OUTS}
    state = snapshot(env, save_state=False)
    for i, (want, final) in enumerate(runs):
        _steps_match(tr, i, want, ("sap_bf", i))
        state_matches(state, i, final, ("sap_bf", i), link_stats=False)
    env.close()


# ---------------------------------------------------------------------------------------- 5. per-environment loads
@pytest.mark.parametrize("protect", [False, True])
def test_sweep_handle_against_the_oracle_of_each_load(protect):
    """make_sweep("rmsa"), loads 50 and 150 x seeds 2 .. 5 in one handle: every environment equals the oracle of its own load and
    seed on decisions, GSNR, margin and final state."""
    from optical_rl_gym_amd import make_sweep
    topo, _ = sh.sweep_case(sh.SWEEP_LOADS[0])
    gate = pref.case_gate(topo, protect=True) if protect else ref.case_gate(topo)
    env = make_sweep("rmsa", topo, loads=list(sh.SWEEP_LOADS), seeds_per_load=sh.SWEEP_SEEDS, seed=sh.SWEEP_SEED0, gn_gate=gate, **sh.SWEEP_KW)
    assert env.batch_size == len(sh.SWEEP_LOADS) * sh.SWEEP_SEEDS and env.gn_protect == protect
    tr = env.run(sh.SWEEP_POLICY, sh.SWEEP_STEPS, outputs=P_OUTS, auto_reset=True)
    assert _kernel(env) == (protect_name(5) if protect else kernel_name("wave", 5, "full", gn=True)), env.last_kernel()
    if not protect:
        assert np.isnan(tr["gn_neighbour_margin_db"]).all()
    _batch_matches(tr, snapshot(env, save_state=False), sh.sweep_runs(protect), "sweep", protect)
    env.close()


# ---------------------------------------------------------------------------------------- 6. a replayed trace
def test_trace_replay_on_a_protecting_handle():
    """record_trace from the protecting generated handle of a case test_gpu_gn_protect.py holds to the oracle; replayed on a
    protecting trace handle under the same policy every output, margin included, and the final occupancy are the same bytes.
    Replayed under llp_ff it is held to ProtectingOracle at the same seeds: the oracle's request stream does not depend on the
    decisions, so the oracle at seed s under llp_ff serves the recorded requests (the step comparison includes them) -- the
    means test_gpu_trace.py uses to feed an oracle a trace."""
    from optical_rl_gym_amd import record_trace
    case, B, n = sh.TRACE_CASE, sh.TRACE_B, sh.TRACE_STEPS
    c = pref.CASES[case]
    topo, kw = topology(c["topology"]), pref.case_kwargs(case)
    seeds = range(c["seed"], c["seed"] + B)
    gen = _handle(topo, kw, seeds, True)
    trace = record_trace(gen, c["policy"], n, outputs=P_OUTS, auto_reset=True)
    first, occ = trace.outputs, gen.occupancy_words().copy()
    gen.close()
    runs = pref.run_batch(case, n_steps=n, batch=B)
    for i, (want, _, fig) in enumerate(runs):
        _steps_match(first, i, want, ("generated", i), RTOL * fig["max_abs_gsnr"])
    tkw = dict(num_spectrum_resources=c["S"], episode_length=kw["episode_length"])
    gate = pref.case_gate(topo, protect=True)
    rep = rmsa_env(topo, B, gn_gate=gate, trace=trace, **tkw)
    again = rep.run(c["policy"], n, outputs=P_OUTS + ("arrival", "holding"), auto_reset=True)
    assert _kernel(rep) == protect_name(5), rep.last_kernel()
    same_bytes({k: first[k] for k in first}, {k: again[k] for k in first}, "replay")
    assert rep.occupancy_words().tobytes() == occ.tobytes()
    rep.close()
    rep = rmsa_env(topo, B, gn_gate=gate, trace=trace, **tkw)
    tr = rep.run("llp_ff", n, outputs=P_OUTS, auto_reset=True)
    state = snapshot(rep, save_state=False)
    rep.close()
    _batch_matches(tr, state, [pref.run_case(case, seed=s, n_steps=n, policy="llp_ff") for s in seeds], "trace llp_ff", True)
