"""The GN gate's rule launches and its protection of the running lightpaths at every shape, what needs no GPU: every batch of
``test_gpu_gn_shapes.py`` pinned from the oracles alone (``gn_shapes_reference.py``, the device's logarithm in them), so that no
comparison there can pass with the code it is about idle -- above eight candidate paths the neighbour check runs and refuses,
``sap_ff_gn`` goes on behind a neighbour refusal and lands on a path 8 or above, ``llp_ff`` has candidates on such paths refused,
the rules' windows are refused on the columns 8 and above and ``next_path`` takes a later path there; with continuous rates more
than 50 rate indices are lit at once among more than 64 running services; and no margin of any kind lies within 1e-6 dB of zero
(the GSNR is held to rtol 1e-9, about 2e-8 dB at 20 dB).  Each test prints its figures."""
import numpy as np
import pytest

import gn_protect_reference as pref
import gn_rules_reference as gref
import gn_shapes_reference as sh
from gpu_support import MANY_PATHS, many_paths_kwargs, many_paths_topology, topology


# ---------------------------------------------------------------------------------------- the pair form of the protecting oracle
def test_a_pair_is_cached_like_a_name(tmp_path):
    """run_case / run_batch of gn_protect_reference on a (topology, kwargs) pair: one run per process, read-only arrays, the
    kwargs' seed onwards, a policy required; the named cases as before."""
    pytest.importorskip("networkx")
    topo, kw = many_paths_topology(sh.K9, tmp_path), many_paths_kwargs(sh.K9)
    a = pref.run_case((topo, kw), policy="sap_ff_gn", n_steps=30)
    assert pref.run_case((topo, dict(kw)), policy="sap_ff_gn", n_steps=30, seed=kw["seed"]) is a and not a[0]["accepted"].flags.writeable
    assert pref.run_batch((topo, kw), policy="sap_ff_gn", n_steps=30, batch=2)[0] is a
    assert pref.run_batch((topo, kw), policy="sap_ff_gn", n_steps=30, batch=2)[1] is pref.run_case((topo, kw), seed=kw["seed"] + 1, policy="sap_ff_gn", n_steps=30)
    assert not np.array_equal(a[0]["request"], pref.run_case((topo, kw), seed=kw["seed"] + 1, policy="sap_ff_gn", n_steps=30)[0]["request"])
    with pytest.raises(AssertionError):
        pref.run_case((topo, kw), n_steps=30)   # a pair has no policy of its own
    case = "nsfnet_s100_l20_spff"
    named = pref.run_case(case, n_steps=30)
    assert pref.run_case(case, n_steps=30, seed=pref.CASES[case]["seed"], policy="sp_ff") is named
    assert pref.run_batch(case, n_steps=30, batch=2)[0] is named
    # ... and a name is what its kwargs are as a pair
    pair = pref.run_case((topology(pref.NSF), pref.case_kwargs(case)), policy="sp_ff", n_steps=30)
    for k in named[0]:
        assert np.array_equal(named[0][k], pair[0][k], equal_nan=named[0][k].dtype.kind == "f"), k
    assert named[2] == pair[2]


# ---------------------------------------------------------------------------------------- protection, many paths
@pytest.mark.parametrize("name,policy", sh.PROTECT_BATCHES)
def test_protecting_batch_is_meaningful(name, policy, tmp_path):
    """Per batch (seeds 3 .. 10, 150 steps): >= 500 neighbour checks, >= 10 neighbour refusals; under sap_ff_gn >= 10 later paths
    taken and >= 5 accepted steps on a path >= 8 after a neighbour check; under llp_ff >= 10 neighbour-refused candidates on a
    path >= 8; no own or neighbour margin, over every candidate evaluated, within 1e-6 dB of zero."""
    pytest.importorskip("networkx")
    topo, kw, runs = sh.protect_batch(name, policy, tmp_path)
    assert len(runs) == sh.PROTECT_B and kw["episode_length"] == 200
    fig = sh.protect_figures(runs)
    print(name, policy, "W", MANY_PATHS[name]["W"], "seeds", sh.protect_seeds(name, policy), fig)
    assert fig["n_checks"] >= 500 and fig["n_rejects"] >= 10, fig
    if policy == "sap_ff_gn":
        assert fig["later_taken"] >= 10 and fig["high_accepted_after_check"] >= 5, fig
    else:
        assert fig["high_neighbour_refused"] >= 10, fig
    assert fig["closest"] >= sh.MARGIN_DB, fig
    for tr, _, f in runs:
        assert int(np.isfinite(tr["margin"]).sum()) == f["n_checks"] and int(np.isfinite(tr["gsnr"]).sum()) == f["checks"]
        assert not np.isfinite(tr["margin"][~np.isfinite(tr["gsnr"])]).any()   # no neighbour check without an own check


def test_protecting_batches_cover_every_word_count():
    assert {MANY_PATHS[name]["W"] for name, policy in sh.PROTECT_BATCHES if policy == "sap_ff_gn"} == {1, 2, 3, 4, 5, 6}
    assert {MANY_PATHS[name]["k"] for name, policy in sh.PROTECT_BATCHES if policy == "llp_ff"} == {32, 12, 10}
    assert all(MANY_PATHS[name]["k"] > 8 for name, _ in sh.PROTECT_BATCHES)


# ---------------------------------------------------------------------------------------- rule launches, many paths
@pytest.mark.parametrize("name,route,rule,mode", sh.RULE_BATCHES)
def test_rule_batch_is_meaningful(name, route, rule, mode, tmp_path):
    """Per batch (seeds 3 .. 6, 150 steps unless RULE_SIZES says more): >= 8 steps the gate refused, >= 8 query rows with a
    refused window in a column >= 8; under check >= 4 accepted steps on a path >= 8; under next_path >= 10 later paths taken and
    >= 2 of them on a path >= 8; no margin within 1e-6 dB."""
    pytest.importorskip("networkx")
    topo, kw, runs = sh.rule_batch(name, route, rule, mode, tmp_path)
    batch, n = sh.rule_size(name, route, rule, mode)
    assert len(runs) == batch <= 8 and n <= 300
    c = MANY_PATHS[name]
    fig = sh.rule_figures(runs, c["S"], c["k"])
    print(name, route, rule, mode, "W", c["W"], "environments", batch, "steps", n, fig)
    assert fig["refused"] >= 8 and fig["high_refused_rows"] >= 8, fig
    if mode == "check":
        assert fig["high_accepted"] >= 4, fig
    else:
        assert fig["later"] >= 10 and fig["later_high"] >= 2, fig
    assert fig["closest"] >= sh.MARGIN_DB, fig
    assert fig["admitted_values"] == (0, 1), fig


def test_the_second_pass_behind_a_restart(tmp_path):
    """next_path: the steps whose taken path lies eight or more behind the path the step started over from -- the rules' scan in
    passes of eight with a start other than 0 reaches its second pass.  Printed per batch; the batches that have one within the
    limits (8 seeds or 300 steps) are those of FAR_BEHIND, each with at least one; the others (k = 9, k = 12, k = 10 under best) have
    none, which DESIGN 4 says."""
    pytest.importorskip("networkx")
    far = {}
    for name, route, rule, mode in sh.RULE_BATCHES:
        if mode == "next_path":
            topo, kw, runs = sh.rule_batch(name, route, rule, mode, tmp_path)
            far[(name, rule)] = sh.rule_figures(runs, MANY_PATHS[name]["S"], MANY_PATHS[name]["k"])["far_behind"]
    print("steps taken eight or more paths behind the restart:", far)
    assert far[(sh.K9, "best")] == far[(sh.K9, "min_cut")] == 0   # (k = 9: a restart path is 1 or above, path 8 less than 8 behind)
    assert {k for k, v in far.items() if v} == set(sh.FAR_BEHIND), far


@pytest.mark.parametrize("name", sh.SHAPES)
def test_first_query_batch_is_meaningful(name, tmp_path):
    """The query of rule "first" before each of 150 steps of llp_lf under check: >= 8 rows with a refused first fit in a column >= 8,
    admitted ones there too, no margin within 1e-6 dB."""
    pytest.importorskip("networkx")
    topo, kw, runs = sh.first_query_batch(name, tmp_path)
    S = MANY_PATHS[name]["S"]
    high = [tr["f_slots"][:, 8:] < S for tr, _ in runs]
    refused = sum(int((h & (tr["f_admitted"][:, 8:] == 0)).any(axis=1).sum()) for h, (tr, _) in zip(high, runs))
    admitted = sum(int((tr["f_admitted"][:, 8:] != 0).sum()) for tr, _ in runs)
    closest = min(float(tr["f_margin"].min()) for tr, _ in runs)
    print(name, "rows with a refused first fit in a column >= 8:", refused, "admitted first fits there:", admitted, "closest %.2g dB" % closest)
    assert refused >= 8 and admitted >= 8 and closest >= sh.MARGIN_DB
    for tr, _ in runs:
        assert np.array_equal(np.where(tr["f_slots"] < S, tr["f_slots"], -1), tr["q_ff_slots"])   # (the reference's first fit, said twice)


@pytest.mark.parametrize("name,rule", sh.PATH_CASES)
def test_path_batch_is_meaningful(name, rule, tmp_path):
    """The agent's path under check: more than half the given paths in 8 .. K - 1, >= 10 accepted and >= 1 refused step there, no
    margin within 1e-6 dB."""
    pytest.importorskip("networkx")
    topo, kw, paths, runs = sh.path_batch(name, rule, tmp_path)
    K = MANY_PATHS[name]["k"]
    assert paths.shape == (sh.N_STEPS, sh.RULE_B) and ((paths >= 8) & (paths < K)).mean() > 0.5 and (paths == K).any()
    high_acc = sum(int(((tr["accepted"] != 0) & (tr["act_path"] >= 8) & (tr["act_path"] < K)).sum()) for tr, _, _ in runs)
    high_ref = sum(int(((tr["accepted"] == 0) & np.isfinite(tr["gsnr"]) & (tr["act_path"] >= 8)).sum()) for tr, _, _ in runs)
    fig = gref.summed(runs)
    print(name, rule, "accepted on a path >= 8:", high_acc, "refused there:", high_ref, fig)
    assert high_acc >= 10 and high_ref >= 1 and fig["closest"] >= sh.MARGIN_DB, fig


def test_rule_batches_cover_every_word_count_and_combination():
    assert {(MANY_PATHS[name]["W"],) + tuple(c) for name, *c in sh.RULE_BATCHES} == {(W,) + c for W in range(1, 7) for c in sh.COMBOS}
    assert {MANY_PATHS[name]["W"] for name in sh.QUERY_SHAPES} == {2, 3, 6}
    assert all(b <= 8 and n <= 300 for b, n in sh.RULE_SIZES.values())


# ---------------------------------------------------------------------------------------- continuous rates
def test_continuous_rates_are_meaningful():
    """NSFNET, S = 320, load 150, rates 100 .. 350, protecting, sap_ff, seeds 2 .. 5 over 300 steps: >= 5 own refusals, >= 10
    neighbour refusals, more than 64 running services at a check, >= 50 distinct rate indices among the services that ran, no
    margin within 1e-6 dB; the gated handle's runs (the step oracle, and the query run of 100 steps) refuse too."""
    runs = sh.continuous_protect_runs()
    fig = sh.protect_figures(runs)
    rates = set()
    for tr, _, _ in runs:
        rates |= set(tr["request"][tr["accepted"] != 0, 3].tolist())
    print("continuous, protecting:", fig, "distinct rates provisioned:", len(rates), "from", min(rates), "to", max(rates))
    assert fig["rejects"] >= 5 and fig["n_rejects"] >= 10 and fig["n_max_running"] > 64, fig
    assert len(rates) >= 50 and min(rates) >= 100 and max(rates) <= 350
    assert fig["closest"] >= sh.MARGIN_DB, fig
    gated = sh.continuous_gated_runs()
    g = dict(checks=sum(f["checks"] for _, _, f in gated), rejects=sum(f["rejects"] for _, _, f in gated),
             max_running=max(f["max_running"] for _, _, f in gated), closest=min(f["closest"] for _, _, f in gated))
    print("continuous, gated:", g)
    assert g["rejects"] >= 5 and g["max_running"] > 64 and g["closest"] >= sh.MARGIN_DB, g
    q = [sh.continuous_query_run(sh.CONT_KW["seed"] + i)[0] for i in range(sh.CONT_B)]
    S = sh.CONT_KW["num_spectrum_resources"]
    qf = dict(refused_windows=sum(int(((tr["q_slots"] < S) & (tr["q_admitted"] == 0)).sum()) for tr in q),
              refused_first_fits=sum(int((np.isfinite(tr["path_ff_gsnr"]) & (tr["path_ff_gn"] == 0)).sum()) for tr in q),
              later=sum(int(tr["later"].sum()) for tr in q),
              closest=min(min(float(tr["q_margin"].min()), float(tr["mask_margin"].min())) for tr in q))
    print("continuous, gated, the queries:", qf)
    assert qf["refused_windows"] >= 10 and qf["refused_first_fits"] >= 10 and qf["later"] >= 1 and qf["closest"] >= sh.MARGIN_DB, qf


# ---------------------------------------------------------------------------------------- per-environment loads
@pytest.mark.parametrize("protect", [False, True])
def test_sweep_environments_are_meaningful(protect):
    """Two loads x four seeds: each load's environments run checks, the heavier load's are refused (by both checks on the
    protecting handle), and no margin lies within 1e-6 dB."""
    runs = sh.sweep_runs(protect)
    assert len(runs) == len(sh.SWEEP_LOADS) * sh.SWEEP_SEEDS
    for g, load in enumerate(sh.SWEEP_LOADS):
        part = runs[g * sh.SWEEP_SEEDS:(g + 1) * sh.SWEEP_SEEDS]
        fig = sh.protect_figures(part) if protect else dict(
            checks=sum(f["checks"] for _, _, f in part), rejects=sum(f["rejects"] for _, _, f in part), closest=min(f["closest"] for _, _, f in part))
        print("sweep, protecting" if protect else "sweep, gated", "load", load, fig)
        assert fig["checks"] > 500 and fig["closest"] >= sh.MARGIN_DB, fig
        if load == 150:
            assert fig["rejects"] >= 5 and (not protect or fig["n_rejects"] >= 10), fig
    light, heavy = runs[0][0], runs[sh.SWEEP_SEEDS][0]   # the same seed under the two loads: another arrival process
    assert not np.array_equal(light["accepted"], heavy["accepted"])
