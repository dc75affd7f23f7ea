"""More than eight candidate paths, what needs no GPU: the six shapes of ``gpu_support.MANY_PATHS`` pinned from the oracle alone,
for the seeds and launch lengths ``test_gpu_many_paths.py`` uses, so that its comparisons cannot pass without the K > 8 code
having had anything to do -- paths 8 and above are taken, the load reaches blocking, the admission check refuses windows on
columns 8 and above, ``sap_ff_gn`` goes on behind a refused path, and no GSNR lies within 1e-6 dB of its threshold (the GSNR is
held to rtol 1e-9, about 2e-8 dB at 20 dB: a decision closer than that could flip legitimately).  Eight words per link cannot have
more than eight paths (8 x 9 > 64 lanes): the shapes stop at six words."""
import os
import re

import numpy as np
import pytest

import gn_candidates_reference as cref
import gn_gate_reference as ref
from conftest import oracle_env_from_kwargs
from gpu_support import MANY_PATHS, MANY_PATHS_SEED as SEED, device_log_in_oracle, many_paths_kwargs, many_paths_topology

SHAPES = list(MANY_PATHS)
K9, K32, K21, K16, K12, K10 = SHAPES
# the policy whose step-parity case must spend 20 steps and more on the paths 8 .. K - 1: the table's, except on the 3x3 grid,
# where only path 8 is one and sap_ff takes it 3 times in 1800 steps at any load -- llp_ff does 32 times at load 8
HIGH_POLICY = dict({name: c["policy"] for name, c in MANY_PATHS.items()}, **{K9: "llp_ff"})
# (shape, policy, j, environments, steps) of every run of the candidate oracle the GPU module compares with
GATED_BATCHES = [(name, MANY_PATHS[name]["policy"], 2, cref.B, 150) for name in (K9, K21, K16, K10)] + \
    [(name, "sap_ff_gn", 1, cref.B, 150) for name in (K32, K12)]
MARGIN_DB = 1e-6


@pytest.mark.parametrize("name", SHAPES)
def test_shape_figures(name, tmp_path):
    """k W <= 64 lanes with k > 8; W by the library's own rule; the grid has the links and the k paths per pair of the table; the
    path records stay below the 14 bits the GN check decodes them from."""
    pytest.importorskip("networkx")
    from optical_rl_gym_amd import build
    c = MANY_PATHS[name]
    text = open(os.path.join(build.CSRC, "orlg_api.hip")).read()
    assert re.search(r"int W = \(S \+ 63\) / 64;\s*\n\s*if \(W == 7\) W = 8;", text)   # the rule restated here
    assert re.search(r"K \* W > 64\) return fail", text)
    W = (c["S"] + 63) // 64
    W = 8 if W == 7 else W
    assert c["W"] == W and c["k"] > 8 and c["k"] * W <= 64 and (name == K9 or (c["k"] + 1) * W > 64)
    topo = many_paths_topology(name, tmp_path)
    N = c["rows"] * c["cols"]
    assert (topo.num_nodes, topo.num_links, topo.k_paths) == (N, c["E"], c["k"])
    assert topo.num_paths == N * (N - 1) // 2 * c["k"] < 1 << 14   # (one record list per unordered pair)
    if name == K32:
        assert topo.num_paths == 3840   # (the largest shipped table, ring36, has 1890 records)
    assert (topo.pair_path_count[~np.eye(N, dtype=bool).ravel()] == c["k"]).all()
    assert c["load"] == (8 if name == K9 else round(0.5 * c["S"] * c["E"] / 40 - 1e-9))
    assert many_paths_kwargs(name) == dict(num_spectrum_resources=c["S"], load=c["load"], mean_service_holding_time=25,
                                           episode_length=200, seed=3)


@pytest.mark.parametrize("name", SHAPES)
def test_paths_eight_and_above_are_taken(name, tmp_path):
    """The step-parity batch (seeds 3 .. 8, 300 steps): at least 20 accepted steps on a path 8 .. K - 1, and blocking is reached;
    with the table's policy as well where that is another one (3x3: sap_ff), at least one."""
    pytest.importorskip("networkx")
    topo, kw, c = many_paths_topology(name, tmp_path), many_paths_kwargs(name), MANY_PATHS[name]
    for policy in {HIGH_POLICY[name], c["policy"]}:
        high, accepted = [], 0
        with device_log_in_oracle():
            for i in range(6):
                o = oracle_env_from_kwargs(topo, kw, seed=SEED + i)
                tr = o.run(policy, 300, reset_on_done=True)
                high.append(int(((tr["act_path"] >= 8) & (tr["act_path"] < c["k"]) & (tr["accepted"] != 0)).sum()))
                accepted += int(tr["accepted"].sum())
                o.close()
        print(name, policy, "steps on a path >= 8 per environment:", high, "accepted share: %.3f" % (accepted / 1800))
        assert sum(high) >= (20 if policy == HIGH_POLICY[name] else 1), (policy, high)
        assert 0 < accepted < 1800, policy


@pytest.mark.parametrize("name,policy,j,batch,n", GATED_BATCHES)
def test_gated_batches_refuse_on_the_high_columns(name, policy, j, batch, n, tmp_path):
    """Every candidate-oracle batch of the GPU module: the gate refuses steps, some path_ff_gn column 8 or above differs from
    path_ff, sap_ff_gn takes a later path in every environment, and no candidate's GSNR is within 1e-6 dB of its threshold."""
    pytest.importorskip("networkx")
    topo, kw = many_paths_topology(name, tmp_path), many_paths_kwargs(name)
    runs = cref.run_batch((topo, kw), j=j, policy=policy, n_steps=n, batch=batch)
    figs = [fig for _, _, fig in runs]
    differ = [int((tr["path_ff_gn"][:, 8:] != tr["path_ff"][:, 8:]).any(axis=1).sum()) for tr, _, _ in runs]
    deep = [int((tr["deeprmsa_gn"][:, 8 * j:] != tr["deeprmsa"][:, 8 * j:]).any(axis=1).sum()) for tr, _, _ in runs]
    print(name, policy, "checks", [f["checks"] for f in figs], "refusals", [f["rejects"] for f in figs], "later path taken",
          [f["later_taken"] for f in figs], "steps with a refused column >= 8", differ, "closest |GSNR - thr| dB",
          ["%.1e" % f["closest"] for f in figs])
    assert all(f["checks"] > 100 for f in figs) and sum(f["rejects"] for f in figs) > 0
    assert sum(differ) > 0 and sum(deep) > 0
    if policy == "sap_ff_gn":
        assert all(f["later_taken"] > 0 for f in figs)
    assert min(f["closest"] for f in figs) >= MARGIN_DB


@pytest.mark.parametrize("name", [K9, K21, K16, K10])
def test_gated_step_case(name, tmp_path):
    """The gated oracle's 301 steps on seed 3 with the shape's policy (test_case_against_the_gated_oracle)."""
    pytest.importorskip("networkx")
    topo, kw, c = many_paths_topology(name, tmp_path), many_paths_kwargs(name), MANY_PATHS[name]
    tr, _, fig = ref.run_case((topo, kw), policy=c["policy"], n_steps=301)
    high = int((np.isfinite(tr["gsnr"]) & (tr["act_path"] >= 8)).sum())
    print(name, fig, "checks on a path >= 8:", high)
    assert fig["checks"] > 250 and fig["rejects"] > 0 and fig["closest"] >= MARGIN_DB and high > 0


def test_a_pair_is_cached_like_a_name(tmp_path):
    """run_case on a (topology, kwargs) pair: one run per process, read-only arrays, and the named cases as before."""
    pytest.importorskip("networkx")
    topo, kw = many_paths_topology(K9, tmp_path), many_paths_kwargs(K9)
    a = ref.run_case((topo, kw), policy="sap_ff", n_steps=40)
    assert ref.run_case((topo, dict(kw)), policy="sap_ff", n_steps=40) is a and not a[0]["accepted"].flags.writeable
    b = cref.run_case((topo, kw), policy="sap_ff_gn", n_steps=40, j=2)
    assert cref.run_case((topo, dict(kw)), policy="sap_ff_gn", n_steps=40, j=2) is b and not b[0]["path_ff_gn"].flags.writeable
    assert cref.run_batch((topo, kw), policy="sap_ff_gn", n_steps=40, j=2, batch=2)[1] is \
        cref.run_case((topo, kw), seed=SEED + 1, policy="sap_ff_gn", n_steps=40, j=2)   # (a pair's batch: its kwargs' seed onwards)
    with pytest.raises(AssertionError):
        ref.run_case((topo, kw), n_steps=40)   # a pair has no policy of its own
    named = ref.run_case("nsfnet_s100_l20_spff", n_steps=40)
    assert ref.run_case("nsfnet_s100_l20_spff", n_steps=40) is named
    assert np.array_equal(named[0]["act_path"], ref.run_case("nsfnet_s100_l20_spff", n_steps=40, policy="sp_ff")[0]["act_path"])
