"""The group kernel's policy pass: the candidate paths' words are ANDed over all the link bytes of a path record --
the bytes past the path's end repeat its first link (``OrlgPathRec``, ``orlg_path_records``) -- and first fit's limit "start below
S - n" is applied by clearing slot S - 1 before the windows are looked for.  Three things can go wrong with that and are held to
the CPU oracle here, decisions and final state, under both step kernels:

1. hop groups: a pass holds paths that end in different groups of four hops (1, 4, 5, 8, 9, 12, 13 and 14 hops for one node
   pair), so a short path keeps reading its padding while a long one in the same wave goes on; idle rows read zero records;
2. the limit: slot S - 1 at bit 63 of the last word, at bit 0 of a word of its own, in mid-word, and in the word before the last
   of the eight-word layout -- on traces that refuse a request whose only window starts at S - n and accept one at S - n - 1;
3. the state format: a batch handed from one kernel to the other continues as the oracle does."""
import functools

import numpy as np
import pytest

import block_cause_reference as bref
from conftest import oracle_env_from_kwargs
from gpu_support import (RMSA_OUTS, device_log_fixture, device_log_in_oracle as oracle_log, everything_matches_oracle,  # noqa: F401
                         external_actions, one_step_launches, rmsa_env, same_bytes, snapshot, state_matches, step_kernel, topology,
                         write_topology)

pytestmark = pytest.mark.gpu

NSFNET = "nsfnet_chen_5-paths_6-modulations"

# ---------------------------------------------------------------------------------------- 1. hop-group boundaries inside one pass
# Fifteen nodes on a ring, and six chords that all end in node 15.  Node 1 has the neighbours 2 and 15 only, so the simple paths
# from 1 to 15 are the edge itself and 1 - 2 - ... - j - 15 for the six chords' j and for j = 14: eight paths of
# 1, 4, 5, 8, 9, 12, 13 and 14 hops.  The lengths put them in the order 5, 1, 14, 9, 4, 13, 8, 12 hops: every pass of three
# (S = 320) and the pass of eight (S = 100) holds paths that end in different hop groups.  Link 0 is the chord of the 13-hop
# path: a record padded with zeros would AND a link in that no other of the eight paths uses.  Nodes 1 and 15 draw 60 % of the
# requests' end points.
RING_N, RING_K = 15, 8
RING_CHORDS = ((13, 60), (4, 140), (5, 60), (8, 120), (9, 80), (12, 90))   # (j, length of the chord j - 15)
RING_HOPS = [5, 1, 14, 9, 4, 13, 8, 12]
# erlang: sap_ff is refused a third (S = 100) and a quarter (S = 320) of its requests, so the later passes run.  All paths but
# the edge itself start 1 - 2 - 3 - 4: the long ones are weighed in every pass that holds them and seldom win
RING_LOAD = {100: 60, 320: 240}
_ring = {}


def ring_topology(tmp_path):
    if not _ring:
        from optical_rl_gym_amd.topology_io import topology_from_txt
        edges = [(j, 15, length) for j, length in RING_CHORDS] + [(i, i + 1, 10) for i in range(1, 14)] + [(14, 15, 20), (15, 1, 110)]
        _ring["topo"] = topology_from_txt(write_topology(tmp_path, "ring15", RING_N, edges), "ring15", k_paths=RING_K)
    return _ring["topo"]


def ring_kwargs(S, **over):
    probs = [0.3] + [0.4 / 13] * 13 + [0.3]
    return dict(dict(num_spectrum_resources=S, load=RING_LOAD[S], mean_service_holding_time=25, episode_length=150, seed=21,
                     node_request_probabilities=probs), **over)


def test_ring_paths(tmp_path):
    """The topology is what the tests below say it is (no GPU in this one: the tables alone)."""
    topo = ring_topology(tmp_path)
    assert topo.k_paths == RING_K and topo.num_links == 21
    base = int(topo.pair_path_base[0 * RING_N + 14])
    assert [int(h) for h in topo.path_hops[base:base + RING_K]] == RING_HOPS
    assert int(topo.path_hops.max()) == 14 and int(topo.path_hops.min()) == 1
    on_link0 = [g for g in range(base, base + RING_K) if 0 in topo.path_links[topo.path_link_off[g]:topo.path_link_off[g + 1]]]
    assert on_link0 == [base + RING_HOPS.index(13)]


RING_POLICIES = ["sp_ff", "sap_ff", "llp_ff", "deeprmsa_sap_ff", "path_ff_external"]


@pytest.mark.parametrize("S", [100, 320])
@pytest.mark.parametrize("policy", RING_POLICIES)
def test_hop_groups_in_one_pass(policy, S, step_kernel, tmp_path, device_log_in_oracle):
    """Six environments (the last quad of the group kernel has two idle rows), 300 steps: every per-step output and the state
    against the oracle.  The route policies run one launch (sp_ff and sap_ff under the group kernel once more without outputs:
    the lean body, the same state byte for byte), the agent's paths 200 launches of one step."""
    topo, kw = ring_topology(tmp_path), ring_kwargs(S)
    B, rm = 6, int(policy.startswith("deeprmsa"))
    env = rmsa_env(topo, B, step_kernel, reward_mode=rm, **kw)
    assert env.words_per_link == (2 if S == 100 else 5)
    actions = None
    if policy == "path_ff_external":
        n = 200
        actions = external_actions(topo, S, n, B, kind="paths")
        tr = one_step_launches(env, policy, n, RMSA_OUTS, actions=actions, auto_reset=True)
    else:
        n = 300
        tr = env.run(policy, n, outputs=RMSA_OUTS, auto_reset=True)
    assert env.last_kernel().startswith("orlg_rmsa_group_kernel" if step_kernel == "group" else "orlg_rmsa_kernel"), env.last_kernel()
    snap = snapshot(env, save_state=False)
    env.close()
    hops_taken = set()
    for i in range(B):
        ot = everything_matches_oracle(topo, kw, tr, i, snap, policy, n, True, actions=actions, seed=kw["seed"] + i, reward_mode=rm)
        pair = (np.minimum(ot["src"], ot["dst"]) == 0) & (np.maximum(ot["src"], ot["dst"]) == 14) & (ot["accepted"] != 0)
        hops_taken |= {RING_HOPS[p] for p in ot["act_path"][pair]}
    assert 0 < tr["accepted"].mean() < 1
    if policy != "sp_ff":   # the pair 1 - 15 takes paths of three hop groups, and paths behind the first pass of three
        assert len({(h - 1) // 4 for h in hops_taken}) >= 3 and hops_taken & set(RING_HOPS[3:]), sorted(hops_taken)
    if step_kernel == "group" and policy in ("sp_ff", "sap_ff"):
        lean = rmsa_env(topo, B, "group", **kw)
        lean.run(policy, n, auto_reset=True)
        assert "body=lean" in lean.last_kernel(), lean.last_kernel()
        same_bytes(snapshot(lean, save_state=False), snap, "lean body")
        lean.close()


# ---------------------------------------------------------------------------------------- 2. the limit at S - n
# (S, load, the eight seeds of the batch): chosen with the oracle on the CPU so that both conditions of _limit_trace hold for
# sap_ff and for sp_ff within 300 steps
LIMIT_CASES = {
    64: (12, (10, 11, 12, 13, 14, 15, 16, 17)),
    65: (12, (10, 11, 12, 13, 14, 15, 16, 17)),
    100: (20, (10, 11, 12, 13, 14, 15, 16, 17)),
    128: (25, (10, 11, 12, 13, 14, 15, 16, 17)),
    320: (60, (10, 11, 12, 13, 14, 15, 16, 17)),
    400: (75, (10, 11, 12, 13, 14, 15, 16, 17)),
}
LIMIT_STEPS = 300
LIMIT_FIELDS = ("act_path", "act_slot", "accepted", "arrival", "holding", "done")


def limit_kwargs(S, load):
    return dict(num_spectrum_resources=S, load=load, mean_service_holding_time=25, episode_length=100)


@functools.lru_cache(maxsize=None)
def _limit_trace(S, load, seed, policy, n=LIMIT_STEPS):
    """One oracle environment on NSFNET, one request at a time: (trace, final state, last_only, edge).  last_only: refused steps
    whose fit level -- of the first path for sp_ff, the highest of the k paths for sap_ff -- is "only the window at S - n"
    (block_cause_reference.path_levels on the occupancy the step met); edge: accepted windows that start at S - n - 1."""
    topo, kw = topology(NSFNET), limit_kwargs(S, load)
    with oracle_log():
        o = oracle_env_from_kwargs(topo, kw, seed=seed)
        rows, last_only, edge = [], 0, 0
        for _ in range(n):
            r, avail = o.request(), o.available_slots()
            row = o.run(policy, 1, reset_on_done=True, fields=list(LIMIT_FIELDS))
            rows.append(row)
            if row["accepted"][0]:
                gid = int(topo.pair_path_base[r.src * topo.num_nodes + r.dst]) + int(row["act_path"][0])
                edge += int(row["act_slot"][0]) == S - bref.number_slots(r.bit_rate, int(topo.path_se[gid])) - 1
            else:
                lv = bref.path_levels(avail, topo, r.src, r.dst, r.bit_rate)
                last_only += int(lv[0] if policy == "sp_ff" else lv.max()) == bref.LAST_WINDOW
        final = dict(available_slots=o.available_slots(), counters=o.counters(), link_stats=o.link_stats(), graph_stats=o.graph_stats(),
                     current_time=o.current_time(), num_running=o.num_running())
        o.close()
    return {f: np.concatenate([row[f] for row in rows]) for f in LIMIT_FIELDS}, final, last_only, edge


@pytest.mark.parametrize("policy", ["sap_ff", "sp_ff"])
@pytest.mark.parametrize("S", sorted(LIMIT_CASES))
def test_limit_below_s_minus_n(S, policy, step_kernel):
    """Eight environments on NSFNET, 300 steps in one launch: decisions and state against the oracle, on traces that hold a refused
    request with a window at S - n only and an accepted window at S - n - 1.  The group kernel runs them once more without
    outputs: the lean body leaves the same state byte for byte."""
    load, seeds = LIMIT_CASES[S]
    runs = [_limit_trace(S, load, seed, policy) for seed in seeds]
    assert sum(r[2] for r in runs) >= 1 and sum(r[3] for r in runs) >= 1, (S, policy, [r[2:] for r in runs])
    env = rmsa_env(NSFNET, len(seeds), step_kernel, seeds=list(seeds), **limit_kwargs(S, load))
    tr = env.run(policy, LIMIT_STEPS, outputs=LIMIT_FIELDS, auto_reset=True)
    snap = snapshot(env, save_state=False)
    env.close()
    for i, (want, final, _, _) in enumerate(runs):
        for f in LIMIT_FIELDS:
            bad = np.flatnonzero(tr[f][:, i] != want[f])
            assert bad.size == 0, (S, policy, i, f, bad[:4], tr[f][bad[:4], i], want[f][bad[:4]])
        state_matches(snap, i, final, (S, policy))
    if step_kernel == "group":   # the launch the headline runs: no outputs, the lean body
        lean = rmsa_env(NSFNET, len(seeds), "group", seeds=list(seeds), **limit_kwargs(S, load))
        lean.run(policy, LIMIT_STEPS, auto_reset=True)
        assert "body=lean" in lean.last_kernel(), lean.last_kernel()
        same_bytes(snapshot(lean, save_state=False), snap, "lean body")
        lean.close()


# ---------------------------------------------------------------------------------------- 3. one kernel continues the other
@pytest.mark.parametrize("order", [("group", "wave"), ("wave", "group")])
@pytest.mark.parametrize("S", [100, 320])
def test_the_other_kernel_continues_a_checkpoint(S, order, tmp_path, device_log_in_oracle):
    """The ring of test 1, sap_ff, six environments: 200 steps under one kernel, its checkpoint loaded into a handle of the other
    kernel, 200 more -- the 400 steps of the oracle, outputs and state."""
    topo, kw = ring_topology(tmp_path), ring_kwargs(S)
    B = 6
    a, b = (rmsa_env(topo, B, kernel, **kw) for kernel in order)
    first = a.run("sap_ff", 200, outputs=RMSA_OUTS, auto_reset=True)
    b.load_state(a.save_state())
    second = b.run("sap_ff", 200, outputs=RMSA_OUTS, auto_reset=True)
    for e, k in zip((a, b), order):
        assert e.last_kernel().startswith("orlg_rmsa_group_kernel" if k == "group" else "orlg_rmsa_kernel"), (k, e.last_kernel())
    tr = {k: np.concatenate([first[k], second[k]]) for k in RMSA_OUTS}
    snap = snapshot(b, save_state=False)
    for i in range(B):
        everything_matches_oracle(topo, kw, tr, i, snap, "sap_ff", 400, True, seed=kw["seed"] + i)
    a.close()
    b.close()
