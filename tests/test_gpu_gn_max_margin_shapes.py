"""The max-margin step kernel ``orlg_rmsa_mm_kernel<W, STATS, CAUSE>`` at the shapes ``test_gpu_gn_max_margin.py`` leaves
out, against the follower of ``gn_max_margin_reference.py`` with the oracle's own values of every step kept:
  1. per word count W in 1, 2, 3, 4, 5, 6, 8 the six instantiations -- three statistics levels, without and with the classifier --:
     the ``full`` launch followed on the oracle with every ``RMSA_OUTS`` output, the link averages and the final snapshot
     (``link_stats``, ``graph_stats``, ``bit_rate_hist``, the pending request) exact, the other five launches the same bytes in every
     output they share; the lighter levels against the reference; the blocking cause of every step;
  2. the same through a ``BatchedDeepRMSAEnv`` handle with ``j = 2`` and the reward +1 / -1;
  3. more than 128 services in the ring (four chunks) and on one path (three compacted chunks), the three routes in turn;
  4. a ring whose head laps, ``RING = true`` in the step against ``RING = false`` in the twin's query;
  5. the launch that takes fewer waves per workgroup than the handle's own, and the refusal where not even one wave fits.
Everything is exact but the GSNR (rtol 1e-9) and the margins (atol 1e-9 x the largest |GSNR| the reference computed): the tolerances of
``gn_max_margin_reference.follow``.  ``test_gn_max_margin_args.py`` pins on the reference alone what each case reaches.  Every launch
asserts its kernel's name."""
import ctypes as C

import numpy as np
import pytest

import block_cause_reference as bcr
import gn_max_margin_reference as mm
import gn_protect_reference as pref
import gn_slots_reference as sl
from gpu_support import (COMPACTNESS, RMSA_OUTS, STATS_LEVELS, _fields, device_log_in_oracle, grid_edges, rmsa_env, same_bytes, snapshot,
                         state_matches, topology, unpack, wave_plan, write_topology)

pytestmark = pytest.mark.gpu

GN = ("gn_gsnr_db", "gn_neighbour_margin_db", "gn_window_margin_db")
LINK_AVG = ("avg_link_compactness", "avg_link_utilization")
FULL_OUTS = RMSA_OUTS + LINK_AVG + GN
DECIDED = ("act_path", "act_slot", "accepted", "done", "request", "arrival", "holding") + GN   # what every statistics level keeps
KEPT = ("done", "reward", "arrival", "holding") + COMPACTNESS + LINK_AVG                       # the oracle's own values, exact
TWIN = ("act_path", "act_slot", "accepted", "gn_gsnr_db", "gn_neighbour_margin_db")


def _mm_name(W, level=2, cause=False):
    return "orlg_rmsa_mm_kernel<%d,%d%s> " % (W, level, ",true" if cause else "")


def _handle(batch, tmp_path, B=mm.SHAPE_B, **over):
    c = sl.BATCHES[batch]
    topo, kw, policy = sl.batch_case(batch, tmp_path)
    kw = dict(kw, seed=mm.batch_seed(batch, "sap", kw), **c["handle"])
    kw.update(over)
    return rmsa_env(topo, B, gn_gate=pref.case_gate(topo, protect=c["protect"]), **kw), topo, kw, policy


def _follow(dev, oracles, route, given=None):
    """every environment of a launch followed on its oracle: (per environment the kept rows of its steps, the kinds' counts); the
    margins' differences are held to their bound here"""
    kept, kinds, diffs = [], dict(admitted=0, near=0, fallback=0, rejection=0), [0.0]
    for i, go in enumerate(oracles):
        rows = []
        for k, v in mm.follow(go, dev, i, route, diffs, given, kept=rows).items():
            kinds[k] += v
        kept.append(rows)
    largest = max(go.max_abs_gsnr for go in oracles)
    assert max(diffs) <= 1e-9 * largest, (max(diffs), largest)
    return kept, kinds


def _rows_match(dev, i, rows, what):
    """environment i of a launch against the oracle's own values of its steps, exact (the decisions, the GSNR and the margins are
    the follower's)"""
    for name in KEPT:
        if name in dev:
            got, want = dev[name][:, i], np.array([row[name] for row in rows]).astype(dev[name].dtype)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (what, i, name, bad[:5], got[bad[:5]], want[bad[:5]])


def _end_matches(snap, i, final, what, level=2):
    """environment i of a snapshot against gn_max_margin_reference.final_state: occupancy, counters, clock, services in progress, the
    histograms and the pending request; at level `full` every link and graph statistic"""
    state_matches(snap, i, final, what, link_stats=level == 2)
    for name, v in final["bit_rate_hist"].items():
        assert np.array_equal(snap["bit_rate_hist." + name][i], v), (what, i, name)
    req = snap["requests"][i]
    assert (req["service_id"], req["src"], req["dst"], req["bit_rate"], req["arrival_time"], req["holding_time"]) == final["request"], (what, i)


def _rank_order(env, i, final, what):
    """running_services() of environment i: the reference's services by ascending release time, nothing past the count"""
    run = env.running_services()
    n = len(final["releases"])
    assert run["count"][i] == n and 0 <= run["head"][i] < env.queue_capacity, (what, i, run["count"][i], n)
    assert np.array_equal(run["release_time"][i, :n], final["releases"]) and np.isnan(run["release_time"][i, n:]).all(), (what, i)
    assert (run["path_gid"][i, :n] >= 0).all() and (run["path_gid"][i, n:] == -1).all(), (what, i)
    return run


def _same(got, want, what):
    assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), (what, got, want)


def _twin_steps(dev, tw, route, given=None, what=()):
    """The launch's rows against the loop it replaces on a handle with the same seeds: max_margin_windows() (RING = false: the query
    linearises the ring), the rule in numpy, an external step -- every decision, GSNR and margin bit-equal.  Returns the query's rows
    of every step: (best_slot [B, K], best_margin [B, K])."""
    S, queries = tw.num_spectrum_resources, []
    for t in range(dev["act_path"].shape[0]):
        slots, margin = tw.max_margin_windows()
        window = unpack(tw.action_masks("slots"), S).astype(bool)
        acts, w, kinds = mm.proposals(slots, margin, mm.first_free_of(window), S, route, None if given is None else given[t])
        r = tw.run("external", 1, actions=acts, outputs=TWIN, auto_reset=True)
        for i, kind in enumerate(kinds):   # an admitted proposal is never refused, a fallback always
            assert bool(r["accepted"][0, i]) == (kind == "admitted"), (what, t, i, kind, acts[i])
        _same(dev["act_path"][t], acts[:, 0], what + (t, "act_path"))
        _same(dev["act_slot"][t], acts[:, 1], what + (t, "act_slot"))
        for name in TWIN[2:]:
            _same(dev[name][t], r[name][0], what + (t, name))
        _same(dev["gn_window_margin_db"][t], w, what + (t, "gn_window_margin_db"))
        queries.append((slots, margin))
    return queries


def _query_matches(query, i, rows, atol, what):
    """max_margin_windows() of environment i against the rows slots() gave the follower before the same step: a path with a surely
    admitted window names a window within BEST_TOL_DB of the reference's best, with its margin; a path without any, none"""
    slots, margin = query
    S = rows["window"].shape[-1]
    sure = rows["mask"] & ~rows["near"]
    for p in range(rows["window"].shape[0]):
        s = int(slots[i, p])
        if sure[p].any():
            assert s < S and (rows["near"][p, s] or rows["w"][p, s] >= np.nanmax(rows["w"][p]) - sl.BEST_TOL_DB), (what, p, s)
            if rows["mask"][p, s]:
                assert abs(margin[i, p] - rows["w"][p, s]) <= atol, (what, p, s, margin[i, p], rows["w"][p, s])
        elif not (rows["mask"][p] | rows["near"][p]).any():
            assert s == S and np.isnan(margin[i, p]), (what, p, s)


def _causes_match(dev, i, rows, what):
    """block_cause of environment i: 0 for an accepted step, "gn" where the step's check refused the proposal (a fallback), and for a
    rejection (k, S) the cause block_cause_reference gives on the state the step met"""
    for t, row in enumerate(rows):
        got = int(dev["block_cause"][t, i])
        if dev["accepted"][t, i]:
            want = bcr.ACCEPTED
        elif row["kind"] == "rejection":
            want = row["rejection_cause"]
        else:
            want = bcr.C_GN
        assert got == want, (what, i, t, row["kind"], got, want)


# ---------------------------------------------------------------------------------------- 1. every instantiation of every word count
@pytest.mark.parametrize("W", sorted(mm.WORD_CASES))
def test_every_instantiation_of_a_word_count(W, tmp_path):
    batch, n, B = mm.WORD_CASES[W], mm.SHAPE_N, mm.SHAPE_B
    c = sl.BATCHES[batch]
    launches = {}
    for lv, level in enumerate(STATS_LEVELS):
        for cause in (False, True):
            env, topo, kw, policy = _handle(batch, tmp_path, stats_level=level)
            assert env.words_per_link == W
            if c["warmup"]:
                env.run(policy, c["warmup"], auto_reset=True)
            outs = (FULL_OUTS if lv == 2 else DECIDED + (COMPACTNESS if lv else ())) + (("block_cause",) if cause else ())
            dev = env.run("sap_mm", n, outputs=outs, auto_reset=True, cause_counts=True if cause else None)
            assert env.last_kernel().startswith(_mm_name(W, lv, cause)), env.last_kernel()
            env.reduce_counters()   # (raises where a release ring overflowed)
            launches[lv, cause] = (dev, snapshot(env, save_state=False))
            env.close()
    full, fsnap = launches[2, False]
    with device_log_in_oracle():
        oracles = [mm.oracle_at(batch, tmp_path, i, "sap") for i in range(B)]
        kept, kinds = _follow(full, oracles, "sap")
        finals = [mm.final_state(go) for go in oracles]
        for go in oracles:
            go.close()
    print(batch, "W", W, kinds)
    assert kinds["admitted"] > 0 and kinds["fallback"] > 0, kinds
    for i in range(B):
        _rows_match(full, i, kept[i], (batch, "full"))
        _end_matches(fsnap, i, finals[i], (batch, "full"))
    assert (full["network_compactness"] > 0).any() and (full["avg_link_utilization"] > 0).any()
    for (lv, cause), (dev, snap) in launches.items():
        what = (batch, STATS_LEVELS[lv], cause)
        for k in dev:   # the same bytes as the launch that keeps every statistic and has no classifier
            if k in full:
                assert dev[k].tobytes() == full[k].tobytes(), what + (k,)
        for k in snap:
            if k in ("occupancy", "current_time", "num_running", "requests") or k.startswith("counters."):
                assert snap[k].tobytes() == fsnap[k].tobytes(), what + (k,)
        if lv == 2:
            same_bytes(snap, fsnap, what)
        for i in range(B):
            if lv < 2:
                _rows_match(dev, i, kept[i], what)
                state_matches(snap, i, finals[i], what, link_stats=False)
            if cause:
                _causes_match(dev, i, kept[i], what)
        if cause:
            assert np.array_equal(dev["block_cause_counts"], bcr.counts_of(dev["block_cause"])), what
            assert (dev["block_cause_counts"].sum(axis=1) == n).all(), what


# ---------------------------------------------------------------------------------------- 2. a DeepRMSA handle
def test_statistics_through_a_deeprmsa_handle():
    from optical_rl_gym_amd import BatchedDeepRMSAEnv
    c = mm.DEEP
    topo = topology(pref.NSF)
    gate = pref.case_gate(topo, protect=True)
    dkw = dict(mean_service_holding_time=25.0, mean_service_inter_arrival_time=25.0 / c["load"], num_spectrum_resources=c["S"],
               episode_length=1000, seed=c["seed"], j=c["j"])
    env = BatchedDeepRMSAEnv(topo, c["B"], gn_gate=gate, **dkw)
    dev = env.run("sap_mm", c["n"], outputs=FULL_OUTS, auto_reset=True)
    assert env.last_kernel().startswith(_mm_name(env.words_per_link)), env.last_kernel()
    snap = snapshot(env)
    with device_log_in_oracle():
        oracles = [mm.warm_oracle(topo, mm.deep_kwargs(), c["seed"] + i, "sap_ff", 0, j=c["j"], reward_mode=1) for i in range(c["B"])]
        kept, kinds = _follow(dev, oracles, "sap")
        for i, go in enumerate(oracles):
            _rows_match(dev, i, kept[i], "deeprmsa")
            _end_matches(snap, i, mm.final_state(go), "deeprmsa")
            go.close()
    assert np.array_equal(dev["reward"], np.where(dev["accepted"].astype(bool), 1.0, -1.0)) and (dev["reward"] < 0).any() and (dev["reward"] > 0).any()
    assert kinds["admitted"] > 0, kinds
    env.close()


# ---------------------------------------------------------------------------------------- 3. more than 128 services
def test_more_than_128_services_in_the_ring_and_on_one_path(tmp_path):
    c, kw = mm.CHUNKS, mm.chunks_kwargs()
    topo = sl.tri_topology(tmp_path)
    gate = pref.case_gate(topo, protect=True)
    env, tw = (rmsa_env(topo, c["B"], gn_gate=gate, queue_capacity=c["queue_capacity"], **kw) for _ in range(2))
    assert env.queue_capacity == c["queue_capacity"] and env.words_per_link == 8
    for e in (env, tw):
        e.run(c["policy"], c["warmup"], auto_reset=True)
    rng = np.random.default_rng(32)
    with device_log_in_oracle():
        oracles = [mm.warm_oracle(topo, kw, kw["seed"] + i, c["policy"], c["warmup"]) for i in range(c["B"])]
        kept = [[] for _ in oracles]
        for name, (route, n) in zip(mm.ROUTES, c["plan"]):
            assert mm.ROUTES[name] == route
            if route == "path":
                given = rng.integers(0, env.k_paths, size=(n, c["B"])).astype(np.int32)
                rows = [env.run(name, 1, actions=given[t], outputs=FULL_OUTS, auto_reset=True) for t in range(n)]
                dev = {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}
            else:
                given, dev = None, env.run(name, n, outputs=FULL_OUTS, auto_reset=True)
            assert env.last_kernel().startswith(_mm_name(8)), env.last_kernel()
            queries = _twin_steps(dev, tw, route, given, (name,))
            rows, kinds = _follow(dev, oracles, route, given)
            atol = 1e-9 * max(go.max_abs_gsnr for go in oracles)
            for i in range(c["B"]):
                _rows_match(dev, i, rows[i], name)
                for t, row in enumerate(rows[i]):
                    _query_matches(queries[t], i, row["rows"], atol, (name, t, i))
                kept[i] += rows[i]
            assert kinds["admitted"] + kinds["near"] > 0, kinds
        env.reduce_counters()   # no overflow
        snap = snapshot(env)
        for i, go in enumerate(oracles):
            # four chunks of the ring, three of the compacted list, at a step the device evaluated
            assert max(row["running"] for row in kept[i]) > 192 and max(row["sharing"] for row in kept[i]) > 128, i
            final = mm.final_state(go)
            _end_matches(snap, i, final, "chunks")
            _rank_order(env, i, final, "chunks")
            go.close()
    assert env.num_running().min() > 192
    assert env.save_state().tobytes() == tw.save_state().tobytes()
    env.close(); tw.close()


# ---------------------------------------------------------------------------------------- 4. a ring whose head laps
def test_the_ring_laps(tmp_path):
    c = mm.LAP
    n, Q = c["n"], c["queue_capacity"]
    env, topo, kw, policy = _handle(c["batch"], tmp_path, B=c["B"], queue_capacity=Q)
    tw = _handle(c["batch"], tmp_path, B=c["B"], queue_capacity=Q)[0]
    assert env.queue_capacity == Q
    outs = DECIDED
    dev = env.run("sap_mm", n, outputs=outs, auto_reset=True)
    assert env.last_kernel().startswith(_mm_name(env.words_per_link)), env.last_kernel()
    _twin_steps(dev, tw, "sap", None, ("lap",))   # RING = false in the twin's query, RING = true in the step
    assert env.save_state().tobytes() == tw.save_state().tobytes()
    env.reduce_counters()   # no overflow
    snap = snapshot(env)
    with device_log_in_oracle():
        oracles = [mm.oracle_at(c["batch"], tmp_path, i, "sap") for i in range(c["B"])]
        kept, kinds = _follow(dev, oracles, "sap")
        for i, go in enumerate(oracles):
            final = mm.final_state(go)
            pops = int(final["counters"]["services_accepted"]) - len(final["releases"])
            lapped = sum(1 for row in kept[i] if row["pops"] % Q + row["running"] > Q)
            print("lap", i, "releases", pops, "steps with a wrapped ring", lapped)
            assert pops >= 2 * Q and lapped >= 10, (i, pops, lapped)
            _rows_match(dev, i, kept[i], "lap")
            _end_matches(snap, i, final, "lap")
            run = _rank_order(env, i, final, "lap")
            assert run["head"][i] == pops % Q, (i, run["head"][i], pops)
            go.close()
    assert kinds["admitted"] > 0 and kinds["fallback"] > 0, kinds
    env.close(); tw.close()


# ---------------------------------------------------------------------------------------- 5. fewer waves per workgroup
def _layout(env):
    fields = _fields("ORLG_SHAPE_FIELDS")
    out = (C.c_int32 * len(fields))()
    env.L.orlg_debug_layout.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int]
    assert env.L.orlg_debug_layout(env.h, out, len(fields)) == len(fields)
    return dict(zip(fields, out))


def _plan(env, B, n):
    lay, wpb = _layout(env), env.launch_info()["envs_per_workgroup"]
    return wave_plan(gated=1, protect=1, max_margin=1, K=env.k_paths, n_steps=n, shared_bytes=lay["l_shared_bytes"], wave_bytes=lay["l_wave_bytes"],
                     extra_per_wave=(4 * lay["Q"] + 15) & ~15, wpb=wpb, B=B), wpb


def test_the_launch_of_fewer_waves_per_workgroup():
    c = mm.FEWER
    topo = topology(pref.CASES[c["case"]]["topology"])
    gate = pref.case_gate(topo, protect=True)
    kw = pref.case_kwargs(c["case"])
    B, n = c["B"], c["n"]
    small, large = (rmsa_env(topo, B, gn_gate=gate, **dict(kw, **over)) for over in ({}, dict(queue_capacity=c["queue_capacity"])))
    assert large.queue_capacity == c["queue_capacity"]
    plan, wpb = _plan(large, B, n)
    assert 0 < plan["wpu"] < wpb and B > 2 * plan["wpu"] and B % plan["wpu"], (plan, wpb)   # several workgroups, the last one partial
    runs = []
    for e in (small, large):
        e.run("sap_ff", c["warmup"], auto_reset=True)
        runs.append(e.run("any_mm", n, outputs=FULL_OUTS, auto_reset=True))
    said = large.last_kernel()
    assert said.startswith(_mm_name(large.words_per_link)), said
    assert " grid=%d block=%d lds=%d" % (plan["nblocks"], 64 * plan["wpu"], plan["lds"]) in said, (said, plan)
    for k in FULL_OUTS:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    assert np.isfinite(runs[0]["gn_window_margin_db"]).any() and (~runs[0]["accepted"].astype(bool)).any()
    same_bytes(snapshot(small, save_state=False), snapshot(large, save_state=False), "fewer waves")
    a, b = small.running_services(), large.running_services()
    assert np.array_equal(a["count"], b["count"]) and a["count"].min() > 0
    for k, v in a.items():   # (the rows are as long as the ring: compared up to each environment's count)
        if v.ndim == 2:
            for i in range(B):
                assert v[i, :a["count"][i]].tobytes() == b[k][i, :a["count"][i]].tobytes(), (k, i)
    for e in (small, large):
        e.reduce_counters()
        e.close()


def test_a_ring_that_leaves_no_room_for_one_wave_is_refused(tmp_path):
    """the handle's own workgroup of one wave fits the LDS, the max-margin kernel's does not: refused before anything is launched, and
    the handle keeps serving every other launch; with half the ring the same shape runs"""
    from optical_rl_gym_amd import OrlgError
    from optical_rl_gym_amd.topology_io import topology_from_txt
    c = mm.REFUSED
    name = "g%dx%d_k%d_s%d" % (c["rows"], c["cols"], c["k"], c["S"])
    edges = grid_edges(c["rows"], c["cols"], np.random.default_rng(5))
    topo = topology_from_txt(write_topology(tmp_path, name, c["rows"] * c["cols"], edges), name, k_paths=c["k"])
    kw = dict(num_spectrum_resources=c["S"], load=c["load"], mean_service_holding_time=25, episode_length=200, seed=3)
    env, half = (rmsa_env(topo, 2, gn_gate=pref.case_gate(topo, protect=True), queue_capacity=Q, **kw) for Q in (c["queue_capacity"], c["fits"]))
    assert env.queue_capacity == c["queue_capacity"]
    plan, wpb = _plan(env, 2, 1)
    assert wpb == 1 and plan["wpu"] == 0 and plan["nblocks"] == 0 and plan["lds"] > 160 * 1024, (plan, wpb)
    env.run("sap_ff", 20, auto_reset=True)
    before = env.save_state().tobytes()
    for policy, actions in (("sap_mm", None), ("any_mm", None), ("path_mm_external", np.zeros(2, np.int32))):
        with pytest.raises(OrlgError, match="%d compacted services \\(%d B\\) exceed the 160 KiB LDS" % (c["queue_capacity"], plan["lds"])):
            env.run(policy, 1, actions=actions)
    assert env.save_state().tobytes() == before
    r = env.run("sap_ff_gn", 5, outputs=("accepted",), auto_reset=True)   # the gated step and the query do not need the room
    assert "orlg_rmsa_kernel<" in env.last_kernel() and r["accepted"].any()
    slots, _ = env.max_margin_windows()
    assert (slots < c["S"]).any()
    plan, wpb = _plan(half, 2, 3)
    assert plan["wpu"] == 1
    half.run("sap_ff", 20, auto_reset=True)
    dev = half.run("sap_mm", 3, outputs=DECIDED, auto_reset=True)
    assert half.last_kernel().startswith(_mm_name(2)) and " block=64 lds=%d" % plan["lds"] in half.last_kernel(), half.last_kernel()
    assert dev["accepted"].any()
    env.close(); half.close()
