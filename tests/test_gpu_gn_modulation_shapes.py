"""The adaptive-modulation kernel ``orlg_rmsa_am_kernel<W, STATS>`` and its query ``orlg_gn_modulation_kernel<W>`` at
the shapes ``test_gpu_gn_modulation.py`` leaves out, against ``gn_modulation_reference.AdaptiveOracle``:
  1. the statistics of a state with levels at ``stats_level="full"``: every per-step output, ``link_stats``, ``graph_stats``,
     ``bit_rate_hist`` and the pending request, after one launch and after launches with and without levels in turn;
  2. ``<W,0>`` and ``<W,1>`` (``stats_level="counters"`` / ``"network"``) against the reference and against the ``full`` launch;
  3. more than eight candidate paths (the path's words ``W`` lanes apart): the fused launch, given paths and candidates from 8 up,
     the query, the query loop; too many path records;
  4. M = 1 and M = 3 levels;  5. more than 128 interferers;  6. a ring whose head laps;  7. the query on ``ring34`` and at one and
  eight words per link;  8. per-environment loads and a DeepRMSA handle.
Everything is exact but ``gn_gsnr_db`` and the query's ``gsnr`` (rtol 1e-9, NaN in place: a wave reduction against a sequential sum).
``test_gn_modulation_args.py`` pins on the reference alone what each shape reaches.  Every test asserts its kernel's name."""
import functools

import numpy as np
import pytest

import gn_audit_reference as aref
import gn_modulation_reference as am
from gpu_support import (COMPACTNESS, MANY_PATHS, MANY_PATHS_SEED, RMSA_OUTS, device_log_in_oracle, many_paths_topology, rmsa_env, snapshot,
                         state_matches, topology)

pytestmark = pytest.mark.gpu

GN = ("gn_gsnr_db", "gn_se")
LINK_AVG = ("avg_link_compactness", "avg_link_utilization")
FULL_OUTS = RMSA_OUTS + LINK_AVG + GN
DECIDED = ("act_path", "act_slot", "accepted", "done", "request", "arrival", "holding") + GN   # what every statistics level keeps
STATS_CASES = ("nsfnet_s128_l25_6dbm", "nsfnet_s320_l150_0dbm")


def _am_name(env, level=2):
    return "orlg_rmsa_am_kernel<%d,%d> " % (env.words_per_link, level)


def _rows_match(dev, i, want, what, t0=0):
    """environment i of the device's per-step outputs against the reference's rows (arrays by name, or a list of row dicts): every
    output the launch asked for, exact; gn_gsnr_db to rtol 1e-9 with NaN in place"""
    if isinstance(want, list):
        want = {k: np.array([row[k] for row in want]) for k in want[0]}
    n = len(want["act_path"])
    sl = slice(t0, t0 + n)
    for name in dev:
        if name == "gn_gsnr_db":
            continue
        got, ref = dev[name][sl, i], want[name]
        bad = np.flatnonzero((got != ref).reshape(n, -1).any(axis=1))
        assert bad.size == 0, (what, i, name, bad[:5], got[bad[:5]], ref[bad[:5]])
    if "gn_gsnr_db" in dev:
        g, w = dev["gn_gsnr_db"][sl, i], want["gsnr"]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, i, "NaN in place")
        ok = ~np.isnan(w)
        np.testing.assert_allclose(g[ok], w[ok], rtol=1e-9, atol=0, err_msg=str((what, i)))


def _end_matches(snap, i, final, what, level=2):
    """environment i of a snapshot against AdaptiveOracle.final(): occupancy, counters, clock, services in progress, the histograms and the
    pending request; at level `full` every link and graph statistic"""
    state_matches(snap, i, final, what, link_stats=level == 2)
    for name, v in final["bit_rate_hist"].items():
        assert np.array_equal(snap["bit_rate_hist." + name][i], v), (what, i, name)
    req = snap["requests"][i]
    assert (req["service_id"], req["src"], req["dst"], req["bit_rate"], req["arrival_time"], req["holding_time"]) == final["request"], (what, i)


def _services_match(env, i, services, gate, what, audit=True):
    """running_services() (rank order, with levels) and qot_audit() of environment i against the reference's services and their audit"""
    svc, gids, rates, releases = services
    run = env.running_services()
    n = len(svc)
    assert run["count"][i] == n, (what, i)
    assert np.array_equal(run["se"][i, :n], [s[3] for s in svc]) and (run["se"][i, n:] == -1).all(), (what, i, "se")
    assert np.array_equal(run["path_gid"][i, :n], gids) and np.array_equal(run["slot"][i, :n], [s[1] for s in svc]), (what, i)
    assert np.array_equal(run["num_slots"][i, :n], [s[2] for s in svc]) and np.array_equal(run["bit_rate"][i, :n], rates), (what, i)
    assert np.array_equal(run["release_time"][i, :n], releases), (what, i)
    if audit:
        a = env.qot_audit(services=True)
        want = aref.audit(svc, gate)
        assert a["n_running"][i] == n, (what, i)
        np.testing.assert_allclose(a["gsnr_db"][i, :n], want["gsnr_db"], rtol=1e-9, atol=0, err_msg=str((what, i)))
        thr = np.array([gate["thresholds_db"][s[3] - 1] for s in svc])
        assert np.array_equal(a["margin_db"][i, :n], a["gsnr_db"][i, :n] - thr), (what, i, "every service at ITS level's threshold")
    return run


def _host_walk(slot, admitted, S, K):
    """sap_ff_am on the rows of modulation_windows() of one environment: (path, slot, se)"""
    first = None
    for p in range(K):
        for m in range(slot.shape[1], 0, -1):
            if slot[p, m - 1] >= S:
                break
            if admitted[p, m - 1]:
                return p, int(slot[p, m - 1]), m
            if first is None:
                first = (p, int(slot[p, m - 1]), m)
    return first if first is not None else (K, S, 0)


def _query_matches(q, i, ao, what):
    """every [k, M] entry of environment i of modulation_windows() against the reference with no early exit, best_se against the host walk;
    returns how many entries had a window, how many of those were refused, and how many lay on paths 8 and above"""
    slot, gsnr, admitted, best = q
    K, M, S = ao.K, ao.M, ao.S
    assert slot.shape[1:] == (K, M) and gsnr.shape == slot.shape == admitted.shape and best.shape[1:] == (K,), what
    assert slot.dtype == np.int16 and gsnr.dtype == np.float64 and admitted.dtype == np.uint8 and best.dtype == np.uint8
    ao.drop_due()
    windows = refused = high = 0
    for p in range(K):
        rows = {m: (s, g, ok) for m, s, _, g, ok in ao.levels_of_path(p)}
        high += len(rows) if p >= 8 else 0
        for m in range(1, M + 1):
            if m in rows:
                assert slot[i, p, m - 1] == rows[m][0] and admitted[i, p, m - 1] == rows[m][2], (what, i, p, m)
                assert np.isclose(gsnr[i, p, m - 1], rows[m][1], rtol=1e-9, atol=0), (what, i, p, m)
                windows, refused = windows + 1, refused + (not rows[m][2])
            else:
                assert slot[i, p, m - 1] == S and np.isnan(gsnr[i, p, m - 1]) and admitted[i, p, m - 1] == 0, (what, i, p, m)
        walk = _host_walk(slot[i, p:p + 1], admitted[i, p:p + 1], S, 1)
        assert best[i, p] == (walk[2] if walk[0] == 0 and admitted[i, p, walk[2] - 1] else 0), (what, i, p)
    return windows, refused, high


def _loop_equals_fused(env, tw, n, outs, what, ao=None, i=0):
    """n steps of sap_ff_am in one launch on `env`, and on its twin `tw` the loop modulation_windows() + host walk + external_am: the same
    bytes in every output and in save_state.  With `ao`, the reference of environment i in the same state: every query of the loop and
    every step against it; returns the launch's outputs and the query entries (with a window, refused, on paths 8 and above)"""
    K, S = env.k_paths, env.num_spectrum_resources
    dev = env.run("sap_ff_am", n, outputs=outs, auto_reset=True)
    assert env.last_kernel().startswith(_am_name(env)), env.last_kernel()
    tally = np.zeros(3, np.int64)
    for t in range(n):
        q = tw.modulation_windows()
        slot, _, admitted, _ = q
        if ao is not None:
            tally += _query_matches(q, i, ao, (what, t))
        acts = np.array([_host_walk(slot[e], admitted[e], S, K) for e in range(env.batch_size)], np.int32)
        r = tw.run("external_am", 1, actions=acts, outputs=outs, auto_reset=True)
        for k in outs:
            assert r[k][0].tobytes() == dev[k][t].tobytes(), (what, t, k, r[k][0], dev[k][t])
        if ao is not None:
            _rows_match(r, i, [ao.step_route("sap")], (what, "loop", t))
    assert tw.last_kernel().startswith(_am_name(tw)), tw.last_kernel()
    assert env.save_state().tobytes() == tw.save_state().tobytes(), what
    return dev, tally


# ---------------------------------------------------------------------------------------- 1. statistics of a state with levels
def _handle(case, batch=am.B, **over):
    c = am.CASES[case]
    topo = topology(c["topology"])
    gate = am.case_gate(topo, c["dbm"])
    return rmsa_env(topo, batch, gn_gate=gate, **am.case_kwargs(case, **over)), topo, gate


@functools.lru_cache(maxsize=None)
def _full_launch(case):
    """the case's one launch at stats_level="full": (outputs, snapshot, what last_kernel() said); run once and shared, read-only"""
    env, _, _ = _handle(case)
    dev = env.run("sap_ff_am", am.CASES[case]["n"], outputs=FULL_OUTS, auto_reset=True)
    said, snap = env.last_kernel(), snapshot(env)
    env.close()
    return dev, snap, said


@pytest.mark.parametrize("case", STATS_CASES)
def test_statistics_at_level_full(case):
    dev, snap, said = _full_launch(case)
    W = (am.CASES[case]["S"] + 63) // 64
    assert said.startswith("orlg_rmsa_am_kernel<%d,2> " % W), said
    for i in range(am.B):
        tr, final, fig, _ = am.run_case(case, i)
        assert fig["released_other"] >= 1   # (a release that must take the level's slots)
        _rows_match(dev, i, tr, case)
        _end_matches(snap, i, final, case)
    assert (dev["reward"] != 0).any() and (dev["network_compactness"] > 0).any() and (dev["avg_link_utilization"] > 0).any()


def test_statistics_after_launches_with_and_without_levels():
    """the plan of test_existing_policies_on_an_adaptive_handle: releases of services with and without a level interleave"""
    env, topo, gate = _handle(am.MIXED_CASE)
    outs = tuple(o for o in FULL_OUTS if o != "gn_se")
    devs = []
    for policy, n in am.MIXED_PLAN:
        devs.append(env.run(policy, n, outputs=outs + (("gn_se",) if policy.endswith("_am") else ()), auto_reset=True))
        assert env.last_kernel().startswith(_am_name(env)), (policy, env.last_kernel())
    snap = snapshot(env)
    for i in range(am.B):
        tr, final, fig, services = am.run_mixed(i)
        assert 1 <= fig["released_other"] < fig["released"]
        t0 = 0
        for (policy, n), dev in zip(am.MIXED_PLAN, devs):
            _rows_match(dev, i, {k: v[t0:t0 + n] for k, v in tr.items()}, (policy, t0))
            t0 += n
        _end_matches(snap, i, final, "mixed")
        if i in (0, 5):
            _services_match(env, i, services, gate, "mixed")
    env.close()


# ---------------------------------------------------------------------------------------- 2. the lighter statistics levels
@pytest.mark.parametrize("level", ["counters", "network"])
@pytest.mark.parametrize("case", STATS_CASES)
def test_the_lighter_statistics_levels(case, level):
    lv = ("counters", "network", "full").index(level)
    outs = DECIDED + (COMPACTNESS if lv >= 1 else ())
    env, topo, gate = _handle(case, stats_level=level)
    dev = env.run("sap_ff_am", am.CASES[case]["n"], outputs=outs, auto_reset=True)
    assert env.last_kernel().startswith(_am_name(env, lv)), env.last_kernel()
    snap = snapshot(env)
    for i in range(am.B):
        tr, final, _, services = am.run_case(case, i)
        _rows_match(dev, i, tr, (case, level))
        state_matches(snap, i, final, (case, level), link_stats=False)
        if i in (0, am.B - 1):
            _services_match(env, i, services, gate, (case, level), audit=False)
    full, fsnap, _ = _full_launch(case)
    for k in outs:   # the same bytes as the launch that keeps every statistic
        assert dev[k].tobytes() == full[k].tobytes(), (case, level, k)
    assert snap["occupancy"].tobytes() == fsnap["occupancy"].tobytes() and snap["current_time"].tobytes() == fsnap["current_time"].tobytes()
    for k in snap:
        if k.startswith("counters."):
            assert snap[k].tobytes() == fsnap[k].tobytes(), (case, level, k)
    env.close()


# ---------------------------------------------------------------------------------------- 3. more than eight candidate paths
def _many(shape, tmp_path, batch=am.B):
    topo = many_paths_topology(shape, tmp_path)
    _, kw, gate, seed, n = am.shape_setup(shape, topo)
    assert seed == MANY_PATHS_SEED and topo.k_paths == MANY_PATHS[shape]["k"] > 8
    return rmsa_env(topo, batch, gn_gate=gate, **kw), topo, kw, gate, n


@pytest.mark.parametrize("shape", list(am.MANY))
def test_many_paths_fused_launch_and_query(shape, tmp_path):
    env, topo, kw, gate, n = _many(shape, tmp_path)
    tw = _many(shape, tmp_path)[0]
    assert env.words_per_link == MANY_PATHS[shape]["W"]
    outs = ("act_path", "act_slot", "accepted", "done", "request") + GN
    dev = env.run("sap_ff_am", n, outputs=outs, auto_reset=True)
    assert env.last_kernel().startswith(_am_name(env)), env.last_kernel()
    tw.run("sap_ff_am", n, auto_reset=True)
    snap = snapshot(env)
    for i in range(am.B):
        tr, final, _, services = am.run_shape(shape, i, topo=topo)
        _rows_match(dev, i, tr, shape)
        _end_matches(snap, i, final, shape)
        if i == 1:
            _services_match(env, i, services, gate, shape)
    acc = dev["accepted"].astype(bool)
    assert (dev["act_path"][acc] >= 8).sum() >= 10, shape   # the paths whose words lie W lanes apart were provisioned
    # the query loop against the fused launch, and every query of environment 1 entry by entry against the reference
    with device_log_in_oracle():
        ao = am.AdaptiveOracle(topo, kw, gate, seed=MANY_PATHS_SEED + 1)
        ao.run_route("sap", n)
        _, (windows, refused, high) = _loop_equals_fused(env, tw, 30, outs, shape, ao, 1)
        ao.close()
    print(shape, "query entries with a window", windows, "refused", refused, "on paths >= 8", high)
    assert windows > refused >= 1 and high >= 1, (shape, windows, refused, high)
    env.close(); tw.close()


@pytest.mark.parametrize("shape", list(am.MANY))
def test_many_paths_given_paths_and_candidates(shape, tmp_path):
    """path_am_external with paths 8 .. k (k: out of range), then external_am with candidates of the reference's walk on paths >= 8"""
    B, warm, n = 4, 60, 30
    env, topo, kw, gate, _ = _many(shape, tmp_path, batch=B)
    K, S, M = topo.k_paths, env.num_spectrum_resources, 6
    outs = ("act_path", "act_slot", "accepted", "done", "request") + GN
    rng = np.random.default_rng(5)
    env.run("sap_ff_am", warm, auto_reset=True)
    kinds = dict(given_accepted=0, given_refused=0, out_of_range=0, candidate_accepted=0, candidate_refused=0)
    with device_log_in_oracle():
        oracles = [am.AdaptiveOracle(topo, kw, gate, seed=MANY_PATHS_SEED + i) for i in range(B)]
        for ao in oracles:
            ao.run_route("sap", warm)
        given = rng.integers(8, K + 1, size=(n, B)).astype(np.int32)
        for t in range(n):
            r = env.run("path_am_external", 1, actions=given[t], outputs=outs, auto_reset=True)
            for i, ao in enumerate(oracles):
                row = ao.step_route("path", given[t, i])
                _rows_match(r, i, [row], (shape, "path_am_external", t, int(given[t, i])))
                kinds["given_accepted"] += row["accepted"]
                kinds["given_refused"] += int(not row["accepted"] and np.isfinite(row["gsnr"]))
                kinds["out_of_range"] += int(given[t, i] == K)
        assert env.last_kernel().startswith(_am_name(env)), env.last_kernel()
        for t in range(n):
            acts = np.zeros((B, 3), np.int32)
            for i, ao in enumerate(oracles):
                p = int(rng.integers(8, K))
                ao.drop_due()
                levels = ao.levels_of_path(p)
                if levels:
                    m, s, _, _, _ = levels[int(rng.integers(0, len(levels)))]
                    acts[i] = (p, s, m)
                else:
                    acts[i] = (p, int(rng.integers(0, S)), int(rng.integers(1, M + 1)))
            r = env.run("external_am", 1, actions=acts, outputs=outs, auto_reset=True)
            for i, ao in enumerate(oracles):
                row = ao.step_external(*[int(v) for v in acts[i]])
                _rows_match(r, i, [row], (shape, "external_am", t, tuple(acts[i])))
                kinds["candidate_accepted"] += row["accepted"]
                kinds["candidate_refused"] += int(not row["accepted"] and np.isfinite(row["gsnr"]))
        assert env.last_kernel().startswith(_am_name(env)), env.last_kernel()
        snap = snapshot(env)
        for i, ao in enumerate(oracles):
            _end_matches(snap, i, ao.final(), shape)
            ao.close()
    print(shape, kinds)
    assert kinds["given_accepted"] > 0 and kinds["out_of_range"] > 0 and kinds["candidate_accepted"] > 0, kinds
    env.close()


def test_too_many_path_records_are_refused_on_the_device(tmp_path):
    from optical_rl_gym_amd import rmsa_gn_gate_parameters
    from gpu_support import many_paths_kwargs
    topo = many_paths_topology(am.MANY_REFUSED, tmp_path)
    with pytest.raises(ValueError, match="path records"):
        rmsa_env(topo, 2, gn_gate=am.case_gate(topo, 6.0), **many_paths_kwargs(am.MANY_REFUSED))
    env = rmsa_env(topo, 2, gn_gate=rmsa_gn_gate_parameters(topo, launch_power_dbm_per_50ghz=6.0), **many_paths_kwargs(am.MANY_REFUSED))
    before = env.save_state().tobytes()
    assert env.L.orlg_set_gn_modulation(env.h, 1) == -1 and b"path records" in env.L.orlg_last_error()
    env.run("sap_ff", 5, auto_reset=True)   # the handle stays what it was: a plain gated one
    assert "orlg_rmsa_kernel<" in env.last_kernel() and env.save_state().tobytes() != before
    env.close()


# ---------------------------------------------------------------------------------------- 4. M = 1 and M = 3
@pytest.mark.parametrize("shape", ["m3_6dbm", "m3_0dbm", "m1_6dbm", "m1_0dbm"])
def test_fewer_levels(shape):
    c = am.SHAPES[shape]
    M = c["M"]
    topo, kw, gate, seed, n = am.shape_setup(shape, topology(c["topology"]))
    env = rmsa_env(topo, am.B, gn_gate=gate, **kw)
    assert env.gn_adaptive and env.modulation_levels == M
    K, S = topo.k_paths, env.num_spectrum_resources
    outs = DECIDED
    dev = env.run("sap_ff_am", n, outputs=outs, auto_reset=True)
    assert env.last_kernel().startswith(_am_name(env)), env.last_kernel()
    snap = snapshot(env)
    for i in range(am.B):
        tr, final, _, services = am.run_shape(shape, i)
        _rows_match(dev, i, tr, shape)
        _end_matches(snap, i, final, shape)
        if i == 0:
            _services_match(env, i, services, gate, shape)
    assert dev["gn_se"].max() == M
    if c["dbm"] == 0.0:   # the all-admitted arm
        assert (dev["accepted"] == np.isfinite(dev["gn_gsnr_db"])).all()
    else:
        assert (~dev["accepted"].astype(bool) & np.isfinite(dev["gn_gsnr_db"])).any()
    # the query has M columns; external_am with a real candidate and with se = M + 1 in turn
    rng = np.random.default_rng(3)
    with device_log_in_oracle():
        oracles = [am.AdaptiveOracle(topo, kw, gate, seed=seed + i) for i in (0, 1)]
        for ao in oracles:
            ao.run_route("sap", n)
        for t in range(10):
            q = env.modulation_windows()
            assert q[0].shape == (am.B, K, M) and q[3].shape == (am.B, K)
            acts = np.zeros((am.B, 3), np.int32)
            acts[:, 0], acts[:, 2] = K, 0   # (the other environments: an action out of range)
            for i, ao in enumerate(oracles):
                _query_matches(q, i, ao, (shape, t))
                p = int(rng.integers(0, K))
                levels = ao.levels_of_path(p)
                if t % 2 == 0 and levels:
                    m, s, _, _, _ = levels[int(rng.integers(0, len(levels)))]
                    acts[i] = (p, s, m)
                else:
                    acts[i] = (p, levels[0][1] if levels else 0, M + 1)
            r = env.run("external_am", 1, actions=acts, outputs=outs, auto_reset=True)
            for i, ao in enumerate(oracles):
                _rows_match(r, i, [ao.step_external(*[int(v) for v in acts[i]])], (shape, "external_am", t, tuple(acts[i])))
                if acts[i, 2] == M + 1:
                    assert r["accepted"][0, i] == 0 and np.isnan(r["gn_gsnr_db"][0, i]) and r["gn_se"][0, i] == 0
        for ao in oracles:
            ao.close()
    assert env.last_kernel().startswith(_am_name(env)), env.last_kernel()
    env.close()


# ---------------------------------------------------------------------------------------- 5. three chunks of interferers
def test_three_chunks_of_interferers():
    shape = "chunks3"
    c = am.SHAPES[shape]
    topo, kw, gate, seed, n = am.shape_setup(shape)
    env = rmsa_env(topo, c["B"], gn_gate=gate, **kw)
    outs = DECIDED
    # the query of environment 0 where it has the most services in progress (the network is full there: no level of any path has a
    # window), and at the first step of more than 128 where the walk checks several levels
    tr0, _, fig0, _ = am.run_shape(shape, 0)
    busy = np.flatnonzero((tr0["n_running"] > 128) & (tr0["n_checked"] >= 2))
    points = sorted({int(busy[0]), fig0["peak_step"]})
    assert len(points) == 2 and tr0["n_running"][fig0["peak_step"]] == fig0["max_running"] > 128
    parts, windows = [], 0
    with device_log_in_oracle():
        ao = am.AdaptiveOracle(topo, kw, gate, seed=seed)
        for a, b in zip([0] + points, points + [n]):
            parts.append(env.run("sap_ff_am", b - a, outputs=outs, auto_reset=True))
            assert env.last_kernel().startswith(_am_name(env)), env.last_kernel()
            ao.run_route("sap", b - a)
            if b < n:
                ao.drop_due()
                assert len(ao.shadow) == tr0["n_running"][b] > 128 and env.num_running()[0] > 128
                windows += _query_matches(env.modulation_windows(), 0, ao, (shape, b))[0]
        ao.close()
    assert windows >= 2
    dev = {k: np.concatenate([p[k] for p in parts]) for k in outs}
    snap = snapshot(env)
    for i in range(c["B"]):
        tr, final, fig, services = am.run_shape(shape, i)
        assert fig["max_running"] > 128
        _rows_match(dev, i, tr, shape)
        _end_matches(snap, i, final, shape)
        _services_match(env, i, services, gate, shape, audit=i in (0, 3))
    env.close()


# ---------------------------------------------------------------------------------------- 6. a ring that laps
def test_the_ring_laps():
    shape = "lap"
    c = am.SHAPES[shape]
    topo, kw, gate, seed, n = am.shape_setup(shape)
    peak = max(am.run_shape(shape, i)[2]["max_running"] for i in range(am.B))
    Q = am.ring_capacity(peak, c["queue_margin"])
    env = rmsa_env(topo, am.B, gn_gate=gate, queue_capacity=peak + c["queue_margin"], **kw)
    assert env.queue_capacity == Q
    outs, chunk = DECIDED, 10
    parts, compared = [], 0
    with device_log_in_oracle():
        oracles = [am.AdaptiveOracle(topo, kw, gate, seed=seed + i) for i in range(am.B)]
        for t in range(0, n, chunk):
            parts.append(env.run("sap_ff_am", chunk, outputs=outs, auto_reset=True))
            for ao in oracles:
                ao.run_route("sap", chunk)
            if compared < 3:   # the query where a ring's live entries wrap at Q, of an environment whose request has a window
                run = env.running_services()
                q = env.modulation_windows()
                for i in np.flatnonzero(run["head"] + run["count"] > Q):
                    assert run["head"][i] < Q and run["count"][i] >= 2
                    if _query_matches(q, int(i), oracles[i], (shape, t, i))[0] >= 1:
                        compared += 1
                        break
        assert compared == 3
        assert env.last_kernel().startswith(_am_name(env)), env.last_kernel()
        env.reduce_counters()   # (raises where a release ring overflowed)
        dev = {k: np.concatenate([p[k] for p in parts]) for k in outs}
        snap = snapshot(env)
        for i, ao in enumerate(oracles):
            tr, final, fig, services = am.run_shape(shape, i)
            assert fig["released"] >= 2 * Q
            _rows_match(dev, i, tr, shape)
            _end_matches(snap, i, final, shape)
            _services_match(env, i, ao.services(), gate, shape, audit=i in (0, am.B - 1))
            ao.close()
    env.close()


# ---------------------------------------------------------------------------------------- 7. the query at the other word counts
@pytest.mark.parametrize("case", ["ring34_s100_l60_6dbm", "nsfnet_s64_l12_6dbm", "nsfnet_s512_l100_6dbm"])
def test_the_query_at_the_other_word_counts(case):
    c = am.CASES[case]
    env, topo, gate = _handle(case)
    K, S, warm = topo.k_paths, env.num_spectrum_resources, 100
    outs = DECIDED
    env.run("sap_ff_am", warm, auto_reset=True)
    windows = refused = 0
    with device_log_in_oracle():
        oracles = [am.AdaptiveOracle(topo, am.case_kwargs(case), gate, seed=c["seed"] + i) for i in (0, 1)]
        for ao in oracles:
            ao.run_route("sap", warm)
        for t in range(10):
            q = env.modulation_windows()
            assert q[0].shape == (am.B, K, 6)
            for i, ao in enumerate(oracles):
                w, r, _ = _query_matches(q, i, ao, (case, t))
                windows, refused = windows + w, refused + r
            for i in range(2, am.B):   # best_se of the others: the host walk on the query's own rows
                for p in range(K):
                    walk = _host_walk(q[0][i, p:p + 1], q[2][i, p:p + 1], S, 1)
                    assert q[3][i, p] == (walk[2] if walk[0] == 0 and q[2][i, p, walk[2] - 1] else 0), (case, t, i, p)
            r = env.run("sap_ff_am", 1, outputs=outs, auto_reset=True)
            for i, ao in enumerate(oracles):
                _rows_match(r, i, [ao.step_route("sap")], (case, t))
        for ao in oracles:
            ao.close()
    assert env.last_kernel().startswith(_am_name(env)), env.last_kernel()
    assert windows > refused >= 1, (case, windows, refused)
    env.close()


# ---------------------------------------------------------------------------------------- 8. per-environment loads, a DeepRMSA handle
def test_per_environment_loads():
    from optical_rl_gym_amd import make_sweep
    c = am.SWEEP
    topo = topology(c["topology"])
    gate = am.case_gate(topo, c["dbm"])
    skw = dict(num_spectrum_resources=c["S"], mean_service_holding_time=am.ref.HOLDING_TIME, episode_length=am.ref.EPISODE_LENGTH)
    env, tw = (make_sweep("rmsa", topo, loads=list(c["loads"]), seeds_per_load=c["seeds_per_load"], seed=c["seed"], gn_gate=gate, **skw)
               for _ in range(2))
    assert env.batch_size == len(c["loads"]) * c["seeds_per_load"] and env.loads.tolist() == [10.0] * 3 + [40.0] * 3
    dev, _ = _loop_equals_fused(env, tw, c["n"], DECIDED, "sweep")   # the twin: query + host walk + external_am, step by step
    snap = snapshot(env)
    for i in range(env.batch_size):
        tr, final, _, services = am.run_sweep(i)
        _rows_match(dev, i, tr, "sweep")
        _end_matches(snap, i, final, "sweep")
        if i in (0, env.batch_size - 1):
            _services_match(env, i, services, gate, "sweep")
    env.close(); tw.close()


def test_a_deeprmsa_handle():
    from optical_rl_gym_amd import BatchedDeepRMSAEnv
    c = am.DEEP
    topo = topology(c["topology"])
    gate = am.case_gate(topo, c["dbm"])
    dkw = dict(mean_service_holding_time=25.0, mean_service_inter_arrival_time=25.0 / c["load"], num_spectrum_resources=c["S"],
               episode_length=1000, seed=c["seed"], j=c["j"])
    env, tw = (BatchedDeepRMSAEnv(topo, c["B"], gn_gate=gate, **dkw) for _ in range(2))
    assert env.gn_adaptive
    outs = DECIDED + ("reward",)
    dev = env.run("sap_ff_am", c["n"], outputs=outs, auto_reset=True)
    assert env.last_kernel().startswith(_am_name(env)), env.last_kernel()
    assert np.array_equal(dev["reward"], np.where(dev["accepted"].astype(bool), 1.0, -1.0)) and (dev["reward"] < 0).any()
    # a state with levels under the class's own heuristic: the path's own spectral efficiency, checked once
    own_outs = tuple(o for o in outs if o != "gn_se")
    own = env.run("deeprmsa_sap_ff", c["n_own"], outputs=own_outs, auto_reset=True)
    assert env.last_kernel().startswith(_am_name(env)), env.last_kernel()
    snap = snapshot(env)
    for i in range(c["B"]):
        tr, own_rows, final, _, services = am.run_deep(i)
        _rows_match(dev, i, tr, "deeprmsa")
        _rows_match(own, i, own_rows, "deeprmsa_sap_ff")
        _end_matches(snap, i, final, "deeprmsa")
        if i == 0:
            _services_match(env, i, services, gate, "deeprmsa")
    # the observation runs on a state with levels, and a second adaptive handle loaded from the snapshot gives the same one
    tw.load_state(env.save_state())
    a, b = env.observation(), tw.observation()
    assert a.shape == (c["B"], env.obs_dim) and np.isfinite(a).all() and a.tobytes() == b.tobytes()
    env.close(); tw.close()
