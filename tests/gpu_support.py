"""Scaffolding of the GPU tests, each piece once: the oracle on the device's logarithm, the step-kernel fixture, handle factories,
the tooling environment, a launch driver, read-backs and their byte-for-byte comparison, the comparison with the oracle, the
expected instantiation names, external actions, the group kernel's launch plan, the action masks, synthetic grids, the shapes
of more than eight candidate paths.  Test modules
import from here and never from each other.  Importing this module needs no GPU and loads neither the library nor the oracle:
both are imported inside the functions that use them."""
import contextlib
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from conftest import load_topology, oracle_env_from_kwargs, phy_oracle_from_kwargs

RMSA_OUTS = ("act_path", "act_slot", "accepted", "done", "reward", "request", "arrival", "holding", "network_compactness",
             "network_compactness_difference")
COMPACTNESS = ("network_compactness", "network_compactness_difference")
PHY_CONTINUOUS_OUTS = ("act_path", "n_channels", "channels", "channels_used_f64", "channels_free_f64", "accepted", "done", "request",
                       "arrival", "holding", "number_cuts_total", "rss_total_metric")
DECISIONS = ("act_path", "act_slot", "accepted", "arrival", "holding")
# the oracle's per-step fields that test_oracle_golden.py and test_many_links.py hold to the reference's traces
INT_FIELDS = ["service_id", "bit_rate", "accepted", "done", "services_processed", "services_accepted",
              "episode_services_processed", "episode_services_accepted", "bit_rate_requested",
              "bit_rate_provisioned", "episode_bit_rate_requested", "episode_bit_rate_provisioned", "free_total"]
FLOAT_FIELDS = ["arrival", "holding", "reward", "network_compactness", "network_compactness_difference",
                "avg_link_compactness", "avg_link_utilization", "fairness", "current_time", "graph_throughput",
                "graph_compactness"]
STATS_LEVELS = ("counters", "network", "full")
# every tooling variable the library reads: the getenv("ORLG_...") calls under csrc/
TOOLING_VARS = ("ORLG_GROUP_WPB", "ORLG_GROUP_CHUNKS", "ORLG_NO_DEFER", "ORLG_NO_CHUNKS", "ORLG_NO_LEAN", "ORLG_GROUP_KERNEL",
                "ORLG_PHY_NODEVEC")


# ---------------------------------------------------------------------------------------- the oracle on the device's logarithm
_log_users = 0


@contextlib.contextmanager
def device_log_in_oracle():
    """Drive the oracle's expovariate with the library's host build of the device log (a host function: no GPU needed).  Nests:
    the oracle goes back to its own logarithm when the outermost user leaves."""
    global _log_users
    import oracle as orc
    from optical_rl_gym_amd import _lib
    orc.set_log_fn(C.cast(_lib.load().orlg_host_log, C.c_void_p).value)
    _log_users += 1
    try:
        yield
    finally:
        _log_users -= 1
        if not _log_users:
            orc.set_log_fn(None)


@pytest.fixture(name="device_log_in_oracle")
def device_log_fixture():
    with device_log_in_oracle():
        yield


@pytest.fixture(params=["wave", "group"])
def step_kernel(request):
    """Both step kernels (include/orlg.h ORLG_KERNEL_*): one wavefront per environment, and four environments per wavefront."""
    yield request.param


# ---------------------------------------------------------------------------------------- handles
@functools.lru_cache(maxsize=None)
def _topology(name):
    return load_topology(name)


def topology(topo_or_name):
    return _topology(topo_or_name) if isinstance(topo_or_name, str) else topo_or_name


def rmsa_env(topo_or_name, batch, kernel="auto", cls=None, **kw):
    from optical_rl_gym_amd import BatchedRMSAEnv
    return (cls or BatchedRMSAEnv)(topology(topo_or_name), batch, step_kernel=kernel, **kw)


def phy_env(topo_or_name, tables, kw, batch, **extra):
    """kw: reference-style keyword arguments (a golden's env_kwargs; what the QoT-aware handle does not know it ignores)."""
    from optical_rl_gym_amd import BatchedPhyRMSAEnv
    pairs, mod, gsnr = tables
    return BatchedPhyRMSAEnv(topology(topo_or_name), batch, modulation_level=mod, connections_detail=pairs, gsnr=gsnr,
                             **dict(kw, **extra))


# ---------------------------------------------------------------------------------------- launches
@contextlib.contextmanager
def tooling_env(**variables):
    """Only the given ORLG_* tooling variables are set inside; the previous environment comes back exactly, also on an error."""
    assert set(variables) <= set(TOOLING_VARS), sorted(set(variables) - set(TOOLING_VARS))
    old = {k: os.environ.pop(k, None) for k in TOOLING_VARS}
    os.environ.update(variables)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def one_step_launches(env, policy, n, outs, actions=None, **kw):
    """n launches of one step; actions [n, B, ...]: row t goes to launch t.  The outputs stacked to [n, B, ...]."""
    cols = {k: [] for k in outs}
    for t in range(n):
        r = env.run(policy, 1, outputs=outs, **(kw if actions is None else dict(kw, actions=actions[t])))
        for k in outs:
            cols[k].append(r[k][0])
    return {k: np.stack(v) for k, v in cols.items()}


def drive(make, launches, outputs=RMSA_OUTS, *, env_vars=None, policy=None, actions=None, each=None):
    """A handle from make() under tooling_env(**env_vars), stepped through `launches` with auto-reset, read back and closed.
    launches: (policy, steps, actions or None[, outputs]) each, or plain step counts of `policy`; actions [n, B, ...]: row t goes
    to step t's launch (launches of one step).  Returns outs (per launch), tr (their concatenation, where the launches asked for
    the same outputs), said (last_kernel() after every launch) and kernels (its first word, the instantiation), each (each(env)
    after every launch) and snap (snapshot)."""
    with tooling_env(**(env_vars or {})):
        env = make()
        outs, said, seen, t = [], [], [], 0
        for launch in launches:
            p, n, a, *o = (policy, launch, None) if isinstance(launch, (int, np.integer)) else launch
            if actions is not None:
                assert n == 1
                a = actions[t]
            outs.append(env.run(p, n, outputs=o[0] if o else outputs, auto_reset=True, actions=a))
            said.append(env.last_kernel())
            if each is not None:
                seen.append(each(env))
            t += n
        snap = snapshot(env)
        env.close()
    tr = None
    if all(o.keys() == outs[0].keys() for o in outs):
        tr = {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}
    return dict(outs=outs, tr=tr, said=said, kernels=[s.split(" ")[0] for s in said], each=seen, snap=snap)


# ---------------------------------------------------------------------------------------- read-backs
def snapshot(env, save_state=True):
    """Everything a handle reads back, each copied: "state" (save_state), "occupancy" (occupancy_words; available_channels of the
    QoT-aware handle), the dictionaries as "counters.<name>", "link_stats.<name>", ..., and the per-environment arrays."""
    s = {}
    if save_state:
        s["state"] = env.save_state()
    s["occupancy"] = env.occupancy_words() if hasattr(env, "occupancy_words") else env.available_channels()
    for get in ("counters", "link_stats", "graph_stats", "bit_rate_hist", "episodes_done", "num_running", "current_time",
                "requests", "episode_stats"):
        if hasattr(env, get):
            v = getattr(env, get)()
            s.update({f"{get}.{k}": x for k, x in v.items()} if isinstance(v, dict) else {get: v})
    return {k: np.array(v, copy=True) for k, v in s.items()}


def same_bytes(a, b, what=""):
    """Two dictionaries of arrays hold the same keys, shapes, dtypes and bytes (-0.0 is not 0.0; equal NaN payloads are equal)."""
    assert a.keys() == b.keys(), (what, sorted(set(a) ^ set(b)))
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        if x.tobytes() != y.tobytes():
            xb, yb = (v.reshape(-1).view(np.uint8).reshape(v.size, -1) for v in (x, y))
            at = tuple(int(j) for j in np.unravel_index(np.flatnonzero((xb != yb).any(axis=1))[0], x.shape))
            raise AssertionError(f"{what}: {k} differs, first at {at}: {x[at]} != {y[at]}")


def available_slots(snap, i, num_links, S):
    """available_slots()[i] from a snapshot's occupancy words"""
    words = np.ascontiguousarray(snap["occupancy"][i]).reshape(num_links, -1)
    return np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little")[:, :S]


# ---------------------------------------------------------------------------------------- against the oracle
def _oracle_run(topo, kw, seed, policy, launches, actions=None):
    with device_log_in_oracle():
        o = oracle_env_from_kwargs(topo, kw, seed=seed)
        traces, t = [], 0
        for n in launches:
            traces.append(o.run(policy, n, reset_on_done=True, actions=None if actions is None else np.ascontiguousarray(actions[t:t + n])))
            t += n
    final = dict(available_slots=o.available_slots(), counters=o.counters(), link_stats=o.link_stats(), graph_stats=o.graph_stats(),
                 current_time=o.current_time(), num_running=o.num_running())
    o.close()
    return traces, final


@functools.lru_cache(maxsize=None)
def oracle_run(name, kw_items, seed, policy, launches):
    """One environment on the oracle (the device's logarithm in it), `launches` a tuple of step counts: (one trace per launch, the
    state after the last).  Run once per process and shared; read-only by agreement."""
    return _oracle_run(topology(name), dict(kw_items), seed, policy, launches)


def decisions_match(tr, i, want, fields, what):
    """per-step outputs of environment i against the oracle's arrays, bit for bit"""
    for f in fields:
        dev = np.ascontiguousarray(tr[f][:, i])
        assert dev.tobytes() == np.ascontiguousarray(want[f]).astype(dev.dtype).tobytes(), (what, i, f)


def state_matches(snap, i, final, what, link_stats=True):
    """environment i of a snapshot against an oracle's final state (what `final` holds of: available_slots, counters,
    current_time, num_running, link_stats, graph_stats -- the last two where the statistics level keeps them)"""
    want = final["available_slots"]
    assert np.array_equal(available_slots(snap, i, *want.shape), want), (what, i)
    for name, v in final["counters"].items():
        assert snap["counters." + name][i] == v, (what, i, name)
    assert snap["current_time"][i] == final["current_time"] and snap["num_running"][i] == final["num_running"], (what, i)
    for group in ("link_stats", "graph_stats") if link_stats else ():
        for name, v in final.get(group, {}).items():
            bad = np.flatnonzero(np.atleast_1d(snap[f"{group}.{name}"][i] != v))
            assert bad.size == 0, (what, i, group, name, bad[:6])


def against_oracle(topo, kw, run, policy, n_or_launches, envs, stats_level, actions=None, seed0=None, fields=None):
    """Environments `envs` of a drive() result against the oracle at seed0 + i (seed0: kw's seed): the decision outputs, the
    compactness outputs where the statistics level keeps them, available_slots, every counter, the clock and the services in
    progress, and at level `full` every link and graph statistic.  topo: a golden topology's name (the oracle's trace is then
    computed once per process) or a topology; actions [n, B, ...]: the external actions of the whole run."""
    level = STATS_LEVELS.index(stats_level)
    launches = (n_or_launches,) if isinstance(n_or_launches, (int, np.integer)) else tuple(n_or_launches)
    seed0 = kw["seed"] if seed0 is None else seed0
    if fields is None:
        fields = DECISIONS + (COMPACTNESS if level >= 1 else ())
    for i in envs:
        if actions is None and isinstance(topo, str):
            traces, final = oracle_run(topo, tuple(sorted(kw.items())), seed0 + i, policy, launches)
        else:
            traces, final = _oracle_run(topology(topo), kw, seed0 + i, policy, launches, None if actions is None else actions[:, i])
        decisions_match(run["tr"], i, {f: np.concatenate([t[f] for t in traces]) for f in fields}, fields, policy)
        state_matches(run["snap"], i, final, policy, link_stats=level == 2)


def everything_matches_oracle(topo, kw, tr, i, snap, policy, n, reset_on_done, actions=None, seed=None, j=1, reward_mode=0):
    """Environment i of a device run (tr: RMSA_OUTS of n steps, snap: its snapshot) against the oracle of these kwargs: every
    per-step output, the state, the histograms and the pending request bit-identical.  Returns the oracle's trace."""
    o = oracle_env_from_kwargs(topo, kw, seed=seed, j=j, reward_mode=reward_mode)
    ot = o.run(policy, n, reset_on_done=reset_on_done, actions=None if actions is None else np.ascontiguousarray(actions[:, i]))
    for f in ("act_path", "act_slot", "accepted", "done", "reward", "arrival", "holding") + COMPACTNESS:
        bad = np.nonzero(tr[f][:, i] != ot[f])[0]
        assert bad.size == 0, (f, i, kw.get("load"), bad[:4], tr[f][bad[:4], i], ot[f][bad[:4]])
    for q, g in enumerate(("service_id", "src", "dst", "bit_rate")):
        assert np.array_equal(tr["request"][:, i, q], ot[g]), (g, i)
    state_matches(snap, i, dict(available_slots=o.available_slots(), counters=o.counters(), link_stats=o.link_stats(),
                                graph_stats=o.graph_stats(), current_time=o.current_time(), num_running=o.num_running()), policy)
    for name, v in o.bit_rate_hist().items():
        assert np.array_equal(snap["bit_rate_hist." + name][i], v), (name, i)
    r, req = o.request(), snap["requests"][i]
    assert (req["service_id"], req["src"], req["dst"], req["bit_rate"], req["arrival_time"], req["holding_time"]) == \
        (r.service_id, r.src, r.dst, r.bit_rate, r.arrival_time, r.holding_time), i
    o.close()
    return ot


def compare_with_oracle(topo, kw, policy, n, batch, kernel, outs=("act_path", "act_slot", "accepted", "arrival", "network_compactness")):
    """A fresh batch against one oracle per environment after one launch of n steps: `outs`, occupancy, counters, link statistics.
    A shape whose four environments do not fit the group kernel's LDS is skipped for that kernel."""
    from optical_rl_gym_amd import OrlgError
    try:
        env = rmsa_env(topo, batch, kernel, **kw)
    except OrlgError as e:
        if kernel == "group" and "LDS" in str(e):
            pytest.skip("four environments of this shape do not fit the LDS: the wave-per-environment kernel serves it")
        raise
    tr = env.run(policy, n, outputs=outs, auto_reset=True)
    occ, cnt = env.available_slots(), env.counters()
    ls = env.link_stats()
    for i in range(batch):
        o = oracle_env_from_kwargs(topo, kw, seed=kw["seed"] + i)
        ot = o.run(policy, n, reset_on_done=True)
        for f in outs:
            assert np.array_equal(tr[f][:, i], ot[f]), (f, i)
        assert np.array_equal(occ[i], o.available_slots()), i
        oc = o.counters()
        for name in oc:
            assert cnt[name][i] == oc[name], (name, i)
        ols = o.link_stats()
        for name in ols:
            assert np.array_equal(ls[name][i], ols[name]), (name, i)
        o.close()
    env.close()
    return tr


def phy_matches_oracle(topo, tables, kw, env, tr, i, snap, policy, n, seed=None):
    """Environment i of a QoT-aware run (tr: the outputs of test_gpu_phy.OUTS, snap: its snapshot) against the oracle of these
    kwargs, bit for bit.  Returns the oracle's trace."""
    o = phy_oracle_from_kwargs(topo, tables, kw, seed=seed)
    ot = o.run(policy, n, reset_on_done=True)
    assert np.array_equal(tr["act_path"][:, i], ot["act_path"]), i
    assert np.array_equal(tr["n_channels"][:, i], ot["n_channels"]), i
    assert np.array_equal(tr["channels"][:, i, :12].astype(np.int32), ot["channels"]), i
    assert np.array_equal(tr["channels_used"][:, i, :12].astype(np.float64), ot["ch_used"]), i
    assert np.array_equal(tr["accepted"][:, i], ot["accepted"]) and np.array_equal(tr["done"][:, i], ot["done"]), i
    assert np.array_equal(tr["request"][:, i, 1], ot["src"]) and np.array_equal(tr["request"][:, i, 3], ot["bit_rate"]), i
    for f in ("arrival", "holding", "number_cuts_total", "rss_total_metric"):
        bad = np.nonzero(tr[f][:, i] != ot[f])[0]
        assert bad.size == 0, (f, i, kw["load"], bad[:4], tr[f][bad[:4], i], ot[f][bad[:4]])
    dc = tr["defrag_counters"][:, i].astype(np.int64)
    assert np.array_equal(dc[:, 1], ot["num_moves_groom"]) and np.array_equal(dc[:, 2], ot["num_defrag_cycle"]), i
    assert np.array_equal(dc[:, 0] / 2 + dc[:, 1], ot["num_moves"]), i
    for name, v in o.counters().items():
        assert snap["counters." + name][i] == v, (name, i)
    assert snap["current_time"][i] == o.current_time() and snap["num_running"][i] == o.num_running(), i
    assert np.array_equal(snap["occupancy"][i], o.available_channels()), i
    assert snap["episode_stats"]["queue_overflow"][i] == 0
    assert env.channel_state(i) == o.channel_state(), i
    o.close()
    return ot


def phy_matches_reference(z, tr, i, n):
    """Environment i against the reference's own trace for the trace's first n steps."""
    assert np.array_equal(tr["act_path"][:n, i], z["act_path"][:n]), i
    assert np.array_equal(tr["channels"][:n, i, :12], z["channels"][:n]), i
    assert np.array_equal(tr["channels_used"][:n, i, :12].astype(np.float64), z["ch_used"][:n]), i
    assert np.array_equal(tr["accepted"][:n, i], z["accepted"][:n]), i
    np.testing.assert_allclose(tr["arrival"][:n, i], z["arrival"][:n], rtol=1e-12)
    assert np.array_equal(tr["number_cuts_total"][:n, i], z["number_cuts_total"][:n]), i
    assert np.array_equal(tr["rss_total_metric"][:n, i], z["rss_total_metric"][:n]), i
    # the all-time counter of the trace, step by step (services_accepted is never reset)
    assert np.array_equal(np.cumsum(tr["accepted"][:n, i].astype(np.int64)), z["services_accepted"][:n]), i
    if "num_moves" in z.files:
        dc = tr["defrag_counters"][:n, i].astype(np.int64)
        assert np.array_equal(dc[:, 0] / 2 + dc[:, 1], z["num_moves"][:n])
        assert np.array_equal(dc[:, 1], z["num_moves_groom"][:n]) and np.array_equal(dc[:, 2], z["num_defrag_cycle"][:n])


# ---------------------------------------------------------------------------------------- against a QoT-aware reference trace
# (fixtures of run_phy_trace, tests/golden/make_golden.py: the float64 shares of a continuous handle included)
PHY_TRACE_COUNTERS = ("services_processed", "services_accepted", "episode_services_processed", "episode_services_accepted",
                      "bit_rate_requested", "bit_rate_provisioned")


def channel_caps(topo, tables, tr, i):
    """ch_cap of the trace: the table's level of every chosen channel on the chosen k-path (the tuple's field 3)."""
    pairs, mod, _ = tables
    rows = topo.pair_table_rows(pairs)
    n = topo.num_nodes
    caps = np.zeros(tr["channels"].shape[:1] + (12,), np.int16)
    for t in range(caps.shape[0]):
        a = int(tr["act_path"][t, i])
        idp = a - 20 if a >= 20 else a
        r = rows[int(tr["request"][t, i, 1]) * n + int(tr["request"][t, i, 2])]
        for q in range(int(tr["n_channels"][t, i])):
            caps[t, q] = mod[r, int(tr["channels"][t, i, q]), idp]
    return caps


def check_trace(topo, tables, tr, i, z, lo, hi):
    """steps lo..hi-1 of env i's per-step outputs against the reference's trace"""
    s = slice(lo, hi)
    assert np.array_equal(tr["request"][:, i, 1], z["src_id"][s]) and np.array_equal(tr["request"][:, i, 2], z["dst_id"][s]), i
    assert np.array_equal(tr["request"][:, i, 3], z["bit_rate"][s]), i
    assert np.array_equal(tr["request"][:, i, 0], z["service_id"][s]), i
    np.testing.assert_allclose(tr["arrival"][:, i], z["arrival"][s], rtol=1e-12, atol=0)
    np.testing.assert_allclose(tr["holding"][:, i], z["holding"][s], rtol=1e-12, atol=0)
    assert np.array_equal(tr["act_path"][:, i], z["act_path"][s]), i
    assert np.array_equal(tr["n_channels"][:, i], z["n_channels"][s]), i
    assert np.array_equal(tr["channels"][:, i, :12], z["channels"][s]), i
    if "channels_used_f64" in tr:   # a continuous handle: the float64 shares, bit for bit
        for f, g in (("channels_used_f64", "ch_used"), ("channels_free_f64", "ch_free")):
            bad = np.argwhere(tr[f][:, i, :12] != z[g][s])
            assert bad.size == 0, (f, i, bad[:3], tr[f][:, i, :12][tuple(bad[:3].T)], z[g][s][tuple(bad[:3].T)])
    else:   # discrete bit rates: whole 100 Gb/s units (the handle has no output for the free share)
        assert np.array_equal(tr["channels_used"][:, i, :12].astype(np.float64), z["ch_used"][s]), i
    if "defrag_counters" in tr:
        dc = tr["defrag_counters"][:, i].astype(np.int64)
        assert np.array_equal(dc[:, 0] / 2 + dc[:, 1], z["num_moves"][s]), i
        assert np.array_equal(dc[:, 1], z["num_moves_groom"][s]) and np.array_equal(dc[:, 2], z["num_defrag_cycle"][s]), i
    assert np.array_equal(channel_caps(topo, tables, tr, i)[:, :12], z["ch_cap"][s]), i
    assert np.array_equal(tr["accepted"][:, i], z["accepted"][s]) and np.array_equal(tr["done"][:, i], z["done"][s]), i
    virtual = (tr["act_path"][:, i] >= 20) & (tr["accepted"][:, i] == 1)
    assert np.array_equal(virtual, z["virtual"][s]), i
    assert np.array_equal(tr["number_cuts_total"][:, i], z["number_cuts_total"][s]), i
    assert np.array_equal(tr["rss_total_metric"][:, i], z["rss_total_metric"][s]), i


def check_state(env, i, z, t):
    """env i after step t (0-based) against the reference's record of that step"""
    cnt = env.counters()
    for name in PHY_TRACE_COUNTERS:
        assert cnt[name][i] == z[name][t], (name, i, t)
    np.testing.assert_allclose(env.current_time()[i], z["current_time"][t], rtol=1e-12, atol=0)
    assert env.num_running()[i] == z["n_running"][t], i
    if not z["done"][t]:   # (the info ratios of a step that ended an episode are gone after the reset)
        info, st = env.info(), env.episode_stats()
        assert info["total_path_length"][i] == z["total_path_length"][t], i
        np.testing.assert_allclose(info["avrage_gsnr"][i], z["avrage_gsnr"][t], rtol=1e-15)
        assert info["average_path_index"][i] == z["average_path_index"][t], i
        assert info["path_index"][i] == z["path_index"][t] and info["physical_paths"][i] == z["physical_paths"][t], i
        # NumPy-2 uint8 wrap of the reference's accumulator: reproduced on the host (as tests/test_gpu_phy.py)
        assert (st["total_modulation_level"][i] % 256) / (st["channels_accepted"][i] + 1) == z["average_mod_level"][t], i


# ---------------------------------------------------------------------------------------- instantiation names
def kernel_name(family, W_or_S, stats, *, hbmq=False, defer=False, traffic=False, trace=False, ff=False, gn=False):
    """The name last_kernel() starts with, as orlg_kernel_name (csrc/orlg_variants.h) spells it: trailing `false` flags left out.
    family: "wave" (ff: the first-fit kernel; defer, gn) or "group" (hbmq, defer, traffic, trace).  W_or_S: words per link (up to 8)
    or a slot count (seven words of slots run on the eight-word layout).  stats: a statistics level's name or number."""
    W = W_or_S if W_or_S <= 8 else (W_or_S + 63) // 64
    W = 8 if W == 7 else W
    level = STATS_LEVELS.index(stats) if isinstance(stats, str) else stats
    if family == "group":
        assert not (ff or gn)
        name, flags = "orlg_rmsa_group_kernel", [hbmq, defer, traffic, trace]
    else:
        assert family == "wave" and not (hbmq or traffic or trace)
        name, flags = "orlg_rmsa_kernel_ff" if ff else "orlg_rmsa_kernel", [defer, gn]
    while flags and not flags[-1]:
        flags.pop()
    return f"{name}<{W},{level}" + "".join(",true" if f else ",false" for f in flags) + ">"


# ---------------------------------------------------------------------------------------- external actions
def external_actions(topo, S, n, batch, seed=123, kind="third_low"):
    """Random external actions [n, batch, 2] int32: paths 0 .. K (K: out of range), slots 0 .. S (S: out of range).
    kind "third_low": a third of the steps aim low (slot // 8), where first-fit neighbours would be -- windows at slot 0, occupied
    ones; "quarter": every slot // 4; "paths": the paths alone, [n, batch] (path_ff_external); "high_paths" (k_paths > 8): as
    "third_low", and five actions of eight have their path redrawn from 8 .. K - 1 -- more than half aim at a path the step
    kernels lay out W lanes apart -- the others keep paths 0 .. K and the slots keep S: out of range in either component."""
    rng = np.random.default_rng(seed)
    paths = rng.integers(0, topo.k_paths + 1, (n, batch))
    if kind == "paths":
        return paths.astype(np.int32)
    slots = rng.integers(0, S + 1, (n, batch))
    a = np.stack([paths, slots // 4 if kind == "quarter" else slots], axis=-1).astype(np.int32)
    if kind in ("third_low", "high_paths"):
        a[::3, :, 1] //= 8
    if kind == "high_paths":
        assert topo.k_paths > 8
        high = rng.integers(8, topo.k_paths, (n, batch))
        a[..., 0] = np.where(rng.random((n, batch)) < 0.625, high, a[..., 0])
    return a


# ---------------------------------------------------------------------------------------- the group kernel's launch plan
KINDS = ("PLAIN", "HBMQ", "DEFER")   # enum OrlgGroupKind
SP, SAP, LLP = 0, 1, 2   # ORLG_POLICY_*
OUT_ACCEPTED, OUT_LINK_COMPACT, OUT_LINK_UTIL = 1 << 2, 1 << 10, 1 << 11   # 1 << ORLG_OUT_*
NSFNET = dict(NW=110, E=22, lint_stride=24)
SHARED = {0: 10448, 2: 14320}
MT_BYTES = 2496   # the workgroup's MT19937 staging buffer; its lock word takes 16 more


@functools.lru_cache(maxsize=None)
def _fields(macro):
    from optical_rl_gym_amd import build
    text = open(os.path.join(build.CSRC, "orlg_api.hip")).read()
    body = re.search(r"#define %s\(X\)((?:[^\n]*\\\n)*[^\n]*)\n" % macro, text).group(1)
    return re.findall(r"X\((?:\w+, )?(\w+)\)", body)


def group_plan(args):
    """orlg_debug_group_plan on inputs by field name: ({kind name: layout}, plan) -- both dicts by field name"""
    from optical_rl_gym_amd import _lib
    IN, LAYOUT, PLAN = _fields("ORLG_GROUP_PLAN_IN"), _fields("ORLG_GROUP_LAYOUT_OUT"), _fields("ORLG_GROUP_PLAN_OUT")
    assert sorted(args) == sorted(IN)
    n_out = 3 * len(LAYOUT) + len(PLAN)
    vin, out = (C.c_int32 * len(IN))(*[args[f] for f in IN]), (C.c_int32 * n_out)()
    f = _lib.load().orlg_debug_group_plan
    f.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.c_int32]
    assert f(vin, len(IN), out, n_out) == n_out
    layouts = {k: dict(zip(LAYOUT, out[i * len(LAYOUT):(i + 1) * len(LAYOUT)])) for i, k in enumerate(KINDS)}
    p = dict(zip(PLAN, out[3 * len(LAYOUT):]))
    p["kind"] = KINDS[p["kind"]]
    return layouts, p


def plan(Q=128, stats=2, B=8, n_steps=1000, policy=SAP, out_mask=0, br_width=0, num_cu=256, resident=256, **overrides):
    """group_plan on NSFNET with 320 slots"""
    args = dict(NSFNET, Q=Q, stats_level=stats, shared_bytes=SHARED[stats], B=B, n_steps=n_steps, policy=policy, out_mask=out_mask,
                br_width=br_width, no_defer=0, no_chunks=0, no_lean=0, wpb=0, chunks=0, num_cu=num_cu, resident=resident)
    assert set(overrides) <= {"no_defer", "no_chunks", "no_lean", "wpb", "chunks"}
    args.update(overrides)
    layouts, p = group_plan(args)
    # what holds for every plan: the workgroup's LDS bytes, and how far the launch moves ticket_base
    chosen, n_quads = layouts[p["kind"]], (B + 3) // 4
    assert 1 <= p["wpb"] <= chosen["wpb_max"]
    assert p["lds_bytes"] == SHARED[stats] + MT_BYTES + 16 + p["wpb"] * chosen["wave_bytes"]
    assert p["ticket_stride"] == (1 if n_steps <= 16 else 0)
    assert p["nblocks"] == min(-(-n_quads // p["wpb"]), resident)
    if p["ticket_stride"]:
        assert p["ticket_advance"] == 0
    elif p["n_chunks"] == 1:
        assert p["ticket_advance"] == n_quads
    else:
        assert p["ticket_advance"] == n_quads * p["n_chunks"] + p["nblocks"] * p["wpb"]
    return layouts, p


# ---------------------------------------------------------------------------------------- valid-action masks
def unpack(words, n):
    """[..., W] uint64 -> [..., n] uint8, bit s of word w = element 64 w + s"""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1, bitorder="little")[..., :n]


def expected_masks(o, K, J, S, reject):
    """The three masks of one oracle environment, from the reference's own queries."""
    deep = np.zeros(K * J + reject, np.uint8)
    ff = np.zeros(K + reject, np.uint8)
    slots = np.zeros((K, S), np.uint8)
    for p in range(K):
        n = o.number_slots(p)
        starts, _ = o.available_blocks(p)
        for b in range(J):
            deep[p * J + b] = b < len(starts)                                   # deeprmsa_env.py:52-54
        slots[p] = [o.is_path_free(p, s, n) for s in range(S)]                 # rmsa_env.py:233-260
        ff[p] = any(slots[p, s] for s in range(0, S - n))                      # rmsa_env.py:974-1008, the bound exclusive
    if reject:
        deep[K * J] = ff[K] = 1
    return deep, ff, slots


def check_against_oracles(env, oracles, where):
    K, J, S, r = env.k_paths, env.j, env.num_spectrum_resources, env.reject_action
    deep, ff, words = env.action_masks("deeprmsa"), env.action_masks("path_ff"), env.action_masks("slots")
    assert deep.shape == (len(oracles), K * J + r) and ff.shape == (len(oracles), K + r)
    assert words.shape == (len(oracles), K, env.words_per_link) and words.dtype == np.uint64
    bits = unpack(words, 64 * env.words_per_link)
    assert not bits[..., S:].any(), where                                        # bits at and beyond S are 0
    for i, o in enumerate(oracles):
        e_deep, e_ff, e_slots = expected_masks(o, K, J, S, r)
        assert np.array_equal(deep[i], e_deep), (where, i, deep[i], e_deep)
        assert np.array_equal(ff[i], e_ff), (where, i, ff[i], e_ff)
        assert np.array_equal(bits[i, :, :S], e_slots), (where, i, np.nonzero(bits[i, :, :S] != e_slots))
    return deep, ff, bits[..., :S]


# ---------------------------------------------------------------------------------------- synthetic grids
def write_topology(tmp_path, name, num_nodes, edges):
    path = tmp_path / (name + ".txt")
    with open(path, "w") as f:
        f.write(f"{num_nodes}\n{len(edges)}\n")
        for a, b, length in edges:
            f.write(f"{a} {b} {length}\n")
    return str(path)


def grid_edges(rows, cols, rng):
    edges = []
    node = lambda r, c: r * cols + c + 1
    for r in range(rows):
        for c in range(cols):
            if c + 1 < cols:
                edges.append((node(r, c), node(r, c + 1), int(rng.integers(60, 400))))
            if r + 1 < rows:
                edges.append((node(r, c), node(r + 1, c), int(rng.integers(60, 400))))
            if r + 1 < rows and c + 1 < cols and (r + c) % 2 == 0:
                edges.append((node(r, c), node(r + 1, c + 1), int(rng.integers(80, 500))))
    return edges


# ---------------------------------------------------------------------------------------- more than eight candidate paths
# The shapes of test_many_paths.py (which pins on the CPU what they exercise) and test_gpu_many_paths.py: grid_edges(rows, cols,
# default_rng(5)) with k candidate paths per pair, S slots = W words per link, E links, load = 0.5 S E / 40 rounded (3x3: 8, where
# llp_ff takes path 8 most often -- DESIGN 4), the device policy of the step-parity cases.  W = 8 cannot have K > 8 (8 x 9 > 64 lanes).
MANY_PATHS = {
    "g3x3_k9_s64": dict(rows=3, cols=3, k=9, S=64, W=1, E=14, load=8, policy="sap_ff"),
    "g4x4_k32_s100": dict(rows=4, cols=4, k=32, S=100, W=2, E=29, load=36, policy="llp_ff"),
    "g4x4_k21_s192": dict(rows=4, cols=4, k=21, S=192, W=3, E=29, load=70, policy="sap_ff"),
    "g4x4_k16_s200": dict(rows=4, cols=4, k=16, S=200, W=4, E=29, load=72, policy="sap_ff"),
    "g4x4_k12_s320": dict(rows=4, cols=4, k=12, S=320, W=5, E=29, load=116, policy="llp_ff"),
    "g3x4_k10_s384": dict(rows=3, cols=4, k=10, S=384, W=6, E=20, load=96, policy="llp_ff"),
}
MANY_PATHS_SEED = 3   # environment i of a batch: seed 3 + i
_many_paths = {}


def many_paths_topology(name, tmp_path):
    """The topology of a MANY_PATHS shape, frozen once per process (the link list is written under the first caller's tmp_path)."""
    if name not in _many_paths:
        from optical_rl_gym_amd.topology_io import topology_from_txt
        c = MANY_PATHS[name]
        edges = grid_edges(c["rows"], c["cols"], np.random.default_rng(5))
        _many_paths[name] = topology_from_txt(write_topology(tmp_path, name, c["rows"] * c["cols"], edges), name, k_paths=c["k"])
    return _many_paths[name]


def many_paths_kwargs(name, **over):
    """BatchedRMSAEnv / oracle keyword arguments of a MANY_PATHS shape (without the topology)."""
    c = MANY_PATHS[name]
    return dict(dict(num_spectrum_resources=c["S"], load=c["load"], mean_service_holding_time=25, episode_length=200,
                     seed=MANY_PATHS_SEED), **over)
