"""The group kernel's LEAN body: a deferred launch (16 steps or more, full statistics) of ``sp_ff`` / ``sap_ff`` with no
per-step output and discrete bit rates runs a body from which the other policies, the outputs and the continuous refill are
compiled out.  It must perform the same operations on the same values as the full body: held byte for byte against the full
body (``ORLG_NO_LEAN``, read at every launch), against the wave-per-environment kernel, and against the C oracle for the first,
a middle and the last environment.  Launches that do not qualify must say ``body=full`` and equal the wave kernel.

B = 5: the last quad has three idle rows; B = 64: several quads.  S = 64, 100, 320: 1, 2 and 5 words per link.  The episode
(11 services) is shorter than every launch, so an auto-reset falls inside each of them."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import load_topology, oracle_env_from_kwargs

pytestmark = pytest.mark.gpu

NSF, US14 = "nsfnet_chen_5-paths_6-modulations", "us14_3-paths_6-modulations"
SEED = 31
LAUNCHES = (16, 100, 300)
ENV_VARS = ("ORLG_NO_LEAN", "ORLG_GROUP_CHUNKS", "ORLG_NO_DEFER", "ORLG_NO_CHUNKS")
OUTS = ("act_path", "act_slot", "accepted", "reward", "done", "request", "arrival", "holding", "network_compactness",
        "network_compactness_difference")
SHAPES = [(name, S, B) for name in (NSF, US14) for S in (64, 100, 320) for B in (5, 64)]


def env_kwargs(S, load=300):
    return dict(num_spectrum_resources=S, load=load, mean_service_holding_time=25, episode_length=11, seed=SEED)


def snapshot(env):
    snap = dict(state=env.save_state(), occ=env.occupancy_words(), episodes=env.episodes_done(), pending=env.requests())
    for prefix, d in (("c", env.counters()), ("l", env.link_stats()), ("g", env.graph_stats()), ("h", env.bit_rate_hist())):
        snap.update({f"{prefix}.{k}": v for k, v in d.items()})
    return {k: np.array(v, copy=True) for k, v in snap.items()}


def same_bytes(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


def drive(make, launches, env_vars=None):
    """launches: (policy, steps, outputs, actions) each; returns the per-launch outputs, the launch descriptions, the state."""
    old = {k: os.environ.pop(k, None) for k in ENV_VARS}
    os.environ.update(env_vars or {})
    try:
        env = make()
        outs, said = [], []
        for policy, n, outputs, actions in launches:
            outs.append(env.run(policy, n, outputs=outputs, auto_reset=True, actions=actions))
            said.append(env.last_kernel())
        snap = snapshot(env)
        env.close()
        return dict(outs=outs, said=said, snap=snap)
    finally:
        for k in ENV_VARS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in old.items() if v is not None})


def rmsa(name, S, B, kernel, **kw):
    from optical_rl_gym_amd import BatchedRMSAEnv
    return lambda: BatchedRMSAEnv(load_topology(name), B, step_kernel=kernel, stats_level="full", **dict(env_kwargs(S), **kw))


def bodies(run):
    return [s.split("body=")[1].split()[0] if "body=" in s else None for s in run["said"]]


@functools.lru_cache(maxsize=None)
def heuristic_runs(name, S, B, policy):
    """One handle stepped through LAUNCHES: lean and full body, whole-launch tickets and 7 forced chunks; the wave kernel."""
    launches = [(policy, n, (), None) for n in LAUNCHES]
    grp = rmsa(name, S, B, "group")
    return dict(lean=drive(grp, launches), full=drive(grp, launches, {"ORLG_NO_LEAN": "1"}),
                lean7=drive(grp, launches, {"ORLG_GROUP_CHUNKS": "7"}),
                full7=drive(grp, launches, {"ORLG_GROUP_CHUNKS": "7", "ORLG_NO_LEAN": "1"}),
                wave=drive(rmsa(name, S, B, "wave"), launches))


@pytest.fixture()
def device_log_in_oracle():
    import oracle as orc
    from optical_rl_gym_amd import _lib
    orc.set_log_fn(C.cast(_lib.load().orlg_host_log, C.c_void_p).value)
    yield
    orc.set_log_fn(None)


@pytest.mark.parametrize("policy", ["sp_ff", "sap_ff"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][:4]}-{s[1]}-B{s[2]}")
def test_lean_equals_full_byte_for_byte(shape, policy):
    name, S, B = shape
    W = (S + 63) // 64
    r = heuristic_runs(name, S, B, policy)
    for lean, full, chunks in (("lean", "full", None), ("lean7", "full7", "7")):
        assert bodies(r[lean]) == ["lean"] * 3 and bodies(r[full]) == ["full"] * 3, (r[lean]["said"], r[full]["said"])
        for said in r[lean]["said"] + r[full]["said"]:
            assert said.split(" ")[0] == f"orlg_rmsa_group_kernel<{W},2,false,true>", said
        if chunks:   # (a launch of 16 steps strides over its quads: no tickets, so no chunks)
            assert all(f"chunks={chunks}" in s for run in (r[lean], r[full]) for s in run["said"][1:]), r[lean]["said"]
        same_bytes(r[lean]["snap"], r[full]["snap"], (lean, full))
    same_bytes(r["lean"]["snap"], r["lean7"]["snap"], "chunks")
    assert (r["lean"]["snap"]["episodes"] >= sum(LAUNCHES) // 11 - 1).all()   # auto-resets inside every launch


@pytest.mark.parametrize("policy", ["sp_ff", "sap_ff"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][:4]}-{s[1]}-B{s[2]}")
def test_lean_against_wave_kernel_and_oracle(shape, policy, device_log_in_oracle):
    name, S, B = shape
    r = heuristic_runs(name, S, B, policy)
    for k in ("lean", "lean7"):
        same_bytes(r[k]["snap"], r["wave"]["snap"], k)
    snap = r["lean"]["snap"]
    topo = load_topology(name)
    bits = np.unpackbits(snap["occ"].view(np.uint8), axis=-1, bitorder="little").reshape(B, topo.num_links, -1)[:, :, :S]
    assert snap["c.services_accepted"].sum() > 0
    if S <= 100:   # (at load 300 a narrow spectrum fills within the run: blocked requests among the steps)
        assert (snap["c.services_accepted"] < snap["c.services_processed"]).any()
    for i in (0, B // 2, B - 1):
        o = oracle_env_from_kwargs(topo, env_kwargs(S), seed=SEED + i)
        o.run(policy, sum(LAUNCHES), reset_on_done=True)
        assert np.array_equal(bits[i], o.available_slots()), i
        for k, v in o.counters().items():
            assert snap["c." + k][i] == v, (k, i)
        for k, v in o.link_stats().items():
            assert np.array_equal(snap["l." + k][i], v), (k, i)
        o.close()


def external_actions(topo, S, n, B, kind):
    rng = np.random.default_rng(5)
    if kind == "external":
        return np.stack([rng.integers(0, topo.k_paths + 1, (n, B)), rng.integers(0, S + 1, (n, B)) // 4], axis=-1).astype(np.int32)
    return rng.integers(0, topo.k_paths + 1, (n, B)).astype(np.int32)


# launches that must not qualify: (id, policy, steps per launch, launches, outputs, handle keywords)
FULL_ONLY = [
    ("done-alone", "sap_ff", 100, 2, ("done",), {}),
    ("outputs", "sp_ff", 100, 2, OUTS, {}),
    ("llp", "llp_ff", 100, 2, (), {}),
    ("deeprmsa", "deeprmsa_sap_ff", 100, 2, (), {}),
    ("external", "external", 1, 40, (), {}),
    ("path-external", "path_ff_external", 1, 40, (), {}),
    ("continuous", "sap_ff", 100, 2, (), dict(bit_rate_selection="continuous", load=100)),
]


@pytest.mark.parametrize("case", FULL_ONLY, ids=lambda c: c[0])
@pytest.mark.parametrize("shape", [(NSF, 320, 5), (US14, 100, 64)], ids=lambda s: f"{s[0][:4]}-{s[1]}-B{s[2]}")
def test_launches_that_do_not_qualify(shape, case):
    name, S, B = shape
    _, policy, n, count, outputs, kw = case
    acts = external_actions(load_topology(name), S, count, B, policy) if "external" in policy else [None] * count
    # (the state of a launch with outputs is compared on launches without: the final lean-eligible shape must stay full here)
    launches = [(policy, n, outputs, acts[t]) for t in range(count)]
    grp = drive(rmsa(name, S, B, "group", **kw), launches)
    wav = drive(rmsa(name, S, B, "wave", **kw), [(p, n_, OUTS if not outputs else outputs, a) for p, n_, _, a in launches])
    assert bodies(grp) == ["full"] * count, grp["said"]
    same_bytes(grp["snap"], wav["snap"], case[0])
    for g, w in zip(grp["outs"], wav["outs"]):
        for k in g:
            assert np.array_equal(g[k], w[k]), (case[0], k)
    if outputs:
        assert sum(int(o["done"].sum()) for o in grp["outs"]) > 0
    # the same launches with outputs, so that the group kernel's path, slot and acceptance are held step by step as well
    if not outputs:
        grp_o = drive(rmsa(name, S, B, "group", **kw), [(p, n_, OUTS, a) for p, n_, _, a in launches])
        assert bodies(grp_o) == ["full"] * count, grp_o["said"]
        same_bytes(grp_o["snap"], wav["snap"], case[0])
        for g, w in zip(grp_o["outs"], wav["outs"]):
            for k in OUTS:
                assert np.array_equal(g[k], w[k]), (case[0], k)


@pytest.mark.parametrize("shape", [(NSF, 320, 5), (US14, 100, 64)], ids=lambda s: f"{s[0][:4]}-{s[1]}-B{s[2]}")
def test_a_handle_that_alternates(shape):
    name, S, B = shape
    launches = [("sap_ff", 100, (), None), ("sap_ff", 100, OUTS, None), ("sap_ff", 100, (), None)]
    alt = drive(rmsa(name, S, B, "group"), launches)
    full = drive(rmsa(name, S, B, "group"), launches, {"ORLG_NO_LEAN": "1"})
    assert bodies(alt) == ["lean", "full", "lean"] and bodies(full) == ["full"] * 3, (alt["said"], full["said"])
    same_bytes(alt["snap"], full["snap"], "state")
    for k in OUTS:
        assert alt["outs"][1][k].tobytes() == full["outs"][1][k].tobytes(), k


@pytest.mark.parametrize("kind", ["traffic", "trace"])
def test_lean_on_traffic_and_trace_handles(kind):
    """The other two DEFER instantiations (per-environment rates; a replayed request trace), S = 320, B = 64."""
    from optical_rl_gym_amd import record_trace
    B, S = 64, 320
    launches = [("sap_ff", n, (), None) for n in LAUNCHES]
    if kind == "traffic":
        make = rmsa(NSF, S, B, "group", load=np.linspace(40.0, 400.0, B))
        suffix = ",true>"
    else:
        gen = rmsa(NSF, S, B, "group")()
        trace = record_trace(gen, "sap_ff", sum(LAUNCHES), auto_reset=True)
        gen.close()
        from optical_rl_gym_amd import BatchedRMSAEnv
        make = lambda: BatchedRMSAEnv(load_topology(NSF), B, trace=trace, step_kernel="group", stats_level="full",
                                      num_spectrum_resources=S, episode_length=11)
        suffix = ",false,true>"
    for env_vars in ({}, {"ORLG_GROUP_CHUNKS": "7"}):
        lean = drive(make, launches, env_vars)
        full = drive(make, launches, dict(env_vars, ORLG_NO_LEAN="1"))
        assert bodies(lean) == ["lean"] * 3 and bodies(full) == ["full"] * 3, (lean["said"], full["said"])
        assert all(s.split(" ")[0] == "orlg_rmsa_group_kernel<5,2,false,true" + suffix for s in lean["said"] + full["said"]), lean["said"]
        same_bytes(lean["snap"], full["snap"], (kind, env_vars))
    assert lean["snap"]["c.services_accepted"].sum() > 0
