"""Request traces without a device: the rules of RequestTrace (the library's own, include/orlg.h orlg_trace), the layouts it
accepts, peak_offered() against a brute-force count, the golden request streams as traces, and the new C symbols."""
import glob
import os
import subprocess

import numpy as np
import pytest
from conftest import GOLDEN, load_golden, load_topology

from optical_rl_gym_amd import RequestTrace, TraceError
from optical_rl_gym_amd import _lib
from optical_rl_gym_amd.batched import DEFAULT_BIT_RATES


def good(n=6, B=3):
    rng = np.random.default_rng(5)
    arrival = np.cumsum(rng.exponential(1.0, (n, B)), axis=0)
    holding = rng.exponential(3.0, (n, B))
    src = rng.integers(0, 5, (n, B)).astype(np.int32)
    dst = (src + 1 + rng.integers(0, 4, (n, B))).astype(np.int32) % 5
    rate = rng.choice(np.array(DEFAULT_BIT_RATES, np.int32), (n, B))
    return dict(arrival=arrival, holding=holding, src=src, dst=dst, bit_rate=rate)


def build(d, **kw):
    return RequestTrace(d["arrival"], d["holding"], d["src"], d["dst"], d["bit_rate"], **kw)


@pytest.mark.parametrize("field, step, env, value, what", [
    ("arrival", 3, 1, -1.0, "arrival"),           # decreasing (and negative at index 0 would be "not a finite time")
    ("arrival", 2, 2, np.nan, "arrival"),
    ("arrival", 4, 0, np.inf, "arrival"),
    ("holding", 1, 1, -0.5, "holding"),
    ("holding", 5, 2, np.nan, "holding"),
    ("dst", 2, 0, None, "source and destination"),
    ("src", 4, 1, -3, "node pair"),
])
def test_every_rule_names_environment_and_index(field, step, env, value, what):
    d = good()
    if value is None:
        d["dst"][step, env] = d["src"][step, env]
    elif field == "arrival" and value == -1.0:
        d["arrival"][step, env] = d["arrival"][step - 1, env] - 1e-9
    else:
        d[field][step, env] = value
    with pytest.raises(TraceError) as ei:
        build(d)
    assert (ei.value.env, ei.value.index) == (env, step), str(ei.value)
    assert what in str(ei.value) and f"environment {env}, request {step}" in str(ei.value)


def test_rules_that_need_the_handle():
    d = good()
    t = build(d)
    t.validate(num_nodes=5, bit_rates=DEFAULT_BIT_RATES)
    d["src"][3, 2] = 9
    d["dst"][3, 2] = 1
    with pytest.raises(TraceError) as ei:
        build(d).validate(num_nodes=5)
    assert (ei.value.env, ei.value.index) == (2, 3)
    d = good()
    d["bit_rate"][4, 1] = 123
    with pytest.raises(TraceError) as ei:
        build(d).validate(num_nodes=5, bit_rates=DEFAULT_BIT_RATES)
    assert (ei.value.env, ei.value.index) == (1, 4) and "bit rate 123" in str(ei.value)
    d["bit_rate"][:] = 50
    d["bit_rate"][2, 0] = 101
    build(d).validate(bit_rate_bounds=(25, 101))
    with pytest.raises(TraceError) as ei:
        build(d).validate(bit_rate_bounds=(25, 100))
    assert (ei.value.env, ei.value.index) == (0, 2) and "outside the bounds" in str(ei.value)


def test_length_and_shapes():
    d = good(n=1)
    with pytest.raises(TraceError, match="at least 2"):
        build(d)
    d = good()
    d["holding"] = d["holding"][:-1]
    with pytest.raises(TraceError, match="shape"):
        build(d)
    d = good()
    with pytest.raises(TraceError, match="batch_size"):
        build(d, batch_size=7)
    d["src"] = d["src"].astype(np.float64)
    with pytest.raises(TypeError):
        build(d)


def test_step_major_env_major_and_broadcast_give_the_same_object():
    d = good(n=6, B=3)
    a = build(d)
    b = build({k: v.T for k, v in d.items()}, layout="env")
    c = build({k: v.T for k, v in d.items()}, batch_size=3)       # only the env-major reading fits
    assert a == b and a == c and a.length == 6 and a.batch_size == 3
    assert a.arrival.shape == (3, 6) and a.arrival.flags["C_CONTIGUOUS"] and a.src.dtype == np.int32
    one = build({k: v[:, 0] for k, v in d.items()}, batch_size=4)
    assert one.batch_size == 4 and all(np.array_equal(one.arrival[i], d["arrival"][:, 0]) for i in range(4))
    assert one == build({k: v[:, 0] for k, v in d.items()}).for_batch(4)
    d2 = good(n=6, B=3)
    d2["holding"][0, 0] += 1.0
    assert a != build(d2)


def brute_force_peak(arrival, holding):
    """The most requests j with arrival[j] <= t <= arrival[j] + holding[j] over all t: the maximum is taken at an arrival."""
    best = 0
    for i in range(arrival.shape[0]):
        a, e = arrival[i], arrival[i] + holding[i]
        for t in a:
            best = max(best, int(np.sum((a <= t) & (t <= e))))
    return best


@pytest.mark.parametrize("seed", range(8))
def test_peak_offered_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    n, B = int(rng.integers(2, 40)), int(rng.integers(1, 5))
    # integer-valued times make ties (an end exactly at an arrival counts: the interval is closed)
    arrival = np.cumsum(rng.integers(0, 3, (B, n)), axis=1).astype(np.float64)
    holding = rng.integers(0, 9, (B, n)).astype(np.float64)
    t = RequestTrace(arrival, holding, np.zeros((B, n), np.int32), np.ones((B, n), np.int32),
                     np.full((B, n), 100, np.int32), layout="env")
    assert t.peak_offered() == brute_force_peak(arrival, holding)


GOLDEN_TRACES = sorted(os.path.basename(p)[:-4] for pat in ("rmsa_*.npz", "phy_*.npz", "cont_*.npz")
                       for p in glob.glob(os.path.join(GOLDEN, pat)))


@pytest.mark.parametrize("case", GOLDEN_TRACES)
def test_golden_streams_are_valid_traces(case):
    z, meta = load_golden(case)
    topo = load_topology(meta["topology"])
    t = RequestTrace.from_golden(z)
    assert t.length == meta["steps"] and t.batch_size == 1
    kw = meta["env_kwargs"]
    if kw.get("bit_rate_selection") == "continuous":
        lo, hi = int(kw.get("bit_rate_lower_bound", 25)), int(kw.get("bit_rate_higher_bound", 100))
        t.validate(num_nodes=topo.num_nodes, bit_rate_bounds=(lo, hi))
    elif "bit_rates" in kw:
        t.validate(num_nodes=topo.num_nodes, bit_rates=kw["bit_rates"])
    else:
        t.validate(num_nodes=topo.num_nodes)
    assert t.peak_offered() >= 1


def test_trace_excludes_generated_traffic_arguments():
    from optical_rl_gym_amd import BatchedDeepRMSAEnv, BatchedPhyRMSAEnv, BatchedRMSAEnv, make
    t = build(good())
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    for extra in (dict(load=50), dict(mean_service_holding_time=25.0), dict(seed=3), dict(seeds=[1, 2, 3])):
        with pytest.raises(ValueError, match="trace="):
            BatchedRMSAEnv(topo, 3, trace=t, **extra)
        with pytest.raises(ValueError, match="trace="):
            BatchedPhyRMSAEnv(topo, 3, modulation_level=None, connections_detail=None, gsnr=None, trace=t, **extra)
    with pytest.raises(ValueError, match="trace="):
        BatchedDeepRMSAEnv(topo, 3, trace=t, mean_service_inter_arrival_time=0.1)
    with pytest.raises(ValueError, match="trace="):
        make("RMSA-v0", topology=topo, trace=t, load=10)
    with pytest.raises(TypeError):
        BatchedRMSAEnv(topo, 3, trace="a file name")


@pytest.mark.parametrize("field, step, env, value, what", [
    ("arrival", 3, 1, "decreasing", "before its predecessor"),
    ("arrival", 2, 2, np.nan, "arrival"),
    ("arrival", 4, 0, np.inf, "arrival"),
    ("holding", 1, 1, -0.5, "holding"),
    ("dst", 2, 0, "same", "source and destination"),
    ("src", 4, 1, 14, "node pair"),
    ("bit_rate", 5, 2, 123, "bit rate 123"),
])
@pytest.mark.parametrize("kind", ["rmsa", "phy"])
def test_the_library_checks_the_same_rules(monkeypatch, kind, field, step, env, value, what):
    """orlg_trace_check (the C side) refuses the same entries and names environment and index in orlg_last_error(); it runs
    before the library looks for a device, so this needs none.  The NumPy rules are switched off to reach it."""
    from conftest import load_phy_tables
    from optical_rl_gym_amd import BatchedPhyRMSAEnv, BatchedRMSAEnv, OrlgError
    d = good()
    if kind == "phy":
        d["bit_rate"][:] = 300
    if value == "same":
        d["dst"][step, env] = d["src"][step, env]
    elif value == "decreasing":
        d["arrival"][step, env] = d["arrival"][step - 1, env] - 1e-9
    else:
        d[field][step, env] = value
    monkeypatch.setattr(RequestTrace, "validate", lambda self, **kw: self)
    t = build(d)
    with pytest.raises(OrlgError) as ei:
        if kind == "rmsa":
            BatchedRMSAEnv(load_topology("nsfnet_chen_5-paths_6-modulations"), 3, trace=t)
        else:
            pairs, mod, gsnr = load_phy_tables("us14_k3")
            BatchedPhyRMSAEnv(load_topology("us14_3-paths_6-modulations"), 3, modulation_level=mod, connections_detail=pairs, gsnr=gsnr,
                              trace=t)
    assert ei.value.code == -1
    assert f"environment {env}, request {step}" in str(ei.value) and what in str(ei.value), str(ei.value)


def test_the_library_refuses_a_short_trace(monkeypatch):
    from optical_rl_gym_amd import BatchedRMSAEnv, OrlgError
    monkeypatch.setattr(RequestTrace, "validate", lambda self, **kw: self)
    with pytest.raises(OrlgError, match="at least 2"):
        BatchedRMSAEnv(load_topology("nsfnet_chen_5-paths_6-modulations"), 3, trace=build(good(n=1)))


def test_new_symbols_in_a_fresh_library(tmp_path):
    new = ["orlg_create_trace", "orlg_phy_create_trace", "orlg_trace_length", "orlg_trace_position",
           "orlg_phy_trace_length", "orlg_phy_trace_position"]
    assert set(new) <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.load()
    assert L.orlg_abi_version() == 3
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(new) <= names
    # (the header declares them)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "orlg.h")).read()
    for s in new:
        assert s + "(" in header
