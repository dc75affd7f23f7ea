"""Where the deferred step loops wait for vector memory: the cold blocks of the DEFER instantiations -- the
link replays after a provision and inside the release loop, the lean body's graph replay, the ring refill and the ring reload
behind it -- end with an explicit drain, and the hot step waits once, between the policy and its first store.  A wait that is
missing shows where those blocks run often and next to each other, so the shapes here force that; every result must stay
what it was.

  many link replays    a ring of four nodes (4 links, 2 candidate paths): the busiest link logs its 40 entries within about 60
                       steps (under sap_ff every link does within about 100), so a launch of 1000 steps works the logs off
                       every few tens of steps.  S = 64 and 320 (one and five
                       words), B = 8 and B = 5 (idle rows in the last quad), launches of 17, 300 and 1000 steps, sap_ff and sp_ff,
                       the lean body (no output) and the full one (one per-step output).  Against the oracle for every
                       environment -- decisions where the launch has an output, counters, link and graph statistics -- and against
                       the wave-per-environment kernel byte for byte, saved state included.
  replay inside the    a request trace on that ring: 44 .. 72 services on one link, then a gap of 30 holding times -- the step
  release loop         that ends the gap releases them all, the link's log fills inside the release loop and is replayed there.
                       1, 2 and 4 chunks, both bodies.  The oracle generates its own traffic and cannot follow a trace: the
                       yardsticks are the wave kernel byte for byte, in its deferred form and (ORLG_NO_DEFER) in the form that
                       keeps no log at all, which the rest of the suite holds to the oracle; and what the trace itself says the
                       counters must be.
  graph replay and     NSFNET, S = 320, B = 64, 200 steps from a freshly seeded batch at an acceptance near 1: a row's sixteenth
  refill in one step   logged provision (the lean body's graph replay) and its ring refill fall close together -- the stagger of
                       the first refill gives every offset within 56 environments.  Against the oracle for every environment
                       and against the wave kernel byte for byte."""
import functools

import numpy as np
import pytest

from gpu_support import against_oracle, device_log_fixture, drive, kernel_name, rmsa_env, same_bytes, topology, write_topology  # noqa: F401

pytestmark = pytest.mark.gpu

NSF = "nsfnet_chen_5-paths_6-modulations"
LAUNCHES = (17, 300, 1000)
SEED = 7
LOAD = {64: 10, 320: 50}   # Erlang: a fifth to a third of a link's slots in use, some blocking
_ring4 = {}


def ring4(tmp_path_factory):
    """Four nodes in a ring, 100 km a link, two candidate paths per pair; frozen once per process."""
    if not _ring4:
        from optical_rl_gym_amd.topology_io import topology_from_txt
        edges = [(1, 2, 100), (2, 3, 100), (3, 4, 100), (4, 1, 100)]
        _ring4["t"] = topology_from_txt(write_topology(tmp_path_factory.mktemp("ring4"), "ring4", 4, edges), "ring4", k_paths=2)
    return _ring4["t"]


def env_kwargs(S):
    return dict(num_spectrum_resources=S, load=LOAD[S], mean_service_holding_time=25, episode_length=200, seed=SEED)


def bodies(run):
    return [s.split("body=")[1].split()[0] if "body=" in s else None for s in run["said"]]


def path_links(topo, src, dst, path):
    g = int(topo.pair_path_base[int(src) * topo.num_nodes + int(dst)]) + int(path)
    return topo.path_links[topo.path_link_off[g]:topo.path_link_off[g + 1]].tolist()


def provisions_per_link(topo, tr, i, lo, hi):
    """how often each link was provisioned on in steps lo .. hi - 1 of environment i"""
    n = np.zeros(topo.num_links, np.int64)
    for t in range(lo, hi):
        if tr["accepted"][t, i]:
            n[path_links(topo, tr["request"][t, i, 1], tr["request"][t, i, 2], tr["act_path"][t, i])] += 1
    return n


# ---------------------------------------------------------------------------------------- many link replays
@functools.lru_cache(maxsize=None)
def _wave_reference(S, B, policy):
    topo = _ring4["t"]
    return drive(lambda: rmsa_env(topo, B, "wave", stats_level="full", **env_kwargs(S)), LAUNCHES,
                 ("act_path", "act_slot", "accepted", "request"), policy=policy)


@pytest.mark.parametrize("body", ["lean", "full"])
@pytest.mark.parametrize("policy", ["sap_ff", "sp_ff"])
@pytest.mark.parametrize("B", [8, 5])
@pytest.mark.parametrize("S", [64, 320])
def test_many_link_replays(S, B, policy, body, tmp_path_factory, device_log_in_oracle):
    topo, kw = ring4(tmp_path_factory), env_kwargs(S)
    outs = () if body == "lean" else ("act_slot",)
    grp = drive(lambda: rmsa_env(topo, B, "group", stats_level="full", **kw), LAUNCHES, outs, policy=policy)
    assert set(grp["kernels"]) == {kernel_name("group", S, "full", defer=True)}, grp["said"]
    assert bodies(grp) == [body] * len(LAUNCHES), grp["said"]
    wav = _wave_reference(S, B, policy)
    # the shape does what it is here for: a provision is one log entry per link of its path, and so is its release; a link that
    # reaches 40 entries (ORLG_LLOG_FLUSH) has every link's log worked off.  200 provisions on the busiest link during the
    # launch of 1000 steps are 400 entries there: ten replays or more in that launch, and no link stays out of them
    for i in range(B):
        per_link = provisions_per_link(topo, wav["tr"], i, sum(LAUNCHES[:2]), sum(LAUNCHES))
        assert per_link.max() >= 200 and per_link.min() >= 100, (i, per_link)
    if outs:
        same_bytes({"act_slot": grp["tr"]["act_slot"]}, {"act_slot": wav["tr"]["act_slot"]}, "outputs")
    same_bytes(grp["snap"], wav["snap"], "state")
    against_oracle(topo, kw, grp, policy, LAUNCHES, range(B), "full", fields=outs)


# ---------------------------------------------------------------------------------------- replay inside the release loop
TRACE_STEPS, TRACE_S, TRACE_B, HOLD = 120, 320, 8, 100.0


def gap_trace(topo):
    """Environment i: 44 + 4 i requests between the same two neighbours, one time unit apart, each staying HOLD; then nothing for 30
    HOLD; then requests over all node pairs again.  The smallest bit rate: four slots on the direct link, so every one of them fits on it."""
    from conftest import DEFAULT_BIT_RATES
    from optical_rl_gym_amd import RequestTrace
    n, B, N = TRACE_STEPS + 20, TRACE_B, topo.num_nodes
    arrival, holding = np.zeros((B, n)), np.full((B, n), HOLD)
    src, dst = np.zeros((B, n), np.int32), np.zeros((B, n), np.int32)
    pairs = [(a, b) for a in range(N) for b in range(N) if a != b]
    for i in range(B):
        k = 44 + 4 * i                      # requests before the gap: steps 0 .. k - 1 provision them, step k - 1 ends the gap
        arrival[i] = np.arange(n, dtype=np.float64) + 1.0
        arrival[i, k:] += 30 * HOLD
        a = i % N
        src[i, :k], dst[i, :k] = a, (a + 1) % N
        for t in range(k, n):
            src[i, t], dst[i, t] = pairs[(t + i) % len(pairs)]
    return RequestTrace(arrival, holding, src, dst, np.full((B, n), min(DEFAULT_BIT_RATES), np.int32), batch_size=B, layout="env")


@functools.lru_cache(maxsize=None)
def _trace_references():
    topo = _ring4["t"]
    trace = gap_trace(topo)
    kw = dict(num_spectrum_resources=TRACE_S, episode_length=1000, queue_capacity=128, trace=trace)
    make = lambda: rmsa_env(topo, TRACE_B, "wave", stats_level="full", **kw)
    outs = ("act_path", "act_slot", "accepted", "request")
    return trace, kw, drive(make, (TRACE_STEPS,), outs, policy="sap_ff"), \
        drive(make, (TRACE_STEPS,), outs, policy="sap_ff", env_vars={"ORLG_NO_DEFER": "1"})


@pytest.mark.parametrize("body", ["lean", "full"])
@pytest.mark.parametrize("chunks", [1, 2, 4])
def test_replay_inside_the_release_loop(chunks, body, tmp_path_factory):
    topo = ring4(tmp_path_factory)
    trace, kw, wav, plain = _trace_references()
    assert wav["kernels"] != plain["kernels"], (wav["said"], plain["said"])   # (the deferred form and the one without a log)
    same_bytes(wav["tr"], plain["tr"], "wave kernel, deferred or not: outputs")
    same_bytes(wav["snap"], plain["snap"], "wave kernel, deferred or not: state")
    # what the trace says: everything is accepted; the step that ends environment i's gap releases its 44 + 4 i services, all
    # of which cross the link between the two neighbours -- more than ORLG_LLOG_FLUSH releases of one link in one step
    assert (wav["tr"]["accepted"] == 1).all()
    for i in range(TRACE_B):
        k = 44 + 4 * i
        assert provisions_per_link(topo, wav["tr"], i, 0, k).max() == k > 40
        running = sum(1 for t in range(TRACE_STEPS) if trace.arrival[i, t] + HOLD > trace.arrival[i, TRACE_STEPS])
        assert wav["snap"]["num_running"][i] == running < TRACE_STEPS - k + 1, (i, running)
        assert wav["snap"]["counters.services_accepted"][i] == TRACE_STEPS, i
    outs = () if body == "lean" else ("act_slot",)
    grp = drive(lambda: rmsa_env(topo, TRACE_B, "group", stats_level="full", **kw), (TRACE_STEPS,), outs, policy="sap_ff",
                env_vars={"ORLG_GROUP_CHUNKS": str(chunks)})
    assert grp["kernels"] == [kernel_name("group", TRACE_S, "full", defer=True, trace=True)], grp["said"]
    assert bodies(grp) == [body], grp["said"]
    if chunks > 1:
        assert f"chunks={chunks}" in grp["said"][0], grp["said"]
    if outs:
        same_bytes({"act_slot": grp["tr"]["act_slot"]}, {"act_slot": wav["tr"]["act_slot"]}, "outputs")
    same_bytes(grp["snap"], wav["snap"], "state")


# ---------------------------------------------------------------------------------------- graph replay and refill in one step
def test_graph_replay_and_refill_in_the_same_step(device_log_in_oracle):
    S, B, n = 320, 64, 200
    kw = dict(num_spectrum_resources=S, load=5, mean_service_holding_time=25, episode_length=1000, seed=SEED)
    make = lambda kernel: lambda: rmsa_env(NSF, B, kernel, stats_level="full", **kw)
    grp = drive(make("group"), (n,), (), policy="sap_ff")
    assert grp["kernels"] == [kernel_name("group", S, "full", defer=True)] and bodies(grp) == ["lean"], grp["said"]
    # acceptance near 1: a row's sixteenth logged provision comes every sixteen steps or so, at every offset from its refills
    assert (grp["snap"]["counters.services_accepted"] >= n - 4).all(), grp["snap"]["counters.services_accepted"].min()
    same_bytes(grp["snap"], drive(make("wave"), (n,), (), policy="sap_ff")["snap"], "state")
    against_oracle(NSF, kw, grp, "sap_ff", n, range(B), "full", fields=())
