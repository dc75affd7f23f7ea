"""The group kernel's step with its dependent LDS chain shortened: a provision's window is cleared INSIDE the statistics pass
(no write pass in front of it), the release queue's head travels as (time, descriptor) in registers, and the policy reads a
path's hop words four to a wait.  Held byte for byte against the wave-per-environment kernel -- per-step outputs, counters, link
statistics, available_slots and save_state of all B environments -- and against the oracle for the first, a middle and the last
environment, at 1, 2, 5 and 8 words per link (S = 400: slot S - 1 is not in the last word), on two topologies, under every
statistics level (`counters` keeps the separate write pass), in deferred launches (whole-launch tickets and 7 forced chunks),
launches of one step (the ring, and so the head's descriptor, in HBM) and launches of 8 steps (LDS ring, not deferred).

B = 10: two rows of the last quad idle and must not touch the last environment's ring or head.  Every case also asserts, from
its own outputs, that the events it is there for occurred (EVENTS below): they are replayed from `arrival`, `holding` and
`accepted` exactly as the kernel's ring sees them (release time = arrival + holding, due when <= the next arrival)."""
import heapq
import math

import numpy as np
import pytest

from gpu_support import against_oracle, device_log_fixture, drive, external_actions, kernel_name, rmsa_env, same_bytes, topology  # noqa: F401

pytestmark = pytest.mark.gpu

B = 10
SEED = 23
NSF, US14 = "nsfnet_chen_5-paths_6-modulations", "us14_3-paths_6-modulations"
DEFER, ONE, EIGHT = (700, 333), (1,) * 200, (8,) * 40

# What a case must show at least once, over its B environments:
#   head    the inserted service became the ring's new head: its release time below every running one
#   multi   two or more releases in one row within one step
#   refill  a release emptied the ring, and the next insert went into the empty ring
#   slot0   an accepted window starts at slot 0          cross   an accepted window crosses a 64-slot word boundary
#   hops    provisioned paths of 1, 4 and 5 hops (the boundary of a batch of four hop words) and one of at least 8 hops, or the
#           topology's longest if that is shorter
EVENTS = ("head", "multi", "refill", "slot0", "cross", "hops")

# (topology, slots, load, policy, statistics level, launches, events)
CASES = [
    (NSF, 64, 300, "sap_ff", "full", DEFER, ("head", "multi", "slot0")),
    (NSF, 64, 2, "sap_ff", "full", DEFER, ("head", "multi", "refill", "slot0")),
    (US14, 100, 300, "deeprmsa_sap_ff", "full", DEFER, ("head", "multi", "slot0", "cross", "hops")),
    (NSF, 320, 50, "llp_ff", "full", DEFER, ("head", "multi", "slot0", "cross")),
    (US14, 400, 600, "sap_ff", "full", DEFER, ("head", "multi", "slot0", "cross")),
    (NSF, 512, 1, "llp_ff", "full", DEFER, ("head", "multi", "refill", "slot0", "cross", "hops")),
    (US14, 64, 300, "llp_ff", "network", DEFER, ("head", "multi", "slot0", "hops")),
    (NSF, 320, 50, "sap_ff", "counters", DEFER, ("head", "multi", "slot0", "cross")),
    (NSF, 320, 50, "deeprmsa_sap_ff", "full", ONE, ("head", "multi", "slot0", "cross")),
    (US14, 64, 2, "sap_ff", "counters", ONE, ("head", "multi", "refill", "slot0", "hops")),
    (NSF, 100, 300, "sap_ff", "full", EIGHT, ("head", "multi", "slot0", "cross")),
    (US14, 400, 2, "deeprmsa_sap_ff", "network", EIGHT, ("head", "multi", "refill", "slot0", "cross")),
    (NSF, 512, 150, "sap_ff", "counters", EIGHT, ("head", "multi", "slot0", "cross", "hops")),
]
# external (path, slot) actions, one launch per step as tests/test_gpu_rmsa.py drives them: paths 0 .. K (K: out of range),
# slots 0 .. S (S: out of range), most windows occupied at load 300; at load 2 nearly every window is free and the long paths
# get provisioned
EXT_CASES = [
    (NSF, 64, 300, "full", ("head", "slot0")),
    (US14, 100, 300, "network", ("head", "multi", "slot0", "cross")),
    (NSF, 320, 2, "counters", ("head", "multi", "refill", "slot0", "cross", "hops")),
]
EXT_STEPS = 200


def env_kwargs(S, load):
    return dict(num_spectrum_resources=S, load=load, mean_service_holding_time=25, episode_length=300, seed=SEED)


def events_of(topo, S, cols):
    """The EVENTS one environment's trace shows, and the hop counts of the paths it provisioned.  cols: act_path, act_slot,
    accepted, src, dst, bit_rate, arrival, holding [n]."""
    ev = set()
    acc = cols["accepted"] != 0
    N = topo.num_nodes
    gid = topo.pair_path_base[cols["src"] * N + cols["dst"]] + np.where(acc, cols["act_path"], 0)
    hops = set(int(h) for h in topo.path_hops[gid[acc]])
    # get_number_slots: ceil(bit_rate / (spectral efficiency x 12.5 GHz)) + 1
    n = np.array([math.ceil(b / (se * 12.5)) + 1 for b, se in zip(cols["bit_rate"], topo.path_se[gid])])
    s = cols["act_slot"]
    if (acc & (s == 0)).any():
        ev.add("slot0")
    if (acc & ((s >> 6) != ((s + n - 1) >> 6))).any():
        ev.add("cross")
    ring, emptied = [], False
    for t in range(len(acc)):
        if acc[t]:
            rel = cols["arrival"][t] + cols["holding"][t]
            if ring and rel < ring[0]:
                ev.add("head")
            if not ring and emptied:
                ev.add("refill")
            emptied = False
            heapq.heappush(ring, rel)
        if t + 1 < len(acc):
            k = 0
            while ring and ring[0] <= cols["arrival"][t + 1]:
                heapq.heappop(ring)
                k += 1
            if k >= 2:
                ev.add("multi")
            if k and not ring:
                emptied = True
    return ev, hops


def with_hops(topo, ev, hops):
    """`hops` joins the events once the hop counts provisioned by the batch hold 1, 4, 5 and a long one."""
    long_hops = min(8, int(topo.path_hops.max()))
    return ev | ({"hops"} if {1, 4, 5} <= hops and any(h >= long_hops for h in hops) else set())


def events_of_batch(topo, S, tr):
    """Union over the environments of a device trace (arrays [n, B])."""
    ev, hops = set(), set()
    for i in range(tr["accepted"].shape[1]):
        cols = {k: tr[k][:, i] for k in ("act_path", "act_slot", "accepted", "arrival", "holding")}
        cols.update(src=tr["request"][:, i, 1], dst=tr["request"][:, i, 2], bit_rate=tr["request"][:, i, 3])
        e, h = events_of(topo, S, cols)
        ev |= e
        hops |= h
    return with_hops(topo, ev, hops)


def _hold(name, S, load, policy, stats, launches, shows, chunks, actions=None):
    topo, kw = topology(name), env_kwargs(S, load)
    make = lambda kernel: lambda: rmsa_env(topo, B, kernel, stats_level=stats, **kw)
    grp = drive(make("group"), launches, policy=policy, env_vars={"ORLG_GROUP_CHUNKS": chunks} if chunks else {}, actions=actions)
    names = set(grp["kernels"])
    # the instantiation each launch shape is there for
    if launches == DEFER and stats == "full":
        assert names == {kernel_name("group", S, stats, defer=True)}, names
    elif launches == DEFER or launches == EIGHT:
        assert names == {kernel_name("group", S, stats)}, names
    else:
        assert all(n.startswith(kernel_name("group", S, stats)[:-1]) for n in names), names
        if S >= 320 and stats == "full":   # (the ring of a small environment fits the LDS in one-step launches too)
            assert names == {kernel_name("group", S, stats, hbmq=True)}, names
    if chunks:
        assert f"chunks={chunks}" in grp["said"][-1], grp["said"][-1]
    wav = drive(make("wave"), launches, policy=policy, actions=actions)
    same_bytes(grp["tr"], wav["tr"], "outputs")
    same_bytes(grp["snap"], wav["snap"], "state")
    if actions is not None:   # in-range actions both accepted and turned down (occupied, or reaching past the last slot)
        inr = (actions[:, :, 0] < topo.k_paths) & (actions[:, :, 1] < S - 16)
        assert (grp["tr"]["accepted"][inr] != 0).any() and (grp["tr"]["accepted"][inr] == 0).any()
    ev = events_of_batch(topo, S, grp["tr"])
    assert set(shows) <= ev, (sorted(set(shows) - ev), sorted(ev))
    # (the counters level keeps no network statistics: its compactness outputs stay 1.0 / 0.0 in both kernels)
    against_oracle(name, kw, grp, policy, sum(launches), (0, 5, B - 1), stats, actions=actions)


def _id(case):
    topo, S, load, policy, stats, launches = case[:6]
    shape = {DEFER: "defer", ONE: "one", EIGHT: "eight"}[launches]
    return f"{topo[:4]}-{S}-{load}-{policy}-{stats}-{shape}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_group_chain_vs_wave_kernel_and_oracle(case, device_log_in_oracle):
    name, S, load, policy, stats, launches, shows = case
    _hold(name, S, load, policy, stats, launches, shows, None)


@pytest.mark.parametrize("case", [c for c in CASES if c[5] == DEFER and c[4] == "full"], ids=_id)
def test_group_chain_in_seven_chunks(case, device_log_in_oracle):
    name, S, load, policy, stats, launches, shows = case
    _hold(name, S, load, policy, stats, launches, shows, "7")


@pytest.mark.parametrize("case", EXT_CASES, ids=lambda c: f"{c[0][:4]}-{c[1]}-{c[2]}-{c[3]}")
def test_group_chain_external_actions(case, device_log_in_oracle):
    name, S, load, stats, shows = case
    topo = topology(name)
    actions = external_actions(topo, S, EXT_STEPS, B)
    # out-of-range paths and slots among the actions (_hold looks for in-range actions accepted and turned down)
    assert (actions[:, :, 0] == topo.k_paths).any() and (actions[:, :, 1] == S).any()
    _hold(name, S, load, "external", stats, (1,) * EXT_STEPS, shows, None, actions)
