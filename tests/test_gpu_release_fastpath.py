"""The two preludes of the group kernel's release pass.  A pass of the release loop of the DEFER
instantiations votes once over the wave: is the entry B behind the ring's head due in any row?  Where it is not, the PLAIN prelude
runs -- every lane of a row serves the head A, its place in the row is its hop, one entry leaves the ring; where it is, the
prelude of the paired release runs (test_gpu_release_pairs.py).  The plain prelude reads A's 16-byte record once and takes hops,
se and the lane's link from registers; both hand the one release pass its arguments, the lane's link among them.  Every result
must stay what it was.

Main comparison: the group kernel against the wave-per-environment kernel byte for byte -- save_state, counters, link and graph
statistics, occupancy of every environment, the per-step output where the launch has one -- and against the oracle for every
environment.  300 steps from reset at 50 Erlang in one deferred launch, with a whole-launch ticket and with 7 forced chunks, lean
(no output) and with one output (the full body):
  NSFNET, S = 64 and 320 (one and five words), B = 5 (three idle rows in the last quad, which must not vote) and B = 8
  ring36, S = 320, B = 5: paths of more than 8 hops, released on lanes 8..15 by the plain prelude, and as an unpaired A by the other
  a request trace (a TRACE handle; the oracle cannot follow one: the yardsticks are the wave kernel in its deferred form and in
  the form that keeps no log, as in test_gpu_step_waits.py) -- the generated traffic with a quiet gap in which every running
  service leaves, then, per quad, in one row X (the quad's LAST row in the first quad, its first in the second) and the others O:
      step 0   every row: a request that leaves before the next arrives          a ring of exactly one entry that is due
      step 1-2 X: two requests on link-disjoint routes, both due at step 2;      a pair in one row only, single releases beside
               O: one request due at step 2, one due at step 3                   it
      step 3   X: a request due at once; O: the one from step 2                  one due service per row: the plain prelude
                                                                                 straight after the other
      step 4-5 X: two requests on the SAME route, both due at step 5;            the vote says "a pair is possible", every row
               O: one due service at step 5                                      releases one service
      step 6-7 X: two requests on link-disjoint routes with EQUAL release times  a B that has A's release time

EVENTS: what a run must show at least once, replayed on the host quad by quad and pass by pass from the WAVE kernel's `arrival`,
`holding`, `accepted`, `request` and `act_path` with the group kernel's rules:
  plain           a pass in which no row has a due B
  paired          a pass in which some row has a due B (the other prelude)
  long_plain      a plain pass that releases a path of more than 8 hops                                               (ring36)
  long_beside     a pass in which one row releases a pair and another an unpaired A of more than 8 hops               (ring36)
  pair_one_row    a pass in which exactly one row releases a pair and every other row of the quad one service          (trace)
  plain_after     the step after a pair_one_row step begins with a plain pass in which every row releases              (trace)
  conflict_only   a pass in which a due B shares a link with its A, no other row has a due B, and every row releases   (trace)
  one             a ring of exactly one entry that is due                                                              (trace)
  tie             a pair whose B has A's release time                                                                  (trace)

Value mutants (profiles/README.md, round 19): the link handed to the release pass taken from hop 0 on every lane fails every case
here.  A vote that leaves out the quad's last row fails none and cannot: the plain prelude sets its own pop count and window, so
where it runs beside a due pair it releases A alone and B one pass later -- the same bytes."""
import bisect
import functools

import numpy as np
import pytest

from gpu_support import RMSA_OUTS, against_oracle, device_log_fixture, drive, kernel_name, rmsa_env, same_bytes, topology  # noqa: F401

pytestmark = pytest.mark.gpu

NSF, RING36 = "nsfnet_chen_5-paths_6-modulations", "ring36_3-paths_6-modulations"
SEED, N_STEPS, LOAD = 10, 300, 50
T0 = 200                 # the trace's first edited request
CHUNKS = {"defer": {}, "chunks": {"ORLG_GROUP_CHUNKS": "7"}}
ONE_OUTPUT = ("act_slot",)
GENERATED = {NSF: {"plain", "paired"}, RING36: {"plain", "paired", "long_plain", "long_beside"}}
TRACED = {"plain", "paired", "pair_one_row", "plain_after", "conflict_only", "one", "tie"}


def env_kwargs(S):
    return dict(num_spectrum_resources=S, load=LOAD, mean_service_holding_time=25, episode_length=200, seed=SEED)


def path_links(topo, src, dst, path):
    g = int(topo.pair_path_base[int(src) * topo.num_nodes + int(dst)]) + int(path)
    return frozenset(topo.path_links[topo.path_link_off[g]:topo.path_link_off[g + 1]].tolist())


def quad_events(topo, tr, rows):
    """The release passes of one wave: the environments `rows` (at most four) in step, pass by pass."""
    ev = set()
    ring = {i: [] for i in rows}     # release times in time order (ties in insert order)
    links = {i: [] for i in rows}    # ... and each entry's links
    arrival, accepted = tr["arrival"], tr["accepted"] != 0
    after_pair = False               # the step before had a pair_one_row pass
    for t in range(accepted.shape[0] - 1):
        for i in rows:
            if accepted[t, i]:
                rel = arrival[t, i] + tr["holding"][t, i]
                k = bisect.bisect_right(ring[i], rel)
                ring[i].insert(k, rel)
                links[i].insert(k, path_links(topo, tr["request"][t, i, 1], tr["request"][t, i, 2], tr["act_path"][t, i]))
        now, first, pair_here = arrival[t + 1], True, False
        while True:
            act = [i for i in rows if ring[i] and ring[i][0] <= now[i]]
            if not act:
                break
            b_due = [i for i in act if len(ring[i]) >= 2 and ring[i][1] <= now[i]]
            ev |= {"one"} if any(len(ring[i]) == 1 for i in act) else set()
            took = {i: 1 for i in act}
            if not b_due:
                ev.add("plain")
                ev |= {"long_plain"} if any(len(links[i][0]) > 8 for i in act) else set()
                ev |= {"plain_after"} if first and after_pair and len(act) == len(rows) == 4 else set()
            else:
                ev.add("paired")
                short = lambda i: len(links[i][0]) <= 8 and len(links[i][1]) <= 8
                pairs = [i for i in b_due if short(i) and not ({x & 63 for x in links[i][0]} & {x & 63 for x in links[i][1]})]
                took.update({i: 2 for i in pairs})
                ev |= {"tie"} if any(ring[i][1] == ring[i][0] for i in pairs) else set()
                ev |= {"long_beside"} if pairs and any(len(links[i][0]) > 8 for i in act if i not in pairs) else set()
                if len(pairs) == 1 and len(act) == len(rows) == 4:
                    ev.add("pair_one_row")
                    pair_here = True
                if not pairs and len(b_due) == 1 and len(act) == len(rows) == 4 and short(b_due[0]) and links[b_due[0]][0] & links[b_due[0]][1]:
                    ev.add("conflict_only")
            for i in act:
                del ring[i][:took[i]], links[i][:took[i]]
            first = False
        after_pair = pair_here
    return ev


def events(topo, tr):
    """... of every wave of the batch: four consecutive environments each, fewer in the last"""
    B = tr["accepted"].shape[1]
    return set().union(*(quad_events(topo, tr, range(q, min(q + 4, B))) for q in range(0, B, 4)))


def routes(topo):
    """Two node pairs whose shortest paths share no link, not modulo 64 either, and have at most 8 hops: what SAP-FF gives two
    requests in an empty network."""
    N = topo.num_nodes
    pairs = [(a, b) for a in range(N) for b in range(a + 1, N)]
    for a, b in pairs:
        la = path_links(topo, a, b, 0)
        for c, d in pairs:
            lb = path_links(topo, c, d, 0)
            if len(la) <= 8 and len(lb) <= 8 and not ({x & 63 for x in la} & {x & 63 for x in lb}):
                return (a, b), (c, d)
    raise AssertionError("no two link-disjoint shortest paths")


def _due(arr, t, u, frac):
    """a holding time with which request t leaves at step u: inside (arrival of u, arrival of u + 1)"""
    return arr[u] + frac * (arr[u + 1] - arr[u]) - arr[t]


def edited_trace(topo, tr, pending):
    """The generated traffic (a wave kernel's outputs and its pending requests) as a request trace with the module's edits."""
    from optical_rl_gym_amd import RequestTrace
    arrival = np.concatenate([tr["arrival"], pending["arrival_time"][None]])
    holding = np.concatenate([tr["holding"], pending["holding_time"][None]])
    req = tr["request"]
    src = np.concatenate([req[:, :, 1], pending["src"][None]])
    dst = np.concatenate([req[:, :, 2], pending["dst"][None]])
    (a, b), (c, d) = routes(topo)
    B = arrival.shape[1]
    assert B % 4 == 0
    for i in range(B):
        arrival[T0:, i] += 1000.0   # (holding times are ~25: everything running at step T0 - 1 leaves before request T0 arrives)
        arr = arrival[:, i]
        assert np.all(np.diff(arr[T0 - 1:]) > 0.0)
        h = holding[:, i]
        x = (i % 4) == (3 if i < 4 else 0)   # the quad's row X
        h[T0] = _due(arr, T0, T0, 0.5)
        if x:
            h[T0 + 1], h[T0 + 2] = _due(arr, T0 + 1, T0 + 2, 0.3), _due(arr, T0 + 2, T0 + 2, 0.6)
            src[T0 + 1, i], dst[T0 + 1, i], src[T0 + 2, i], dst[T0 + 2, i] = a, b, c, d
            h[T0 + 3] = _due(arr, T0 + 3, T0 + 3, 0.5)
            h[T0 + 4], h[T0 + 5] = _due(arr, T0 + 4, T0 + 5, 0.3), _due(arr, T0 + 5, T0 + 5, 0.6)
            src[T0 + 4, i], dst[T0 + 4, i], src[T0 + 5, i], dst[T0 + 5, i] = a, b, a, b
            src[T0 + 6, i], dst[T0 + 6, i], src[T0 + 7, i], dst[T0 + 7, i] = a, b, c, d
            for frac in (0.25, 0.3, 0.35, 0.4, 0.45, 0.5, 0.55):   # B leaves with A: a holding time whose sum is A's release time
                h[T0 + 6] = _due(arr, T0 + 6, T0 + 7, frac)
                rel_a = arr[T0 + 6] + h[T0 + 6]
                g = rel_a - arr[T0 + 7]
                tie = [v for v in (g, np.nextafter(g, np.inf), np.nextafter(g, 0.0)) if v > 0.0 and arr[T0 + 7] + v == rel_a]
                if tie:
                    break
            assert tie, i
            h[T0 + 7] = tie[0]
        else:
            for t in range(T0 + 1, T0 + 8):   # one due service per step from step T0 + 2 on
                h[t] = _due(arr, t, t + 1, 0.5)
    from conftest import DEFAULT_BIT_RATES
    rate = np.concatenate([req[:, :, 3], pending["bit_rate"][None]])
    rate[T0:T0 + 8] = min(DEFAULT_BIT_RATES)   # (at most 21 slots on any path: every edited request fits an empty network of 64)
    return RequestTrace(arrival, holding, src, dst, rate, batch_size=B, layout="step")


# ---------------------------------------------------------------------------------------- the runs
def _bodies(run):
    return [s.split("body=")[1].split()[0] if "body=" in s else None for s in run["said"]]


@functools.lru_cache(maxsize=None)
def _wave(name, S, B):
    """The wave kernel on the generated traffic: every output (the events are replayed from these), the state."""
    return drive(lambda: rmsa_env(name, B, "wave", stats_level="full", **env_kwargs(S)), (N_STEPS,), RMSA_OUTS, policy="sap_ff")


@functools.lru_cache(maxsize=None)
def _wave_traced(S, B):
    """The trace and the wave kernel on it, in its deferred form and in the one that keeps no log."""
    topo, gen = topology(NSF), _wave(NSF, S, B)
    trace = edited_trace(topo, gen["tr"], gen["snap"]["requests"])
    kw = dict(num_spectrum_resources=S, episode_length=200, trace=trace)
    make = lambda: rmsa_env(NSF, B, "wave", stats_level="full", **kw)
    return trace, kw, drive(make, (N_STEPS,), RMSA_OUTS, policy="sap_ff"), \
        drive(make, (N_STEPS,), RMSA_OUTS, policy="sap_ff", env_vars={"ORLG_NO_DEFER": "1"})


def _group(name, S, B, kw, shape, body, **flags):
    outs = () if body == "lean" else ONE_OUTPUT
    grp = drive(lambda: rmsa_env(name, B, "group", stats_level="full", **kw), (N_STEPS,), outs, policy="sap_ff", env_vars=CHUNKS[shape])
    assert grp["kernels"] == [kernel_name("group", S, "full", defer=True, **flags)], grp["said"]
    assert _bodies(grp) == [body], grp["said"]
    if shape == "chunks":
        assert "chunks=7" in grp["said"][0], grp["said"]
    return grp, outs


GEN_CASES = [(NSF, S, B) for S in (64, 320) for B in (5, 8)] + [(RING36, 320, 5)]


@pytest.mark.parametrize("body", ["lean", "full"])
@pytest.mark.parametrize("shape", ["defer", "chunks"])
@pytest.mark.parametrize("case", GEN_CASES, ids=lambda c: f"{c[0][:4]}-{c[1]}-{c[2]}")
def test_release_preludes_vs_wave_kernel_and_oracle(case, shape, body, device_log_in_oracle):
    name, S, B = case
    topo, kw, wav = topology(name), env_kwargs(S), _wave(name, S, B)
    ev = events(topo, wav["tr"])
    assert GENERATED[name] <= ev, sorted(GENERATED[name] - ev)
    grp, outs = _group(name, S, B, kw, shape, body)
    if outs:
        same_bytes(grp["tr"], {k: wav["tr"][k] for k in outs}, "outputs")
    same_bytes(grp["snap"], wav["snap"], "state")
    against_oracle(name, kw, grp, "sap_ff", N_STEPS, range(B), "full", fields=outs)


@pytest.mark.parametrize("body", ["lean", "full"])
@pytest.mark.parametrize("shape", ["defer", "chunks"])
@pytest.mark.parametrize("S", [64, 320])
def test_release_preludes_on_a_trace(S, shape, body):
    B = 8
    topo = topology(NSF)
    trace, kw, wav, plain = _wave_traced(S, B)
    assert wav["kernels"] != plain["kernels"], (wav["said"], plain["said"])   # (the deferred form and the one without a log)
    same_bytes(wav["tr"], plain["tr"], "wave kernel, deferred or not: outputs")
    same_bytes(wav["snap"], plain["snap"], "wave kernel, deferred or not: state")
    assert np.array_equal(wav["tr"]["arrival"], trace.arrival[:, :N_STEPS].T)
    # what the trace says: the edited requests meet an empty network and are all accepted on their shortest paths
    assert (wav["tr"]["accepted"][T0:T0 + 8] == 1).all() and (wav["tr"]["act_path"][T0:T0 + 8] == 0).all()
    ev = events(topo, wav["tr"])
    assert TRACED <= ev, sorted(TRACED - ev)
    grp, outs = _group(NSF, S, B, kw, shape, body, trace=True)
    if outs:
        same_bytes(grp["tr"], {k: wav["tr"][k] for k in outs}, "outputs")
    same_bytes(grp["snap"], wav["snap"], "state")
