"""The group kernel's release-queue insert: chunks of 16 entries anchored at the ring's last entry, scanned from the top or --
where the ring is in LDS -- from the head upward, whichever end is nearer to the new entry's place.  A scan from the
head moves the earlier entries and the head DOWN one slot, so the ring in LDS drifts against the ring the state holds; the state
store rotates it back and writes the (+inf, 0) of the popped slots itself.

Main comparison: the group kernel against the wave-per-environment kernel byte for byte -- per-step outputs, counters, link
statistics, available_slots and save_state of every environment -- and against the oracle for the first, a middle and the last
environment.  NSFNET, B = 5 (three idle rows in the last quad) and B = 64, S = 64 / 100 / 320, 300 steps at 10 and at 50 Erlang
(rings of under 16, of 17 to 32 and of more than 32 entries), `queue_capacity` 16 and 32 (the library rounds a capacity up to its
minimum of 64 slots: Q below is the ring's real size) at a low load, where the head drifts down more than Q slots in one ticket;
deferred launches with whole-launch tickets and with 7 forced chunks -- with outputs (full body), and without, lean and with
ORLG_NO_LEAN -- 8-step launches, one-step launches (the ring in HBM where it does not fit: from the top only).  Every case runs
twice: on the generated traffic, where the oracle can follow, and on that traffic as a request trace (a TRACE handle) with
edits per environment: one holding time changed so that the release time EQUALS the head's, the middle entry's (the one compared
for the side) or the last entry's, by the environment's index; a quiet gap in which every running service leaves; after it an
insert into the empty ring, then one into the ring of one that is earlier (a downward insert right after the ring was emptied
and refilled), becomes the head and is the next step's first release.  One case overflows its ring.

EVENTS: what a run must show at least once over its environments, replayed on the host from `arrival`, `holding`, `accepted`
(a sorted list, bisect_right: release time = arrival + holding, due when <= the next arrival, ties behind) with the kernel's
rule for the side (down when strictly earlier than entry q_n // 2) and its tickets (the ring in LDS starts every ticket at the
state's head):
  small / mid / big   an insert into a ring of 1 .. 15 / 17 .. 32 / more than 32 entries
  lower / upper       an insert on either side of the middle entry
  up16 / down16       an insert that moved more than 16 entries up / down
  wrapdown            the head in LDS went from slot 0 to slot Q - 1
  drift               more than Q downward inserts in one ticket
  tie_head / tie_mid / tie_last   an equal release time with the head, the middle, the last entry        (trace run only)
  empty / one         an insert into an empty ring (after a pop emptied it) / into a ring of one          (trace run only)
  first               an insert that became the head and was the next step's first release                (trace run only)
  down_after_empty    the insert into the ring of one that the emptied ring's first insert left: downward (trace run only)"""
import bisect

import numpy as np
import pytest

from gpu_support import RMSA_OUTS as OUTS, against_oracle, device_log_fixture, drive, kernel_name, rmsa_env, same_bytes, snapshot, tooling_env, topology  # noqa: F401

pytestmark = pytest.mark.gpu

NSF = "nsfnet_chen_5-paths_6-modulations"
SEED, N_STEPS = 41, 300
SHAPES = {"defer": (N_STEPS,), "chunks": (N_STEPS,), "one": (1,) * N_STEPS, "eight": (8,) * 37 + (4,)}
TICKET = {"defer": N_STEPS, "chunks": (N_STEPS + 6) // 7, "one": 1, "eight": 8}   # steps per ticket (orlg_group_tickets)
TRACED = {"tie_head", "tie_mid", "tie_last", "empty", "one", "first"}
HALVES = {"lower", "upper", "small"}
BIG = HALVES | {"mid", "big", "up16", "down16"}

# (slots, batch, load, queue_capacity, launch shape, events of the generated run).  Load 50 on 320 slots runs ~38 services, load 10
# about ten; S = 64 and 100 hold fewer (a request takes up to a third of a link of 64)
CASES = [
    (320, 5, 50, 0, "defer", BIG | {"wrapdown"}),
    (320, 64, 50, 0, "chunks", BIG | {"wrapdown"}),
    (100, 5, 10, 0, "defer", HALVES | {"wrapdown", "drift"}),
    (64, 64, 10, 0, "chunks", HALVES | {"wrapdown"}),
    (320, 5, 10, 16, "defer", HALVES | {"wrapdown", "drift"}),
    (100, 64, 10, 32, "defer", HALVES | {"wrapdown", "drift"}),
    (64, 5, 10, 16, "chunks", HALVES | {"wrapdown"}),
    (320, 64, 50, 0, "eight", BIG),
    (100, 5, 50, 32, "eight", HALVES),
    (320, 5, 50, 256, "one", BIG),          # the ring in HBM
    (64, 64, 50, 0, "one", HALVES),
]


def ring_slots(load, capacity):
    """Q as orlg_create sizes it: the capacity asked for, or load + 10 sigma; whole rows of 16, at least 64."""
    q = capacity if capacity > 0 else int(load + 10.0 * np.sqrt(load))
    return max(64, (q + 15) // 16 * 16)


def env_kwargs(S, load):
    return dict(num_spectrum_resources=S, load=load, mean_service_holding_time=25, episode_length=200, seed=SEED)


def ring_replay(arrival, holding, accepted, Q, ticket, two_sided=True):
    """One environment's ring, step by step.  Returns (events, rings): rings[t] = the release times in the ring, sorted, when
    step t's insert looks at it."""
    ev, rings = set(), []
    ring, ids = [], []            # release times in time order (ties in insert order), and the steps that put them there
    head = lds = 0                # the state's head, the head in LDS
    down_n = 0                    # downward inserts of this ticket
    emptied = after_empty = False
    new_head = None               # the step whose insert became the head, until something else does or it leaves
    for t in range(len(accepted)):
        if t % ticket == 0:
            lds, down_n = head, 0
        rings.append(list(ring))
        if accepted[t]:
            rel, n = arrival[t] + holding[t], len(ring)
            k = bisect.bisect_right(ring, rel)
            ev |= {"small"} if 0 < n < 16 else {"mid"} if 16 < n <= 32 else {"big"} if n > 32 else set()
            if n == 0 and emptied:
                ev.add("empty")
            if n == 1:
                ev.add("one")
            if n:
                ev |= {name for name, at in (("tie_head", 0), ("tie_mid", n // 2), ("tie_last", n - 1)) if ring[at] == rel}
                low = rel < ring[n // 2]
                ev.add("lower" if low else "upper")
                if low and two_sided:
                    if k > 16:
                        ev.add("down16")
                    if lds == 0:
                        ev.add("wrapdown")
                    lds, down_n = (lds - 1) % Q, down_n + 1
                    if down_n > Q:
                        ev.add("drift")
                    if after_empty and n == 1:
                        ev.add("down_after_empty")
                elif n - k > 16:
                    ev.add("up16")
            after_empty = n == 0 and emptied
            emptied = False
            if k == 0:
                new_head = t
            ring.insert(k, rel)
            ids.insert(k, t)
        if t + 1 < len(accepted):
            pops = 0
            while ring and ring[0] <= arrival[t + 1]:
                ring.pop(0)
                if pops == 0 and ids[0] == new_head:
                    ev.add("first")
                ids.pop(0)
                new_head = None
                head, lds, pops = (head + 1) % Q, (lds + 1) % Q, pops + 1
            if pops and not ring:
                emptied = True
    return ev, rings


def events(tr, Q, ticket, two_sided):
    ev = set()
    for i in range(tr["accepted"].shape[1]):
        ev |= ring_replay(tr["arrival"][:, i], tr["holding"][:, i], tr["accepted"][:, i] != 0, Q, ticket, two_sided)[0]
    return ev


def edited_trace(tr, pending, Q, ticket):
    """The generated traffic as a request trace.  Environment i: a tie with the head / the middle entry / the last entry
    (i % 3) at a step from 100 on; every running service gone before request 200; request 200 stays beyond request 202,
    request 201 leaves before it."""
    from optical_rl_gym_amd import RequestTrace
    arrival = np.concatenate([tr["arrival"], pending["arrival_time"][None]])
    holding = np.concatenate([tr["holding"], pending["holding_time"][None]])
    for i in range(arrival.shape[1]):
        acc = tr["accepted"][:, i] != 0
        _, rings = ring_replay(tr["arrival"][:, i], tr["holding"][:, i], acc, Q, ticket)
        done = False
        for t in range(100, 190):   # (nothing before step t changes, so the ring at step t is the generated run's)
            ring = rings[t]
            if not acc[t] or len(ring) < 3:
                continue
            want = ring[(0, len(ring) // 2, len(ring) - 1)[i % 3]]
            h = want - arrival[t, i]
            for cand in (h, np.nextafter(h, np.inf), np.nextafter(h, 0.0)):
                if cand > 0.0 and arrival[t, i] + cand == want:
                    holding[t, i] = cand
                    done = True
                    break
            if done:
                break
        assert done, i
        arrival[200:, i] += 1000.0   # (holding times are ~25: everything running at step 199 leaves before request 200 arrives)
        assert arrival[202, i] > arrival[201, i] >= arrival[200, i]
        holding[200, i] = arrival[202, i] - arrival[200, i] + 50.0
        holding[201, i] = 0.5 * (arrival[202, i] - arrival[201, i])
    req = tr["request"]
    return RequestTrace(arrival, holding, np.concatenate([req[:, :, 1], pending["src"][None]]),
                        np.concatenate([req[:, :, 2], pending["dst"][None]]), np.concatenate([req[:, :, 3], pending["bit_rate"][None]]),
                        batch_size=arrival.shape[1], layout="step")


def _drive(B, kw, kernel, launches, capacity, outputs=OUTS, **env_vars):
    return drive(lambda: rmsa_env(topology(NSF), B, kernel, stats_level="full", queue_capacity=capacity, **kw), launches, outputs,
                 policy="sap_ff", env_vars=env_vars)


def _same(grp, wav, what):
    same_bytes(grp["tr"], wav["tr"], what + ": outputs")
    same_bytes(grp["snap"], wav["snap"], what + ": state")


def _bodies(run):
    return {s.split("body=")[1].split()[0] if "body=" in s else None for s in run["said"]}


def _group_and_wave(S, B, kw, shape, capacity, trace):
    """The group kernel with outputs against the wave kernel; on the long launches also without outputs: the lean body and the
    full one leave the state the launch with outputs left."""
    launches = SHAPES[shape]
    chunks = {"ORLG_GROUP_CHUNKS": "7"} if shape == "chunks" else {}
    grp = _drive(B, kw, "group", launches, capacity, **chunks)
    hbmq = shape == "one" and S >= 320
    if shape in ("defer", "chunks"):
        assert set(grp["kernels"]) == {kernel_name("group", S, "full", defer=True, trace=trace)}, grp["said"]
    elif hbmq:
        assert set(grp["kernels"]) == {kernel_name("group", S, "full", hbmq=True, trace=trace)}, grp["said"]
    if shape == "chunks":
        assert "chunks=7" in grp["said"][-1], grp["said"][-1]
    wav = _drive(B, kw, "wave", launches, capacity)
    _same(grp, wav, shape)
    if shape in ("defer", "chunks"):
        lean = _drive(B, kw, "group", launches, capacity, outputs=(), **chunks)
        full = _drive(B, kw, "group", launches, capacity, outputs=(), ORLG_NO_LEAN="1", **chunks)
        assert _bodies(lean) == {"lean"} and _bodies(full) == {"full"}, (lean["said"], full["said"])
        same_bytes(lean["snap"], grp["snap"], shape + ": lean body")
        same_bytes(full["snap"], grp["snap"], shape + ": full body without outputs")
    return grp, wav, not hbmq


def _id(case):
    return "-".join(str(c) for c in case[:5])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_queue_insert_vs_wave_kernel_and_oracle(case, device_log_in_oracle):
    S, B, load, capacity, shape, want = case
    kw, Q, ticket = env_kwargs(S, load), ring_slots(load, capacity), TICKET[shape]
    grp, wav, two_sided = _group_and_wave(S, B, kw, shape, capacity, False)
    ev = events(grp["tr"], Q, ticket, two_sided)
    want = want - (set() if two_sided else {"down16", "wrapdown", "drift"})
    assert want <= ev, sorted(want - ev)
    against_oracle(NSF, kw, grp, "sap_ff", N_STEPS, (0, B // 2, B - 1), "full")
    # the same traffic as a trace, with a tie, a drained ring and a downward insert into the ring of one in every environment
    trace = edited_trace(wav["tr"], wav["snap"]["requests"], Q, ticket)
    tkw = dict(num_spectrum_resources=S, episode_length=200, trace=trace)
    tg, _, _ = _group_and_wave(S, B, tkw, shape, Q, True)
    assert np.array_equal(tg["tr"]["arrival"], trace.arrival[:, :N_STEPS].T)
    ev = events(tg["tr"], Q, ticket, two_sided)
    want = TRACED | ({"down_after_empty"} if two_sided else set())
    assert want <= ev, sorted(want - ev)


@pytest.mark.parametrize("env_vars", [{}, {"ORLG_NO_LEAN": "1"}, {"ORLG_GROUP_CHUNKS": "7"}], ids=["lean", "full", "chunks"])
def test_overflowed_ring_leaves_the_wave_kernels_state(env_vars):
    """queue_capacity=16 (64 slots) at 150 Erlang: far more services than slots.  Both kernels report the overflow, and lose the
    same releases: the states are equal byte for byte.  (A state load takes min(n_running, Q) entries, and n_running counts the
    lost services too: after an overflow a ticket boundary is visible, so the wave kernel is stepped in the chunks' launches.)"""
    from optical_rl_gym_amd import OrlgError
    kw = dict(env_kwargs(320, 150), episode_length=1000)
    snaps = {}
    for kernel in ("group", "wave"):
        with tooling_env(**(env_vars if kernel == "group" else {})):
            env = rmsa_env(NSF, 5, kernel, stats_level="full", queue_capacity=16, **kw)
            for n in (600,) if kernel == "group" or "ORLG_GROUP_CHUNKS" not in env_vars else (86,) * 6 + (84,):
                env.run("sap_ff", n)
            with pytest.raises(OrlgError) as ei:
                env.synchronize()
            assert ei.value.code == -4, kernel
            snaps[kernel] = snapshot(env)
            env.close()
    assert snaps["group"]["num_running"].max() > 64   # (the services an overflow lost stay counted)
    same_bytes(snaps["group"], snaps["wave"], "overflow")
