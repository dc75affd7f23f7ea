"""Most-used assignment and the best-window-over-all-paths route on the device (``include/orlg.h`` ``orlg_step_window``,
``orlg_slot_usage``, ``orlg_path_most_used``): the nine names of ``WINDOW_POLICIES`` against the numpy restatement
of the definitions driving the oracle with external actions, one step at a time (``usage_reference.py``;
``test_window_rules.py`` holds that module to brute force and shows that the new names differ from first fit and from sap on
these shapes).  Both step kernels, every kind of handle, every launch shape, with and without the blocking cause, the two
queries; and that a launch under an old policy name runs the kernel it ran.  Integer-exact: no tolerance anywhere.

B = 8 unless said, 200 steps from an empty network, ``episode_length=50`` (three auto-resets inside a launch), seeds 10 + i,
holding time 25: the setup of ``block_cause_reference``."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import assign_reference as ar
import block_cause_reference as bcr
import cut_reference as cr
import gn_gate_reference as ggr
import usage_reference as ref
from gpu_support import (MANY_PATHS_SEED, RMSA_OUTS, STATS_LEVELS, device_log_fixture, drive, external_actions, kernel_name,  # noqa: F401
                         many_paths_kwargs, many_paths_topology, one_step_launches, rmsa_env, same_bytes, snapshot, step_kernel,
                         tooling_env, topology)

pytestmark = pytest.mark.gpu

NSF = ref.NSFNET
RING34, RING36 = "ring34_3-paths_6-modulations", "ring36_3-paths_6-modulations"
B, N = ref.N_ENVS, ref.N_STEPS
DECIDED = ("act_path", "act_slot", "accepted")


def usage_kernel(kernel, S, stats="full", cause=False, traffic=False, trace=False):
    """The instantiation a launch under a new name reports: the plain kind of either kernel with the ASSIGN flag, no
    CUT flag and the USAGE flag last."""
    W = (S + 63) // 64
    W, level = 8 if W == 7 else W, STATS_LEVELS.index(stats)
    t = lambda flag: str(bool(flag)).lower()
    if kernel == "group":
        return f"orlg_rmsa_group_kernel<{W},{level},false,false,{t(traffic)},{t(trace)},{t(cause)},true,false,true>"
    return f"orlg_rmsa_kernel<{W},{level},false,false,{t(cause)},true,false,true>"


def make_env(S, load, kernel, batch=B, **kw):
    return rmsa_env(NSF, batch, kernel, **bcr.shape_kwargs(S, load, **kw))


def decisions_hold(tr, want, envs, what):
    """act_path, act_slot, accepted of environment i (column i of tr) equal the reference run want(i), step by step"""
    for i in envs:
        w = want(i)
        for k in DECIDED:
            bad = np.flatnonzero(tr[k][:, i] != w[k][:len(tr[k])])
            assert bad.size == 0, (what, i, k, bad[:6], tr[k][bad[:6], i], w[k][bad[:6]])


def oracle_state_holds(env, topo, kw, seed0, runs, n, what):
    """occupancy, counters, clock and link statistics of the handle equal those of the oracle driven through `external` with the
    reference's actions; runs: {environment: its reference run}"""
    from gpu_support import _oracle_run, state_matches
    snap = snapshot(env)
    for i, w in runs.items():
        actions = np.stack([w["act_path"][:n], w["act_slot"][:n]], axis=-1).astype(np.int32)
        _, final = _oracle_run(topo, kw, seed0 + i, "external", (n,), actions)
        state_matches(snap, i, final, (what, i))


# ---------------------------------------------------------------------------------------- 1. one launch, against the reference
@pytest.mark.parametrize("name", ref.LAUNCHED)
@pytest.mark.parametrize("S,load", ref.SHAPES)
def test_one_launch_against_the_reference(S, load, name, step_kernel):
    """W = 1, W = 2 with a last word that is not full, W = 5.  The decisions step by step; the state afterwards -- occupancy,
    counters, link statistics -- for two environments of the batch (the others are held through their decisions: a step's
    decision depends on everything before it)."""
    env = make_env(S, load, step_kernel)
    tr = env.run(name, N, outputs=DECIDED, auto_reset=True)
    assert env.last_kernel().split()[0] == usage_kernel(step_kernel, S), env.last_kernel()
    assert tr["act_slot"].shape == (N, B)
    decisions_hold(tr, lambda i: ref.nsfnet_steps(S, load, name, i), range(B), (S, name, step_kernel))
    oracle_state_holds(env, topology(NSF), bcr.shape_kwargs(S, load), ref.SEED0, {i: ref.nsfnet_steps(S, load, name, i) for i in (0, B - 1)}, N,
                       (S, name))
    env.close()
    # (what test_window_rules.py shows of the reference: the comparison is not one of first fits, nor of sap's paths)
    want = ref.stacked(S, load, name)
    acc = want["accepted"] == 1
    if ref.NAMES[name][1] == "most_used":
        assert (acc & (tr["act_slot"] != want["ff_slot"])).sum(axis=0).min() >= 1
    if name == "any_ff_full":
        assert (tr["act_path"] != want["sap_path"]).sum(axis=0).min() >= 1


def path_actions(topo, S):
    """random paths that include k and values out of range on either side"""
    actions = external_actions(topo, S, N, B, kind="paths")
    actions[5::17] = -1
    actions[7::19] = topo.k_paths + 3
    actions[3::23] = topo.k_paths
    return actions


@pytest.mark.parametrize("S,load", ref.SHAPES)
def test_path_only_actions(S, load, step_kernel, device_log_in_oracle):
    topo = topology(NSF)
    actions = path_actions(topo, S)
    env = make_env(S, load, step_kernel)
    tr = one_step_launches(env, "path_mu_external", N, DECIDED, actions=actions, auto_reset=True)
    assert env.last_kernel().split()[0] == usage_kernel(step_kernel, S), env.last_kernel()
    env.close()
    runs = {}

    def want(i):
        if i not in runs:
            runs[i] = ref.oracle_steps(topo, bcr.shape_kwargs(S, load), ref.SEED0 + i, "path_mu_external", N, paths=actions[:, i])
        return runs[i]

    decisions_hold(tr, want, range(B), S)
    assert (tr["act_path"] == topo.k_paths).any() and (tr["accepted"] == 1).any()
    assert ((tr["act_path"] == topo.k_paths) == (tr["act_slot"] == S)).all()
    # out of range, and in range without a window
    assert ((actions < 0) | (actions >= topo.k_paths)).any() and ((actions >= 0) & (actions < topo.k_paths) & (tr["accepted"] == 0)).any()


# ---------------------------------------------------------------------------------------- 2. every launch shape, the same bits
@pytest.mark.parametrize("policy", ["any_mu", "llp_mu", "any_bf"])
def test_launch_shapes_give_the_same_bits(policy, step_kernel):
    S, load = 100, 20
    env = make_env(S, load, step_kernel)
    one = env.run(policy, N, outputs=RMSA_OUTS, auto_reset=True)
    env.close()
    env = make_env(S, load, step_kernel)
    steps = one_step_launches(env, policy, N, RMSA_OUTS, auto_reset=True)
    # (a launch of one step asks the group kernel's plan for the queue in HBM: a launch under these names stays on the plain kind)
    assert env.last_kernel().split()[0] == usage_kernel(step_kernel, S), env.last_kernel()
    env.close()
    same_bytes(steps, one, "one-step launches")
    env = make_env(S, load, step_kernel)
    a, b = env.run(policy, 7, outputs=RMSA_OUTS, auto_reset=True), env.run(policy, N - 7, outputs=RMSA_OUTS, auto_reset=True)
    env.close()
    same_bytes({k: np.concatenate([a[k], b[k]]) for k in a}, one, "7 + 193")
    if step_kernel == "group":   # tickets in chunks of steps: successive chunks of a quad may run on different waves
        with tooling_env(ORLG_GROUP_CHUNKS="7"):
            env = make_env(S, load, "group")
            chunks = env.run(policy, N, outputs=RMSA_OUTS, auto_reset=True)
            assert "chunks=7" in env.last_kernel() and env.last_kernel().split()[0] == usage_kernel("group", S), env.last_kernel()
            env.close()
        same_bytes(chunks, one, "chunks")


def test_wave_and_group_continue_each_other():
    """100 steps on one kernel, the state saved and loaded into a handle on the other, 100 more: the bits of one launch"""
    S, load, policy = 320, 50, "any_mu"
    env = make_env(S, load, "wave")
    one = env.run(policy, N, outputs=RMSA_OUTS, auto_reset=True)
    end = snapshot(env)
    env.close()
    for first, second in (("wave", "group"), ("group", "wave")):
        a, b = make_env(S, load, first), make_env(S, load, second)
        ta = a.run(policy, 100, outputs=RMSA_OUTS, auto_reset=True)
        b.load_state(a.save_state())
        tb = b.run(policy, N - 100, outputs=RMSA_OUTS, auto_reset=True)
        assert b.last_kernel().split()[0] == usage_kernel(second, S), b.last_kernel()
        same_bytes({k: np.concatenate([ta[k], tb[k]]) for k in ta}, one, (first, second))
        same_bytes(snapshot(b), end, (first, second, "state"))
        a.close(); b.close()


# ---------------------------------------------------------------------------------------- 3. state and kernels
@pytest.mark.parametrize("stats", STATS_LEVELS)
def test_state_equals_the_external_run_and_old_kernels_stay(stats, step_kernel):
    """The same requests driven through `external` with the reference's actions -- another instantiation -- leave a byte-identical
    snapshot and identical other outputs; and the next launch under sap_ff on that handle reports its old kernel."""
    S, load, name = 320, 50, "any_mu"
    outs = RMSA_OUTS if stats != "counters" else tuple(o for o in RMSA_OUTS if "compactness" not in o)
    want = ref.stacked(S, load, name)
    actions = np.stack([want["act_path"], want["act_slot"]], axis=-1).astype(np.int32)   # [N, B, 2]
    make = lambda: make_env(S, load, step_kernel, stats_level=stats)
    ext = drive(make, [("external", 1, None, outs)] * N, actions=actions)
    env = make()
    got = one_step_launches(env, name, N, outs, auto_reset=True)
    assert env.last_kernel().split()[0] == usage_kernel(step_kernel, S, stats), env.last_kernel()
    snap = snapshot(env)
    env.run("sap_ff", 200, auto_reset=True)
    said = env.last_kernel()
    if step_kernel == "group":
        assert said.split()[0] == kernel_name("group", S, stats, defer=stats == "full"), said
        assert ("body=lean" in said) == (stats == "full"), said
    else:
        assert said.split()[0] == kernel_name("wave", S, stats, ff=True, defer=stats == "full"), said
    env.close()
    assert not set(ext["kernels"]) & {usage_kernel(step_kernel, S, stats)}, ext["said"][-1]
    same_bytes(got, ext["tr"], "outputs")
    same_bytes(snap, ext["snap"], "snapshot")
    decisions_hold(got, lambda i: {k: want[k][:, i] for k in DECIDED}, range(B), stats)


def test_old_rules_after_a_new_one(step_kernel, device_log_in_oracle):
    """40 steps of any_mu, then 40 each of sap_bf, sap_mc and sap_ff on the same handle: each reports the kernel it reported and
    decides what its reference decides on the state the launches before it left."""
    S, load, n, topo = 320, 50, 40, topology(NSF)
    env = make_env(S, load, step_kernel)
    parts, said = [], []
    for policy in ("any_mu", "sap_bf", "sap_mc", "sap_ff"):
        parts.append(env.run(policy, n, outputs=DECIDED, auto_reset=True))
        said.append(env.last_kernel().split()[0])
    env.close()
    assign = usage_kernel(step_kernel, S).replace(",true,false,true>", ",true>")
    assert said[0] == usage_kernel(step_kernel, S) and said[1] == assign and said[2] == assign.replace(",true>", ",true,true>"), said
    assert said[3] == (kernel_name("group", S, "full", defer=True) if step_kernel == "group" else kernel_name("wave", S, "full", ff=True, defer=True)), said
    from conftest import oracle_env_from_kwargs
    differs = 0
    for i in range(B):
        o = oracle_env_from_kwargs(topo, bcr.shape_kwargs(S, load), seed=ref.SEED0 + i)
        for t in range(4 * n):
            r, avail = o.request(), o.available_slots().copy()
            q = t // n
            mu = ref.propose(avail, topo, r.src, r.dst, r.bit_rate, "any", "most_used")
            p, s = (mu, ar.propose(avail, topo, r.src, r.dst, r.bit_rate, "sap", "best"),
                    cr.propose(avail, topo, r.src, r.dst, r.bit_rate, "sap")[:2],
                    ar.propose(avail, topo, r.src, r.dst, r.bit_rate, "sap", "first"))[q]
            acc = int(o.run("external", 1, reset_on_done=True, actions=np.array([[p, s]], np.int32), fields=["accepted"])["accepted"][0])
            got = parts[q]
            assert (got["act_path"][t % n, i], got["act_slot"][t % n, i], got["accepted"][t % n, i]) == (p, s, acc), (i, t)
            differs += q > 0 and (p, s) != mu
        o.close()
    assert differs >= 10   # the later launches are not the first one's rule


# ---------------------------------------------------------------------------------------- 4. with the blocking cause
@pytest.mark.parametrize("name", ["any_mu", "sap_mu", "any_bf"])
@pytest.mark.parametrize("S,load", [(64, 10), (320, 50)])
def test_with_the_blocking_cause(S, load, name, step_kernel):
    env = make_env(S, load, step_kernel)
    plain = env.run(name, N, outputs=RMSA_OUTS, auto_reset=True)
    env.close()
    env = make_env(S, load, step_kernel)
    tr = env.run(name, N, outputs=RMSA_OUTS + ("block_cause",), cause_counts=True, auto_reset=True)
    assert env.last_kernel().split()[0] == usage_kernel(step_kernel, S, cause=True), env.last_kernel()
    env.close()
    same_bytes({k: v for k, v in tr.items() if not k.startswith("block_cause")}, plain, "the outputs without the cause")
    want = ref.stacked(S, load, name)
    bad = np.argwhere(tr["block_cause"] != want["cause"])
    assert bad.size == 0, (name, bad[:6])
    assert np.array_equal(tr["block_cause_counts"], bcr.counts_of(want["cause"]))
    assert (tr["block_cause_counts"].sum(axis=1) == N).all()
    seen = np.bincount(tr["block_cause"].ravel(), minlength=8)
    assert seen[bcr.ACCEPTED] > 0 and seen[1:].sum() > 0, seen
    assert not seen[bcr.C_LAST_WINDOW:].any(), seen   # sap / any: cause <= alignment


# ---------------------------------------------------------------------------------------- 5. the queries
@pytest.mark.parametrize("S,load", ref.SHAPES)
def test_queries_before_every_step(S, load, step_kernel):
    """slot_usage and path_most_used before each of 200 one-step launches and after the last; they leave the state as it is."""
    name = "any_mu"
    env = make_env(S, load, step_kernel)
    runs = [ref.nsfnet_steps(S, load, name, i) for i in range(B)]
    for t in range(N + 1):
        before = env.save_state() if t % 50 == 0 else None
        U = env.slot_usage()
        usage, slots = env.path_most_used()
        if before is not None:
            assert np.array_equal(before, env.save_state())
            assert U.dtype == np.uint8 and U.shape == (B, S) and usage.dtype == np.int32 and slots.dtype == np.int16
            assert usage.shape == (B, 5) == slots.shape
            again = env.path_most_used(usage_out=np.zeros((B, 5), np.int32), slots_out=np.zeros((B, 5), np.int16))
            assert np.array_equal(again[0], usage) and np.array_equal(again[1], slots)
            assert np.array_equal(env.slot_usage(out=np.full((B, S), 77, np.uint8)), U)
        for i, w in enumerate(runs):
            assert np.array_equal(U[i], w["slot_usage"][t]), (t, i)
            assert np.array_equal(usage[i], w["mu_usage"][t]) and np.array_equal(slots[i], w["mu_slots"][t]), (t, i)
        assert ((usage == -1) == (slots == S)).all()
        if t < N:
            env.run(name, 1, auto_reset=True)
    env.close()
    assert (usage > 0).any()


def test_queries_into_pinned_and_device_buffers():
    """Pageable, pinned and device (torch) buffers, either one alone: the same bytes.  In a child process: torch has to create its
    HIP context before the library does."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys
        import numpy as np, torch
        torch.zeros(1, device="cuda")
        sys.path[:0] = [%r, %r]
        from conftest import load_topology
        from optical_rl_gym_amd import BatchedRMSAEnv
        env = BatchedRMSAEnv(load_topology("nsfnet_chen_5-paths_6-modulations"), 64, num_spectrum_resources=320, load=50,
                             mean_service_holding_time=25, episode_length=50, seed=10)
        env.run("sap_mu", 150, auto_reset=True)
        U = env.slot_usage()
        usage, slots = env.path_most_used()
        assert (usage > 0).any() and (usage == -1).any() and ((usage == -1) == (slots == 320)).all() and U.max() > 1
        pu = torch.full((64, 320), 77, dtype=torch.uint8).pin_memory()
        pc, ps = torch.full((64, 5), 77, dtype=torch.int32).pin_memory(), torch.full((64, 5), 77, dtype=torch.int16).pin_memory()
        env.slot_usage(out=pu)
        env.path_most_used(usage_out=pc, slots_out=ps)
        env.synchronize()
        assert pu.numpy().tobytes() == U.tobytes() and pc.numpy().tobytes() == usage.tobytes() and ps.numpy().tobytes() == slots.tobytes()
        du = torch.full((64, 320), 77, dtype=torch.uint8, device="cuda")
        dc, ds = torch.full((64, 5), 77, dtype=torch.int32, device="cuda"), torch.full((64, 5), 77, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        env.slot_usage(out=du)
        env.path_most_used(usage_out=dc, slots_out=ds)
        env.synchronize()
        assert du.cpu().numpy().tobytes() == U.tobytes()
        assert dc.cpu().numpy().tobytes() == usage.tobytes() and ds.cpu().numpy().tobytes() == slots.tobytes()
        only = np.full((64, 5), 77, np.int16)
        assert env.L.orlg_path_most_used(env.h, None, only.ctypes.data) == 0 and only.tobytes() == slots.tobytes()
        only = np.full((64, 5), 77, np.int32)
        assert env.L.orlg_path_most_used(env.h, only.ctypes.data, None) == 0 and only.tobytes() == usage.tobytes()
        env.close()
        print("usage buffers ok")
    """) % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "usage buffers ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------- 6. where the arithmetic can go wrong
def _path_links(topo, gid):
    return np.asarray(topo.path_links[topo.path_link_off[gid]:topo.path_link_off[gid + 1]], np.int64)


def _load_occupancy(env, avail):
    """avail [B, E, S] (1 = free) put in the place of the handle's occupancy through save_state / load_state: the occupancy words
    are found in the snapshot by their bytes (a fresh handle: every valid slot free)."""
    words = env.occupancy_words()
    state = env.save_state()
    at = state.tobytes().find(words.tobytes())
    assert at >= 0 and state.tobytes().find(words.tobytes(), at + 1) < 0, "the occupancy words were not found once in the snapshot"
    Bn, E, W = words.shape
    bits = np.zeros((Bn, E, 64 * W), np.uint8)
    bits[:, :, :avail.shape[2]] = avail
    new = np.packbits(bits, axis=-1, bitorder="little").view(np.uint64).reshape(Bn, E, W)
    state[at:at + words.nbytes] = np.frombuffer(new.tobytes(), np.uint8)
    env.load_state(state)
    assert np.array_equal(env.available_slots(), avail)


HAND_MADE = ("empty", "at0", "at_end", "straddle", "tie_words", "tie_paths", "all_but_path", "random")


def _hand_made(kind, topo, S, req, rng):
    """an availability array [E, S] for the pending request `req`, built around its first candidate path"""
    E = topo.num_links
    base = int(topo.pair_path_base[req["src"] * topo.num_nodes + req["dst"]])
    links0 = _path_links(topo, base)
    n0 = bcr.number_slots(int(req["bit_rate"]), int(topo.path_se[base]))
    others = np.setdiff1d(np.arange(E), np.unique(np.concatenate([_path_links(topo, base + p) for p in range(topo.k_paths)])))
    off_path0 = np.setdiff1d(np.arange(E), links0)
    avail = np.ones((E, S), np.uint8)
    if kind == "at0":
        avail[off_path0, :n0] = 0
    elif kind == "at_end":
        avail[off_path0, S - n0:] = 0
    elif kind == "straddle":
        avail[off_path0, 64 - n0 // 2:64 - n0 // 2 + n0] = 0
    elif kind == "tie_words":      # the same usage in word 0 and in word 1 (and a lower one further up): the lowest start
        use = others if others.size else off_path0[:1]
        avail[use[0], 20:20 + n0] = 0
        avail[use[0], 70:70 + n0] = 0
        avail[use[0], S - 1] = 0
    elif kind == "tie_paths":      # every slot used on the same number of links, every candidate path free: equal usage per slot
        avail[others, :] = 0
    elif kind == "all_but_path":   # one slot occupied on every link but the first path's
        avail[off_path0, 37] = 0
    elif kind == "random":
        avail = (rng.random((E, S)) > 0.12).astype(np.uint8)
        avail[links0, 5:5 + n0] = 1
    return avail


@pytest.mark.parametrize("name", ["any_mu", "sap_mu", "llp_mu", "any_bf", "any_ef", "any_lf", "any_ff_full"])
def test_hand_made_occupancies(name, step_kernel):
    """Occupancies built around the pending request of each environment and loaded through load_state: one step and both queries
    against the reference, and the reference says that the cases were met."""
    S, topo = 100, topology(NSF)
    route, rule = ref.NAMES[name]
    rng = np.random.default_rng(11)
    env = make_env(S, 20, step_kernel, batch=len(HAND_MADE))
    reqs = env.requests()
    avail = np.stack([_hand_made(kind, topo, S, reqs[i], rng) for i, kind in enumerate(HAND_MADE)])
    _load_occupancy(env, avail)
    U = env.slot_usage()
    usage, slots = env.path_most_used()
    tr = env.run(name, 1, outputs=DECIDED)
    assert env.last_kernel().split()[0] == usage_kernel(step_kernel, S), env.last_kernel()
    env.close()
    met = {}
    for i, kind in enumerate(HAND_MADE):
        src, dst, br = int(reqs[i]["src"]), int(reqs[i]["dst"]), int(reqs[i]["bit_rate"])
        assert np.array_equal(U[i], ref.slot_usage(avail[i])), kind
        wu, ws = ref.path_most_used(avail[i], topo, src, dst, br)
        assert np.array_equal(usage[i], wu) and np.array_equal(slots[i], ws), (kind, usage[i], wu, slots[i], ws)
        p, s = ref.propose(avail[i], topo, src, dst, br, route, rule)
        assert (tr["act_path"][0, i], tr["act_slot"][0, i], tr["accepted"][0, i]) == (p, s, int(p < topo.k_paths)), (kind, p, s)
        n0 = ref.candidates(avail[i], topo, src, dst, br)[0][1]
        met[kind] = {"empty": (wu == 0).all() and (ws == 0).all(), "at0": ws[0] == 0 and wu[0] > 0, "at_end": ws[0] == S - n0 and wu[0] > 0,
                     "straddle": ws[0] < 64 < ws[0] + n0 and wu[0] > 0, "tie_words": ws[0] == 20 and wu[0] == n0,
                     "tie_paths": (wu >= 0).sum() >= 2 and len(set((wu[wu >= 0] // np.maximum(1, [c[1] for c in ref.candidates(avail[i], topo, src, dst, br)])[wu >= 0]).tolist())) == 1,
                     "all_but_path": wu[0] == topo.num_links - len(_path_links(topo, int(topo.pair_path_base[src * topo.num_nodes + dst]))) and ws[0] <= 37 < ws[0] + n0,
                     "random": True}[kind]
    assert all(met.values()), met


def test_windows_of_more_than_a_word(step_kernel, device_log_in_oracle):
    """bit rate 1000 at spectral efficiency 1 is 81 slots: a window's sum reaches two words on."""
    kw = dict(num_spectrum_resources=320, load=30, mean_service_holding_time=25, episode_length=50, seed=ref.SEED0,
              bit_rates=[100, 1000])
    topo = topology(NSF)
    env = rmsa_env(NSF, 4, step_kernel, **kw)
    tr = env.run("any_mu", N, outputs=DECIDED, auto_reset=True)
    usage, slots = env.path_most_used()
    U = env.slot_usage()
    env.close()
    runs = [ref.oracle_steps(topo, kw, ref.SEED0 + i, "any_mu", N) for i in range(4)]
    decisions_hold(tr, lambda i: runs[i], range(4), "long windows")
    for i in range(4):
        assert np.array_equal(usage[i], runs[i]["mu_usage"][N]) and np.array_equal(slots[i], runs[i]["mu_slots"][N])
        assert np.array_equal(U[i], runs[i]["slot_usage"][N])
    assert max(int(r["n_slots"][r["accepted"] == 1].max()) for r in runs) >= 64
    assert sum(int(((r["n_slots"] >= 64) & (r["usage"] > 0)).sum()) for r in runs) > 0


# ---------------------------------------------------------------------------------------- 7. large shapes
LARGE_NAMES = ("sap_mu", "any_mu", "any_bf")
LARGE_N = 100


def large_shape_holds(topo, kw, kernel, seed0, batch, what, names=LARGE_NAMES):
    out = {}
    for name in names:
        env = rmsa_env(topo, batch, kernel, **kw)
        tr = env.run(name, LARGE_N, outputs=DECIDED, auto_reset=True)
        assert env.last_kernel().split()[0] == usage_kernel(kernel, kw["num_spectrum_resources"]), env.last_kernel()
        usage, slots = env.path_most_used()
        U = env.slot_usage()
        env.close()
        runs = [ref.oracle_steps(topo, kw, seed0 + i, name, LARGE_N) for i in range(batch)]
        decisions_hold(tr, lambda i: runs[i], range(batch), (what, name))
        for i in range(batch):
            assert np.array_equal(U[i], runs[i]["slot_usage"][LARGE_N]), (what, i)
            assert np.array_equal(usage[i], runs[i]["mu_usage"][LARGE_N]) and np.array_equal(slots[i], runs[i]["mu_slots"][LARGE_N]), (what, i)
        assert (tr["accepted"] == 1).any()
        out[name] = runs
    return out


@pytest.mark.parametrize("name,kernel", [("g3x3_k9_s64", "wave"), ("g3x3_k9_s64", "group"), ("g4x4_k12_s320", "wave"),
                                         ("g4x4_k12_s320", "group")])
def test_more_than_eight_paths(name, kernel, tmp_path, device_log_in_oracle):
    """k = 9 and 12: more than one pass of eight paths in the wave kernel, several passes per row in the group kernel; and on an
    empty network every path proposes the same window: the lowest path wins over the pass boundary."""
    topo, kw = many_paths_topology(name, tmp_path), many_paths_kwargs(name)
    runs = large_shape_holds(topo, kw, kernel, MANY_PATHS_SEED, 6, name)
    assert max(int(r["act_path"][r["accepted"] == 1].max()) for r in runs["any_mu"]) >= 8   # a path of the second pass is chosen
    env = rmsa_env(topo, 6, kernel, **kw)
    reqs = env.requests()
    S, E = kw["num_spectrum_resources"], topo.num_links
    # every link used on slot 0, except the links of paths 8 .. k - 1: the first eight paths have equal proposals at slot 1 or
    # none better than the later ones'; the reference decides, and some environment's winner ties with a path of the other pass
    avail = np.ones((6, E, S), np.uint8)
    ties = 0
    for i in range(6):
        base = int(topo.pair_path_base[int(reqs[i]["src"]) * topo.num_nodes + int(reqs[i]["dst"])])
        late = np.unique(np.concatenate([_path_links(topo, base + p) for p in range(8, topo.k_paths)]))
        avail[i, np.setdiff1d(np.arange(E), late), :] = 0   # only paths made of the late paths' links keep a window
    _load_occupancy(env, avail)
    usage, slots = env.path_most_used()
    tr = env.run("any_mu", 1, outputs=DECIDED)
    env.close()
    for i in range(6):
        src, dst, br = int(reqs[i]["src"]), int(reqs[i]["dst"]), int(reqs[i]["bit_rate"])
        wu, ws = ref.path_most_used(avail[i], topo, src, dst, br)
        assert np.array_equal(usage[i], wu) and np.array_equal(slots[i], ws), i
        p, s = ref.propose(avail[i], topo, src, dst, br, "any", "most_used")
        assert (tr["act_path"][0, i], tr["act_slot"][0, i]) == (p, s), i
        ties += int(p >= 8 or (p < topo.k_paths and (wu[8:] == wu[p]).any()))
    assert ties >= 1


@pytest.mark.parametrize("name,S,load", [(RING34, 100, 60), (RING36, 100, 60), (NSF, 448, 80), (NSF, 512, 90)])
def test_many_links_hops_and_words(name, S, load, step_kernel, device_log_in_oracle):
    """238 links (E above 32, counts above 127 in a byte counter); seven words on the eight-word layout (S = 448) and eight words;
    usage above 16 bits needs many links AND many slots: asked of the query where the rings meet it."""
    kw = dict(num_spectrum_resources=S, load=load, mean_service_holding_time=25, episode_length=200, seed=5)
    topo = topology(name)
    runs = large_shape_holds(topo, kw, step_kernel, 5, 3, (name, S, step_kernel), names=("sap_mu", "any_mu"))
    if topo.num_links > 32:
        assert max(int(r["slot_usage"].max()) for r in runs["any_mu"]) > 32


def test_usage_above_sixteen_bits(step_kernel):
    """The 34-node ring's 238 links all used on every slot but for the first path's links: a window of 300 slots (bit rate 7475 at
    spectral efficiency 2) has the usage 300 x (238 - hops) > 65 535."""
    topo, S, batch = topology(RING34), 512, 4
    env = rmsa_env(topo, batch, step_kernel, num_spectrum_resources=S, load=20, mean_service_holding_time=25, episode_length=200, seed=5,
                   bit_rates=[7475])
    reqs = env.requests()
    E = topo.num_links
    avail = np.ones((batch, E, S), np.uint8)
    for i in range(batch):
        base = int(topo.pair_path_base[int(reqs[i]["src"]) * topo.num_nodes + int(reqs[i]["dst"])])
        avail[i, np.setdiff1d(np.arange(E), _path_links(topo, base)), :] = 0
    _load_occupancy(env, avail)
    U = env.slot_usage()
    usage, slots = env.path_most_used()
    tr = env.run("any_mu", 1, outputs=DECIDED)
    env.close()
    for i in range(batch):
        src, dst, br = int(reqs[i]["src"]), int(reqs[i]["dst"]), int(reqs[i]["bit_rate"])
        assert np.array_equal(U[i], ref.slot_usage(avail[i])), i
        wu, ws = ref.path_most_used(avail[i], topo, src, dst, br)
        assert np.array_equal(usage[i], wu) and np.array_equal(slots[i], ws), (i, usage[i], wu)
        assert (tr["act_path"][0, i], tr["act_slot"][0, i]) == ref.propose(avail[i], topo, src, dst, br, "any", "most_used"), i
    assert usage.max() > 65535 and U.max() > 127


def test_paths_of_fourteen_hops(step_kernel, device_log_in_oracle):
    """The routes seldom take the longest paths of the 36-node ring: an agent names them."""
    topo = topology(RING36)
    kw = dict(num_spectrum_resources=100, load=20, mean_service_holding_time=25, episode_length=200, seed=5)
    paths = np.random.default_rng(7).integers(0, topo.k_paths, (LARGE_N, 3)).astype(np.int32)
    env = rmsa_env(topo, 3, step_kernel, **kw)
    tr = one_step_launches(env, "path_mu_external", LARGE_N, DECIDED, actions=paths, auto_reset=True)
    env.close()
    runs = [ref.oracle_steps(topo, kw, 5 + i, "path_mu_external", LARGE_N, paths=paths[:, i]) for i in range(3)]
    decisions_hold(tr, lambda i: runs[i], range(3), "14 hops")
    hops = np.asarray(topo.path_hops)
    assert hops.max() == 14 and sum(int(((r["accepted"] == 1) & (r["usage"] > 0)).sum()) for r in runs) >= 1


# ---------------------------------------------------------------------------------------- 8. other handles, batch sizes
def test_sweep_handle_on_the_group_kernel():
    from optical_rl_gym_amd import make_sweep
    loads, seeds, S = (10.0, 20.0), 4, 100
    env = make_sweep("rmsa", topology(NSF), loads=loads, seeds_per_load=seeds, seed=ref.SEED0, step_kernel="group",
                     num_spectrum_resources=S, mean_service_holding_time=25, episode_length=50)
    tr = env.run("any_mu", N, outputs=DECIDED + ("block_cause",), cause_counts=True, auto_reset=True)
    assert env.last_kernel().split()[0] == usage_kernel("group", S, cause=True, traffic=True), env.last_kernel()
    tr2 = env.run("sap_mu", 50, outputs=DECIDED, auto_reset=True)
    assert env.last_kernel().split()[0] == usage_kernel("group", S, traffic=True), env.last_kernel()
    batch, env_loads = env.batch_size, [float(x) for x in env.loads]
    env.close()
    assert tr2["accepted"].shape == (50, batch)
    decisions_hold(tr, lambda i: ref.nsfnet_steps(S, env_loads[i], "any_mu", i % seeds), range(batch), "sweep")
    for i in range(batch):
        assert np.array_equal(tr["block_cause"][:, i], ref.nsfnet_steps(S, env_loads[i], "any_mu", i % seeds)["cause"]), i
    assert np.array_equal(tr["block_cause_counts"], bcr.counts_of(tr["block_cause"]))


def test_trace_handle_on_the_group_kernel():
    from optical_rl_gym_amd import record_trace
    S, load = 100, 20
    gen = make_env(S, load, "group")
    trace = record_trace(gen, "sap_mu", N, auto_reset=True)
    assert gen.last_kernel().split()[0] == usage_kernel("group", S), gen.last_kernel()
    gen.close()
    env = rmsa_env(NSF, B, "group", trace=trace, num_spectrum_resources=S, episode_length=50)
    tr = env.run("sap_mu", N, outputs=DECIDED, auto_reset=True)
    assert env.last_kernel().split()[0] == usage_kernel("group", S, trace=True), env.last_kernel()
    env.close()
    decisions_hold(tr, lambda i: ref.nsfnet_steps(S, load, "sap_mu", i), range(B), "trace")


def test_partial_quad(step_kernel):
    S, load = 64, 10
    env = make_env(S, load, step_kernel, batch=5)
    tr = env.run("llp_mu", N, outputs=DECIDED, auto_reset=True)
    U = env.slot_usage()
    env.close()
    decisions_hold(tr, lambda i: ref.nsfnet_steps(S, load, "llp_mu", i), range(5), "B=5")
    for i in range(5):
        assert np.array_equal(U[i], ref.nsfnet_steps(S, load, "llp_mu", i)["slot_usage"][N]), i


def test_large_batch_on_tickets(step_kernel, device_log_in_oracle):
    """B = 4100 x 50 steps: several rounds, environments handed out by the ticket counter; the first and the last four
    environments against the reference."""
    S, load, batch, n = 100, 20, 4100, 50
    env = make_env(S, load, step_kernel, batch=batch)
    tr = env.run("any_mu", n, outputs=DECIDED, auto_reset=True)
    assert env.last_kernel().split()[0] == usage_kernel(step_kernel, S), env.last_kernel()
    usage, slots = env.path_most_used()
    env.close()
    topo = topology(NSF)
    runs = {i: ref.oracle_steps(topo, bcr.shape_kwargs(S, load), ref.SEED0 + i, "any_mu", n)
            for i in [0, 1, 2, 3, batch - 4, batch - 3, batch - 2, batch - 1]}
    decisions_hold(tr, lambda i: runs[i], list(runs), "B=4100")
    for i, r in runs.items():
        assert np.array_equal(usage[i], r["mu_usage"][n]) and np.array_equal(slots[i], r["mu_slots"][n]), i
    assert ((tr["act_path"] == 5) == (tr["accepted"] == 0)).all()


# ---------------------------------------------------------------------------------------- 9. refusals on the device side
def _step_window(env, route, rule, n_steps=10, actions=None):
    ap = None if actions is None else actions.ctypes.data_as(C.c_void_p)
    rc = env.L.orlg_step_window(env.h, route, rule, n_steps, ap, 1, None, None)
    return rc, env.L.orlg_last_error().decode()


def test_the_library_refuses_before_it_launches(step_kernel):
    from optical_rl_gym_amd import _lib
    P, MU, BW = _lib.POLICIES, _lib.RULE_MOST_USED, _lib.ROUTE_BEST_WINDOW
    env = make_env(100, 20, step_kernel, batch=4)
    env.run("sap_ff", 20, auto_reset=True)
    before, said = snapshot(env), env.last_kernel()
    acts = np.zeros((4, 2), np.int32)
    for policy, n, a in (("external", 1, acts), ("deeprmsa_sp_ff", 10, None), ("deeprmsa_sap_ff", 10, None),
                         ("deeprmsa_external", 1, acts[:, 0].copy()), ("sap_ff_gn", 10, None)):
        rc, msg = _step_window(env, P[policy], MU, n, a)
        assert rc == -1 and "route" in msg, (policy, rc, msg)
    for route in (-2, 8, 9, 99, 100, 102):   # unknown routes, the device's own values and the fewest-cuts route among them
        rc, msg = _step_window(env, route, MU)
        assert rc == -1 and "route" in msg, (route, rc, msg)
    for rule in (0, 5, 6, 99, 101, -1):      # ORLG_ASSIGN_FIRST, the device's own values, unknown ones
        for route in (P["sap_ff"], BW):
            rc, msg = _step_window(env, route, rule)
            assert rc == -1 and "rule" in msg, (route, rule, rc, msg)
    # no other entry point knows the two values
    assert env.L.orlg_step_assign(env.h, P["sap_ff"], MU, 10, None, 1, None, None) == -1
    assert env.L.orlg_step_assign(env.h, BW, 1, 10, None, 1, None, None) == -1 and env.L.orlg_step_assign(env.h, 9, 1, 10, None, 1, None, None) == -1
    assert env.L.orlg_step_assign(env.h, P["sap_ff"], 6, 10, None, 1, None, None) == -1
    assert env.L.orlg_step_min_cut(env.h, BW, 10, None, 1, None, None) == -1 and env.L.orlg_step(env.h, BW, 10, None, 1, None) == -1
    assert env.L.orlg_slot_usage(env.h, None) == -1 and env.L.orlg_path_most_used(env.h, None, None) == -1
    assert env.last_kernel() == said
    same_bytes(snapshot(env), before, "nothing ran")
    # a pair orlg_step_assign serves is orlg_step_assign: the ASSIGN instantiation
    rc, msg = _step_window(env, P["sap_ff"], 3, 20)
    assert rc == 0, msg
    assert env.last_kernel().split()[0] == usage_kernel(step_kernel, 100).replace(",true,false,true>", ",true>"), env.last_kernel()
    rc, msg = _step_window(env, BW, MU, 20)
    assert rc == 0, msg
    assert env.last_kernel().split()[0] == usage_kernel(step_kernel, 100), env.last_kernel()
    env.close()


def test_a_gated_handle_is_refused():
    from optical_rl_gym_amd import _lib
    case = "nsfnet_s320_l150_sapff"
    topo, kw, _ = ggr.resolve_case(case)
    env = rmsa_env(topo, 4, gn_gate=ggr.case_gate(topo), **kw)
    before = snapshot(env)
    for route, rule in ((0, 100), (1, 100), (2, 100), (_lib.ROUTE_BEST_WINDOW, 100), (_lib.ROUTE_BEST_WINDOW, 1), (1, 3)):
        rc, msg = _step_window(env, route, rule)
        assert rc == -1 and "gn_gate" in msg, (route, rule, rc, msg)
    rc, msg = _step_window(env, 6, 100, 1, np.zeros(4, np.int32))
    assert rc == -1 and "gn_gate" in msg, (rc, msg)
    with pytest.raises(ValueError, match="gn_gate"):
        env.run("any_mu", 10)
    same_bytes(snapshot(env), before, "nothing ran")
    env.close()


# ---------------------------------------------------------------------------------------- 10. the drop-in surface
@pytest.mark.parametrize("name", ["sap_mu", "any_mu", "any_bf"])
def test_view_callback_equals_the_device_policy(name, step_kernel):
    import optical_rl_gym_amd as pkg
    kw = dict(num_spectrum_resources=100, load=20, mean_service_holding_time=25, episode_length=200, seed=10)
    dev = rmsa_env(NSF, 1, step_kernel, **kw)
    tr = dev.run(name, 100, outputs=DECIDED)
    dev.close()
    view = pkg.make("RMSA-v0", topology=topology(NSF), **kw)
    heuristic = pkg.window_heuristic(*ref.NAMES[name])
    for t in range(100):
        a = heuristic(view)
        assert tuple(a) == (tr["act_path"][t, 0], tr["act_slot"][t, 0]), t
        served = view.current_service
        view.step(a)
        assert served.accepted == bool(tr["accepted"][t, 0]), t
    view.close()
