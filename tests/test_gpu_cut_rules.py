"""The fewest-cuts window on the device (``include/orlg.h`` ``orlg_step_min_cut`` / ``orlg_path_min_cuts``): the rule
MIN_CUT on the routes sp / sap / llp, on an agent's path and on the route "fewest cuts", against the numpy restatement of the
definitions driving the oracle with external actions, one step at a time (``cut_reference.py``; ``test_cut_rules.py`` holds that
module to brute force and shows that the rule differs from first fit and best fit on these shapes).  Both step kernels, every
kind of handle, every launch shape, with and without the blocking cause, the query; and that a launch under an old policy name
runs the kernel it ran.  Integer-exact: no tolerance anywhere.

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
import cut_reference as ref
import gn_gate_reference as ggr
from gpu_support import (MANY_PATHS_SEED, RMSA_OUTS, STATS_LEVELS, device_log_fixture, drive, external_actions, kernel_name,  # noqa: F401
                         many_paths_kwargs, many_paths_topology, one_step_launches, rmsa_env, same_bytes, snapshot, step_kernel,
                         tooling_env, topology)

pytestmark = pytest.mark.gpu

NSF = ref.NSFNET
RING34, RING36 = "ring34_3-paths_6-modulations", "ring36_3-paths_6-modulations"
B, N = ref.N_ENVS, ref.N_STEPS
DECIDED = ("act_path", "act_slot", "accepted")


def assign_kernel(kernel, S, stats="full", cause=False, traffic=False, trace=False):
    """The instantiation a launch under the rule reports: the plain kind of either kernel with the ASSIGN and the CUT
    flag last."""
    W = (S + 63) // 64
    W, level = 8 if W == 7 else W, STATS_LEVELS.index(stats)
    t = lambda flag: str(bool(flag)).lower()
    if kernel == "group":
        return f"orlg_rmsa_group_kernel<{W},{level},false,false,{t(traffic)},{t(trace)},{t(cause)},true,true>"
    return f"orlg_rmsa_kernel<{W},{level},false,false,{t(cause)},true,true>"


def make_env(S, load, kernel, batch=B, **kw):
    return rmsa_env(NSF, batch, kernel, **bcr.shape_kwargs(S, load, **kw))


def decisions_hold(tr, want, envs, what):
    """act_path, act_slot, accepted of environment i (column i of tr) equal the reference run want(i), step by step"""
    for i in envs:
        w = want(i)
        for k in DECIDED:
            bad = np.flatnonzero(tr[k][:, i] != w[k][:len(tr[k])])
            assert bad.size == 0, (what, i, k, bad[:6], tr[k][bad[:6], i], w[k][bad[:6]])


def path_actions(topo, S):
    """random paths that include k and values out of range on either side"""
    actions = external_actions(topo, S, N, B, kind="paths")
    actions[5::17] = -1
    actions[7::19] = topo.k_paths + 3
    actions[3::23] = topo.k_paths
    return actions


# ---------------------------------------------------------------------------------------- 1. one launch, against the reference
@pytest.mark.parametrize("route", ref.ROUTES)
@pytest.mark.parametrize("S,load", ref.SHAPES)
def test_one_launch_against_the_reference(S, load, route, step_kernel):
    """W = 1, 2 and 5: the neighbours of a window cross word boundaries, and S = 100 is a last word that is not full."""
    env = make_env(S, load, step_kernel)
    tr = env.run(ref.POLICY[route], N, outputs=DECIDED, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel(step_kernel, S), env.last_kernel()
    env.close()
    assert tr["act_slot"].shape == (N, B)
    decisions_hold(tr, lambda i: ref.nsfnet_steps(S, load, route, i), range(B), (S, route, step_kernel))
    want = ref.stacked(S, load, route)   # (what test_cut_rules.py shows of the reference: the comparison is not one of first or best fits)
    d_ff = (tr["act_slot"] != want["ff_slot"]) | (tr["act_path"] != want["ff_path"])
    d_bf = (tr["act_slot"] != want["bf_slot"]) | (tr["act_path"] != want["bf_path"])
    assert (d_ff & d_bf).sum(axis=0).min() >= 10


@pytest.mark.parametrize("S,load", ref.SHAPES)
def test_path_only_actions(S, load, step_kernel, device_log_in_oracle):
    topo = topology(NSF)
    actions = path_actions(topo, S)
    env = make_env(S, load, step_kernel)
    tr = one_step_launches(env, "path_mc_external", N, DECIDED, actions=actions, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel(step_kernel, S), env.last_kernel()
    env.close()
    runs = {}

    def want(i):
        if i not in runs:
            runs[i] = ref.oracle_steps(topo, bcr.shape_kwargs(S, load), ref.SEED0 + i, "path", N, paths=actions[:, i])
        return runs[i]

    decisions_hold(tr, want, range(B), S)
    assert (tr["act_path"] == topo.k_paths).any() and (tr["accepted"] == 1).any()
    assert ((tr["act_path"] == topo.k_paths) == (tr["act_slot"] == S)).all()


# ---------------------------------------------------------------------------------------- 2. every launch shape, the same bits
@pytest.mark.parametrize("policy", ["min_cut", "llp_mc"])
def test_launch_shapes_give_the_same_bits(policy, step_kernel):
    S, load = 100, 20
    env = make_env(S, load, step_kernel)
    one = env.run(policy, N, outputs=RMSA_OUTS, auto_reset=True)
    env.close()
    env = make_env(S, load, step_kernel)
    steps = one_step_launches(env, policy, N, RMSA_OUTS, auto_reset=True)
    # (a launch of one step asks the group kernel's plan for the queue in HBM: a launch under the rule stays on the plain kind)
    assert env.last_kernel().split()[0] == assign_kernel(step_kernel, S), env.last_kernel()
    env.close()
    same_bytes(steps, one, "one-step launches")
    if step_kernel == "group":   # tickets in chunks of steps: successive chunks of a quad may run on different waves
        with tooling_env(ORLG_GROUP_CHUNKS="7"):
            env = make_env(S, load, "group")
            chunks = env.run(policy, N, outputs=RMSA_OUTS, auto_reset=True)
            assert "chunks=7" in env.last_kernel() and env.last_kernel().split()[0] == assign_kernel("group", S), env.last_kernel()
            env.close()
        same_bytes(chunks, one, "chunks")


# ---------------------------------------------------------------------------------------- 3. state and kernels
@pytest.mark.parametrize("stats", STATS_LEVELS)
def test_state_equals_the_external_run_and_old_kernels_stay(stats, step_kernel):
    """The same requests driven through `external` with the reference's actions -- another instantiation -- leave a byte-identical
    snapshot and identical other outputs; and the next launch under sap_ff on that handle reports its old kernel."""
    S, load, route = 320, 50, "min_cut"
    outs = RMSA_OUTS if stats != "counters" else tuple(o for o in RMSA_OUTS if "compactness" not in o)
    want = ref.stacked(S, load, route)
    actions = np.stack([want["act_path"], want["act_slot"]], axis=-1).astype(np.int32)   # [N, B, 2]
    make = lambda: make_env(S, load, step_kernel, stats_level=stats)
    ext = drive(make, [("external", 1, None, outs)] * N, actions=actions)
    env = make()
    got = one_step_launches(env, ref.POLICY[route], N, outs, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel(step_kernel, S, stats), env.last_kernel()
    snap = snapshot(env)
    env.run("sap_ff", 200, auto_reset=True)
    said = env.last_kernel()
    if step_kernel == "group":
        assert said.split()[0] == kernel_name("group", S, stats, defer=stats == "full"), said
        assert ("body=lean" in said) == (stats == "full"), said
    else:
        assert said.split()[0] == kernel_name("wave", S, stats, ff=True, defer=stats == "full"), said
    env.close()
    assert not set(ext["kernels"]) & {assign_kernel(step_kernel, S, stats)}, ext["said"][-1]
    same_bytes(got, ext["tr"], "outputs")
    same_bytes(snap, ext["snap"], "snapshot")
    decisions_hold(got, lambda i: {k: want[k][:, i] for k in DECIDED}, range(B), stats)


def test_a_classic_rule_after_the_cut_rule(step_kernel, device_log_in_oracle):
    """50 steps of sap_mc, then 50 of sap_bf on the same handle: sap_bf reports the kernel it reported and decides what the
    reference's best fit decides on the state the fewest-cuts windows left."""
    S, load, n, topo = 320, 50, 50, topology(NSF)
    env = make_env(S, load, step_kernel)
    first = env.run("sap_mc", n, outputs=DECIDED, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel(step_kernel, S), env.last_kernel()
    tr = env.run("sap_bf", n, outputs=DECIDED, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel(step_kernel, S).replace(",true,true>", ",true>"), env.last_kernel()   # the ASSIGN instantiation
    env.close()
    from conftest import oracle_env_from_kwargs
    differs = 0
    for i in range(B):
        o = oracle_env_from_kwargs(topo, bcr.shape_kwargs(S, load), seed=ref.SEED0 + i)
        for t in range(2 * n):
            r, avail = o.request(), o.available_slots().copy()
            p, s = ref.propose(avail, topo, r.src, r.dst, r.bit_rate, "sap")[:2] if t < n else \
                ar.propose(avail, topo, r.src, r.dst, r.bit_rate, "sap", "best")
            acc = int(o.run("external", 1, reset_on_done=True, actions=np.array([[p, s]], np.int32), fields=["accepted"])["accepted"][0])
            got = first if t < n else tr
            assert (got["act_path"][t % n, i], got["act_slot"][t % n, i], got["accepted"][t % n, i]) == (p, s, acc), (i, t)
            if t >= n:
                differs += (p, s) != ref.propose(avail, topo, r.src, r.dst, r.bit_rate, "sap")[:2]
        o.close()
    assert differs >= 10   # the second launch is not the first one's rule


# ---------------------------------------------------------------------------------------- 4. with the blocking cause
@pytest.mark.parametrize("route", ["sap", "min_cut", "sp"])
@pytest.mark.parametrize("S,load", [(64, 10), (320, 50)])
def test_with_the_blocking_cause(S, load, route, step_kernel):
    policy = ref.POLICY[route]
    env = make_env(S, load, step_kernel)
    plain = env.run(policy, N, outputs=RMSA_OUTS, auto_reset=True)
    env.close()
    env = make_env(S, load, step_kernel)
    tr = env.run(policy, N, outputs=RMSA_OUTS + ("block_cause",), cause_counts=True, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel(step_kernel, S, cause=True), env.last_kernel()
    env.close()
    same_bytes({k: v for k, v in tr.items() if not k.startswith("block_cause")}, plain, "the outputs without the cause")
    want = ref.stacked(S, load, route)
    bad = np.argwhere(tr["block_cause"] != want["cause"])
    assert bad.size == 0, (policy, bad[:6])
    assert np.array_equal(tr["block_cause_counts"], bcr.counts_of(want["cause"]))
    assert (tr["block_cause_counts"].sum(axis=1) == N).all()
    seen = np.bincount(tr["block_cause"].ravel(), minlength=8)
    assert seen[bcr.ACCEPTED] > 0 and seen[1:].sum() > 0, seen
    if route != "sp":
        assert not seen[bcr.C_LAST_WINDOW:].any(), seen   # sap / fewest-cuts: cause <= alignment


# ---------------------------------------------------------------------------------------- 5. the query
@pytest.mark.parametrize("S,load", ref.SHAPES)
def test_path_min_cuts_equals_the_reference(S, load, step_kernel):
    """After 0, 50 and 200 steps; the query leaves the state as it is."""
    route = "sap"
    env = make_env(S, load, step_kernel)
    done = 0
    for upto in (0, 50, 200):
        if upto > done:
            env.run(ref.POLICY[route], upto - done, auto_reset=True)
            done = upto
        before = env.save_state()
        cuts, slots = env.path_min_cuts()
        assert cuts.dtype == np.int16 and slots.dtype == np.int16 and cuts.shape == (B, 5) == slots.shape
        again = env.path_min_cuts(cuts_out=np.zeros((B, 5), np.int16), slots_out=np.zeros((B, 5), np.int16))
        assert np.array_equal(before, env.save_state())
        assert np.array_equal(again[0], cuts) and np.array_equal(again[1], slots)
        for i in range(B):
            w = ref.nsfnet_steps(S, load, route, i)
            assert np.array_equal(cuts[i], w["min_cuts"][upto]) and np.array_equal(slots[i], w["min_slots"][upto]), (upto, i)
        assert ((cuts == -1) == (slots == S)).all()
    env.close()
    assert (cuts > 0).any() or S == 64


def test_path_min_cuts_into_pinned_and_device_buffers():
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
        env.run("sap_mc", 150, auto_reset=True)
        cuts, slots = env.path_min_cuts()
        assert (cuts > 0).any() and (cuts == -1).any() and ((cuts == -1) == (slots == 320)).all()
        pc, ps = (torch.full((64, 5), 77, dtype=torch.int16).pin_memory() for _ in range(2))
        env.path_min_cuts(cuts_out=pc, slots_out=ps)
        env.synchronize()
        assert pc.numpy().tobytes() == cuts.tobytes() and ps.numpy().tobytes() == slots.tobytes()
        dc, ds = (torch.full((64, 5), 77, dtype=torch.int16, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        env.path_min_cuts(cuts_out=dc, slots_out=ds)
        env.synchronize()
        assert dc.cpu().numpy().tobytes() == cuts.tobytes() and ds.cpu().numpy().tobytes() == slots.tobytes()
        only = np.full((64, 5), 77, np.int16)
        assert env.L.orlg_path_min_cuts(env.h, None, only.ctypes.data) == 0 and only.tobytes() == slots.tobytes()
        only[:] = 77
        assert env.L.orlg_path_min_cuts(env.h, only.ctypes.data, None) == 0 and only.tobytes() == cuts.tobytes()
        env.close()
        print("min cuts buffers ok")
    """) % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "min cuts buffers ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------- 6. where the arithmetic can go wrong
def test_where_the_arithmetic_can_go_wrong(step_kernel):
    """The device's outputs (held to the reference above and here) met every case that the lanes' words make special: a left
    neighbour in the previous word, a right neighbour in the next word, the spectrum's two ends, a window preferred to a lower
    one for its cuts, chosen paths of one hop, and -- the routes never take the topology's longest paths here -- windows on paths
    of the longest hop count in the device's own path_min_cuts, asked at the steps where the reference says some environment's
    pending request has one."""
    S, load, topo = 320, 50, topology(NSF)
    met = dict(left_prev_word=0, right_next_word=0, at0=0, at_end=0, fewer_than_lowest=0, one_hop=0, longest_window=0)
    longest = int(np.max(topo.path_hops))

    def longest_paths(w, t):   # [k] bool: the candidate paths of environment w's request pending before step t with the most hops
        src, dst = w["request"][t, :2]
        base = int(topo.pair_path_base[src * topo.num_nodes + dst])
        return np.asarray(topo.path_hops[base:base + topo.k_paths]) == longest

    for route in ("sap", "min_cut"):
        runs = [ref.nsfnet_steps(S, load, route, i) for i in range(B)]
        stops = sorted({t for w in runs for t in range(N) if (longest_paths(w, t) & (w["min_cuts"][t] >= 0)).any()})[:4]
        env = make_env(S, load, step_kernel)
        parts, done = [], 0
        for t in stops + [N]:
            if t > done:
                parts.append(env.run(ref.POLICY[route], t - done, outputs=DECIDED, auto_reset=True))
                done = t
            cuts, slots = env.path_min_cuts()
            for i, w in enumerate(runs):
                assert np.array_equal(cuts[i], w["min_cuts"][t]) and np.array_equal(slots[i], w["min_slots"][t]), (route, t, i)
                if t < N:
                    met["longest_window"] += int((longest_paths(w, t) & (cuts[i] >= 0)).sum())
        env.close()
        tr = {k: np.concatenate([p[k] for p in parts]) for k in DECIDED}
        decisions_hold(tr, lambda i: runs[i], range(B), route)
        want = ref.stacked(S, load, route)
        acc = tr["accepted"] == 1
        s, n = tr["act_slot"], want["n_slots"]
        met["left_prev_word"] += int((acc & (s % 64 == 0) & (s > 0)).sum())
        met["right_next_word"] += int((acc & ((s + n) // 64 > s // 64) & (s + n < S)).sum())
        met["at0"] += int((acc & (s == 0)).sum())
        met["at_end"] += int((acc & (s == S - n)).sum())
        met["fewer_than_lowest"] += int((acc & (want["cuts"] > 0) & (want["lowest_cuts"] > want["cuts"])).sum())
        met["one_hop"] += int((acc & (want["hops"] == 1)).sum())
    print(met)
    assert all(v > 0 for v in met.values()), met


# ---------------------------------------------------------------------------------------- 7. large shapes, long windows
LARGE_ROUTES = ("sap", "min_cut")
LARGE_N = 100


def large_shape_holds(topo, kw, kernel, seed0, batch, what):
    for route in LARGE_ROUTES:
        env = rmsa_env(topo, batch, kernel, **kw)
        tr = env.run(ref.POLICY[route], LARGE_N, outputs=DECIDED, auto_reset=True)
        assert env.last_kernel().split()[0] == assign_kernel(kernel, kw["num_spectrum_resources"]), env.last_kernel()
        cuts, slots = env.path_min_cuts()
        env.close()
        runs = [ref.oracle_steps(topo, kw, seed0 + i, route, LARGE_N) for i in range(batch)]
        decisions_hold(tr, lambda i: runs[i], range(batch), (what, route))
        for i in range(batch):
            assert np.array_equal(cuts[i], runs[i]["min_cuts"][LARGE_N]) and np.array_equal(slots[i], runs[i]["min_slots"][LARGE_N]), (what, i)
        assert (tr["accepted"] == 1).any()
    return runs


@pytest.mark.parametrize("name,kernel", [("g3x3_k9_s64", "wave"), ("g3x3_k9_s64", "group"), ("g4x4_k12_s320", "wave"),
                                         ("g4x4_k12_s320", "group")])
def test_more_than_eight_paths(name, kernel, tmp_path, device_log_in_oracle):
    """k = 9 and 12: more than one pass of eight paths in the wave kernel, several passes per row in the group kernel"""
    runs = large_shape_holds(many_paths_topology(name, tmp_path), many_paths_kwargs(name), kernel, MANY_PATHS_SEED, 6, name)
    assert max(int(r["act_path"][r["accepted"] == 1].max()) for r in runs) >= 3   # (the last route run: fewest cuts)


@pytest.mark.parametrize("name,S,load", [(RING34, 100, 60), (RING36, 100, 60), (NSF, 448, 80), (NSF, 512, 90)])
def test_many_links_hops_and_words(name, S, load, step_kernel, device_log_in_oracle):
    """238 links; paths of 14 hops; seven words on the eight-word layout (S = 448) and eight words (two paths per row of the group
    kernel)."""
    kw = dict(num_spectrum_resources=S, load=load, mean_service_holding_time=25, episode_length=200, seed=5)
    large_shape_holds(topology(name), kw, step_kernel, 5, 3, (name, S, step_kernel))


def test_paths_of_fourteen_hops(step_kernel, device_log_in_oracle):
    """The routes seldom take the longest paths of the 36-node ring: an agent names them.  A window on a path of 14 hops is chosen
    with cuts > 0, and counts up to 9 are met (the fourth plane of the counter)."""
    topo = topology(RING36)
    kw = dict(num_spectrum_resources=100, load=20, mean_service_holding_time=25, episode_length=200, seed=5)
    paths = np.random.default_rng(7).integers(0, topo.k_paths, (LARGE_N, 3)).astype(np.int32)
    env = rmsa_env(topo, 3, step_kernel, **kw)
    tr = one_step_launches(env, "path_mc_external", LARGE_N, DECIDED, actions=paths, auto_reset=True)
    env.close()
    runs = [ref.oracle_steps(topo, kw, 5 + i, "path", LARGE_N, paths=paths[:, i]) for i in range(3)]
    decisions_hold(tr, lambda i: runs[i], range(3), "14 hops")
    assert sum(int(((r["hops"] == 14) & (r["cuts"] > 0)).sum()) for r in runs) >= 1
    assert max(int(r["cuts"].max()) for r in runs) >= 8


def test_windows_of_more_than_a_word(step_kernel, device_log_in_oracle):
    """bit rate 1000 at spectral efficiency 1 is 81 slots: the right neighbour lies two words on."""
    kw = dict(num_spectrum_resources=320, load=30, mean_service_holding_time=25, episode_length=50, seed=ref.SEED0,
              bit_rates=[100, 1000])
    topo = topology(NSF)
    import inspect
    from optical_rl_gym_amd import BatchedRMSAEnv
    if "bit_rates" not in inspect.signature(BatchedRMSAEnv.__init__).parameters:   # the handle cannot express the bit rates
        pytest.skip("BatchedRMSAEnv takes no bit_rates=: a request of 64 slots or more cannot be made")
    env = rmsa_env(NSF, 4, step_kernel, **kw)
    tr = env.run("min_cut", N, outputs=DECIDED, auto_reset=True)
    cuts, slots = env.path_min_cuts()
    env.close()
    runs = [ref.oracle_steps(topo, kw, ref.SEED0 + i, "min_cut", N) for i in range(4)]
    decisions_hold(tr, lambda i: runs[i], range(4), "long windows")
    for i in range(4):
        assert np.array_equal(cuts[i], runs[i]["min_cuts"][N]) and np.array_equal(slots[i], runs[i]["min_slots"][N])
    long = [r["n_slots"][r["accepted"] == 1] for r in runs]
    assert max(int(v.max()) for v in long) >= 64
    assert sum(int(((r["n_slots"] >= 64) & (r["cuts"] > 0)).sum()) for r in runs) > 0


# ---------------------------------------------------------------------------------------- 8. other handles, batch sizes
def test_sweep_handle_on_the_group_kernel():
    from optical_rl_gym_amd import make_sweep
    loads, seeds, S = (10.0, 20.0), 4, 100
    env = make_sweep("rmsa", topology(NSF), loads=loads, seeds_per_load=seeds, seed=ref.SEED0, step_kernel="group",
                     num_spectrum_resources=S, mean_service_holding_time=25, episode_length=50)
    tr = env.run("min_cut", N, outputs=DECIDED + ("block_cause",), cause_counts=True, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel("group", S, cause=True, traffic=True), env.last_kernel()
    tr2 = env.run("sap_mc", 50, outputs=DECIDED, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel("group", S, traffic=True), env.last_kernel()
    batch, env_loads = env.batch_size, [float(x) for x in env.loads]
    env.close()
    assert tr2["accepted"].shape == (50, batch)
    decisions_hold(tr, lambda i: ref.nsfnet_steps(S, env_loads[i], "min_cut", i % seeds), range(batch), "sweep")
    for i in range(batch):
        assert np.array_equal(tr["block_cause"][:, i], ref.nsfnet_steps(S, env_loads[i], "min_cut", i % seeds)["cause"]), i
    assert np.array_equal(tr["block_cause_counts"], bcr.counts_of(tr["block_cause"]))


def test_trace_handle_on_the_group_kernel():
    from optical_rl_gym_amd import record_trace
    S, load = 100, 20
    gen = make_env(S, load, "group")
    trace = record_trace(gen, "sap_mc", N, auto_reset=True)
    assert gen.last_kernel().split()[0] == assign_kernel("group", S), gen.last_kernel()
    gen.close()
    env = rmsa_env(NSF, B, "group", trace=trace, num_spectrum_resources=S, episode_length=50)
    tr = env.run("sap_mc", N, outputs=DECIDED, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel("group", S, trace=True), env.last_kernel()
    env.close()
    decisions_hold(tr, lambda i: ref.nsfnet_steps(S, load, "sap", i), range(B), "trace")


def test_partial_quad(step_kernel):
    S, load = 64, 10
    env = make_env(S, load, step_kernel, batch=6)
    tr = env.run("llp_mc", N, outputs=DECIDED, auto_reset=True)
    env.close()
    decisions_hold(tr, lambda i: ref.nsfnet_steps(S, load, "llp", i), range(6), "B=6")


def test_large_batch_on_tickets(step_kernel, device_log_in_oracle):
    """B = 4100 x 50 steps: several rounds, environments handed out by the ticket counter; the first and the last four
    environments against the reference."""
    S, load, batch, n = 100, 20, 4100, 50
    env = make_env(S, load, step_kernel, batch=batch)
    tr = env.run("min_cut", n, outputs=DECIDED, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel(step_kernel, S), env.last_kernel()
    cuts, slots = env.path_min_cuts()
    env.close()
    topo = topology(NSF)
    runs = {i: ref.oracle_steps(topo, bcr.shape_kwargs(S, load), ref.SEED0 + i, "min_cut", n)
            for i in [0, 1, 2, 3, batch - 4, batch - 3, batch - 2, batch - 1]}
    decisions_hold(tr, lambda i: runs[i], list(runs), "B=4100")
    for i, r in runs.items():
        assert np.array_equal(cuts[i], r["min_cuts"][n]) and np.array_equal(slots[i], r["min_slots"][n]), i
    assert ((tr["act_path"] == 5) == (tr["accepted"] == 0)).all()


# ---------------------------------------------------------------------------------------- 9. refusals on the device side
def _step_min_cut(env, route, n_steps=10, actions=None):
    ap = None if actions is None else actions.ctypes.data_as(C.c_void_p)
    rc = env.L.orlg_step_min_cut(env.h, route, n_steps, ap, 1, None, None)
    return rc, env.L.orlg_last_error().decode()


def test_the_library_refuses_before_it_launches(step_kernel):
    from optical_rl_gym_amd import _lib
    P = _lib.POLICIES
    env = make_env(100, 20, step_kernel, batch=4)
    env.run("sap_ff", 20, auto_reset=True)
    before, said = snapshot(env), env.last_kernel()
    acts = np.zeros((4, 2), np.int32)
    for policy, n, a in (("external", 1, acts), ("deeprmsa_sp_ff", 10, None), ("deeprmsa_sap_ff", 10, None),
                         ("deeprmsa_external", 1, acts[:, 0].copy()), ("sap_ff_gn", 10, None)):
        rc, msg = _step_min_cut(env, P[policy], n, a)
        assert rc == -1 and "route" in msg, (policy, rc, msg)
    for route in (-2, 8, 9, 99, 101):   # unknown routes, the device's own value of the fewest-cuts route among them
        rc, msg = _step_min_cut(env, route)
        assert rc == -1 and "route" in msg, (route, rc, msg)
    # orlg_step_assign knows its five rules and no route but a policy
    rc = env.L.orlg_step_assign(env.h, P["sap_ff"], 5, 10, None, 1, None, None)
    assert rc == -1 and "unknown assignment rule" in env.L.orlg_last_error().decode()
    for rule in (1, 3, 5):   # the policy answers before the rule, as it did
        for route in (8, _lib.ROUTE_FEWEST_CUTS):
            assert env.L.orlg_step_assign(env.h, route, rule, 10, None, 1, None, None) == -1
            assert "unknown policy" in env.L.orlg_last_error().decode()
    assert env.L.orlg_step(env.h, 8, 10, None, 1, None) == -1 and env.L.orlg_step(env.h, _lib.ROUTE_FEWEST_CUTS, 10, None, 1, None) == -1
    assert env.L.orlg_path_min_cuts(env.h, None, None) == -1
    assert env.last_kernel() == said
    same_bytes(snapshot(env), before, "nothing ran")
    rc, msg = _step_min_cut(env, _lib.ROUTE_FEWEST_CUTS, 20)
    assert rc == 0, msg
    assert env.last_kernel().split()[0] == assign_kernel(step_kernel, 100), env.last_kernel()
    env.close()


def test_a_gated_handle_is_refused():
    from optical_rl_gym_amd import _lib
    case = "nsfnet_s320_l150_sapff"
    topo, kw, _ = ggr.resolve_case(case)
    env = rmsa_env(topo, 4, gn_gate=ggr.case_gate(topo), **kw)
    before = snapshot(env)
    for route in (0, 1, 2, _lib.ROUTE_FEWEST_CUTS):
        rc, msg = _step_min_cut(env, route)
        assert rc == -1 and "gn_gate" in msg, (route, rc, msg)
    rc, msg = _step_min_cut(env, 6, 1, np.zeros(4, np.int32))
    assert rc == -1 and "gn_gate" in msg, (rc, msg)
    with pytest.raises(ValueError, match="gn_gate"):
        env.run("min_cut", 10)
    same_bytes(snapshot(env), before, "nothing ran")
    env.close()


# ---------------------------------------------------------------------------------------- 10. the drop-in surface
def test_view_callback_equals_the_device_policy(step_kernel):
    import optical_rl_gym_amd as pkg
    kw = dict(num_spectrum_resources=100, load=20, mean_service_holding_time=25, episode_length=200, seed=10)
    dev = rmsa_env(NSF, 1, step_kernel, **kw)
    tr = dev.run("sap_mc", 100, outputs=DECIDED)
    dev.close()
    view = pkg.make("RMSA-v0", topology=topology(NSF), **kw)
    heuristic = pkg.min_cut_heuristic("sap")
    for t in range(100):
        a = heuristic(view)
        assert tuple(a) == (tr["act_path"][t, 0], tr["act_slot"][t, 0]), t
        served = view.current_service
        view.step(a)
        assert served.accepted == bool(tr["accepted"][t, 0]), t
    other = pkg.min_cut_heuristic("min_cut")(view)
    cuts, slots = view._batched.path_min_cuts()
    has = np.flatnonzero(cuts[view._index] >= 0)
    if has.size:
        best = has[np.argmin(cuts[view._index][has])]
        assert tuple(other) == (best, slots[view._index][best])
    view.close()
