"""Blocking cause per step and fit level per candidate path on the device (``include/orlg.h`` ``orlg_step_diag`` /
``orlg_path_fit_levels``) against the numpy restatement of the definitions applied to the oracle's occupancy, one
step at a time (``block_cause_reference.py``; ``test_block_cause.py`` holds that module to brute force and shows that every code
occurs on these shapes).  Both step kernels, every policy family, every launch shape, every kind of handle; and that asking for
a cause changes nothing else -- not the state, not another output, not the kernel of a launch that does not ask.

B = 8 unless said, 200 steps from an empty network, ``episode_length=50`` (three auto-resets inside a launch), seeds 10 + i,
holding time 25: the setup of the issue's table."""
import functools
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import block_cause_reference as ref
import gn_gate_reference as ggr
from conftest import oracle_env_from_kwargs
from gpu_support import (MANY_PATHS_SEED, RMSA_OUTS, STATS_LEVELS, device_log_fixture, drive, external_actions, kernel_name,  # noqa: F401
                         many_paths_kwargs, many_paths_topology, rmsa_env, same_bytes, snapshot, step_kernel, tooling_env, topology)

pytestmark = pytest.mark.gpu

NSF = ref.NSFNET
RING34, RING36 = "ring34_3-paths_6-modulations", "ring36_3-paths_6-modulations"
B, N = ref.N_ENVS, ref.N_STEPS
SHAPES = ((64, 10), (100, 20), (320, 50))
POLICIES = ("sp_ff", "sap_ff", "llp_ff", "deeprmsa_sap_ff")


def cause_kernel(kernel, S, stats="full", gn=False, traffic=False, trace=False):
    """The instantiation a cause launch reports: the plain kind of either kernel with the CAUSE flag last."""
    W = (S + 63) // 64
    W, level = 8 if W == 7 else W, STATS_LEVELS.index(stats)
    if kernel == "group":
        return f"orlg_rmsa_group_kernel<{W},{level},false,false,{str(traffic).lower()},{str(trace).lower()},true>"
    return f"orlg_rmsa_kernel<{W},{level},false,{str(gn).lower()},true>"


def make_env(S, load, kernel, policy="sap_ff", batch=B, **kw):
    if policy.startswith("deeprmsa"):   # the DeepRMSA handle: load = holding / inter-arrival (exact for these loads)
        from optical_rl_gym_amd import BatchedDeepRMSAEnv
        return BatchedDeepRMSAEnv(topology(NSF), batch, step_kernel=kernel, num_spectrum_resources=S, mean_service_holding_time=25.0,
                                  mean_service_inter_arrival_time=25.0 / load, episode_length=50, seed=ref.SEED0, **kw)
    return rmsa_env(NSF, batch, kernel, **ref.shape_kwargs(S, load, **kw))


def cause_run(env, policy, n, outputs=(), **kw):
    return env.run(policy, n, outputs=tuple(outputs) + ("block_cause",), cause_counts=True, auto_reset=True, **kw)


def counts_hold(tr, n):
    """cause_counts == bincount(block_cause) per environment, rows sum to n, code 7 never"""
    assert tr["block_cause"].dtype == np.uint8 and tr["block_cause_counts"].dtype == np.int32
    assert np.array_equal(tr["block_cause_counts"], ref.counts_of(tr["block_cause"]))
    assert (tr["block_cause_counts"].sum(axis=1) == n).all() and not tr["block_cause_counts"][:, 7].any()


def reference_holds(tr, policy, S, load, envs=range(B), n=N, what=""):
    for i in envs:
        want = ref.nsfnet_steps(S, load, policy, i, n)
        assert np.array_equal(tr["accepted"][:, i], want["accepted"]), (what, i)
        bad = np.flatnonzero(tr["block_cause"][:, i] != want["cause"])
        assert bad.size == 0, (what, i, bad[:6], tr["block_cause"][bad[:6], i], want["cause"][bad[:6]], want["levels"][bad[:6]])


# ---------------------------------------------------------------------------------------- 1. one launch, against the reference
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("S,load", SHAPES)
def test_one_launch_against_the_reference(S, load, policy, step_kernel):
    env = make_env(S, load, step_kernel, policy)
    tr = cause_run(env, policy, N, outputs=("accepted",))
    assert env.last_kernel().split()[0] == cause_kernel(step_kernel, S), env.last_kernel()
    env.close()
    assert tr["block_cause"].shape == (N, B) and tr["block_cause_counts"].shape == (B, 8)
    counts_hold(tr, N)
    reference_holds(tr, policy, S, load, what=(policy, S, step_kernel))
    seen = np.bincount(tr["block_cause"].ravel(), minlength=8)
    if S < 320 and not policy.startswith("deeprmsa"):   # (what test_block_cause.py shows of the reference on these shapes)
        assert all(seen[c] > 0 for c in (range(6) if policy == "sp_ff" else range(5))), seen
    assert seen[ref.ACCEPTED] > 0 and (seen[1:] > 0).sum() >= 2, seen


# ---------------------------------------------------------------------------------------- 2. every launch shape, the same bits
@pytest.mark.parametrize("policy", ["sp_ff", "llp_ff"])
def test_launch_shapes_give_the_same_bits(policy, step_kernel):
    S, load = 100, 20
    env = make_env(S, load, step_kernel)
    one = cause_run(env, policy, N, outputs=("accepted",))
    env.close()
    env = make_env(S, load, step_kernel)
    cols, total = [], np.zeros((B, 8), np.int64)
    for _ in range(N):
        r = cause_run(env, policy, 1)
        counts_hold(r, 1)
        cols.append(r["block_cause"][0])
        total += r["block_cause_counts"]
    # (a launch of one step asks the group kernel's plan for the queue in HBM: a cause launch stays on the plain kind)
    assert env.last_kernel().split()[0] == cause_kernel(step_kernel, S), env.last_kernel()
    env.close()
    assert np.array_equal(np.stack(cols), one["block_cause"]) and np.array_equal(total, one["block_cause_counts"])
    if step_kernel == "group":   # tickets in chunks of steps: successive chunks of a quad may run on different waves
        with tooling_env(ORLG_GROUP_CHUNKS="7"):
            env = make_env(S, load, "group")
            chunks = cause_run(env, policy, N, outputs=("accepted",))
            assert "chunks=7" in env.last_kernel() and env.last_kernel().split()[0] == cause_kernel("group", S), env.last_kernel()
            env.close()
        same_bytes(chunks, one, "chunks")
    reference_holds(one, policy, S, load, what=(policy, step_kernel))


# ---------------------------------------------------------------------------------------- 3. no side effects
@pytest.mark.parametrize("stats", STATS_LEVELS)
def test_a_cause_launch_changes_nothing_else(stats, step_kernel):
    """The snapshot and every other output of a cause run equal those of the same run without it (two launches: 150 steps, then
    50); and a launch that does not ask runs the kernel it ran before, on the very handle that just ran a cause launch."""
    S, load = 320, 50
    outs = RMSA_OUTS if stats != "counters" else tuple(o for o in RMSA_OUTS if "compactness" not in o)
    make = lambda: make_env(S, load, step_kernel, stats_level=stats)
    plain = drive(make, [("sap_ff", 150, None, outs), ("sap_ff", 50, None, outs)])
    with_cause = []

    def run_both():
        env = make()
        for n in (150, 50):
            with_cause.append(cause_run(env, "sap_ff", n, outputs=outs))
            assert env.last_kernel().split()[0] == cause_kernel(step_kernel, S, stats), env.last_kernel()
        snap = snapshot(env)
        # the next launch without a cause output: the kernel such a launch always ran (first fit / deferred / lean)
        env.run("sap_ff", 200, auto_reset=True)
        said = env.last_kernel()
        if step_kernel == "group":
            assert said.split()[0] == kernel_name("group", S, stats, defer=stats == "full"), said
            assert ("body=lean" in said) == (stats == "full"), said
        else:
            assert said.split()[0] == kernel_name("wave", S, stats, ff=True, defer=stats == "full"), said
        env.close()
        return snap

    snap = run_both()
    same_bytes(snap, plain["snap"], "snapshot")
    for got, want in zip(with_cause, plain["outs"]):
        same_bytes({k: v for k, v in got.items() if not k.startswith("block_cause")}, want, "outputs")
    assert set(plain["kernels"]) == {kernel_name(step_kernel, S, stats, ff=step_kernel == "wave", defer=stats == "full")}, plain["said"]
    tr = {k: np.concatenate([r[k] for r in with_cause]) for k in ("block_cause", "accepted")}
    reference_holds(tr, "sap_ff", S, load, what=stats)


# ---------------------------------------------------------------------------------------- 4. agents' actions
@pytest.mark.parametrize("policy", ["external", "path_ff_external", "deeprmsa_external"])
def test_external_actions(policy, step_kernel, device_log_in_oracle):
    """Actions out of range in either component, windows that are not free, paths without a fit, blocks that do not exist: the
    cause is the same function of the occupancy, and POLICY occurs."""
    S, load, j, topo = 100, 20, 2, topology(NSF)
    if policy == "external":
        actions = external_actions(topo, S, N, B)
    elif policy == "path_ff_external":
        actions = external_actions(topo, S, N, B, kind="paths")
    else:
        actions = np.random.default_rng(7).integers(0, topo.k_paths * j + 1, (N, B)).astype(np.int32)
    env = make_env(S, load, step_kernel, j=j)
    cols, total = {"block_cause": [], "accepted": []}, np.zeros((B, 8), np.int64)
    for t in range(N):
        r = cause_run(env, policy, 1, outputs=("accepted",), actions=actions[t])
        for k in cols:
            cols[k].append(r[k][0])
        total += r["block_cause_counts"]
    assert env.last_kernel().split()[0] == cause_kernel(step_kernel, S), env.last_kernel()
    env.close()
    tr = {k: np.stack(v) for k, v in cols.items()}
    assert np.array_equal(total, ref.counts_of(tr["block_cause"]))
    for i in range(B):
        want = ref.oracle_steps(topo, ref.shape_kwargs(S, load), ref.SEED0 + i, policy, N, actions=actions[:, i], j=j)
        assert np.array_equal(tr["accepted"][:, i], want["accepted"]), (policy, i)
        assert np.array_equal(tr["block_cause"][:, i], want["cause"]), (policy, i)
    seen = np.bincount(tr["block_cause"].ravel(), minlength=8)
    assert seen[ref.C_POLICY] > 0 and seen[ref.ACCEPTED] > 0 and seen[6] == 0, seen


# ---------------------------------------------------------------------------------------- 5. behind the GN-model admission check
GATED_CASE, GATED_B, GATED_N = "nsfnet_s320_l150_sapff", 4, 300


@functools.lru_cache(maxsize=None)
def gated_reference(policy, i):
    return ref.gated_steps(GATED_CASE, GATED_N, policy=policy, seed=ggr.CASES[GATED_CASE]["seed"] + i)


@pytest.mark.parametrize("policy", ["sap_ff", "sap_ff_gn"])
def test_gated_handle(policy):
    """cause == GN exactly where the check ran and the step is not accepted (gn_gsnr_db not NaN), the rest as without a gate; all
    three outputs of orlg_step_diag in one call."""
    topo, kw, _ = ggr.resolve_case(GATED_CASE)
    env = rmsa_env(topo, GATED_B, gn_gate=ggr.case_gate(topo), **kw)
    tr = cause_run(env, policy, GATED_N, outputs=("accepted", "gn_gsnr_db"))
    assert env.last_kernel().split()[0] == cause_kernel("wave", kw["num_spectrum_resources"], gn=True), env.last_kernel()
    env.close()
    counts_hold(tr, GATED_N)
    refused_by_gate = (tr["accepted"] == 0) & ~np.isnan(tr["gn_gsnr_db"])
    assert np.array_equal(tr["block_cause"] == ref.C_GN, refused_by_gate)
    for i in range(GATED_B):
        want = gated_reference(policy, i)
        assert np.array_equal(tr["accepted"][:, i], want["accepted"]), (policy, i)
        assert np.array_equal(tr["block_cause"][:, i], want["cause"]), (policy, i)
    seen = np.bincount(tr["block_cause"].ravel(), minlength=8)
    assert seen[ref.C_GN] > 0 and seen[ref.ACCEPTED] > 0, seen


# ---------------------------------------------------------------------------------------- 6. a sweep handle, a trace handle
def test_sweep_handle_on_the_group_kernel():
    from optical_rl_gym_amd import make_sweep, traffic
    loads, seeds, S = (10.0, 20.0, 40.0), 4, 100
    env = make_sweep("rmsa", topology(NSF), loads=loads, seeds_per_load=seeds, seed=ref.SEED0, step_kernel="group",
                     num_spectrum_resources=S, mean_service_holding_time=25, episode_length=50)
    tr = cause_run(env, "sap_ff", N, outputs=("accepted",))
    assert env.last_kernel().split()[0] == cause_kernel("group", S, traffic=True), env.last_kernel()
    counts_hold(tr, N)
    for i in range(env.batch_size):
        want = ref.nsfnet_steps(S, float(env.loads[i]), "sap_ff", i % seeds)
        assert np.array_equal(tr["block_cause"][:, i], want["cause"]), i
    shares = traffic.blocking_shares_by_group(tr["block_cause_counts"], env.groups, env.num_groups, loads=env.loads)
    env.close()
    assert shares["loads"].tolist() == list(loads) and shares["steps"].tolist() == [seeds * N] * 3
    blocked = 1 - shares["shares"][:, 0]
    assert blocked[0] < blocked[1] < blocked[2] and np.allclose(shares["shares"].sum(axis=1), 1)


def test_trace_handle_on_the_group_kernel():
    from optical_rl_gym_amd import record_trace
    S, load = 100, 20
    gen = make_env(S, load, "group")
    trace = record_trace(gen, "sap_ff", N, auto_reset=True)
    gen.close()
    env = rmsa_env(NSF, B, "group", trace=trace, num_spectrum_resources=S, episode_length=50)
    tr = cause_run(env, "sap_ff", N, outputs=("accepted",))
    assert env.last_kernel().split()[0] == cause_kernel("group", S, trace=True), env.last_kernel()
    env.close()
    counts_hold(tr, N)
    reference_holds(tr, "sap_ff", S, load, what="trace")


# ---------------------------------------------------------------------------------------- 7. idle tail rows; many quads, tickets
def test_idle_tail_rows_of_the_group_kernel():
    S, load = 64, 10
    env = make_env(S, load, "group", batch=6)
    tr = cause_run(env, "llp_ff", N, outputs=("accepted",))
    env.close()
    counts_hold(tr, N)
    reference_holds(tr, "llp_ff", S, load, envs=range(6), what="B=6")


def test_large_batch_on_tickets(step_kernel):
    """B = 4100 x 50 steps: several quads per wave, environments handed out by the ticket counter; counts against per-step for
    every environment, the first and the last environment against the reference.  The caller's counts buffer arrives filled."""
    S, load, batch, n = 100, 20, 4100, 50
    env = make_env(S, load, step_kernel, batch=batch)
    counts = np.full((batch, 8), 77, np.int32)
    tr = env.run("sap_ff", n, outputs=("accepted", "block_cause"), cause_counts=counts, auto_reset=True)
    assert tr["block_cause_counts"] is counts
    assert env.last_kernel().split()[0] == cause_kernel(step_kernel, S), env.last_kernel()
    env.close()
    counts_hold(tr, n)
    assert np.array_equal(tr["block_cause"] == ref.ACCEPTED, tr["accepted"] == 1)
    for i in (0, batch - 1):
        want = ref.nsfnet_steps(S, load, "sap_ff", i, n)
        assert np.array_equal(tr["block_cause"][:, i], want["cause"]), i


def test_device_buffers_are_written_in_place():
    """block_cause, cause_counts (arriving filled: the library zeroes them on the stream) and path_fit_levels into torch device
    tensors equal the same launches into host arrays, on both kernels.  In a child process: torch has to create its HIP context
    before the library does."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys
        import numpy as np, torch
        torch.zeros(1, device="cuda")
        sys.path[:0] = [%r, %r]
        from gpu_support import rmsa_env
        import block_cause_reference as ref
        B, n = 8, 200
        for kernel in ("wave", "group"):
            host, dev = (rmsa_env(ref.NSFNET, B, kernel, **ref.shape_kwargs(100, 20)) for _ in range(2))
            want = host.run("sp_ff", n, outputs=("block_cause",), cause_counts=True, auto_reset=True)
            cause = torch.full((n, B), 9, dtype=torch.uint8, device="cuda")
            counts = torch.full((B, 8), 77, dtype=torch.int32, device="cuda")
            levels = torch.full((B, dev.k_paths), 9, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            got = dev.run("sp_ff", n, out={"block_cause": cause}, cause_counts=counts, auto_reset=True)
            assert got["block_cause"] is cause and got["block_cause_counts"] is counts
            assert dev.path_fit_levels(out=levels) is levels
            dev.synchronize()
            assert np.array_equal(cause.cpu().numpy(), want["block_cause"]), kernel
            assert np.array_equal(counts.cpu().numpy(), want["block_cause_counts"]), kernel
            assert np.array_equal(levels.cpu().numpy(), host.path_fit_levels()), kernel
            assert len(np.unique(want["block_cause"])) >= 5
            host.close(); dev.close()
        print("device buffers ok")
    """) % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "device buffers ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------- 8. fit levels of every candidate path
def levels_hold(env, topo, kw, policy, steps, seed0, what):
    """path_fit_levels after every count of `steps` (cumulative) against the reference on one oracle per environment, and against
    the masks: levels == 4 is path_ff, levels >= 3 is any bit of the slots mask."""
    seen, oracles = set(), [oracle_env_from_kwargs(topo, kw, seed=seed0 + i) for i in range(env.batch_size)]
    done = 0
    for upto in steps:
        if upto > done:
            env.run(policy, upto - done, auto_reset=True)
            for o in oracles:
                o.run(policy, upto - done, reset_on_done=True, fields=[])
            done = upto
        lv = env.path_fit_levels()
        assert lv.shape == (env.batch_size, env.k_paths) and lv.dtype == np.uint8
        for i, o in enumerate(oracles):
            r = o.request()
            want = ref.path_levels(o.available_slots(), topo, r.src, r.dst, r.bit_rate)
            assert np.array_equal(lv[i], want), (what, upto, i, lv[i], want)
        assert np.array_equal(lv == ref.FIT, env.action_masks("path_ff")[:, :env.k_paths] == 1), (what, upto)
        assert np.array_equal(lv >= ref.LAST_WINDOW, env.action_masks("slots").any(axis=2)), (what, upto)
        seen |= set(np.unique(lv).tolist())
    for o in oracles:
        o.close()
    return seen


@pytest.mark.parametrize("S,load", SHAPES)
def test_fit_levels_on_nsfnet(S, load, step_kernel, device_log_in_oracle):
    env = make_env(S, load, step_kernel)
    seen = levels_hold(env, topology(NSF), ref.shape_kwargs(S, load), "sap_ff", (0, 50, 200), ref.SEED0, (S, step_kernel))
    out = np.full((B, env.k_paths), 9, np.uint8)
    assert env.path_fit_levels(out=out) is out and np.array_equal(out, env.path_fit_levels())
    env.close()
    assert ref.FIT in seen and len(seen) >= 3, seen


@pytest.mark.parametrize("name", ["g3x3_k9_s64", "g4x4_k12_s320"])
def test_fit_levels_with_more_than_eight_paths(name, tmp_path, device_log_in_oracle):
    topo, kw = many_paths_topology(name, tmp_path), many_paths_kwargs(name)
    env = rmsa_env(topo, 6, "wave", **kw)
    seen = levels_hold(env, topo, kw, "sap_ff", (0, 50, 200), MANY_PATHS_SEED, name)
    env.close()
    assert ref.FIT in seen and min(seen) < ref.LAST_WINDOW, seen


MANY_LINKS = {RING34: dict(num_spectrum_resources=100, load=60), RING36: dict(num_spectrum_resources=512, load=500)}


@pytest.mark.parametrize("name", [RING34, RING36])
def test_fit_levels_over_many_links_and_hops(name, device_log_in_oracle):
    """ring34: 238 links, the candidate paths over every range of 64 link ids; ring36: paths of 14 hops, eight words per link."""
    topo = topology(name)
    kw = dict(MANY_LINKS[name], mean_service_holding_time=25, episode_length=200, seed=5)
    env = rmsa_env(topo, 3, "wave", **kw)
    seen = levels_hold(env, topo, kw, "sap_ff", (0, 50, 200), 5, name)
    env.close()
    assert ref.FIT in seen and min(seen) < ref.LAST_WINDOW, seen


# ---------------------------------------------------------------------------------------- the classifiers beyond NSFNET's shape
@pytest.mark.parametrize("name,kernel", [("g3x3_k9_s64", "wave"), ("g3x3_k9_s64", "group"), ("g4x4_k12_s320", "wave")])
def test_cause_with_more_than_eight_paths(name, kernel, tmp_path, device_log_in_oracle):
    topo, kw = many_paths_topology(name, tmp_path), many_paths_kwargs(name)
    env = rmsa_env(topo, 6, kernel, **kw)
    tr = cause_run(env, "sp_ff", N, outputs=("accepted",))
    env.close()
    counts_hold(tr, N)
    for i in range(6):
        want = ref.oracle_steps(topo, kw, MANY_PATHS_SEED + i, "sp_ff", N)
        assert np.array_equal(tr["block_cause"][:, i], want["cause"]), (name, kernel, i)
    assert len(np.unique(tr["block_cause"])) >= 3


@pytest.mark.parametrize("name,S,load", [(RING34, 100, 60), (RING36, 100, 60), (NSF, 512, 90)])
def test_cause_over_many_links_hops_and_words(name, S, load, step_kernel, device_log_in_oracle):
    """238 links; paths of 14 hops (two passes of links in either layout); eight words per link (two paths, or links, per row of
    the group kernel)."""
    topo = topology(name)
    kw = dict(num_spectrum_resources=S, load=load, mean_service_holding_time=25, episode_length=200, seed=5)
    env = rmsa_env(topo, 3, step_kernel, **kw)
    tr = cause_run(env, "sp_ff", N, outputs=("accepted",))
    assert env.last_kernel().split()[0] == cause_kernel(step_kernel, S), env.last_kernel()
    env.close()
    counts_hold(tr, N)
    for i in range(3):
        want = ref.oracle_steps(topo, kw, 5 + i, "sp_ff", N)
        assert np.array_equal(tr["block_cause"][:, i], want["cause"]), (name, step_kernel, i)
    assert len(np.unique(tr["block_cause"])) >= 2
