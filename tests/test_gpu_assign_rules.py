"""Spectrum-assignment rules on the device (``include/orlg.h`` ``orlg_step_assign``): last, best and exact fit and
the first fit of the whole range, on the routes sp / sap / llp and on an agent's path, against the numpy restatement of the
definitions driving the oracle with external actions, one step at a time (``assign_reference.py``; ``test_assign_rules.py`` holds
that module to brute force and shows that the rules differ from the reference's first fit on these shapes).  Both step kernels,
every kind of handle, every launch shape, with and without the blocking cause; and that a launch under an old policy name runs
the kernel it ran.  Integer-exact: no tolerance anywhere.

B = 8 unless said, 200 steps from an empty network, ``episode_length=50`` (three auto-resets inside a launch), seeds 10 + i,
holding time 25: the setup of ``block_cause_reference``."""
import ctypes as C

import numpy as np
import pytest

import assign_reference as ref
import block_cause_reference as bcr
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
    """The instantiation a launch under a new rule reports: the plain kind of either kernel with the ASSIGN flag last."""
    W = (S + 63) // 64
    W, level = 8 if W == 7 else W, STATS_LEVELS.index(stats)
    t = lambda flag: str(bool(flag)).lower()
    if kernel == "group":
        return f"orlg_rmsa_group_kernel<{W},{level},false,false,{t(traffic)},{t(trace)},{t(cause)},true>"
    return f"orlg_rmsa_kernel<{W},{level},false,false,{t(cause)},true>"


def make_env(S, load, kernel, batch=B, **kw):
    return rmsa_env(NSF, batch, kernel, **bcr.shape_kwargs(S, load, **kw))


def decisions_hold(tr, want, envs, what):
    """act_path, act_slot, accepted of environment i (column i of tr) equal the reference run want(i), step by step"""
    for i in envs:
        w = want(i)
        for k in DECIDED:
            bad = np.flatnonzero(tr[k][:, i] != w[k][:len(tr[k])])
            assert bad.size == 0, (what, i, k, bad[:6], tr[k][bad[:6], i], w[k][bad[:6]])


# ---------------------------------------------------------------------------------------- 1. one launch, against the reference
@pytest.mark.parametrize("rule", ref.NEW_RULES)
@pytest.mark.parametrize("route", ref.ROUTES)
@pytest.mark.parametrize("S,load", ref.SHAPES)
def test_one_launch_against_the_reference(S, load, route, rule, step_kernel):
    """W = 1, 2 and 5: blocks cross word boundaries, and S = 100 is a last word that is not full."""
    env = make_env(S, load, step_kernel)
    tr = env.run(ref.policy_name(route, rule), N, outputs=DECIDED, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel(step_kernel, S), env.last_kernel()
    env.close()
    assert tr["act_slot"].shape == (N, B)
    decisions_hold(tr, lambda i: ref.nsfnet_steps(S, load, route, rule, i), range(B), (S, route, rule, step_kernel))
    first = ref.stacked(S, load, route, rule)
    if rule != "first_full":   # (what test_assign_rules.py shows of the reference: the comparison is not one of first fits)
        assert ((tr["act_slot"] != first["first_slot"]) | (tr["act_path"] != first["first_path"])).sum() >= 10


# ---------------------------------------------------------------------------------------- 2. every launch shape, the same bits
@pytest.mark.parametrize("policy", ["llp_bf", "sap_lf", "sp_ef"])
def test_launch_shapes_give_the_same_bits(policy, step_kernel):
    S, load = 100, 20
    env = make_env(S, load, step_kernel)
    one = env.run(policy, N, outputs=RMSA_OUTS, auto_reset=True)
    env.close()
    env = make_env(S, load, step_kernel)
    steps = one_step_launches(env, policy, N, RMSA_OUTS, auto_reset=True)
    # (a launch of one step asks the group kernel's plan for the queue in HBM: a launch under a rule stays on the plain kind)
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
    S, load, route, rule = 320, 50, "sap", "best"
    outs = RMSA_OUTS if stats != "counters" else tuple(o for o in RMSA_OUTS if "compactness" not in o)
    want = ref.stacked(S, load, route, rule)
    actions = np.stack([want["act_path"], want["act_slot"]], axis=-1).astype(np.int32)   # [N, B, 2]
    make = lambda: make_env(S, load, step_kernel, stats_level=stats)
    ext = drive(make, [("external", 1, None, outs)] * N, actions=actions)
    env = make()
    got = one_step_launches(env, ref.policy_name(route, rule), N, outs, auto_reset=True)
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


# ---------------------------------------------------------------------------------------- 4. with the blocking cause
@pytest.mark.parametrize("policy_of", [("sap", "last"), ("llp", "exact"), ("sp", "best")])
@pytest.mark.parametrize("S,load", [(64, 10), (320, 50)])
def test_with_the_blocking_cause(S, load, policy_of, step_kernel):
    route, rule = policy_of
    policy = ref.policy_name(route, rule)
    env = make_env(S, load, step_kernel)
    plain = env.run(policy, N, outputs=RMSA_OUTS, auto_reset=True)
    env.close()
    env = make_env(S, load, step_kernel)
    tr = env.run(policy, N, outputs=RMSA_OUTS + ("block_cause",), cause_counts=True, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel(step_kernel, S, cause=True), env.last_kernel()
    env.close()
    same_bytes({k: v for k, v in tr.items() if not k.startswith("block_cause")}, plain, "the outputs without the cause")
    want = ref.stacked(S, load, route, rule)
    bad = np.argwhere(tr["block_cause"] != want["cause"])
    assert bad.size == 0, (policy, bad[:6])
    assert np.array_equal(tr["block_cause_counts"], bcr.counts_of(want["cause"]))
    assert (tr["block_cause_counts"].sum(axis=1) == N).all()
    seen = np.bincount(tr["block_cause"].ravel(), minlength=8)
    assert seen[bcr.ACCEPTED] > 0 and seen[1:].sum() > 0, seen
    if route != "sp":
        assert not seen[bcr.C_LAST_WINDOW:].any(), seen   # sap / llp under a new rule: cause <= alignment


# ---------------------------------------------------------------------------------------- 5. path-only actions
@pytest.mark.parametrize("rule", ref.NEW_RULES)
def test_path_only_actions(rule, step_kernel, device_log_in_oracle):
    """Random paths that include k and values out of range on either side: the rejection (k, S)."""
    S, load, topo = 100, 20, topology(NSF)
    actions = external_actions(topo, S, N, B, kind="paths")
    actions[5::17] = -1
    actions[7::19] = topo.k_paths + 3
    env = make_env(S, load, step_kernel)
    tr = one_step_launches(env, ref.policy_name("path", rule), N, DECIDED, actions=actions, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel(step_kernel, S), env.last_kernel()
    env.close()
    runs = {}

    def want(i):
        if i not in runs:
            runs[i] = ref.oracle_steps(topo, bcr.shape_kwargs(S, load), ref.SEED0 + i, "path", rule, N, paths=actions[:, i])
        return runs[i]

    decisions_hold(tr, want, range(B), rule)
    assert (tr["act_path"] == topo.k_paths).any() and (tr["accepted"] == 1).any()
    assert ((tr["act_path"] == topo.k_paths) == (tr["act_slot"] == S)).all()


# ---------------------------------------------------------------------------------------- 6. a sweep handle, a trace handle
def test_sweep_handle_on_the_group_kernel():
    from optical_rl_gym_amd import make_sweep
    loads, seeds, S = (10.0, 20.0), 4, 100
    env = make_sweep("rmsa", topology(NSF), loads=loads, seeds_per_load=seeds, seed=ref.SEED0, step_kernel="group",
                     num_spectrum_resources=S, mean_service_holding_time=25, episode_length=50)
    tr = env.run("sap_bf", N, outputs=DECIDED + ("block_cause",), cause_counts=True, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel("group", S, cause=True, traffic=True), env.last_kernel()
    tr2 = env.run("llp_lf", 50, outputs=DECIDED, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel("group", S, traffic=True), env.last_kernel()
    batch, env_loads = env.batch_size, [float(x) for x in env.loads]
    env.close()
    assert tr2["accepted"].shape == (50, batch)
    decisions_hold(tr, lambda i: ref.nsfnet_steps(S, env_loads[i], "sap", "best", i % seeds), range(batch), "sweep")
    for i in range(batch):
        assert np.array_equal(tr["block_cause"][:, i], ref.nsfnet_steps(S, env_loads[i], "sap", "best", i % seeds)["cause"]), i
    assert np.array_equal(tr["block_cause_counts"], bcr.counts_of(tr["block_cause"]))


def test_trace_handle_on_the_group_kernel():
    from optical_rl_gym_amd import record_trace
    S, load = 100, 20
    gen = make_env(S, load, "group")
    trace = record_trace(gen, "sap_lf", N, auto_reset=True)
    assert gen.last_kernel().split()[0] == assign_kernel("group", S), gen.last_kernel()
    gen.close()
    env = rmsa_env(NSF, B, "group", trace=trace, num_spectrum_resources=S, episode_length=50)
    tr = env.run("sap_lf", N, outputs=DECIDED, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel("group", S, trace=True), env.last_kernel()
    env.close()
    decisions_hold(tr, lambda i: ref.nsfnet_steps(S, load, "sap", "last", i), range(B), "trace")


# ---------------------------------------------------------------------------------------- 7. large shapes
LARGE_POLICIES = (("sap", "best"), ("llp", "last"))
LARGE_N = 100


def large_shape_holds(topo, kw, kernel, seed0, batch, what):
    for route, rule in LARGE_POLICIES:
        env = rmsa_env(topo, batch, kernel, **kw)
        tr = env.run(ref.policy_name(route, rule), LARGE_N, outputs=DECIDED, auto_reset=True)
        assert env.last_kernel().split()[0] == assign_kernel(kernel, kw["num_spectrum_resources"]), env.last_kernel()
        env.close()
        decisions_hold(tr, lambda i: ref.oracle_steps(topo, kw, seed0 + i, route, rule, LARGE_N), range(batch), (what, route, rule))
        assert (tr["accepted"] == 1).any()


@pytest.mark.parametrize("name,kernel", [("g3x3_k9_s64", "wave"), ("g3x3_k9_s64", "group"), ("g4x4_k12_s320", "wave")])
def test_more_than_eight_paths(name, kernel, tmp_path, device_log_in_oracle):
    large_shape_holds(many_paths_topology(name, tmp_path), many_paths_kwargs(name), kernel, MANY_PATHS_SEED, 6, name)


@pytest.mark.parametrize("name,S,load", [(RING34, 100, 60), (RING36, 100, 60), (NSF, 448, 80), (NSF, 512, 90)])
def test_many_links_hops_and_words(name, S, load, step_kernel, device_log_in_oracle):
    """238 links; paths of 14 hops; seven words on the eight-word layout (S = 448) and eight words (two paths per row of the group
    kernel)."""
    kw = dict(num_spectrum_resources=S, load=load, mean_service_holding_time=25, episode_length=200, seed=5)
    large_shape_holds(topology(name), kw, step_kernel, 5, 3, (name, S, step_kernel))


# ---------------------------------------------------------------------------------------- 8. batch sizes
def test_partial_quad(step_kernel):
    S, load = 64, 10
    env = make_env(S, load, step_kernel, batch=6)
    tr = env.run("llp_ef", N, outputs=DECIDED, auto_reset=True)
    env.close()
    decisions_hold(tr, lambda i: ref.nsfnet_steps(S, load, "llp", "exact", i), range(6), "B=6")


def test_large_batch_on_tickets(step_kernel):
    """B = 4100 x 50 steps: several rounds, environments handed out by the ticket counter; the first and the last four
    environments against the reference."""
    S, load, batch, n = 100, 20, 4100, 50
    env = make_env(S, load, step_kernel, batch=batch)
    tr = env.run("sap_bf", n, outputs=DECIDED, auto_reset=True)
    assert env.last_kernel().split()[0] == assign_kernel(step_kernel, S), env.last_kernel()
    env.close()
    topo = topology(NSF)
    decisions_hold(tr, lambda i: ref.oracle_steps(topo, bcr.shape_kwargs(S, load), ref.SEED0 + i, "sap", "best", n),
                   [0, 1, 2, 3, batch - 4, batch - 3, batch - 2, batch - 1], "B=4100")
    assert ((tr["act_path"] == 5) == (tr["accepted"] == 0)).all()


# ---------------------------------------------------------------------------------------- 9. refusals on the device side
def _step_assign(env, policy, rule, n_steps=10, actions=None):
    from optical_rl_gym_amd import _lib
    ap = None if actions is None else actions.ctypes.data_as(C.c_void_p)
    rc = env.L.orlg_step_assign(env.h, _lib.POLICIES[policy], rule, n_steps, ap, 1, None, None)
    return rc, env.L.orlg_last_error().decode()


def test_the_library_refuses_before_it_launches(step_kernel):
    env = make_env(100, 20, step_kernel, batch=4)
    env.run("sap_ff", 20, auto_reset=True)
    before, said = snapshot(env), env.last_kernel()
    acts = np.zeros((4, 2), np.int32)
    for policy, n, a in (("external", 1, acts), ("deeprmsa_sp_ff", 10, None), ("deeprmsa_sap_ff", 10, None),
                         ("deeprmsa_external", 1, acts[:, 0].copy()), ("sap_ff_gn", 10, None)):
        for rule in (1, 2, 3, 4):
            rc, msg = _step_assign(env, policy, rule, n, a)
            assert rc == -1 and ("route" in msg or "gn_gate" in msg), (policy, rule, rc, msg)
    for rule in (-1, 5, 99):
        rc, msg = _step_assign(env, "sap_ff", rule)
        assert rc == -1 and "unknown assignment rule" in msg, (rule, rc, msg)
    assert env.last_kernel() == said
    same_bytes(snapshot(env), before, "nothing ran")
    # rule 0 is orlg_step_diag: the kernel that launches
    rc, msg = _step_assign(env, "sap_ff", 0, 20)
    assert rc == 0, msg
    assert env.last_kernel().split()[0] == kernel_name(step_kernel, 100, "full", ff=step_kernel == "wave", defer=True), env.last_kernel()
    env.close()


def test_a_gated_handle_is_refused():
    case = "nsfnet_s320_l150_sapff"
    topo, kw, _ = ggr.resolve_case(case)
    env = rmsa_env(topo, 4, gn_gate=ggr.case_gate(topo), **kw)
    for rule in (1, 2, 3, 4):
        for policy in ("sp_ff", "sap_ff", "llp_ff"):
            rc, msg = _step_assign(env, policy, rule)
            assert rc == -1 and "gn_gate" in msg, (policy, rule, rc, msg)
    with pytest.raises(ValueError, match="gn_gate"):
        env.run("sap_bf", 10)
    rc, msg = _step_assign(env, "sap_ff", 0)
    assert rc == 0, msg
    env.close()


# ---------------------------------------------------------------------------------------- 10. the drop-in surface
def test_view_callback_equals_the_device_policy(step_kernel):
    import optical_rl_gym_amd as pkg
    kw = dict(num_spectrum_resources=100, load=20, mean_service_holding_time=25, episode_length=200, seed=10)
    dev = rmsa_env(NSF, 1, step_kernel, **kw)
    tr = dev.run("sap_bf", 100, outputs=DECIDED)
    dev.close()
    view = pkg.make("RMSA-v0", topology=topology(NSF), **kw)
    heuristic = pkg.assignment_heuristic("sap", "best")
    for t in range(100):
        a = heuristic(view)
        assert tuple(a) == (tr["act_path"][t, 0], tr["act_slot"][t, 0]), t
        served = view.current_service
        view.step(a)
        assert served.accepted == bool(tr["accepted"][t, 0]), t
    wrapped = pkg.PathOnlyFirstFitAction(view, assign="last")
    assert wrapped.policy == "path_lf_external"
    mask = wrapped.action_masks()
    for p in range(view.k_paths):
        assert mask[p] == (wrapped.action(p) != (view.k_paths, 100)), p
    view.close()
