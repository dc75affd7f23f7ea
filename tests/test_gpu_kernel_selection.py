"""Which kernel instantiation every host selection path launches (csrc/orlg_variants.h: a launch builds a key from its
parameters, the key picks the kernel and words ``last_kernel()``).  The expected names are spelled by ``gpu_support.kernel_name``, which ``test_gpu_support.py`` holds to the written-out table; after each launch
the first token of ``last_kernel()`` must be that name and ``services_accepted`` what the C oracle has after the same steps.

RMSA: NSFNET with 320 slots, 8 environments; both step kernels, every statistics level, launches of 1, 8 and 20 steps (the
group kernel: release queue in HBM, the plain instantiation, the deferred link statistics under full statistics), each on a plain
handle, one with per-environment traffic and one that replays a trace, with ``sp_ff`` (the first-fit wave kernel) and ``llp_ff``
(the general one).  The bit rates are 3 x the reference's defaults (at most 289 of the 320 slots per request): some of 20 requests
block, and the accepted count tells environments and policies apart (the oracle's counts are required to differ).  The release
queue has 384 slots on every handle: the group kernel leaves the queue in HBM for launches of at most four steps only where that
lets more waves into a workgroup than the 12 it is capped at, and with the default capacities (128 slots at load 50, 64 for a
trace of 21 requests) 12 waves fit anyway at the lower statistics levels.  With 384 slots a wave's region is 22 336 B (25 152 B
with the link statistics) of the 160 KiB: 6 (5) waves with the queue in LDS, 12 without.
QoT-aware: US14 with its golden tables, 4 environments; ``bmfa`` and external actions (the oracle's own ``bmfa`` decisions), with
and without the periodic defragmentation and the GN-model gate, continuous bit rates, a trace.  The oracle has no continuous
mode: that case is held to the reference's own trace (golden ``cont_us14_s24_bmfa``), which is what the oracle stands for."""
import numpy as np
import pytest

from conftest import DEFAULT_BIT_RATES, load_golden, load_phy_tables, load_topology, oracle_env_from_kwargs, phy_oracle_from_kwargs
from gpu_support import device_log_fixture, kernel_name, phy_env as make_phy, rmsa_env  # noqa: F401

pytestmark = pytest.mark.gpu

B, STEPS = 8, (1, 8, 20)
BIT_RATES = [3 * r for r in DEFAULT_BIT_RATES]
KW = dict(num_spectrum_resources=320, mean_service_holding_time=25, episode_length=1000, bit_rates=BIT_RATES, queue_capacity=384)
LOADS, SEEDS_PER_LOAD = (20.0, 200.0), 4   # the handle with per-environment traffic
POLICIES = ("sp_ff", "llp_ff")



def expected_name(kernel, policy, kind, stats, launch):
    """After launches of 1, 8 and 20 steps (launch 0, 1, 2).  The group kernel: the release queue in HBM for the one step, the
    deferred link statistics for the 20 under full statistics; a handle with per-environment traffic or a trace has instantiations
    of its own.  The wave-per-environment kernels read traffic and trace at run time: one set of names for the three kinds of
    handle, the first-fit kernel for sp_ff, and the deferred link statistics for the 20 steps under full statistics."""
    defer = launch == 2 and stats == "full"
    if kernel == "group":
        return kernel_name("group", 320, stats, hbmq=launch == 0, defer=defer, traffic=kind == "traffic", trace=kind == "trace")
    return kernel_name("wave", 320, stats, ff=policy == "sp_ff", defer=defer)


def env_kwargs(kind, i):
    """what environment i of a handle of this kind simulates, as kwargs of the oracle"""
    if kind == "traffic":
        return dict(KW, load=LOADS[i // SEEDS_PER_LOAD], seed=10 + i % SEEDS_PER_LOAD)
    return dict(KW, load=50, seed=10 + i)


_oracle = {}


def oracle_reference(topo, kind, policy):
    """services_accepted of every environment after 1, 8 and 20 steps, and the 21 requests of each (20 served, one pending).
    Computed once per (kind, policy); the device log must be installed in the oracle (device_log_in_oracle)."""
    key = (kind, policy)
    if key not in _oracle:
        accepted = np.zeros((len(STEPS), B), np.int64)
        cols = {f: [] for f in ("arrival", "holding", "src", "dst", "bit_rate")}
        for i in range(B):
            o = oracle_env_from_kwargs(topo, env_kwargs(kind, i))
            parts, done = [], 0
            for q, n in enumerate(STEPS):
                parts.append(o.run(policy, n - done, reset_on_done=True))
                done = n
                accepted[q, i] = o.counters()["services_accepted"]
            r = o.request()
            for f, last in zip(cols, (r.arrival_time, r.holding_time, r.src, r.dst, r.bit_rate)):
                cols[f].append(np.append(np.concatenate([p[f] for p in parts]), last))
            o.close()
        _oracle[key] = (accepted, {f: np.stack(v) for f, v in cols.items()})
    return _oracle[key]


def make_handle(topo, kind, policy, kernel, stats):
    from optical_rl_gym_amd import RequestTrace, make_sweep
    if kind == "plain":
        return rmsa_env(topo, B, kernel, stats_level=stats, load=50, seed=10, **KW)
    if kind == "traffic":
        return make_sweep("rmsa", topo, loads=LOADS, seeds_per_load=SEEDS_PER_LOAD, seed=10, step_kernel=kernel, stats_level=stats, **KW)
    # the oracle's own request streams of the plain handle (env-major [B][21]), replayed
    _, req = oracle_reference(topo, "plain", policy)
    trace = RequestTrace(req["arrival"], req["holding"], req["src"].astype(np.int32), req["dst"].astype(np.int32),
                         req["bit_rate"].astype(np.int32), batch_size=B, layout="env")
    kw = {k: v for k, v in KW.items() if k != "mean_service_holding_time"}
    return rmsa_env(topo, B, kernel, stats_level=stats, trace=trace, **kw)


def test_the_oracle_counts_tell_the_cases_apart(nsfnet, device_log_in_oracle):
    """(what makes the accepted counts below a check: requests block within 20 steps, differently per policy and environment)"""
    sp, _ = oracle_reference(nsfnet, "plain", "sp_ff")
    llp, _ = oracle_reference(nsfnet, "plain", "llp_ff")
    sweep, _ = oracle_reference(nsfnet, "traffic", "sp_ff")
    assert (sp[2] < 20).any() and len(set(sp[2].tolist())) > 1
    assert not np.array_equal(sp, llp) and not np.array_equal(sp, sweep)


@pytest.mark.parametrize("stats", ["counters", "network", "full"])
@pytest.mark.parametrize("kernel", ["wave", "group"])
def test_rmsa_selection(nsfnet, device_log_in_oracle, kernel, stats):
    for launch, n in enumerate(STEPS):
        for kind in ("plain", "traffic", "trace"):
            for policy in POLICIES:
                want, _ = oracle_reference(nsfnet, "plain" if kind == "trace" else kind, policy)
                env = make_handle(nsfnet, kind, policy, kernel, stats)
                env.run(policy, n, outputs=("accepted",))
                case = (kernel, stats, n, kind, policy)
                print(case, env.last_kernel(), env.counters()["services_accepted"].tolist(), want[launch].tolist())
                assert env.last_kernel().split(" ")[0] == expected_name(kernel, policy, kind, stats, launch), (case, env.last_kernel())
                assert np.array_equal(env.counters()["services_accepted"], want[launch]), case
                env.close()


# ------------------------------------------------------------------------------------------------ QoT-aware
PB, PN = 4, 20
PHY_KW = dict(load=1400, mean_service_holding_time=25, episode_length=200, seed=10, grooming=False)
DEFRAG = dict(defrag_period=6, number_moves=5, metric="cut")
PHY_CASES = [   # (id, defragmentation, GN gate, external actions, expected name)
    ("bmfa", False, False, False, "orlg_phy_kernel<5,false,false,0>"),
    ("bmfa-defrag", True, False, False, "orlg_phy_kernel<5,true,false,0>"),
    ("bmfa-gn", False, True, False, "orlg_phy_kernel<5,false,true,0>"),
    ("bmfa-defrag-gn", True, True, False, "orlg_phy_kernel<5,true,true,0>"),
    ("external", False, False, True, "orlg_phy_kernel<5,false,false,-1>"),
    ("external-defrag", True, False, True, "orlg_phy_kernel<5,true,false,-1>"),
    ("external-gn", False, True, True, "orlg_phy_kernel<5,false,true,-1>"),
    ("external-defrag-gn", True, True, True, "orlg_phy_kernel<5,true,true,-1>")]


@pytest.fixture(scope="module")
def us14():
    return load_topology("us14_3-paths_6-modulations"), load_phy_tables("us14_k3")


@pytest.mark.parametrize("case,defrag,gn,external,name", PHY_CASES, ids=[c[0] for c in PHY_CASES])
def test_phy_selection(us14, device_log_in_oracle, case, defrag, gn, external, name):
    from optical_rl_gym_amd import gn_gate_parameters
    topo, tables = us14
    kw = dict(PHY_KW, **(DEFRAG if defrag else {}), **(dict(gn_gate=gn_gate_parameters(topo)) if gn else {}))
    env = make_phy(topo, tables, kw, PB)
    oracles = [phy_oracle_from_kwargs(topo, tables, kw, seed=10 + i) for i in range(PB)]
    if not external:
        env.run("bmfa", PN, outputs=("accepted",), auto_reset=True)
        assert env.last_kernel().split(" ")[0] == name, env.last_kernel()
        for o in oracles:
            o.run("bmfa", PN, reset_on_done=True)
    else:   # the oracle's own bmfa decisions, one launch per step
        for t in range(PN):
            paths, chans, acts = np.full(PB, -2, np.int32), np.full((PB, 14), -1, np.int16), []
            for i, o in enumerate(oracles):
                a = o.policy("bmfa")
                paths[i] = a.path
                for q in range(a.n):
                    chans[i, q] = a.ch[q] | (int(a.used[q]) << 9)
                acts.append(a)
            env.run("external", 1, act_path=paths, act_channels=chans, outputs=("accepted",), auto_reset=True)
            assert env.last_kernel().split(" ")[0] == name, (t, env.last_kernel())
            for i, o in enumerate(oracles):
                o.step(acts[i])
    got = env.counters()["services_accepted"]
    want = [o.counters()["services_accepted"] for o in oracles]
    print(case, env.last_kernel(), got.tolist(), want)
    assert got.tolist() == want
    for o in oracles:
        o.close()
    env.close()


def test_phy_selection_continuous(us14):
    """the reference's own trace at seed 24 in every environment (the oracle has no continuous mode)"""
    z, meta = load_golden("cont_us14_s24_bmfa")
    topo, tables = us14
    kw = meta["env_kwargs"]
    env = make_phy(topo, tables, kw, PB, seeds=[kw["seed"]] * PB)
    tr = env.run("bmfa", PN, outputs=("accepted", "act_path"), auto_reset=True)
    print(env.last_kernel(), env.counters()["services_accepted"].tolist(), int(z["services_accepted"][PN - 1]))
    assert env.last_kernel().split(" ")[0] == "orlg_phy_kernel<5,false,false,0,true>", env.last_kernel()
    assert env.counters()["services_accepted"].tolist() == [int(z["services_accepted"][PN - 1])] * PB
    for i in range(PB):
        assert np.array_equal(tr["act_path"][:, i], z["act_path"][:PN]), i
    env.close()


def test_phy_selection_trace(us14):
    """the reference's stream of golden phy_us14_s10_bmfa replayed; the oracle (on libm, as the reference) at the same seed"""
    import oracle as orc
    from optical_rl_gym_amd import RequestTrace
    z, meta = load_golden("phy_us14_s10_bmfa")
    topo, tables = us14
    kw = meta["env_kwargs"]
    env = make_phy(topo, tables, {k: v for k, v in kw.items() if k not in ("load", "mean_service_holding_time", "seed")}, PB,
                   trace=RequestTrace.from_golden(z, batch_size=PB))
    env.run("bmfa", PN, outputs=("accepted",), auto_reset=True)
    orc.set_log_fn(None)
    o = phy_oracle_from_kwargs(topo, tables, kw)
    o.run("bmfa", PN, reset_on_done=True)
    print(env.last_kernel(), env.counters()["services_accepted"].tolist(), o.counters()["services_accepted"])
    assert env.last_kernel().split(" ")[0] == "orlg_phy_kernel<5,false,false,0,false,true>", env.last_kernel()
    assert env.counters()["services_accepted"].tolist() == [o.counters()["services_accepted"]] * PB
    o.close(); env.close()
