"""The RMSA step kernels above 64 and above 128 links, device against oracle (the oracle on the library's host build of the device
logarithm, every comparison exact): ``ring34`` (238 links: 238 % 4 = 2, % 8 = 6, % 16 = 14; numpy's pairwise sum splits 112 + 126)
and ``ring36`` (108 links, paths of 14 hops), the link lists of ``tests/golden/topology_txt/`` whose figures
``test_many_links.py`` pins and on which ``test_oracle_golden.py`` holds the oracle to the reference.  What only does anything
different at these sizes: the split of ``np_mean``, the second pass of ``link_replay<64>`` and the fifteen of ``link_replay<16>``,
link ids of 128 and above read back from a byte, ``lint_stride`` 240 against 238 links, a partial last chunk of eight links in the
reset path.  ``last_kernel()`` is asserted wherever a test is about one instantiation.  (The GN-model admission check above 64
links: the ``ring3*`` cases of ``gn_gate_reference.CASES`` in ``test_gpu_rmsa_gn_gate.py``.)"""
import ctypes as C

import numpy as np
import pytest

import gpu_support as gs
from conftest import oracle_env_from_kwargs
from gpu_support import check_against_oracles, decisions_match, device_log_in_oracle, kernel_name, rmsa_env, snapshot, state_matches, tooling_env, topology

pytestmark = pytest.mark.gpu

RING34, RING36 = "ring34_3-paths_6-modulations", "ring36_3-paths_6-modulations"
LIGHT = dict(S=100, load=60)     # two words per link, a queue of 144 slots
HEAVY = dict(S=320, load=300)    # five words per link, a queue of 480 slots
B, SEED, EPISODE = 3, 5, 200     # environment i: seed 5 + i; two episode ends (full-network link updates) in 300 steps
DECISIONS = ("act_path", "act_slot", "accepted", "done")
LINK_OUTS = ("avg_link_compactness", "avg_link_utilization", "network_compactness", "network_compactness_difference")
LLOG_FLUSH = 40                  # ORLG_LLOG_FLUSH (csrc/orlg_link_stats.h)


def _kw(S, load, seed=SEED):
    return dict(num_spectrum_resources=S, load=load, mean_service_holding_time=25, episode_length=EPISODE, seed=seed)


def _env(name, shape, kernel, **extra):
    return rmsa_env(name, B, kernel, **_kw(**shape), **extra)


def _kernel(env):
    return env.last_kernel().split()[0]


def oracle_run(name, S, load, i, policy, launches):
    return gs.oracle_run(name, tuple(sorted(_kw(S, load).items())), SEED + i, policy, launches)


def _decisions_match(tr, i, want, what):
    decisions_match(tr, i, want, DECISIONS, what)   # (these launches ask for neither arrival nor holding)


def _read_state(env):
    return snapshot(env, save_state=False)


# ---------------------------------------------------------------------------------------- the per-step link averages
@pytest.mark.parametrize("kernel", ["wave", "group"])
@pytest.mark.parametrize("name", [RING34, RING36])
def test_link_averages_are_exact(name, kernel):
    """avg_link_compactness and avg_link_utilization of every step, np.mean over 238 links (numpy's pairwise sum split 112 + 126)
    and over 108 (one block): equal to the oracle's, whose own sum test_oracle_golden.py holds to the reference's on these
    networks.  Asking for them selects the instantiations that keep the link statistics up to date in place."""
    env = _env(name, LIGHT, kernel)
    tr = env.run("sap_ff", 300, outputs=DECISIONS + LINK_OUTS, auto_reset=True)
    assert _kernel(env) == kernel_name(kernel, 2, "full", ff=kernel == "wave"), env.last_kernel()
    st = _read_state(env)
    for i in range(B):
        (want,), final = oracle_run(name, LIGHT["S"], LIGHT["load"], i, "sap_ff", (300,))
        _decisions_match(tr, i, want, name)
        for f in LINK_OUTS:
            bad = np.flatnonzero(tr[f][:, i] != want[f])
            assert bad.size == 0, (f, i, bad[:4], tr[f][bad[:4], i], want[f][bad[:4]])
        assert len(np.unique(want["avg_link_utilization"])) > 150   # (it moves with every provision and release)
        state_matches(st, i, final, name)
    env.close()


# ---------------------------------------------------------------------------------------- deferred link statistics
def _log_entries(topo, tr, t0):
    """What the links log during a launch, from the oracle's trace of it (t0: the clock at its start): one entry per provision and
    per release of a service provisioned in it, one per episode end.  A lower bound: releases of earlier services come on top."""
    cnt = np.zeros(topo.num_links, np.int64)
    now = np.concatenate([[t0], tr["current_time"]])
    for i in np.flatnonzero(tr["accepted"]):
        g = int(topo.pair_path_base[tr["src"][i] * topo.num_nodes + tr["dst"][i]]) + int(tr["act_path"][i])
        links = topo.path_links[topo.path_link_off[g]:topo.path_link_off[g + 1]]
        cnt[links] += 1 + (tr["arrival"][i] + tr["holding"][i] <= now[-1])
    return cnt + int(tr["done"].sum())


@pytest.mark.parametrize("kernel", ["wave", "group"])
def test_deferred_link_statistics_equal_the_ones_kept_in_place(kernel):
    """ring34, S = 320, load 300: a launch of 300 steps and one of 600 without the link outputs run the instantiations that log
    the links' updates and replay them one link per lane (link_replay<64>: two passes over 238 links; link_replay<16> of the group
    kernel: fifteen).  In the second launch links below and above id 64 log ORLG_LLOG_FLUSH entries and more, so the replay runs
    inside the launch (in the first, 300 steps, a link reaches about 35: worked off at its end).  The same launches under
    ORLG_NO_DEFER on a second handle; both against the oracle, and byte for byte against each other."""
    launches = (300, 600)
    deferred, plain = (kernel_name(kernel, 5, "full", ff=kernel == "wave", defer=d) for d in (True, False))
    topo = topology(RING34)
    a = _env(RING34, HEAVY, kernel)
    for n in launches:
        a.run("sap_ff", n, auto_reset=True)
        assert _kernel(a) == deferred, a.last_kernel()
    with tooling_env(ORLG_NO_DEFER="1"):
        b = _env(RING34, HEAVY, kernel)
        for n in launches:
            b.run("sap_ff", n, auto_reset=True)
            assert _kernel(b) == plain, b.last_kernel()
        sb = b.save_state()
    sa, sb_state = _read_state(a), _read_state(b)
    full = 0
    for i in range(B):
        (t1, t2), final = oracle_run(RING34, HEAVY["S"], HEAVY["load"], i, "sap_ff", launches)
        entries = _log_entries(topo, t2, t1["current_time"][-1])
        full += entries[:64].max() >= LLOG_FLUSH and entries[64:].max() >= LLOG_FLUSH
        state_matches(sa, i, final, "deferred")
        state_matches(sb_state, i, final, "in place")
    assert full == B, full   # every environment replays inside the second launch, full logs in both passes of link_replay<64>
    assert a.save_state().tobytes() == sb.tobytes()
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------- statistics levels, launches of one step
def _group_plan(env, stats, n_steps):
    """(shape, layouts, kind) of a launch of the group kernel on this handle's shape: orlg_debug_layout into orlg_debug_group_plan"""
    fields = gs._fields("ORLG_SHAPE_FIELDS")
    out = (C.c_int32 * len(fields))()
    env.L.orlg_debug_layout.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int]
    assert env.L.orlg_debug_layout(env.h, out, len(fields)) == len(fields)
    shape = dict(zip(fields, out))
    args = dict(NW=shape["NW"], E=shape["E"], Q=shape["Q"], lint_stride=shape["lint_stride"], stats_level=stats,
                shared_bytes=shape["l_shared_bytes"], B=B, n_steps=n_steps, policy=gs.SAP, out_mask=gs.OUT_ACCEPTED, br_width=0,
                no_defer=0, no_chunks=0, no_lean=0, wpb=0, chunks=0, num_cu=256, resident=256)
    layouts, p = gs.group_plan(args)
    return shape, layouts, p["kind"]


@pytest.mark.parametrize("kernel", ["wave", "group"])
@pytest.mark.parametrize("stats", ["counters", "network", "full"])
def test_statistics_levels_and_launches_of_one_step(stats, kernel):
    """ring34, S = 320, load 300, every statistics level: one launch of 300 steps on one handle, 300 launches of one step on
    another; decisions, counters and occupancy against the oracle (the network compactness too where the level keeps it, the link
    and graph statistics at "full").  The group kernel at E = 238, S = 320, Q = 480 holds one wave per workgroup with the release
    queue in LDS; without the link statistics two fit when the queue stays in HBM, and the launches of one step take that
    instantiation -- asserted from the plan of the handle's own shape."""
    level = ("counters", "network", "full").index(stats)
    outs = DECISIONS + (("network_compactness",) if level >= 1 else ())
    long_run, short = _env(RING34, HEAVY, kernel, stats_level=stats), _env(RING34, HEAVY, kernel, stats_level=stats)
    tl = long_run.run("sap_ff", 300, outputs=outs, auto_reset=True)
    parts = []
    for _ in range(300):
        parts.append(short.run("sap_ff", 1, outputs=outs, auto_reset=True))
    ts = {k: np.concatenate([p[k] for p in parts]) for k in outs}
    assert _kernel(long_run) == kernel_name(kernel, 5, level, ff=kernel == "wave", defer=level == 2), long_run.last_kernel()
    if kernel == "wave":
        assert _kernel(short) == kernel_name("wave", 5, level, ff=True), short.last_kernel()
    else:
        shape, layouts, kind = _group_plan(short, level, 1)
        assert (shape["E"], shape["lint_stride"], shape["Q"], shape["NW"]) == (238, 240, 480, 1190)
        assert layouts["PLAIN"]["wpb_max"] >= 1 and (level < 2 or layouts["DEFER"]["wpb_max"] >= 1)   # it fits: nothing to skip
        assert kind == ("HBMQ" if level < 2 else "PLAIN")
        assert _kernel(short) == kernel_name("group", 5, level, hbmq=kind == "HBMQ"), short.last_kernel()
    sl, ss = _read_state(long_run), _read_state(short)
    for i in range(B):
        (want,), final = oracle_run(RING34, HEAVY["S"], HEAVY["load"], i, "sap_ff", (300,))
        for what, tr, st in (("300 steps", tl, sl), ("300 x 1 step", ts, ss)):
            _decisions_match(tr, i, want, (stats, what))
            if level >= 1:
                assert np.array_equal(tr["network_compactness"][:, i], want["network_compactness"]), (stats, what, i)
            state_matches(st, i, final, (stats, what), link_stats=level == 2)
    assert long_run.save_state().tobytes() == short.save_state().tobytes()
    long_run.close()
    short.close()


# ---------------------------------------------------------------------------------------- checkpoint
@pytest.mark.parametrize("kernel", ["wave", "group"])
def test_checkpoint_continues_alike(kernel):
    """ring34 (the span cache's rows are 240 entries apart for 238 links): 150 steps, save_state, 150 more; a fresh handle loads the
    snapshot and runs the same 150 -- outputs and saved state byte for byte; the original against the oracle's 300 steps."""
    outs = DECISIONS + ("arrival", "network_compactness")
    a = _env(RING34, LIGHT, kernel)
    first = a.run("sap_ff", 150, outputs=outs, auto_reset=True)
    snap = a.save_state()
    second = a.run("sap_ff", 150, outputs=outs, auto_reset=True)
    b = _env(RING34, LIGHT, kernel)
    b.load_state(snap)
    again = b.run("sap_ff", 150, outputs=outs, auto_reset=True)
    for name in outs:
        assert again[name].tobytes() == second[name].tobytes(), name
    assert a.save_state().tobytes() == b.save_state().tobytes()
    sa, sb = _read_state(a), _read_state(b)
    for i in range(B):
        (want,), final = oracle_run(RING34, LIGHT["S"], LIGHT["load"], i, "sap_ff", (300,))
        _decisions_match({k: np.concatenate([first[k], second[k]]) for k in DECISIONS}, i, want, "checkpoint")
        state_matches(sa, i, final, "original")
        state_matches(sb, i, final, "restored")
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------- valid-action masks
def test_action_masks_over_links_of_every_range():
    """The three masks of the whole batch on ring34 after 200 steps against the oracle's is_path_free for every (path, slot): the
    candidate paths of the pending requests run over links of every range of 64 ids, 128 and above among them."""
    env = _env(RING34, LIGHT, "wave")
    env.run("sap_ff", 200, auto_reset=True)
    topo = topology(RING34)
    oracles, ranges = [], set()
    with device_log_in_oracle():
        for i in range(B):
            o = oracle_env_from_kwargs(topo, _kw(**LIGHT), seed=SEED + i)
            o.run("sap_ff", 200, reset_on_done=True, fields=[])
            r = o.request()
            base = int(topo.pair_path_base[r.src * topo.num_nodes + r.dst])
            ranges |= {int(l) >> 6 for l in topo.path_links[topo.path_link_off[base]:topo.path_link_off[base + topo.k_paths]]}
            oracles.append(o)
    assert ranges == {0, 1, 2, 3}, ranges
    _, _, bits = check_against_oracles(env, oracles, "ring34")
    assert 0 < bits.mean() < 1
    for o in oracles:
        o.close()
    env.close()


# ---------------------------------------------------------------------------------------- the group kernel in chunks of steps
def test_group_kernel_chunks_carry_238_links_through_hbm():
    """ORLG_GROUP_CHUNKS=3: a 300-step launch of the group kernel as three chunks of 100 steps, the quad's state stored and loaded
    at every boundary; equal to the launch in one piece and to the oracle."""
    outs = DECISIONS + ("arrival", "network_compactness")
    whole = _env(RING34, HEAVY, "group")
    tw = whole.run("sap_ff", 300, outputs=outs, auto_reset=True)
    assert whole.last_kernel().endswith("chunks=1"), whole.last_kernel()
    with tooling_env(ORLG_GROUP_CHUNKS="3"):
        cut = _env(RING34, HEAVY, "group")
        tc = cut.run("sap_ff", 300, outputs=outs, auto_reset=True)
    assert _kernel(cut) == _kernel(whole) == kernel_name("group", 5, "full", defer=True) and cut.last_kernel().endswith("chunks=3"), cut.last_kernel()
    for name in outs:
        assert tc[name].tobytes() == tw[name].tobytes(), name
    assert cut.save_state().tobytes() == whole.save_state().tobytes()
    st = _read_state(cut)
    for i in range(B):
        (want,), final = oracle_run(RING34, HEAVY["S"], HEAVY["load"], i, "sap_ff", (300,))
        _decisions_match(tc, i, want, "chunks")
        state_matches(st, i, final, "chunks")
    whole.close()
    cut.close()
