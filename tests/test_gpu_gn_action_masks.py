"""Action masks that know the GN-model admission check (``orlg_gn_action_masks``: kinds ``path_ff_gn`` / ``deeprmsa_gn``) and the
policy ``sap_ff_gn`` on the device, held to the CPU reference of ``gn_candidates_reference.py``: masks exact, GSNR
rows to rtol 1e-9 (the tolerance ``test_gpu_rmsa_gn_gate.py`` uses for the same arithmetic) with NaN in the same places; to the
gated step itself bit for bit; and to each other across launch lengths, batch sizes, buffers and views."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import gn_candidates_reference as cref
import gn_gate_reference as ref
from conftest import load_topology
from gpu_support import kernel_name, rmsa_env, snapshot, state_matches

pytestmark = pytest.mark.gpu

RTOL = 1e-9
B = cref.B
OUTS = ("act_path", "act_slot", "accepted", "done", "request", "reward", "gn_gsnr_db")
NSFNET = "nsfnet_chen_5-paths_6-modulations"


def _gsnr_matches(dev, want, what):
    assert np.array_equal(np.isnan(dev), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.allclose(dev[ok], want[ok], rtol=RTOL, atol=0), (what, float(np.max(np.abs(dev[ok] / want[ok] - 1))))


def _gated_env(case, batch=B, j=1, gate_over=None, **over):
    c = ref.CASES[case]
    topo = load_topology(c["topology"])
    return rmsa_env(topo, batch, gn_gate=ref.case_gate(topo, **(gate_over or {})), j=j, **ref.case_kwargs(case, **over)), topo, c


def _gn_masks(env):
    """both new masks with their GSNR rows, the rejection's column checked and cut off"""
    K, j, r = env.k_paths, env.j, env.reject_action
    ff, ff_g = env.action_masks("path_ff_gn", gsnr_out=True)
    dp, dp_g = env.action_masks("deeprmsa_gn", gsnr_out=True)
    assert ff.shape == (env.batch_size, K + r) and dp.shape == (env.batch_size, K * j + r)
    assert ff_g.shape == (env.batch_size, K) and dp_g.shape == (env.batch_size, K * j)
    if r:
        assert (ff[:, K] == 1).all() and (dp[:, K * j] == 1).all()
    return ff[:, :K], ff_g, dp[:, :K * j], dp_g


def _masks_match(env, runs, t, what):
    """the device's masks of now against row t of the reference's runs (one per environment)"""
    ff, ff_g, dp, dp_g = _gn_masks(env)
    for i, (tr, _, _) in enumerate(runs):
        assert np.array_equal(ff[i], tr["path_ff_gn"][t]), (what, t, i, ff[i], tr["path_ff_gn"][t], ff_g[i], tr["path_ff_gsnr"][t])
        assert np.array_equal(dp[i], tr["deeprmsa_gn"][t]), (what, t, i, dp[i], tr["deeprmsa_gn"][t])
        _gsnr_matches(ff_g[i], tr["path_ff_gsnr"][t], (what, "path_ff", t, i))
        _gsnr_matches(dp_g[i], tr["deeprmsa_gsnr"][t], (what, "deeprmsa", t, i))
    return ff, ff_g


# ---------------------------------------------------------------------------------------- 1. oracle parity
@pytest.mark.parametrize("case,j,n,extra", [
    ("nsfnet_s320_l50_sapff", 1, 300, {}),
    ("nsfnet_s100_l20_spff", 2, 300, dict(allow_rejection=True)),
    ("jpn12_s320_l150_sapff", 1, 300, dict(queue_capacity=128)),   # the release ring wraps: more provisions than slots
    ("ring34_s100_l60_sapff", 1, 300, {}),                          # 238 links: four words of link set per running service
    ("ring36_s512_l500_sapff", 1, 100, {}),                         # eight words per link, candidates of up to 14 hops
])
def test_masks_against_the_oracle(case, j, n, extra):
    """The case's policy steps eight environments one launch per step; before every step (after reset, then after each step
    but the last) both masks are exact and both GSNR rows agree with the reference."""
    env, topo, c = _gated_env(case, j=j, **extra)
    runs = cref.run_batch(case, j=j, n_steps=n)
    if "queue_capacity" in extra:
        assert all(fig["provisions"] > extra["queue_capacity"] > fig["max_running"] for _, _, fig in runs)
    steps = []
    for t in range(n):
        _masks_match(env, runs, t, case)
        steps.append(env.run(c["policy"], 1, outputs=OUTS, auto_reset=True))
    tr = {k: np.concatenate([s[k] for s in steps]) for k in OUTS}
    state = snapshot(env, save_state=False)
    for i, (want, final, _) in enumerate(runs):
        for name in ("act_path", "act_slot", "accepted", "done", "request"):
            assert np.array_equal(tr[name][:, i], want[name]), (case, name, i)
        _gsnr_matches(tr["gn_gsnr_db"][:, i], want["gsnr"], (case, i))
        state_matches(state, i, final, (case, i))
    env.close()


# ---------------------------------------------------------------------------------------- 2. mask == step, bit for bit
def test_mask_is_the_step_bit_for_bit():
    """B = 64, NSFNET-320 at load 50, j = 2, the state after 150 steps: for every action of Discrete(k j) and every path, the
    step from that state accepts exactly where the mask says so and its gn_gsnr_db has the bytes of the mask's GSNR column."""
    env, topo, c = _gated_env("nsfnet_s320_l50_sapff", batch=64, j=2)
    env.run("sap_ff", 150, auto_reset=True)
    state = env.save_state()
    ff, ff_g, dp, dp_g = _gn_masks(env)
    K, j = topo.k_paths, 2
    assert 0 < dp.mean() < 1 and 0 < ff.mean() < 1 and np.isnan(dp_g).any() and np.isfinite(dp_g[:, 1::2]).any()
    refused = 0
    for a in range(K * j):
        env.load_state(state)
        r = env.step_deeprmsa(np.full(64, a, np.int32), outputs=("accepted", "gn_gsnr_db"))
        assert np.array_equal(r["accepted"], dp[:, a]), a
        assert np.ascontiguousarray(r["gn_gsnr_db"]).tobytes() == np.ascontiguousarray(dp_g[:, a]).tobytes(), a
        refused += int((np.isfinite(dp_g[:, a]) & (dp[:, a] == 0)).sum())
    for p in range(K):
        env.load_state(state)
        r = env.step_path_first_fit(np.full(64, p, np.int32), outputs=("accepted", "gn_gsnr_db"))
        assert np.array_equal(r["accepted"], ff[:, p]), p
        assert np.ascontiguousarray(r["gn_gsnr_db"]).tobytes() == np.ascontiguousarray(ff_g[:, p]).tobytes(), p
    assert refused > 0   # (windows that are free and that the gate refuses)
    env.close()


# ---------------------------------------------------------------------------------------- 3. sap_ff_gn
@pytest.mark.parametrize("case", ["jpn12_s320_l150_sapff", "nsfnet_s320_l50_sapff"])
def test_sap_ff_gn_against_the_oracle(case):
    """300 launches of one step against the reference (decisions, requests, counters, occupancy, clock exact, GSNR to rtol 1e-9),
    each against the path_ff_gn mask taken just before it; then one launch of 300 steps: the same bytes."""
    env, topo, c = _gated_env(case)
    K, n = topo.k_paths, cref.N_STEPS
    runs = cref.run_batch(case, policy="sap_ff_gn")
    steps = []
    for t in range(n):
        ff, ff_g = _masks_match(env, runs, t, case)
        r = env.run("sap_ff_gn", 1, outputs=OUTS, auto_reset=True)
        assert env.last_kernel().startswith(kernel_name("wave", env.words_per_link, "full", gn=True)), env.last_kernel()
        # the step accepts iff a column of the mask is set; it then shows the first such column and that column's GSNR
        acc = r["accepted"][0] != 0
        assert np.array_equal(acc, ff.any(axis=1)), t
        first = ff.argmax(axis=1)
        assert np.array_equal(r["act_path"][0][acc], first[acc]), t
        assert r["gn_gsnr_db"][0][acc].tobytes() == ff_g[acc, first[acc]].tobytes(), t
        # refused: the first candidate that was checked, the first path with a fit; no fit at all: the rejection, no check
        has_fit = np.isfinite(ff_g).any(axis=1)
        shown = np.where(has_fit, np.isfinite(ff_g).argmax(axis=1), K)
        assert np.array_equal(r["act_path"][0][~acc], shown[~acc]), t
        rej = ~acc & has_fit
        assert r["gn_gsnr_db"][0][rej].tobytes() == ff_g[rej, shown[rej]].tobytes(), t
        assert np.isnan(r["gn_gsnr_db"][0][~has_fit]).all() and (r["act_slot"][0][~has_fit] == c["S"]).all(), t
        steps.append(r)
    tr = {k: np.concatenate([s[k] for s in steps]) for k in OUTS}
    state = snapshot(env)
    for i, (want, final, fig) in enumerate(runs):
        for name in ("act_path", "act_slot", "accepted", "done", "request"):
            assert np.array_equal(tr[name][:, i], want[name]), (case, name, i)
        _gsnr_matches(tr["gn_gsnr_db"][:, i], want["gsnr"], (case, i))
        state_matches(state, i, final, (case, i))
    env.close()
    env, _, _ = _gated_env(case)
    long = env.run("sap_ff_gn", n, outputs=OUTS, auto_reset=True)
    for k in OUTS:
        assert long[k].tobytes() == tr[k].tobytes(), k
    assert env.save_state().tobytes() == state["state"].tobytes()
    env.close()


def test_sap_ff_gn_beyond_the_resident_waves():
    """B = 4200, across the boundary between the environments taken statically and by ticket: the first eight environments have
    the bytes of B = 8, and environments on both sides of the boundary agree with the reference."""
    case, n = "nsfnet_s320_l50_sapff", 200
    small, _, c = _gated_env(case)
    big, _, _ = _gated_env(case, batch=4200)
    a, b = small.run("sap_ff_gn", n, outputs=OUTS, auto_reset=True), big.run("sap_ff_gn", n, outputs=OUTS, auto_reset=True)
    assert big.last_kernel().startswith("orlg_rmsa_kernel<5,2,false,true>"), big.last_kernel()
    for k in OUTS:
        assert np.ascontiguousarray(b[k][:, :B]).tobytes() == a[k].tobytes(), k
    for i in (4095, 4096, 4199):
        want, _, _ = cref.run_case(case, seed=c["seed"] + i, policy="sap_ff_gn", n_steps=n)
        for name in ("act_path", "act_slot", "accepted", "done"):
            assert np.array_equal(b[name][:, i], want[name]), (name, i)
        _gsnr_matches(b["gn_gsnr_db"][:, i], want["gsnr"], i)
    # the masks of the large batch: the first eight environments as the small batch's
    for x, y in zip(_gn_masks(small), _gn_masks(big)):
        assert np.ascontiguousarray(y[:B]).tobytes() == x.tobytes()
    small.close()
    big.close()


def test_a_gate_that_passes_everything():
    """At 0 dBm per 50 GHz the gate refuses nothing on NSFNET: sap_ff_gn is sap_ff byte for byte, and the _gn masks are the plain
    ones."""
    case = "nsfnet_s320_l50_sapff"
    a, _, _ = _gated_env(case, j=2, gate_over=dict(launch_power_dbm_per_50ghz=0.0), allow_rejection=True)
    b, _, _ = _gated_env(case, j=2, gate_over=dict(launch_power_dbm_per_50ghz=0.0), allow_rejection=True)
    for n in (1, 120, 1):
        ra, rb = a.run("sap_ff_gn", n, outputs=OUTS, auto_reset=True), b.run("sap_ff", n, outputs=OUTS, auto_reset=True)
        for k in OUTS:
            assert ra[k].tobytes() == rb[k].tobytes(), (n, k)
        assert a.save_state().tobytes() == b.save_state().tobytes(), n
        assert a.action_masks("path_ff_gn").tobytes() == a.action_masks("path_ff").tobytes(), n
        assert a.action_masks("deeprmsa_gn").tobytes() == a.action_masks("deeprmsa").tobytes(), n
    assert 0 < a.action_masks("deeprmsa")[:, :-1].mean() < 1
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------- 4. buffers
def test_buffers_pageable_pinned_device():
    """The new masks and GSNR rows into pageable, pinned and device (torch) buffers: the same bytes.  In a child process: torch
    has to create its HIP context before the library does."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys
        import numpy as np, torch
        torch.zeros(1, device="cuda")
        sys.path[:0] = [%r, %r]
        import gn_gate_reference as ref
        from conftest import load_topology
        from optical_rl_gym_amd import BatchedRMSAEnv
        case = "nsfnet_s320_l50_sapff"
        topo = load_topology(ref.CASES[case]["topology"])
        env = BatchedRMSAEnv(topo, 64, gn_gate=ref.case_gate(topo), j=2, allow_rejection=True, **ref.case_kwargs(case))
        env.run("sap_ff_gn", 150, auto_reset=True)
        for kind in ("path_ff_gn", "deeprmsa_gn"):
            m, g = env.action_masks(kind, gsnr_out=True)
            assert env.action_masks(kind).tobytes() == m.tobytes()            # the mask alone
            assert 0 < m[:, :-1].mean() < 1 and np.isfinite(g).any() and (kind == "path_ff_gn" or np.isnan(g).any())
            ms, gs = env.action_mask_shape(kind)[0], env.action_mask_gsnr_shape(kind)[0]
            hm, hg = np.full(ms, 9, np.uint8), np.full(gs, 7.0)
            r = env.action_masks(kind, out=hm, gsnr_out=hg)
            assert r[0] is hm and r[1] is hg and hm.tobytes() == m.tobytes() and hg.tobytes() == g.tobytes()
            pm, pg = torch.full(ms, 9, dtype=torch.uint8).pin_memory(), torch.full(gs, 7.0, dtype=torch.float64).pin_memory()
            env.action_masks(kind, out=pm, gsnr_out=pg)
            env.synchronize()
            assert pm.numpy().tobytes() == m.tobytes() and pg.numpy().tobytes() == g.tobytes()
            dm, dg = torch.full(ms, 9, dtype=torch.uint8, device="cuda"), torch.full(gs, 7.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            env.action_masks(kind, out=dm, gsnr_out=dg)
            env.synchronize()
            assert dm.cpu().numpy().tobytes() == m.tobytes() and dg.cpu().numpy().tobytes() == g.tobytes()
            # mixed: device mask, pageable GSNR
            dm.fill_(9); hg[:] = 7.0; torch.cuda.synchronize()
            env.action_masks(kind, out=dm, gsnr_out=hg)
            env.synchronize()
            assert dm.cpu().numpy().tobytes() == m.tobytes() and hg.tobytes() == g.tobytes()
        env.close()
        print("gn mask buffers ok")
    """) % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "gn mask buffers ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_the_existing_masks_do_not_know_the_gate():
    """The kinds deeprmsa, path_ff, slots and the fused observation mask on a gated handle: byte-identical to the same calls on a
    handle without a gate loaded with the same snapshot."""
    case = "nsfnet_s320_l50_sapff"
    gated, topo, c = _gated_env(case, batch=32, j=2, allow_rejection=True)
    plain = rmsa_env(topo, 32, j=2, allow_rejection=True, **ref.case_kwargs(case))
    gated.run("sap_ff", 150, auto_reset=True)
    plain.load_state(gated.save_state())
    for kind in ("deeprmsa", "path_ff", "slots"):
        assert gated.action_masks(kind).tobytes() == plain.action_masks(kind).tobytes(), kind
    (og, mg), (op, mp) = gated.observation(return_mask=True), plain.observation(return_mask=True)
    assert og.tobytes() == op.tobytes() and mg.tobytes() == mp.tobytes()
    assert (gated.action_masks("path_ff_gn") != gated.action_masks("path_ff")).any()   # (the gate does refuse windows here)
    gated.close()
    plain.close()


# ---------------------------------------------------------------------------------------- 5. views
def test_views():
    from optical_rl_gym_amd import (BatchedDeepRMSAEnv, DeepRMSAEnv, PathOnlyFirstFitAction, RMSAEnv,
                                    evaluate_heuristic_batched, shortest_available_path_first_fit_gn)
    topo = load_topology(NSFNET)
    gate = ref.case_gate(topo)
    dkw = dict(mean_service_holding_time=25.0, mean_service_inter_arrival_time=0.5, num_spectrum_resources=320, seed=21, j=2)
    deep, batched = DeepRMSAEnv(topology=topo, gn_gate=gate, **dkw), BatchedDeepRMSAEnv(topo, 1, gn_gate=gate, **dkw)
    differ = 0
    for t in range(120):
        m, want = deep.action_masks(gn=True), batched.action_masks("deeprmsa_gn")[0].astype(bool)
        assert m.dtype == bool and np.array_equal(m, want), t
        assert np.array_equal(deep.action_masks(), batched.action_masks("deeprmsa")[0].astype(bool)), t
        differ += int((m != deep.action_masks()).any())
        a = int(np.flatnonzero(deep.action_masks())[t % int(deep.action_masks().sum())]) if deep.action_masks().any() else 0
        _, _, _, info = deep.step(a)
        batched.step_deeprmsa(np.array([a], np.int32))
        assert deep._last_served.accepted == bool(m[a]), (t, a)   # the gated mask is what the step did
    assert differ > 0
    deep.close()
    batched.close()
    # PathOnlyFirstFitAction, and the callback against the device policy
    kw = dict(num_spectrum_resources=320, load=50, mean_service_holding_time=25, seed=10, episode_length=200)
    view = PathOnlyFirstFitAction(RMSAEnv(topology=topo, gn_gate=gate, **kw))
    dev = rmsa_env(topo, 1, gn_gate=gate, **kw)
    with pytest.raises(ValueError, match="slot matrix"):
        view.env.action_masks(gn=True)
    for t in range(150):
        assert np.array_equal(view.action_masks(gn=True), dev.action_masks("path_ff_gn")[0].astype(bool)), t
        p, s = shortest_available_path_first_fit_gn(view.env)
        _, _, done, info = view.env.step((p, s))
        r = dev.run("sap_ff_gn", 1, outputs=OUTS)
        assert (p, s) == (int(r["act_path"][0, 0]), int(r["act_slot"][0, 0])), t
        assert view.env._last_served.accepted == bool(r["accepted"][0, 0]) and done == bool(r["done"][0, 0]), t
        assert np.array([info["gn_gsnr_db"]]).tobytes() == r["gn_gsnr_db"][0].tobytes(), t
    assert np.array_equal(view.env._batched.occupancy_words(), dev.occupancy_words())
    view.env.close()
    dev.close()
    # evaluate_heuristic_batched drives the policy by name
    env = rmsa_env(topo, 4, gn_gate=gate, **dict(kw, episode_length=50))
    rewards, lengths, _ = evaluate_heuristic_batched(env, "sap_ff_gn", n_eval_episodes=2)
    assert rewards.shape == (2, 4) and (lengths == 49).all() and (rewards > 0).all()
    env.close()


# ---------------------------------------------------------------------------------------- 6. the library's own refusals
def test_refusals_of_the_library():
    from optical_rl_gym_amd import OrlgError, _lib
    topo = load_topology(NSFNET)
    kw = dict(num_spectrum_resources=100, load=20, mean_service_holding_time=25, seed=1)
    env = rmsa_env(topo, 4, **kw)
    with pytest.raises(OrlgError, match="gn_gate") as e:
        env.run("sap_ff_gn", 1)
    assert e.value.code == -1
    io = _lib.StepIO()
    assert env.L.orlg_step(env.h, 7, 1, None, 0, C.byref(io)) == -1 and b"gn_gate" in env.L.orlg_last_error()
    assert env.L.orlg_step(env.h, 8, 1, None, 0, C.byref(io)) == -1 and b"unknown policy" in env.L.orlg_last_error()
    m, g = np.zeros((4, topo.k_paths), np.uint8), np.zeros((4, topo.k_paths))
    pm, pg = m.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p)
    assert env.L.orlg_gn_action_masks(env.h, pm, pg, None, None) == -1 and b"gn_gate" in env.L.orlg_last_error()
    assert env.L.orlg_gn_action_masks(None, pm, pg, None, None) == -1
    env.run("sap_ff", 3)   # the handle goes on
    env.close()
    env = rmsa_env(topo, 4, gn_gate=ref.case_gate(topo), **kw)
    assert env.L.orlg_gn_action_masks(env.h, None, None, None, None) == -1 and b"null argument" in env.L.orlg_last_error()
    assert env.L.orlg_step(env.h, 8, 1, None, 0, C.byref(io)) == -1 and b"unknown policy" in env.L.orlg_last_error()
    assert env.L.orlg_gn_action_masks(env.h, None, pg, None, None) == 0 and np.isfinite(g).any()   # a GSNR row alone
    env.close()
