"""More than eight candidate paths per pair (``orlg_create`` takes any ``k_paths * words_per_link <= 64``): every kernel that lays
the candidates out differently above eight, held to the oracle on the six shapes of ``gpu_support.MANY_PATHS`` -- k = 9 at one
word per link, 32 at two, 21 at three, 16 at four, 12 at five, 10 at six; eight words per link cannot have more than eight paths
(8 x 9 > 64 lanes).  ``test_many_paths.py`` pins on the CPU that these shapes and seeds reach what the tests here are about (paths
8 and above taken, blocking, refusals of the admission check on columns 8 and above, a later path taken by ``sap_ff_gn``, no
decision closer than 1e-6 dB).  What runs here for the first time ("More than eight candidate paths"): the step
kernel's candidates packed W lanes apart and its general policy loop for ``sap_ff`` / ``sp_ff`` / ``sap_ff_gn`` (no ``_ff``
instantiation, the retry behind a refused path), the group kernel's passes of 16 / W paths, the observation kernel's
path-by-path block scan, the second and later passes of the action-mask kernel, the gated masks' W-lane layout, the path query
of the single-environment view, and the GN-gated family at one, three, four and six words per link.  Everything is exact except
the GSNR, held to rtol 1e-9 (``test_gpu_rmsa_gn_gate.py``: wave reduction against sequential sum)."""
import numpy as np
import pytest

import gn_candidates_reference as cref
import gn_gate_reference as ref
from conftest import deeprmsa_to_rmsa_kwargs, oracle_env_from_kwargs
from gpu_support import (COMPACTNESS, DECISIONS, MANY_PATHS, MANY_PATHS_SEED as SEED, RMSA_OUTS, against_oracle,  # noqa: F401
                         check_against_oracles, device_log_fixture, drive, everything_matches_oracle, external_actions, kernel_name,
                         many_paths_kwargs, many_paths_topology, one_step_launches, rmsa_env, same_bytes, snapshot, state_matches,
                         step_kernel)

pytestmark = pytest.mark.gpu

RTOL = 1e-9
SHAPES = list(MANY_PATHS)
K9, K32, K21, K16, K12, K10 = SHAPES
GN_OUTS = ("act_path", "act_slot", "accepted", "done", "request", "reward", "gn_gsnr_db")


def _shape(name, tmp_path):
    return many_paths_topology(name, tmp_path), many_paths_kwargs(name), MANY_PATHS[name]


def _env(topo, batch, kernel, **kw):
    """A handle on the kernel asked for; a shape whose four environments do not fit the group kernel's LDS is skipped for it
    (test_the_group_kernel_serves_the_shapes counts them)."""
    from optical_rl_gym_amd import OrlgError
    try:
        return rmsa_env(topo, batch, kernel, **kw)
    except OrlgError as e:
        if kernel == "group" and "LDS" in str(e):
            pytest.skip("four environments of this shape do not fit the LDS: the wave-per-environment kernel serves it")
        raise


def _kernel(env):
    return env.last_kernel().split()[0]


def _high(ot, K):
    """accepted steps of an oracle trace on a path the kernels lay out above the first eight"""
    return int(((ot["act_path"] >= 8) & (ot["act_path"] < K) & (ot["accepted"] != 0)).sum())


def _gsnr_matches(dev, want, what):
    assert np.array_equal(np.isnan(dev), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.allclose(dev[ok], want[ok], rtol=RTOL, atol=0), (what, float(np.max(np.abs(dev[ok] / want[ok] - 1))))


# ---------------------------------------------------------------------------------------- 1. step parity, both kernels
STEP_CASES = [(name, MANY_PATHS[name]["policy"], 1) for name in SHAPES] + \
    [(K9, "llp_ff", 1), (K21, "llp_ff", 1), (K21, "deeprmsa_sap_ff", 2), (K10, "deeprmsa_sap_ff", 2)]


@pytest.mark.parametrize("name,policy,j", STEP_CASES)
def test_step_parity(name, policy, j, step_kernel, tmp_path, device_log_in_oracle):
    """Six environments (seeds 3 .. 8), 300 steps in one launch, full statistics: every per-step output, occupancy, counters,
    link and graph statistics, histograms, the pending request and the clock against the oracle.  The wave kernel has no
    first-fit instantiation above eight paths: sap_ff runs the general kernel."""
    topo, kw, c = _shape(name, tmp_path)
    B, n, rm = 6, 300, int(policy.startswith("deeprmsa"))
    env = _env(topo, B, step_kernel, j=j, reward_mode=rm, **kw)
    assert env.words_per_link == c["W"]
    tr = env.run(policy, n, outputs=RMSA_OUTS, auto_reset=True)
    said = _kernel(env)
    if step_kernel == "wave":   # (300 steps without the link averages: the link statistics are deferred)
        assert said == kernel_name("wave", c["W"], "full", defer=True) and "_ff" not in said, env.last_kernel()
    else:
        assert said.startswith(f"orlg_rmsa_group_kernel<{c['W']},2"), env.last_kernel()
    snap = snapshot(env, save_state=False)
    high = 0
    for i in range(B):
        ot = everything_matches_oracle(topo, kw, tr, i, snap, policy, n, True, seed=SEED + i, j=j, reward_mode=rm)
        high += _high(ot, c["k"])
    assert high > 0 and 0 < tr["accepted"].mean() < 1, (high, tr["accepted"].mean())
    env.close()


def test_the_group_kernel_serves_the_shapes(tmp_path):
    """At least four of the six shapes fit the group kernel's LDS with their staged tables (the others are skipped above)."""
    from optical_rl_gym_amd import OrlgError
    served = []
    for name in SHAPES:
        topo, kw, c = _shape(name, tmp_path)
        try:
            env = rmsa_env(topo, 6, "group", **kw)
        except OrlgError as e:
            assert "LDS" in str(e), e
            continue
        env.run(c["policy"], 2, auto_reset=True)
        assert _kernel(env).startswith("orlg_rmsa_group_kernel"), env.last_kernel()
        served.append(name)
        env.close()
    print("group kernel serves", served)
    assert len(served) >= 4, served


@pytest.mark.parametrize("stats", ["counters", "network"])
def test_lighter_statistics_levels(stats, step_kernel, tmp_path):
    """k = 16, S = 200 at the two cheaper statistics levels: decisions, counters, occupancy and clock (the network compactness
    where the level keeps it) against the oracle."""
    topo, kw, c = _shape(K16, tmp_path)
    run = drive(lambda: _env(topo, 6, step_kernel, stats_level=stats, **kw), [300], policy=c["policy"],
                outputs=DECISIONS + (COMPACTNESS if stats == "network" else ()))
    if step_kernel == "wave":
        assert run["kernels"] == [kernel_name("wave", c["W"], stats)], run["said"]
    else:
        assert run["kernels"][0].startswith(f"orlg_rmsa_group_kernel<{c['W']},{('counters', 'network').index(stats)}"), run["said"]
    against_oracle(topo, kw, run, c["policy"], 300, range(6), stats, seed0=SEED)


# ---------------------------------------------------------------------------------------- 2. agent-driven actions
@pytest.mark.parametrize("name,policy,j", [(K32, "external", 1), (K10, "external", 1), (K21, "path_ff_external", 1),
                                           (K9, "path_ff_external", 1), (K16, "deeprmsa_external", 1),
                                           (K12, "deeprmsa_external", 3)])
def test_agent_actions_aimed_at_the_high_paths(name, policy, j, step_kernel, tmp_path, device_log_in_oracle):
    """150 launches of one step with the caller's actions, compared step by step with the oracle: (path, slot) pairs of which
    more than half name a path 8 .. K - 1, occupied windows and components out of range among them; paths 0 .. K for
    PathOnlyFirstFitAction; DeepRMSA actions 0 .. K j + 1.  The window of the named path is read W lanes apart."""
    topo, kw, c = _shape(name, tmp_path)
    K, S, B, n = c["k"], c["S"], 6, 150
    if policy == "external":
        actions = external_actions(topo, S, n, B, kind="high_paths")
        assert ((actions[..., 0] >= 8) & (actions[..., 0] < K)).mean() >= 0.5
        assert (actions[..., 0] == K).any() and (actions[..., 1] == S).any()
    elif policy == "path_ff_external":
        actions = external_actions(topo, S, n, B, kind="paths")
        assert actions.min() == 0 and actions.max() == K
    else:
        actions = np.random.default_rng(7).integers(0, K * j + 2, (n, B)).astype(np.int32)
        assert actions.max() == K * j + 1
    rm = int(policy == "deeprmsa_external")
    env = _env(topo, B, step_kernel, j=j, reward_mode=rm, **kw)
    tr = one_step_launches(env, policy, n, RMSA_OUTS, actions=actions, auto_reset=True)
    if step_kernel == "wave":
        assert _kernel(env) == kernel_name("wave", c["W"], "full"), env.last_kernel()
    else:
        assert _kernel(env).startswith(f"orlg_rmsa_group_kernel<{c['W']},2"), env.last_kernel()
    snap = snapshot(env, save_state=False)
    high = occupied = 0
    for i in range(B):
        ot = everything_matches_oracle(topo, kw, tr, i, snap, policy, n, True, actions=actions, seed=SEED + i, j=j, reward_mode=rm)
        high += _high(ot, K)
        if policy == "external":   # a window in the lower half of the spectrum ends inside it: refused means occupied
            a = actions[:, i]
            occupied += int(((a[:, 0] >= 8) & (a[:, 0] < K) & (a[:, 1] < S // 2) & (ot["accepted"] == 0)).sum())
    assert high >= 10, high   # (route = a / j >= 8 taken and accepted)
    assert policy != "external" or occupied > 0
    env.close()


# ---------------------------------------------------------------------------------------- 3. chunked = whole, hand-over
CONTINUE_OUTS = ("act_path", "act_slot", "accepted", "arrival", "network_compactness", "done")


def test_chunked_launches_equal_one_launch(step_kernel, tmp_path):
    """k = 12, S = 320, llp_ff: 1 x 300 steps == 300 x 1 step == seven uneven chunks, every read-back byte for byte."""
    topo, kw, c = _shape(K12, tmp_path)
    a, b, d = (_env(topo, 5, step_kernel, **kw) for _ in range(3))
    ta = a.run(c["policy"], 300, outputs=CONTINUE_OUTS, auto_reset=True)
    tb = [b.run(c["policy"], 1, outputs=CONTINUE_OUTS, auto_reset=True) for _ in range(300)]
    td = [d.run(c["policy"], n, outputs=CONTINUE_OUTS, auto_reset=True) for n in (1, 33, 32, 64, 100, 69, 1)]
    assert ((ta["act_path"] >= 8) & (ta["act_path"] < c["k"])).any()
    for parts in (tb, td):
        same_bytes(ta, {k: np.concatenate([t[k] for t in parts]) for k in ta}, "outputs")
    for env in (b, d):
        same_bytes(snapshot(a), snapshot(env), "state")
    for env in (a, b, d):
        env.close()


def test_kernels_continue_each_other(tmp_path):
    """One state format above eight paths too: a batch handed from the wave kernel to the group kernel and back (save_state /
    load_state) equals an uninterrupted run, outputs and every read-back byte for byte."""
    topo, kw, c = _shape(K12, tmp_path)
    B = 7   # not a multiple of four: the last wave of the group kernel has an idle row
    whole, a = rmsa_env(topo, B, "wave", **kw), rmsa_env(topo, B, "wave", **kw)
    b = _env(topo, B, "group", **kw)
    t_ref = whole.run(c["policy"], 300, outputs=CONTINUE_OUTS, auto_reset=True)
    parts, cur, other = [], a, b
    for n in (60, 1, 100, 39, 100):
        parts.append(cur.run(c["policy"], n, outputs=CONTINUE_OUTS, auto_reset=True))
        other.load_state(cur.save_state())
        cur, other = other, cur
    assert _kernel(a).startswith("orlg_rmsa_kernel<5,2") and _kernel(b).startswith("orlg_rmsa_group_kernel<5,2"), \
        (a.last_kernel(), b.last_kernel())
    same_bytes(t_ref, {k: np.concatenate([p[k] for p in parts]) for k in CONTINUE_OUTS}, "outputs")
    same_bytes(snapshot(whole), snapshot(cur), "state")
    for env in (whole, a, b):
        env.close()


# ---------------------------------------------------------------------------------------- 4. queries
@pytest.mark.parametrize("name,j,allow_rejection", [(K9, 1, False), (K32, 2, True), (K21, 3, False), (K16, 1, True),
                                                    (K12, 2, False), (K10, 3, True)])
def test_masks_against_the_oracle(name, j, allow_rejection, tmp_path, device_log_in_oracle):
    """The masks deeprmsa (the observation kernel's path-by-path scan), path_ff and slots (the mask kernel's passes of eight paths)
    of four environments after reset, after 60 and after 200 steps, against the oracle's own queries."""
    topo, kw, c = _shape(name, tmp_path)
    B, K = 4, c["k"]
    env = rmsa_env(topo, B, j=j, allow_rejection=allow_rejection, **kw)
    oracles = [oracle_env_from_kwargs(topo, kw, seed=SEED + i, j=j) for i in range(B)]
    seen = np.zeros(2, np.int64)
    for where, n in (("reset", 0), ("60 steps", 60), ("200 steps", 140)):
        if n:
            env.run(c["policy"], n, auto_reset=True)
            for o in oracles:
                o.run(c["policy"], n, reset_on_done=True, fields=[])
        deep, ff, bits = check_against_oracles(env, oracles, (name, where))
        high = np.concatenate([deep[:, 8 * j:K * j].ravel(), ff[:, 8:K].ravel()])
        seen += (int((high == 0).sum()), int((high == 1).sum()))
        assert 0 < bits[:, 8:].mean() < 1 or not n, where
    assert seen.min() > 0, seen   # (columns of the paths 8 and above, valid and not)
    for o in oracles:
        o.close()
    env.close()


@pytest.mark.parametrize("name,j", [(K9, 1), (K32, 2), (K16, 3), (K10, 2)])
def test_deeprmsa_observation(name, j, tmp_path, device_log_in_oracle):
    """BatchedDeepRMSAEnv.observation() above eight paths -- block starts and lengths, slot counts, free slots and free runs path
    by path -- after every one of 120 agent-driven steps: equal to the oracle's, alone and with the fused mask, float32 ==
    float32(float64); the fused mask equals the mask kind "deeprmsa", which check_against_oracles holds to the oracle."""
    from optical_rl_gym_amd import BatchedDeepRMSAEnv
    topo, _, c = _shape(name, tmp_path)
    K, B = c["k"], 3
    meta_kw = dict(j=j, mean_service_holding_time=25.0, mean_service_inter_arrival_time=25.0 / c["load"],
                   num_spectrum_resources=c["S"], episode_length=200, seed=SEED)
    env = rmsa_env(topo, B, cls=BatchedDeepRMSAEnv, **meta_kw)
    kw, jj = deeprmsa_to_rmsa_kwargs(meta_kw)
    oracles = [oracle_env_from_kwargs(topo, kw, seed=SEED + i, j=jj, reward_mode=1) for i in range(B)]
    rng = np.random.default_rng(11)
    missing = 0
    for t in range(120):
        a = rng.integers(0, K * j + 1, B).astype(np.int32)
        r = env.run("deeprmsa_external", 1, actions=a, auto_reset=True, outputs=("act_path", "act_slot", "accepted", "reward", "done"))
        obs = env.observation()
        fused, mask = env.observation(return_mask=True)
        assert fused.tobytes() == obs.tobytes(), t
        assert mask.tobytes() == env.action_masks("deeprmsa").tobytes(), t
        assert np.array_equal(env.observation(dtype=np.float32), obs.astype(np.float32)), t
        f32, mask32 = env.observation(dtype=np.float32, return_mask=True)
        assert np.array_equal(f32, obs.astype(np.float32)) and mask32.tobytes() == mask.tobytes(), t
        for i, o in enumerate(oracles):
            ot = o.run("deeprmsa_external", 1, reset_on_done=True, actions=a[i:i + 1].copy())
            for f in ("act_path", "act_slot", "accepted", "reward", "done"):
                assert r[f][0, i] == ot[f][0], (f, t, i)
            oo = o.observation()
            assert np.array_equal(obs[i], oo), (t, i, np.nonzero(obs[i] != oo), obs[i], oo)
        missing += int((mask[:, 8 * j:K * j] == 0).sum())
    assert missing > 0   # (blocks that do not exist on the paths 8 and above: the -1 entries of the observation)
    check_against_oracles(env, oracles, name)
    for o in oracles:
        o.close()
    env.close()


def test_rmsa_view_on_21_paths(tmp_path):
    """The single-environment view stepped with shortest_available_path_first_fit, which reads the view's path query (21
    candidates, three lanes each), against the device policy on a twin handle."""
    from optical_rl_gym_amd import RMSAEnv, shortest_available_path_first_fit
    topo, kw, c = _shape(K21, tmp_path)
    view, dev = RMSAEnv(topology=topo, **kw), rmsa_env(topo, 1, **kw)
    high = 0
    for t in range(100):
        p, s = shortest_available_path_first_fit(view)
        _, _, done, _ = view.step((p, s))
        r = dev.run("sap_ff", 1, outputs=("act_path", "act_slot", "accepted", "done"))
        assert (p, s) == (int(r["act_path"][0, 0]), int(r["act_slot"][0, 0])), t
        assert view._last_served.accepted == bool(r["accepted"][0, 0]) and done == bool(r["done"][0, 0]), t
        high += int(8 <= p < c["k"])
    assert high > 0
    assert np.array_equal(view._batched.occupancy_words(), dev.occupancy_words())
    view.close()
    dev.close()


# ---------------------------------------------------------------------------------------- 5. the gated family
GATED_SHAPES = [K9, K21, K16, K10]   # one, three, four and six words per link (two, five and eight: gn_gate_reference.CASES)


def _gated_env(name, tmp_path, batch, j=1, seeds=None, **gate_over):
    topo, kw, c = _shape(name, tmp_path)
    dev_kw = dict(kw)
    if seeds is not None:
        dev_kw.pop("seed")
    return rmsa_env(topo, batch, gn_gate=ref.case_gate(topo, **gate_over), j=j, seeds=seeds, **dev_kw), topo, kw, c


def _gn_masks(env):
    """both gated masks with their GSNR rows"""
    K, j = env.k_paths, env.j
    ff, ff_g = env.action_masks("path_ff_gn", gsnr_out=True)
    dp, dp_g = env.action_masks("deeprmsa_gn", gsnr_out=True)
    assert ff.shape == ff_g.shape == (env.batch_size, K) and dp.shape == dp_g.shape == (env.batch_size, K * j)
    return ff, ff_g, dp, dp_g


def _masks_match(env, runs, t, what):
    """the device's masks of now against row t of the reference's runs (one per environment)"""
    ff, ff_g, dp, dp_g = _gn_masks(env)
    for i, (tr, _, _) in enumerate(runs):
        assert np.array_equal(ff[i], tr["path_ff_gn"][t]), (what, t, i, ff[i], tr["path_ff_gn"][t], ff_g[i], tr["path_ff_gsnr"][t])
        assert np.array_equal(dp[i], tr["deeprmsa_gn"][t]), (what, t, i, dp[i], tr["deeprmsa_gn"][t])
        _gsnr_matches(ff_g[i], tr["path_ff_gsnr"][t], (what, "path_ff", t, i))
        _gsnr_matches(dp_g[i], tr["deeprmsa_gsnr"][t], (what, "deeprmsa", t, i))
    return ff, ff_g


def _runs_match(tr, state, runs, what):
    for i, (want, final, _) in enumerate(runs):
        for f in ("act_path", "act_slot", "accepted", "done", "request"):
            assert np.array_equal(tr[f][:, i], want[f]), (what, f, i)
        _gsnr_matches(tr["gn_gsnr_db"][:, i], want["gsnr"], (what, i))
        state_matches(state, i, final, (what, i))


@pytest.mark.parametrize("name", GATED_SHAPES)
def test_case_against_the_gated_oracle(name, tmp_path):
    """Eight environments on seed 3, the shape's policy: 300 steps in one launch, one more in its own."""
    env, topo, kw, c = _gated_env(name, tmp_path, 8, seeds=[SEED] * 8)
    a, b = (env.run(c["policy"], n, outputs=GN_OUTS, auto_reset=True) for n in (300, 1))
    tr = {k: np.concatenate([a[k], b[k]]) for k in a}
    assert _kernel(env) == kernel_name("wave", c["W"], "full", gn=True), env.last_kernel()
    want, final, fig = ref.run_case((topo, kw), policy=c["policy"], n_steps=301)
    assert int(np.isfinite(tr["gn_gsnr_db"][:, 0]).sum()) == fig["checks"] and fig["rejects"] > 0
    _runs_match(tr, snapshot(env, save_state=False), [(want, final, fig)] * 8, name)
    env.close()


@pytest.mark.parametrize("name", GATED_SHAPES)
def test_gn_masks_against_the_oracle(name, tmp_path):
    """j = 2, the shape's policy, eight environments stepped one launch per step: before every one of 150 steps both gated masks
    are exact and both GSNR rows agree with the reference (the candidates' words are read W lanes apart)."""
    env, topo, kw, c = _gated_env(name, tmp_path, cref.B, j=2)
    n = 150
    runs = cref.run_batch((topo, kw), j=2, policy=c["policy"], n_steps=n)
    assert any((tr["path_ff_gn"][:, 8:] != tr["path_ff"][:, 8:]).any() for tr, _, _ in runs)
    steps = []
    for t in range(n):
        _masks_match(env, runs, t, name)
        steps.append(env.run(c["policy"], 1, outputs=GN_OUTS, auto_reset=True))
    assert _kernel(env) == kernel_name("wave", c["W"], "full", gn=True), env.last_kernel()
    _runs_match({k: np.concatenate([s[k] for s in steps]) for k in GN_OUTS}, snapshot(env, save_state=False), runs, name)
    env.close()


@pytest.mark.parametrize("name", [K32, K12])
def test_sap_ff_gn_against_the_oracle(name, tmp_path):
    """sap_ff_gn above eight paths runs the general policy loop, which starts over behind the refused path: 150 launches of one
    step against the reference, each against the path_ff_gn mask taken just before it; then one launch of 150 steps: the same
    bytes."""
    env, topo, kw, c = _gated_env(name, tmp_path, cref.B)
    K, S, n = c["k"], c["S"], 150
    runs = cref.run_batch((topo, kw), policy="sap_ff_gn", n_steps=n)
    assert all(fig["later_taken"] > 0 for _, _, fig in runs) and sum(fig["rejects"] for _, _, fig in runs) > 0
    steps = []
    for t in range(n):
        ff, ff_g = _masks_match(env, runs, t, name)
        r = env.run("sap_ff_gn", 1, outputs=GN_OUTS, auto_reset=True)
        assert _kernel(env) == kernel_name("wave", c["W"], "full", gn=True), env.last_kernel()
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
        assert np.isnan(r["gn_gsnr_db"][0][~has_fit]).all() and (r["act_slot"][0][~has_fit] == S).all(), t
        steps.append(r)
    tr = {k: np.concatenate([s[k] for s in steps]) for k in GN_OUTS}
    state = snapshot(env)
    _runs_match(tr, state, runs, name)
    env.close()
    env, _, _, _ = _gated_env(name, tmp_path, cref.B)
    long = env.run("sap_ff_gn", n, outputs=GN_OUTS, auto_reset=True)
    for k in GN_OUTS:
        assert long[k].tobytes() == tr[k].tobytes(), k
    assert env.save_state().tobytes() == state["state"].tobytes()
    env.close()


def test_mask_is_the_step_bit_for_bit(tmp_path):
    """k = 12, S = 320, j = 2, B = 64, the state after 150 steps: for each of the 24 DeepRMSA actions and each of the 12 paths, the
    step from that state accepts exactly where the mask says so and its gn_gsnr_db has the bytes of the mask's GSNR column; among
    the columns of the paths 8 and above are windows that are free and that the gate refuses."""
    env, topo, kw, c = _gated_env(K12, tmp_path, 64, j=2)
    env.run(c["policy"], 150, auto_reset=True)
    state = env.save_state()
    ff, ff_g, dp, dp_g = _gn_masks(env)
    K, j = c["k"], 2
    assert 0 < dp.mean() < 1 and 0 < ff.mean() < 1 and np.isnan(dp_g).any() and np.isfinite(dp_g[:, 1::2]).any()
    for a in range(K * j):
        env.load_state(state)
        r = env.step_deeprmsa(np.full(64, a, np.int32), outputs=("accepted", "gn_gsnr_db"))
        assert np.array_equal(r["accepted"], dp[:, a]), a
        assert np.ascontiguousarray(r["gn_gsnr_db"]).tobytes() == np.ascontiguousarray(dp_g[:, a]).tobytes(), a
    for p in range(K):
        env.load_state(state)
        r = env.step_path_first_fit(np.full(64, p, np.int32), outputs=("accepted", "gn_gsnr_db"))
        assert np.array_equal(r["accepted"], ff[:, p]), p
        assert np.ascontiguousarray(r["gn_gsnr_db"]).tobytes() == np.ascontiguousarray(ff_g[:, p]).tobytes(), p
    assert (np.isfinite(dp_g[:, 8 * j:]) & (dp[:, 8 * j:] == 0)).any() and (np.isfinite(ff_g[:, 8:]) & (ff[:, 8:] == 0)).any()
    env.close()


# ---------------------------------------------------------------------------------------- 6. a gate that passes everything
def test_a_gate_that_passes_everything_is_the_ungated_kernel(tmp_path):
    """k = 16, S = 200, thresholds at -1e9: every per-step output and the saved state byte-identical to a handle without a gate
    on the same seeds, for sap_ff (the ungated general kernel above eight paths, not the first-fit one) and llp_ff."""
    topo, kw, c = _shape(K16, tmp_path)
    outs = ("act_path", "act_slot", "accepted", "done", "reward", "request", "arrival", "holding", "network_compactness",
            "network_compactness_difference", "avg_link_compactness", "avg_link_utilization")
    B = 16
    gated = rmsa_env(topo, B, gn_gate=ref.case_gate(topo, thresholds_db=[-1e9] * 6), **kw)
    plain = rmsa_env(topo, B, "wave", **kw)
    for policy, n in (("sap_ff", 300), ("llp_ff", 40), ("sap_ff", 1)):
        a = gated.run(policy, n, outputs=outs + ("gn_gsnr_db",), auto_reset=True)
        b = plain.run(policy, n, outputs=outs, auto_reset=True)
        assert _kernel(gated) == kernel_name("wave", 4, "full", gn=True), gated.last_kernel()
        assert _kernel(plain) == kernel_name("wave", 4, "full"), plain.last_kernel()
        for f in outs:
            assert a[f].tobytes() == b[f].tobytes(), (policy, n, f)
        assert np.array_equal(np.isfinite(a["gn_gsnr_db"]), a["act_path"] < c["k"])   # every proposal was checked, and passed
        assert np.array_equal(a["accepted"] != 0, a["act_path"] < c["k"])
        assert ((a["act_path"] >= 8) & (a["act_path"] < c["k"])).any() or n == 1
        assert gated.save_state().tobytes() == plain.save_state().tobytes(), (policy, n)
    gated.close()
    plain.close()
