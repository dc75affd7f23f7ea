"""Max-margin assignment inside the step (``include/orlg.h`` ``orlg_step_max_margin``; ``sap_mm``, ``any_mm``,
``path_mm_external``) on the device.  Per batch of ``gn_slots_reference.BATCHES`` and route:
  1. the oracle, following: one launch of n steps with all outputs, then ``gn_max_margin_reference.follow`` on every environment;
  2. the twin, exact: a second handle with the same seeds stepped one step at a time by ``max_margin_windows()`` +
     ``action_masks("slots")``, the rule in numpy and ``run("external", 1)`` -- every decision, GSNR, margin and window margin
     bit-equal at every step, the saved states equal at the end, an admitted proposal never refused.
Then, once on nsfnet_s100: chunked launches, auto_reset, cause_counts, a replayed trace, per-environment loads, an action out of
range, a DeepRMSA handle, B = 20 000 into device tensors, and the kernels' names.  Every test here needs the new policy names."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import gn_max_margin_reference as mm
import gn_protect_reference as pref
import gn_slots_reference as sl
from gpu_support import rmsa_env, topology, unpack

pytestmark = pytest.mark.gpu

NSF100 = "nsfnet_s100_l20_spff"
DECIDED = ("act_path", "act_slot", "accepted", "gn_gsnr_db", "gn_neighbour_margin_db")
OUTS = DECIDED + ("gn_window_margin_db", "request", "done")
NAMES = list(mm.ROUTES)


def _handle(batch, tmp_path, route="path", **over):
    c = sl.BATCHES[batch]
    topo, kw, policy = sl.batch_case(batch, tmp_path)
    kw = dict(kw, seed=mm.batch_seed(batch, route, kw))
    kw.update(c["handle"])
    kw.update(over)
    B = kw.pop("batch", c["B"])
    return rmsa_env(topo, B, gn_gate=pref.case_gate(topo, protect=c["protect"]), **kw), topo, policy


def _twin_step(tw, route, given=None, outs=DECIDED, **kw):
    """one step of the loop the fused launch replaces: the query, the rule on the host, an external step"""
    S = tw.num_spectrum_resources
    slots, margin = tw.max_margin_windows()
    window = unpack(tw.action_masks("slots"), S).astype(bool)
    acts, w, kinds = mm.proposals(slots, margin, mm.first_free_of(window), S, route, given)
    r = tw.run("external", 1, actions=acts, outputs=outs, **kw)
    for i, kind in enumerate(kinds):   # an admitted proposal is never refused, a fallback always
        assert bool(r["accepted"][0, i]) == (kind == "admitted"), (i, kind, acts[i])
    return acts, w, kinds, r


def _same(got, want, what):
    assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), (what, got, want)


def _against_twin(dev, tw, route, given=None, what=(), **kw):
    """the rows of a fused launch (or of several, concatenated) against the twin stepped alongside; returns the kinds seen"""
    seen = dict(admitted=0, fallback=0, rejection=0)
    for t in range(dev["act_path"].shape[0]):
        acts, w, kinds, r = _twin_step(tw, route, None if given is None else given[t], **kw)
        for k in kinds:
            seen[k] += 1
        _same(dev["act_path"][t], acts[:, 0], what + (t, "act_path"))
        _same(dev["act_slot"][t], acts[:, 1], what + (t, "act_slot"))
        for name in DECIDED[2:]:
            _same(dev[name][t], r[name][0], what + (t, name))
        if "gn_window_margin_db" in dev:
            _same(dev["gn_window_margin_db"][t], w, what + (t, "gn_window_margin_db"))
    return seen


def _launch(env, name, n, rng, outs=OUTS, **kw):
    """n steps of a max-margin policy: one launch, or -- the agent's path -- n launches of one step; (rows, the paths given)"""
    if name != "path_mm_external":
        return env.run(name, n, outputs=outs, **kw), None
    given = rng.integers(0, env.k_paths, size=(n, env.batch_size)).astype(np.int32)
    rows = [env.run(name, 1, actions=given[t], outputs=outs, **kw) for t in range(n)]
    return {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}, given


# ---------------------------------------------------------------------------------------- 1. and 2. per batch and route
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("batch", list(sl.BATCHES))
def test_batch_follows_the_oracle_and_equals_the_twin(batch, name, tmp_path):
    c, route = sl.BATCHES[batch], mm.ROUTES[name]
    env, topo, policy = _handle(batch, tmp_path, route)
    tw, _, _ = _handle(batch, tmp_path, route)
    assert bool(env.gn_protect) == c["protect"]
    for e in (env, tw):
        if c["warmup"]:
            e.run(policy, c["warmup"], auto_reset=True)
    dev, given = _launch(env, name, c["n"], np.random.default_rng(32), auto_reset=True)
    assert "orlg_rmsa_mm_kernel<%d," % env.words_per_link in env.last_kernel(), env.last_kernel()
    seen = _against_twin(dev, tw, route, given, (batch, name), auto_reset=True)
    assert env.save_state().tobytes() == tw.save_state().tobytes()
    if not c["protect"]:
        assert np.isnan(dev["gn_neighbour_margin_db"]).all()
    # the oracle follows every environment of the launch
    kinds = dict(admitted=0, near=0, fallback=0, rejection=0)
    diffs, largest = [0.0], 0.0
    for i in range(c["B"]):
        go = mm.oracle_at(batch, tmp_path, i, route)
        try:
            for k, v in mm.follow(go, dev, i, route, diffs, given).items():
                kinds[k] += v
            largest = max(largest, go.max_abs_gsnr)
        finally:
            go.close()
    print(batch, name, seen, kinds, "largest margin difference", max(diffs), "bound", 1e-9 * largest)
    assert max(diffs) <= 1e-9 * largest   # margins: atol 1e-9 x the largest |GSNR| the reference computed in the batch
    assert seen["admitted"] > 0 and kinds["admitted"] + kinds["near"] == seen["admitted"] and kinds["fallback"] == seen["fallback"]
    env.close(); tw.close()


# ---------------------------------------------------------------------------------------- 3. once, on nsfnet_s100
def test_two_launches_equal_one(tmp_path):
    for name in ("sap_mm", "any_mm"):
        one, _, _ = _handle(NSF100, tmp_path)
        two, _, _ = _handle(NSF100, tmp_path)
        a = one.run(name, 100, outputs=OUTS, auto_reset=True)
        b = [two.run(name, n, outputs=OUTS, auto_reset=True) for n in (37, 63)]
        for k in a:
            _same(a[k], np.concatenate([r[k] for r in b]), (name, k))
        assert one.save_state().tobytes() == two.save_state().tobytes()
        one.close(); two.close()


def test_auto_reset_across_an_episode_boundary(tmp_path):
    env, _, _ = _handle(NSF100, tmp_path, episode_length=30)
    tw, _, _ = _handle(NSF100, tmp_path, episode_length=30)
    dev = env.run("sap_mm", 70, outputs=OUTS, auto_reset=True)
    assert dev["done"].sum() == 2 * env.batch_size and (dev["request"][:, :, 0] < 30).all()   # two episodes end inside the launch
    _against_twin(dev, tw, "sap", None, ("auto_reset",), auto_reset=True)
    assert env.save_state().tobytes() == tw.save_state().tobytes()
    env.close(); tw.close()


def test_cause_counts_say_gn_for_a_fallback(tmp_path):
    from optical_rl_gym_amd import BLOCK_CAUSES
    env, _, _ = _handle(NSF100, tmp_path)
    n = 100
    r = env.run("sap_mm", n, outputs=OUTS + ("block_cause",), cause_counts=True, auto_reset=True)
    assert env.last_kernel().split(" ")[0].startswith("orlg_rmsa_mm_kernel<") and env.last_kernel().split(" ")[0].endswith(",true>"), env.last_kernel()
    counts = r["block_cause_counts"]
    assert (counts.sum(axis=1) == n).all()
    gn = BLOCK_CAUSES.index("gn")
    fallback = ~r["accepted"].astype(bool) & np.isfinite(r["gn_gsnr_db"])
    assert fallback.sum() > 0 and np.isnan(r["gn_window_margin_db"][fallback]).all()
    assert (r["block_cause"][fallback] == gn).all() and (r["block_cause"] == gn).sum() == fallback.sum()
    assert np.array_equal(counts[:, gn], fallback.sum(axis=0))
    assert (r["block_cause"][r["accepted"].astype(bool)] == 0).all()
    env.close()


def test_a_replayed_trace_and_per_environment_loads(tmp_path):
    from optical_rl_gym_amd import make_sweep, record_trace
    c = sl.BATCHES[NSF100]
    topo, kw, policy = sl.batch_case(NSF100, tmp_path)
    gate = pref.case_gate(topo, protect=True)
    gen, _, _ = _handle(NSF100, tmp_path)
    trace = record_trace(gen, "sap_ff", 60, outputs=("accepted",), auto_reset=True)
    gen.close()
    tkw = dict(num_spectrum_resources=kw["num_spectrum_resources"], episode_length=kw["episode_length"])
    rep, tw = (rmsa_env(topo, c["B"], gn_gate=gate, trace=trace, **tkw) for _ in range(2))
    dev = rep.run("any_mm", 59, outputs=OUTS, auto_reset=True)
    assert "orlg_rmsa_mm_kernel" in rep.last_kernel()
    _against_twin(dev, tw, "any", None, ("trace",), auto_reset=True)
    assert rep.save_state().tobytes() == tw.save_state().tobytes()
    rep.close(); tw.close()
    skw = {k: v for k, v in kw.items() if k not in ("load", "seed")}
    env, tw = (make_sweep("rmsa", topo, loads=[10, 40], seeds_per_load=3, seed=5, gn_gate=gate, **skw) for _ in range(2))
    dev = env.run("sap_mm", 50, outputs=OUTS, auto_reset=True)
    _against_twin(dev, tw, "sap", None, ("sweep",), auto_reset=True)
    assert env.save_state().tobytes() == tw.save_state().tobytes()
    env.close(); tw.close()


def test_an_action_out_of_range_is_the_rejection(tmp_path):
    env, _, _ = _handle(NSF100, tmp_path)
    tw, _, _ = _handle(NSF100, tmp_path)
    K, S, B = env.k_paths, env.num_spectrum_resources, env.batch_size
    rng = np.random.default_rng(4)
    for e in (env, tw):
        e.run("sap_ff", 20, auto_reset=True)
    for t in range(B):
        given = rng.integers(0, K, size=B).astype(np.int32)
        given[t] = (K, -1, K + 7, 1 << 20)[t % 4]
        r = env.run("path_mm_external", 1, actions=given, outputs=OUTS + ("block_cause",))
        assert (r["act_path"][0, t], r["act_slot"][0, t], r["accepted"][0, t]) == (K, S, 0)
        assert np.isnan(r["gn_gsnr_db"][0, t]) and np.isnan(r["gn_window_margin_db"][0, t]) and r["block_cause"][0, t] != 0
        _against_twin(r, tw, "path", given[None], ("range", t))
    assert env.save_state().tobytes() == tw.save_state().tobytes()
    env.close(); tw.close()


def test_a_deeprmsa_handle(tmp_path):
    from optical_rl_gym_amd import BatchedDeepRMSAEnv
    topo, kw, _ = sl.batch_case(NSF100, tmp_path)
    gate = pref.case_gate(topo, protect=True)
    dkw = dict(mean_service_holding_time=25.0, mean_service_inter_arrival_time=25.0 / 20, num_spectrum_resources=100, episode_length=1000, seed=13, j=2)
    env, tw = (BatchedDeepRMSAEnv(topo, 4, gn_gate=gate, **dkw) for _ in range(2))
    dev = env.run("sap_mm", 60, outputs=OUTS + ("reward",), auto_reset=True)
    assert "orlg_rmsa_mm_kernel" in env.last_kernel()
    assert np.array_equal(dev["reward"], np.where(dev["accepted"].astype(bool), 1.0, -1.0)) and (dev["reward"] < 0).any()
    _against_twin(dev, tw, "sap", None, ("deeprmsa",), auto_reset=True)
    assert env.save_state().tobytes() == tw.save_state().tobytes()
    env.close(); tw.close()


def test_kernel_names_and_the_old_launch_on_the_same_handle(tmp_path):
    env, _, _ = _handle(NSF100, tmp_path)
    W = env.words_per_link
    env.run("sap_mm", 3)
    assert env.last_kernel().startswith("orlg_rmsa_mm_kernel<%d,2> " % W), env.last_kernel()
    env.run("sap_ff_gn", 3)
    assert env.last_kernel().startswith("orlg_rmsa_kernel<%d,2,false,true,false,false,false,false,true> " % W), env.last_kernel()
    L, before = env.L, env.save_state().tobytes()
    for args, word in (((0, 1, None), b"route"), ((2, 1, None), b"route"), ((7, 1, None), b"route"), ((100, 1, None), b"route"),
                       ((1, 0, None), b"n_steps"), ((101, -3, None), b"n_steps"), ((6, 1, None), b"action array")):
        assert L.orlg_step_max_margin(env.h, args[0], args[1], args[2], 0, None, None, None) == -1 and word in L.orlg_last_error(), args
    assert env.save_state().tobytes() == before   # refused before anything is launched
    with pytest.raises(ValueError, match="gn_rule"):
        env.run("sap_mm", 1, gn_rule="check")
    with pytest.raises(ValueError, match="MAX_MARGIN_POLICIES"):
        env.run("sap_ff", 1, outputs=("gn_window_margin_db",))
    env.close()
    topo, kw, _ = sl.batch_case(NSF100, tmp_path)
    plain = rmsa_env(topo, 2, **kw)
    L = plain.L
    assert L.orlg_step_max_margin(plain.h, 1, 1, None, 0, None, None, None) == -1 and b"gn_gate" in L.orlg_last_error()
    plain.close()


def test_the_batched_driver_runs_the_names(tmp_path):
    from optical_rl_gym_amd import evaluate_heuristic_batched
    env, _, _ = _handle(NSF100, tmp_path, episode_length=40)
    twin, _, _ = _handle(NSF100, tmp_path, episode_length=40)
    rewards, lengths, _ = evaluate_heuristic_batched(env, "sap_mm", n_eval_episodes=2)
    assert "orlg_rmsa_mm_kernel" in env.last_kernel() and (lengths == 39).all()
    twin.reset(only_episode_counters=True)
    acc = twin.run("sap_mm", 39, outputs=("accepted",))["accepted"]
    assert np.array_equal(rewards[0], acc.sum(axis=0))
    env.close(); twin.close()


def test_device_buffers_and_a_batch_larger_than_the_grid():
    """B = 20 000 with outputs into torch device tensors: every wave takes several environments off the work queue; the rows of the
    first and the last four environments equal those of a handle of eight with the same seeds, byte for byte.  In a child process:
    torch has to create its HIP context before the library does."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys
        import numpy as np, torch
        torch.zeros(1, device="cuda")
        sys.path[:0] = [%r, %r]
        import gn_protect_reference as pref
        from conftest import load_topology
        from optical_rl_gym_amd import BatchedRMSAEnv
        topo = load_topology(pref.NSF)
        kw = dict(num_spectrum_resources=100, load=20, mean_service_holding_time=25)
        B, n = 20000, 25
        seeds = np.arange(B) + 5
        ends = np.r_[0:4, B - 4:B]
        big = BatchedRMSAEnv(topo, B, gn_gate=pref.case_gate(topo, protect=True), seeds=seeds, **kw)
        small = BatchedRMSAEnv(topo, 8, gn_gate=pref.case_gate(topo, protect=True), seeds=seeds[ends], **kw)
        names = {"act_path": torch.int32, "act_slot": torch.int32, "accepted": torch.uint8, "gn_gsnr_db": torch.float64,
                 "gn_neighbour_margin_db": torch.float64, "gn_window_margin_db": torch.float64}
        for policy in ("sap_mm", "any_mm"):
            out = {k: torch.full((n, B), 7, dtype=d, device="cuda") for k, d in names.items()}
            torch.cuda.synchronize()
            big.run(policy, n, out=out, auto_reset=True)
            big.synchronize()
            assert "orlg_rmsa_mm_kernel" in big.last_kernel()
            want = small.run(policy, n, outputs=tuple(names), auto_reset=True)
            for k in names:
                assert out[k].cpu().numpy()[:, ends].tobytes() == want[k].tobytes(), (policy, k)
            assert np.isfinite(want["gn_window_margin_db"]).any()
        big.close(); small.close()
        print("gn max margin buffers ok")
    """) % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "gn max margin buffers ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
