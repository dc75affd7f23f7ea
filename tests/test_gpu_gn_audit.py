"""The GN-model audit of the running lightpaths (``include/orlg.h`` ``orlg_gn_audit``, ``orlg_get_running_services``) on
the device, held to the CPU restatement of ``gn_audit_reference.py``: the running services exact (the release time bitwise), GSNR
to rtol 1e-9 (the tolerance of the gate), margins and the ASE / NLI parts to atol = 1e-9 x the largest |GSNR| of the
case -- the same tolerance carried to a difference of a GSNR and a threshold --, ``n_running`` and ``n_below`` exact
(``test_gn_audit_args.py`` holds every margin of the cases 1e-4 dB away from zero).  Every test here calls ``qot_audit`` or
``running_services``."""
import numpy as np
import pytest

import gn_audit_reference as aref
import gn_protect_reference as pref
from conftest import load_topology
from gpu_support import rmsa_env

pytestmark = pytest.mark.gpu

RTOL = 1e-9
PARTS = ("gsnr_db", "margin_db", "osnr_ase_db", "snr_nli_db")
STEP_OUTS = ("act_path", "act_slot", "accepted", "done", "reward", "request", "gn_gsnr_db")
# the default release ring of the two ring cases (480 and 736 slots, sized from the load) is longer than the ~450 releases of 600
# steps, so its head never laps: a ring just above the most services these cases run, so that the live part meets the ring's end
QUEUE_CAPACITY = {"ring34_s320_l300_llpff": 224, "ring36_s512_l500_sapff": 192}


def _env(case, protect, B=aref.B, seeds=None, **over):
    """protect: True / False = a protecting / a gated handle, None = no gate"""
    c = pref.CASES[case]
    topo = load_topology(c["topology"])
    kw = pref.case_kwargs(case, **over)
    kw.pop("seed")
    gate = None if protect is None else pref.case_gate(topo, protect=protect)
    seeds = [aref.SEEDS[case] + i for i in range(B)] if seeds is None else seeds
    return rmsa_env(topo, B, gn_gate=gate, seeds=seeds, **kw), topo, c


def _device_is_consistent(a, run, Q):
    """what the device's output promises about itself"""
    n = a["n_running"]
    assert np.array_equal(n, run["count"]) and a["gsnr_db"].shape == (len(n), Q)
    past = np.arange(Q)[None, :] >= n[:, None]
    for k in PARTS:
        assert np.array_equal(np.isnan(a[k]), past), k
    for k, fill in (("path_gid", -1), ("slot", -1), ("num_slots", -1), ("bit_rate", -1)):
        assert (run[k][past] == fill).all() and (run[k][~past] >= 0).all(), k
    assert np.array_equal(np.isnan(run["release_time"]), past)
    assert ((run["head"] >= 0) & (run["head"] < Q)).all()
    for i in range(len(n)):
        if n[i] == 0:
            assert a["n_below"][i] == 0 and a["worst_rank"][i] == -1 and np.isnan(a["min_margin_db"][i]), i
        else:
            m, w = a["margin_db"][i, :n[i]], int(a["worst_rank"][i])
            assert m[w].tobytes() == a["min_margin_db"][i].tobytes() and w == int(np.argmin(m)), i   # bitwise; the lowest rank
            assert a["n_below"][i] == int((m < 0).sum()), i
            assert np.all(np.diff(run["release_time"][i, :n[i]]) >= 0), i


def _matches(a, i, want, atol, what):
    """the audit of environment i against a reference audit (gn_audit_reference.audit)"""
    n = want["n_running"]
    assert a["n_running"][i] == n and a["n_below"][i] == want["n_below"], (what, a["n_running"][i], n, a["n_below"][i], want["n_below"])
    if not n:
        return
    dev, ref = a["gsnr_db"][i, :n], want["gsnr_db"]
    assert np.allclose(dev, ref, rtol=RTOL, atol=0), (what, float(np.max(np.abs(dev / ref - 1))))
    for k in PARTS[1:]:
        assert np.allclose(a[k][i, :n], want[k], rtol=0, atol=atol), (what, k, float(np.max(np.abs(a[k][i, :n] - want[k]))), atol)
    assert abs(a["min_margin_db"][i] - want["min_margin_db"]) <= atol, what


def _matches_running(env, topo, gate, a, run, envs, what):
    """the audit of some environments against the reference fed from running_services(); returns the largest |GSNR|"""
    top = 0.0
    for i in envs:
        want = aref.audit(aref.services_of_running(run, i, topo), gate)
        if want["n_running"]:
            top = max(top, float(np.max(np.abs(want["gsnr_db"]))))
        _matches(a, i, want, RTOL * max(top, 1.0), (what, i))
    return top


@pytest.mark.parametrize("protect", [False, True], ids=["gated", "protecting"])
@pytest.mark.parametrize("case", aref.CASES)
def test_case_against_the_oracle(case, protect):
    """B = 8 environments on the case's seed + 0 .. 7, audited after 0, 1, 2, 50, 200, 400 and 600 steps."""
    env, topo, c = _env(case, protect, queue_capacity=QUEUE_CAPACITY.get(case, 0))
    Q = env.queue_capacity
    refs = [aref.run_checkpoints(case, aref.SEEDS[case] + i, protect) for i in range(aref.B)]
    top = max([float(np.max(np.abs(cp["audit"]["gsnr_db"]))) for r in refs for cp in r.values() if cp["audit"]["n_running"]])
    done, wrapped, most = 0, 0, 0
    for at in aref.CHECKPOINTS:
        if at > done:
            env.run(c["policy"], at - done, auto_reset=True)
            done = at
        run, a = env.running_services(), env.qot_audit(services=True)
        _device_is_consistent(a, run, Q)
        wrapped += int((run["head"] + run["count"] > Q).sum())
        most = max(most, int(run["count"].max()))
        for i, r in enumerate(refs):
            cp, n = r[at], r[at]["audit"]["n_running"]
            assert run["count"][i] == n, (at, i)
            svc = cp["services"]
            assert np.array_equal(run["path_gid"][i, :n], cp["path_gid"]), (at, i)
            assert np.array_equal(run["slot"][i, :n], [s[1] for s in svc]) and np.array_equal(run["num_slots"][i, :n], [s[2] for s in svc]), (at, i)
            assert np.array_equal(run["bit_rate"][i, :n], cp["bit_rate"]), (at, i)
            assert run["release_time"][i, :n].tobytes() == cp["release"].tobytes(), (at, i)
            _matches(a, i, cp["audit"], RTOL * top, (case, protect, at, i))
        if at == 0:
            assert (a["n_running"] == 0).all() and np.isnan(a["min_margin_db"]).all() and (a["worst_rank"] == -1).all()
        # the summary alone is the same summary
        b = env.qot_audit()
        assert set(b) == {"n_running", "n_below", "worst_rank", "min_margin_db"}
        for k in b:
            assert b[k].tobytes() == a[k].tobytes(), (at, k)
    print(case, protect, "Q", Q, "most running", most, "states with the live part across the ring's end", wrapped)
    assert wrapped >= 1   # the walk met the wrap: the live part straddled the ring's end in an audited state
    env.close()


def _trace(topo, n):
    from optical_rl_gym_amd import RequestTrace
    N = topo.num_nodes
    pairs = [(s, d) for s in range(N) for d in range(N) if s != d]
    src, dst = (np.array([pairs[i % len(pairs)][k] for i in range(n)], np.int32) for k in (0, 1))
    return RequestTrace(np.arange(1, n + 1, dtype=np.float64), np.full(n, 1e9), src, dst, np.full(n, 200, np.int32))


@pytest.mark.parametrize("name", [pref.NSF, "ring34_3-paths_6-modulations"])
def test_exact_chunk_shapes(name):
    """An ungated trace handle whose services never leave, stepped one request at a time: audited (with gate=) when environment 0
    runs exactly 1, 2, 63, 64, 65, 128 and 129 services -- the edges of the chunks of 64 lanes."""
    topo = load_topology(name)
    gate = pref.case_gate(topo, protect=False)
    n_req = 400
    env = rmsa_env(topo, 2, num_spectrum_resources=320, episode_length=n_req, trace=_trace(topo, n_req))
    assert env.gn_gate is None
    sizes, reached = (1, 2, 63, 64, 65, 128, 129), []
    for _ in range(n_req - 2):
        env.run("sap_ff", 1)
        n = int(env.num_running()[0])
        if n in sizes and n not in reached:
            reached.append(n)
            run, a = env.running_services(), env.qot_audit(gate=gate, services=True)
            assert run["count"][0] == n
            _device_is_consistent(a, run, env.queue_capacity)
            _matches_running(env, topo, gate, a, run, (0, 1), (name, n))
        if n >= sizes[-1]:
            break
    print(name, "reached", reached)
    assert 64 in reached and 65 in reached and reached == [s for s in sizes if s <= max(reached)]
    env.close()


def test_a_gate_given_with_the_call():
    case = "nsfnet_s320_l150_sapff"
    env, topo, c = _env(case, False)
    twin, _, _ = _env(case, False)
    for e in (env, twin):
        e.run(c["policy"], 200, auto_reset=True)
    own = env.qot_audit(services=True)
    same = env.qot_audit(gate=pref.case_gate(topo, protect=False), services=True)
    also = env.qot_audit(gate=pref.case_gate(topo, protect=True), services=True)   # protect_running is ignored there
    for k in own:
        assert own[k].tobytes() == same[k].tobytes() == also[k].tobytes(), k
    # the same lightpaths at 0 dBm per 50 GHz: the reference at 0 dBm, nothing below a threshold any more
    g0 = pref.case_gate(topo, protect=False, launch_power_dbm_per_50ghz=0.0)
    run, cold = env.running_services(), env.qot_audit(gate=g0, services=True)
    _matches_running(env, topo, g0, cold, run, range(aref.B), "0 dBm")
    assert own["n_below"].sum() > 0 and cold["n_below"].sum() == 0 and not np.array_equal(own["gsnr_db"], cold["gsnr_db"])
    # ... and the handle's own gate is what it was: the audit again, and the next gated step against a twin that never overrode
    again = env.qot_audit(services=True)
    for k in own:
        assert own[k].tobytes() == again[k].tobytes(), k
    a, b = (e.run(c["policy"], 1, outputs=STEP_OUTS, auto_reset=True) for e in (env, twin))
    for k in STEP_OUTS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.isfinite(a["gn_gsnr_db"]).any()
    assert env.save_state().tobytes() == twin.save_state().tobytes()
    env.close(); twin.close()


def test_continuous_bit_rates():
    topo = load_topology(pref.NSF)
    gate = pref.case_gate(topo, protect=False)
    env = rmsa_env(topo, 4, gn_gate=gate, num_spectrum_resources=320, load=150, mean_service_holding_time=25, seed=5,
                   bit_rate_selection="continuous", bit_rate_lower_bound=150, bit_rate_higher_bound=300)
    tr = env.run("sap_ff", 200, outputs=("accepted", "request"), auto_reset=True)
    run, a = env.running_services(), env.qot_audit(services=True)
    _device_is_consistent(a, run, env.queue_capacity)
    live = run["bit_rate"][run["bit_rate"] >= 0]
    assert live.min() >= 150 and live.max() <= 300 and len(np.unique(live)) > 21   # the rates themselves, not their indices
    assert set(live) <= set(tr["request"][..., 3][tr["accepted"] != 0])
    assert _matches_running(env, topo, gate, a, run, range(4), "continuous") > 0
    env.close()


def test_per_environment_loads_by_group():
    topo = load_topology(pref.NSF)
    gate = pref.case_gate(topo, protect=False)
    loads, groups = np.array([50, 50, 50, 150, 150, 300, 300, 300.0]), np.array([0, 0, 0, 1, 1, 2, 2, 2], np.int32)
    env = rmsa_env(topo, 8, gn_gate=gate, num_spectrum_resources=320, load=loads, mean_service_holding_time=25, seed=9, groups=groups)
    empty = env.qot_audit(by_group=True)["by_group"]
    assert (empty["services"] == 0).all() and (empty["below"] == 0).all() and np.isnan(empty["min_margin_db"]).all()
    env.run("sap_ff", 300, auto_reset=True)
    run, a = env.running_services(), env.qot_audit(services=True, by_group=True)
    _matches_running(env, topo, gate, a, run, range(8), "sweep")
    g = a["by_group"]
    for k in range(3):
        of = groups == k
        assert g["services"][k] == a["n_running"][of].sum() and g["below"][k] == a["n_below"][of].sum()
        assert g["min_margin_db"][k] == np.nanmin(a["min_margin_db"][of])
    assert g["services"][0] < g["services"][1] < g["services"][2] and g["below"].sum() > 0
    env.close()


def test_the_group_kernel_without_a_gate():
    """step_kernel="group" serves no gate; its traffic is audited with a gate given with the call"""
    topo = load_topology(pref.NSF)
    gate = pref.case_gate(topo, protect=False)
    env = rmsa_env(topo, 8, kernel="group", num_spectrum_resources=320, load=150, mean_service_holding_time=25, seed=4)
    env.run("sap_ff", 300, auto_reset=True)
    assert "group" in env.last_kernel(), env.last_kernel()
    with pytest.raises(ValueError, match="gate="):
        env.qot_audit()
    summary = np.zeros((8, 24), np.uint8)
    assert env.L.orlg_gn_audit(env.h, None, summary.ctypes.data, None, None, None, None) == -1
    assert b"no gn_gate" in env.L.orlg_last_error() and not summary.any()
    assert env.L.orlg_gn_audit(env.h, None, None, None, None, None, None) == -1 and b"null argument" in env.L.orlg_last_error()
    run, a = env.running_services(), env.qot_audit(gate=gate, services=True)
    assert np.array_equal(run["count"], env.num_running())
    _device_is_consistent(a, run, env.queue_capacity)
    assert _matches_running(env, topo, gate, a, run, range(8), "group") > 0
    assert a["n_below"].sum() > 0   # nothing gated this traffic at +6 dBm
    env.close()


def test_a_deeprmsa_handle_and_the_views():
    from optical_rl_gym_amd import BatchedDeepRMSAEnv, RMSAEnv, shortest_available_path_first_fit
    topo = load_topology(pref.NSF)
    gate = pref.case_gate(topo, protect=True)
    env = BatchedDeepRMSAEnv(topo, 4, j=2, gn_gate=gate, num_spectrum_resources=320, mean_service_holding_time=25.0,
                             mean_service_inter_arrival_time=25.0 / 150, seed=3)
    env.run("deeprmsa_sap_ff", 200, auto_reset=True)
    run, a = env.running_services(), env.qot_audit(services=True)
    _device_is_consistent(a, run, env.queue_capacity)
    assert _matches_running(env, topo, gate, a, run, range(4), "deeprmsa") > 0
    env.close()
    # RMSA-v0: the view's audit is environment 0 of a batched twin
    kw = dict(num_spectrum_resources=320, load=150, mean_service_holding_time=25, episode_length=1000)
    view = RMSAEnv(topology=topo, seed=13, gn_gate=pref.case_gate(topo, protect=False), **kw)
    twin = rmsa_env(topo, 2, gn_gate=pref.case_gate(topo, protect=False), seeds=[13, 14], **kw)
    for _ in range(60):
        view.step(shortest_available_path_first_fit(view))
    twin.run("sap_ff", 60)
    v, run, a = view.qot_audit(), twin.running_services(), twin.qot_audit(services=True)
    n = int(a["n_running"][0])
    assert v["n_running"] == n > 10 and v["n_below"] == a["n_below"][0] and v["worst_rank"] == a["worst_rank"][0]
    assert v["min_margin_db"] == a["min_margin_db"][0] and len(v["services"]) == n
    for r, s in enumerate(v["services"]):
        for k in PARTS:
            assert s[k] == a[k][0, r], (r, k)
        for k in ("path_gid", "slot", "num_slots", "bit_rate", "release_time"):
            assert s[k] == run[k][0, r], (r, k)
    cold = view.qot_audit(gate=pref.case_gate(topo, launch_power_dbm_per_50ghz=0.0))
    assert cold["n_running"] == n and cold["min_margin_db"] != v["min_margin_db"]
    view.close(); twin.close()


def test_preallocated_buffers():
    case = "nsfnet_s320_l150_sapff"
    env, topo, c = _env(case, False)
    env.run(c["policy"], 200, auto_reset=True)
    B, Q = env.batch_size, env.queue_capacity
    want, run = env.qot_audit(services=True), env.running_services()
    # numpy: the caller's arrays come back
    bufs = {k: np.zeros((B, Q)) for k in ("gsnr_db", "snr_nli_db")}
    got = env.qot_audit(out=bufs)
    assert got["gsnr_db"] is bufs["gsnr_db"] and "margin_db" not in got
    assert got["gsnr_db"].tobytes() == want["gsnr_db"].tobytes() and got["snr_nli_db"].tobytes() == want["snr_nli_db"].tobytes()
    rb = {"count": np.zeros(B, np.int32), "release_time": np.zeros((B, Q))}
    r2 = env.running_services(out=rb)
    assert r2["count"] is rb["count"] and r2["release_time"].tobytes() == run["release_time"].tobytes()
    with pytest.raises(ValueError):
        env.qot_audit(out={"gsnr_db": np.zeros((B, Q + 1))})
    with pytest.raises(TypeError):
        env.qot_audit(out={"gsnr_db": np.zeros((B, Q), np.float32)})
    with pytest.raises(ValueError, match="no buffer named"):
        env.qot_audit(out={"gsnr": np.zeros((B, Q))})
    env.close()


def test_device_buffers():
    """torch device tensors are written in place, the summary records too.  In a child process: torch has to create its HIP context
    before the library does."""
    import os, subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys
        import numpy as np, torch
        torch.zeros(1, device="cuda")
        sys.path[:0] = [%r, %r]
        import gn_protect_reference as pref
        from conftest import load_topology
        from optical_rl_gym_amd import BatchedRMSAEnv
        case = "nsfnet_s320_l150_sapff"
        topo = load_topology(pref.CASES[case]["topology"])
        env = BatchedRMSAEnv(topo, 8, gn_gate=pref.case_gate(topo, protect=False), **pref.case_kwargs(case))
        env.run("sap_ff", 200, auto_reset=True)
        B, Q = env.batch_size, env.queue_capacity
        want, run = env.qot_audit(services=True), env.running_services()
        parts = env.AUDIT_SERVICE_FIELDS
        dev = {k: torch.full((B, Q), 7.0, dtype=torch.float64, device="cuda") for k in parts}
        dev["summary"] = torch.full((B, 24), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        got = env.qot_audit(out=dev)
        env.synchronize()
        for k in parts:
            assert got[k] is dev[k] and got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
        for k in ("n_running", "n_below", "worst_rank", "min_margin_db"):
            assert got[k].is_cuda and got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
        grouped = env.qot_audit(out={"summary": dev["summary"]}, by_group=True)["by_group"]
        assert grouped["services"][0] == want["n_running"].sum() and grouped["below"][0] == want["n_below"].sum()
        rd = {"count": torch.zeros(B, dtype=torch.int32, device="cuda"), "slot": torch.zeros((B, Q), dtype=torch.int16, device="cuda"),
              "release_time": torch.zeros((B, Q), dtype=torch.float64, device="cuda")}
        env.running_services(out=rd)
        env.synchronize()
        for k in rd:
            assert rd[k].cpu().numpy().tobytes() == run[k].tobytes(), k
        env.close()
        print("audit buffers ok")
    """) % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "audit buffers ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_one_audit_across_the_grids_stride():
    """B = 4200, more environments than the grid has waves: environments 0, 4095, 4096 and 4199 bitwise as the same seeds audited
    on a handle of B = 8."""
    case = "nsfnet_s320_l150_sapff"
    big, topo, c = _env(case, False, B=4200)
    picks = [0, 4095, 4096, 4199]
    small, _, _ = _env(case, False, seeds=[aref.SEEDS[case] + i for i in picks] * 2)
    for e in (big, small):
        e.run(c["policy"], 200, auto_reset=True)
    assert big.queue_capacity == small.queue_capacity
    a, b = big.qot_audit(services=True), small.qot_audit(services=True)
    ra, rb = big.running_services(), small.running_services()
    for j, i in enumerate(picks):
        for k in a:
            assert a[k][i].tobytes() == b[k][j].tobytes(), (i, k)
        for k in ra:
            assert ra[k][i].tobytes() == rb[k][j].tobytes(), (i, k)
        assert a["n_running"][i] > 30
    assert (a["n_running"] > 0).all()
    big.close(); small.close()
