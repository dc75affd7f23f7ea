"""The one launch of the queries that give every environment a wave (``launch_wave_query``, csrc/orlg_api_query.hip) at two
workgroup sizes.  NSFNET with 320 slots, B = 5 -- no multiple of any number of waves per workgroup --, once with the default
release queue and once with ``queue_capacity=4096``, which leaves room for two waves per workgroup where the default has eight.
Both handles get the same seeds and the same 60 steps of ``sap_ff`` and then the same gate; each of the ten queries must return
the same arrays on both (the per-service arrays up to each environment's count: their row length is the queue's capacity).

So that the launch is not held to itself alone, the rule windows of the protecting handle are held to the admission oracle of
``gn_admission_reference.py``, with the tolerances of ``test_gpu_gn_admission.py``: slots and ``admitted`` exact, GSNR to rtol
1e-9, the neighbour margin to atol = 1e-9 x the largest |GSNR| of the oracle's run.  The gate is the one that refuses nothing on
NSFNET (0 dBm per 50 GHz), so the oracle's 60 gated steps leave the state of the handles' 60 ungated ones -- which the decisions of
those steps are compared for."""
import ctypes as C

import numpy as np
import pytest

import gn_admission_reference as adm
import gn_protect_reference as pref
from conftest import load_topology
from gpu_support import rmsa_env

pytestmark = pytest.mark.gpu

CASE, B, N = "nsfnet_s320_l50_sapff", 5, 60
GATE = dict(launch_power_dbm_per_50ghz=0.0)
RTOL = 1e-9
STEP_OUTS = ("act_path", "act_slot", "accepted")


def _gate(env, protect):
    """what the constructor does with gn_gate=, on a handle that has stepped"""
    from optical_rl_gym_amd import _lib, osnr
    if env.gn_gate is None:
        env.gn_gate = osnr.check_rmsa_gn_gate(pref.case_gate(env.topology, protect=False, **GATE), env.topology, "auto")
        gg, keep = env._gn_gate_struct(env.gn_gate)
        _lib.check(env.L.orlg_set_gn_gate(env.h, C.byref(gg)))
    env.gn_gate["protect_running"] = bool(protect)
    _lib.check(env.L.orlg_set_gn_protect(env.h, int(protect)))


def _queries(env):
    """the ten queries of a gated handle that does not protect: {name: array}"""
    out = {}
    out["observation"] = env.observation()
    out["observation_f32"], out["observation_mask"] = env.observation(dtype=np.float32, return_mask=True)
    out["path_ff"], out["slots"] = env.action_masks("path_ff"), env.action_masks("slots")
    out["fit_levels"] = env.path_fit_levels()
    out["min_cuts"], out["min_cut_slots"] = env.path_min_cuts()
    out["slot_usage"] = env.slot_usage()
    out["most_used"], out["most_used_slots"] = env.path_most_used()
    for kind in env.GN_MASK_KINDS:
        out[kind], out[kind + "_gsnr"] = env.action_masks(kind, gsnr_out=True)
    out.update(zip(("gn_windows_slots", "gn_windows_gsnr", "gn_windows_admitted"), env.path_rule_windows("best")))
    for kind in env.ADMISSION_MASK_KINDS:
        out.update(zip((f"adm_{kind}", f"adm_{kind}_gsnr", f"adm_{kind}_margin"), env.admission_masks(kind, gsnr_out=True, margin_out=True)))
    out.update(zip(("adm_windows_slots", "adm_windows_gsnr", "adm_windows_margin", "adm_windows_admitted"), env.admission_windows("min_cut")))
    audit = env.qot_audit(services=True)
    count = audit["n_running"]
    for k, v in audit.items():   # [B] summaries; [B, Q] per service, compared up to each environment's count
        out["audit_" + k] = v if v.ndim == 1 else [v[i, :count[i]] for i in range(B)]
    return out


def test_the_queries_do_not_depend_on_the_waves_per_workgroup():
    topo = load_topology(pref.CASES[CASE]["topology"])
    small, large = (rmsa_env(topo, B, **pref.case_kwargs(CASE, **over)) for over in ({}, dict(queue_capacity=4096)))
    wpb = [e.launch_info()["envs_per_workgroup"] for e in (small, large)]
    print("waves per workgroup:", wpb)
    assert large.queue_capacity == 4096 and wpb[1] in (1, 2) and wpb[0] > wpb[1] and B % wpb[0] and (wpb[1] == 1 or B % wpb[1])
    steps = [e.run("sap_ff", N, outputs=STEP_OUTS, auto_reset=True) for e in (small, large)]
    for f in STEP_OUTS:
        assert np.array_equal(steps[0][f], steps[1][f]), f
    for e in (small, large):
        _gate(e, protect=False)
    a, b = _queries(small), _queries(large)
    assert a.keys() == b.keys()
    for name in a:
        rows = zip(a[name], b[name]) if isinstance(a[name], list) else [(a[name], b[name])]
        for i, (x, y) in enumerate(rows):
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (name, i)
    assert a["audit_n_running"].min() > 0 and np.isfinite(a["adm_windows_gsnr"]).any() and a["slot_usage"].any()
    # the protecting handle's rule windows against the admission oracle
    for e in (small, large):
        _gate(e, protect=True)
    dev = [e.admission_windows("best") for e in (small, large)]
    for x, y in zip(*dev):
        assert x.tobytes() == y.tobytes()
    slots, gsnr, margin, admitted = dev[0]
    seed = pref.CASES[CASE]["seed"]
    for i in range(B):
        tr, _, fig = adm.run_case(CASE, seed=seed + i, n_steps=N + 1, rules=("best",), gate_items=tuple(GATE.items()))
        for f in STEP_OUTS:   # the gate refused nothing: the oracle stands where the handles stand
            assert np.array_equal(steps[0][f][:, i], tr[f][:N]), (f, i)
        assert np.array_equal(slots[i], tr["best_slots"][N]) and np.array_equal(admitted[i], tr["best_mask"][N]), i
        for d, w, tol in ((gsnr[i], tr["best_gsnr"][N], dict(rtol=RTOL, atol=0)),
                          (margin[i], tr["best_margin"][N], dict(rtol=0, atol=RTOL * fig["max_abs_gsnr"]))):
            assert np.array_equal(np.isnan(d), np.isnan(w)), (i, d, w)
            assert np.allclose(d[~np.isnan(w)], w[~np.isnan(w)], **tol), (i, d, w)
    assert np.isfinite(gsnr).any() and np.isfinite(margin).any()
    small.close(); large.close()
