"""A gate that protects the running lightpaths (``include/orlg.h`` ``orlg_set_gn_protect``), what needs no GPU: the
parameters, the refusals that come before the library is called, the entry points, and -- from the protecting oracle alone
(``gn_protect_reference.py``, the device's logarithm in it) -- the conditions that make the GPU comparison of
``test_gpu_gn_protect.py`` meaningful for every one of its cases."""
import numpy as np
import pytest

import gn_protect_reference as pref
from conftest import load_topology
from optical_rl_gym_amd import BatchedDeepRMSAEnv, BatchedRMSAEnv, _lib, osnr, rmsa_gn_gate_parameters

EIGHT = {"launch_power_density_w_hz", "frequency_start_hz", "slot_width_hz", "attenuation_normalized", "noise_figure",
         "link_num_spans", "link_span_length_km", "thresholds_db"}


@pytest.fixture(scope="module")
def topo():
    return load_topology(pref.NSF)


# ---------------------------------------------------------------------------------------- parameters
def test_the_key_appears_only_on_request(topo):
    assert set(rmsa_gn_gate_parameters(topo)) == EIGHT
    assert set(rmsa_gn_gate_parameters(topo, protect_running=False)) == EIGHT
    g = rmsa_gn_gate_parameters(topo, protect_running=True, launch_power_dbm_per_50ghz=6.0)
    assert set(g) == EIGHT | {"protect_running"} and g["protect_running"] is True
    plain = rmsa_gn_gate_parameters(topo, launch_power_dbm_per_50ghz=6.0)
    for name in EIGHT:
        assert np.array_equal(g[name], plain[name]), name
    # check_rmsa_gn_gate carries the key, and only then
    assert set(osnr.check_rmsa_gn_gate(plain, topo)) == EIGHT
    assert osnr.check_rmsa_gn_gate(g, topo)["protect_running"] is True
    assert set(osnr.check_rmsa_gn_gate(dict(plain, protect_running=False), topo)) == EIGHT


def test_prototypes():
    assert len(_lib.PROTOTYPES["orlg_set_gn_protect"][1]) == 2 and len(_lib.PROTOTYPES["orlg_step_gn_protect"][1]) == 8
    assert "orlg_set_gn_protect" in _lib.EXPORTED_SYMBOLS and "orlg_step_gn_protect" in _lib.EXPORTED_SYMBOLS
    assert _lib.BLOCK_CAUSES[6] == "gn" and _lib.NUM_CAUSES == 8   # (the causes stay as they are)


# ---------------------------------------------------------------------------------------- refusals before the library is called
class _NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although the arguments are wrong")


def _shell(gn_gate, cls=BatchedRMSAEnv, B=3, k=5):
    env = cls.__new__(cls)
    env.L, env.h = _NoLibrary(), None
    env.batch_size, env.k_paths, env.j, env.reject_action, env.words_per_link = B, k, 1, 0, 5
    env.gn_gate = gn_gate
    return env


PROTECTING, GATED = {"protect_running": True}, {"any": 1}


@pytest.mark.parametrize("cls", [BatchedRMSAEnv, BatchedDeepRMSAEnv])
def test_masks_rules_and_windows_are_refused_on_a_protecting_handle(cls):
    env = _shell(PROTECTING, cls)
    assert env.gn_protect and not _shell(GATED, cls).gn_protect and not _shell(None, cls).gn_protect
    for kind in BatchedRMSAEnv.GN_MASK_KINDS:
        with pytest.raises(ValueError, match="protects its running lightpaths"):
            env.action_masks(kind)
        with pytest.raises(ValueError, match="protects its running lightpaths"):
            env.action_masks(kind, gsnr_out=True)
    for mode in _lib.GN_RULE_MODES:
        for name in ("sap_bf", "sap_mc", "sap_lf"):
            with pytest.raises(ValueError, match="protects its running lightpaths"):
                env.run(name, 10, gn_rule=mode)
    for rule in _lib.GN_PATH_WINDOW_RULES:
        with pytest.raises(ValueError, match="protects its running lightpaths"):
            env.path_rule_windows(rule)
    # ... and a rule without the keyword stays refused as on every gated handle
    with pytest.raises(ValueError, match="does not run on a handle with a GN-model admission check"):
        env.run("sap_bf", 10)


def test_protection_without_a_gate(topo, monkeypatch):
    """protect_running lives in the gate's dictionary: there is no way to ask for it without a gate, and a gate that is refused is
    refused before the library loads, with the key as without."""
    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    with pytest.raises(TypeError):
        BatchedRMSAEnv(topo, 2, num_spectrum_resources=100, seed=1, protect_running=True)
    g = rmsa_gn_gate_parameters(topo, protect_running=True)
    with pytest.raises(ValueError, match="group"):
        BatchedRMSAEnv(topo, 2, num_spectrum_resources=100, seed=1, gn_gate=g, step_kernel="group", load=10, mean_service_holding_time=10)
    with pytest.raises(ValueError, match="thresholds_db has 3 entries"):
        BatchedRMSAEnv(topo, 2, num_spectrum_resources=100, seed=1, gn_gate=dict(g, thresholds_db=g["thresholds_db"][:3]))
    with pytest.raises((KeyError, ValueError, TypeError)):
        BatchedRMSAEnv(topo, 2, num_spectrum_resources=100, seed=1, gn_gate={"protect_running": True})


# ---------------------------------------------------------------------------------------- the cases, from the oracle alone
@pytest.mark.parametrize("case", list(pref.CASES))
def test_case_is_meaningful(case):
    """The neighbour check runs, refuses between 2 % and 60 % of what it checks, and no own margin and no neighbour margin lies
    within 1e-4 dB of zero (the device sums the interferers in another order: ~1e-15 relative)."""
    tr, final, fig = pref.run_case(case)
    print(case, fig)
    assert fig["n_checks"] > 0
    assert 0.02 * fig["n_checks"] <= fig["n_rejects"] <= 0.6 * fig["n_checks"]
    assert fig["closest"] > 1e-4 and fig["n_closest"] > 1e-4
    assert int(np.isfinite(tr["gsnr"]).sum()) == fig["checks"] and int(np.isfinite(tr["margin"]).sum()) == fig["n_checks"]
    assert int(tr["accepted"].sum()) == fig["checks"] - fig["rejects"] - fig["n_rejects"]
    assert not np.isfinite(tr["margin"][~np.isfinite(tr["gsnr"])]).any()   # no neighbour check without an own check


def test_two_cases_see_more_than_64_running_services_at_a_neighbour_check():
    assert sum(pref.run_case(case)[2]["n_max_running"] > 64 for case in pref.CASES) >= 2


def test_ring_cases_use_links_beyond_the_first_64():
    """Above 64 links the device keeps a link set -- a victim's, the candidate's -- in four mask words and selects one by
    link >> 6.  In each ring case (238 and 108 links) some check sees running services on links of EVERY range of 64 link ids at
    once, so links beyond the first 64 are in use and every word is exercised.  (Counted as distinct links lit at one check the
    three cases reach 64, 106 and 59; over the whole run 95, 116 and 62: ring36 never has more than 64 distinct links lit, which
    is why the condition is on the ranges.)"""
    for case, c in pref.CASES.items():
        if c["topology"].startswith("ring"):
            E = load_topology(c["topology"]).num_links
            fig = pref.run_case(case)[2]
            assert E > 64 and fig["link_ranges"] == (E + 63) // 64, (case, fig)


@pytest.mark.parametrize("case", pref.SAP_GN_CASES)
def test_sap_ff_gn_goes_on_behind_a_neighbour_refusal(case):
    """At least 5 requests are accepted on a later path after the neighbour check refused an earlier one, and no margin of either
    kind, over every candidate the policy evaluated, lies within 1e-4 dB of zero."""
    tr, final, fig = pref.run_case(case, policy="sap_ff_gn")
    print(case, fig)
    assert fig["later_taken"] >= 5
    assert fig["any_closest"] > 1e-4
