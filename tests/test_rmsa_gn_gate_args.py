"""GN-model admission check of the slot-based environments, what needs no GPU: the parameters (``rmsa_gn_gate_parameters``),
the refusals that come before the library is loaded, and -- from the CPU gated oracle alone (``gn_gate_reference.py``) -- the
conditions that make the GPU comparison of ``test_gpu_rmsa_gn_gate.py`` meaningful for every one of its cases."""
import numpy as np
import pytest

import gn_gate_reference as ref
from conftest import load_topology
from optical_rl_gym_amd import BatchedDeepRMSAEnv, BatchedRMSAEnv, gn_gate_parameters, osnr, rmsa_gn_gate_parameters


@pytest.fixture(scope="module")
def topo():
    return load_topology("nsfnet_chen_5-paths_6-modulations")


def test_parameters(topo):
    g = rmsa_gn_gate_parameters(topo)
    E = topo.num_links
    assert set(g) == {"launch_power_density_w_hz", "frequency_start_hz", "slot_width_hz", "attenuation_normalized", "noise_figure",
                      "link_num_spans", "link_span_length_km", "thresholds_db"}
    assert g["launch_power_density_w_hz"] == 1e-3 / 50e9 and g["frequency_start_hz"] == 191.7e12 and g["slot_width_hz"] == 12.5e9
    # spans, attenuation, noise figure and thresholds: the conventions of the QoT-aware gate
    q = gn_gate_parameters(topo)
    for name in ("attenuation_normalized", "noise_figure"):
        assert g[name] == q[name]
    for name in ("link_num_spans", "link_span_length_km", "thresholds_db"):
        assert np.array_equal(g[name], q[name])
    assert g["link_num_spans"].shape == (E,) and g["link_num_spans"].dtype == np.int32 and (g["link_num_spans"] >= 1).all()
    assert g["link_span_length_km"].shape == (E,) and (g["link_span_length_km"] <= 80.0).all()
    assert np.allclose(g["thresholds_db"], [0.5 * (a + b) for a, b in osnr.TABLE_THRESHOLDS_DB], rtol=0, atol=0)
    h = rmsa_gn_gate_parameters(topo, launch_power_dbm_per_50ghz=6.0, frequency_start_hz=190e12, channel_width=6.25,
                                thresholds_db=[3.0, 1.0, 2.0, 4.0, 5.0, 6.0])
    assert h["launch_power_density_w_hz"] == 1e-3 * 10 ** 0.6 / 50e9 and h["frequency_start_hz"] == 190e12
    assert h["slot_width_hz"] == 6.25e9 and list(h["thresholds_db"]) == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]


def _refused(topo, match, cls=BatchedRMSAEnv, **kw):
    with pytest.raises(ValueError, match=match):
        cls(topo, 2, num_spectrum_resources=100, seed=1, **kw)


def test_refusals_before_the_library_loads(topo, monkeypatch):
    from optical_rl_gym_amd import _lib

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    g = rmsa_gn_gate_parameters(topo)
    _refused(topo, "group", gn_gate=g, step_kernel="group", load=10, mean_service_holding_time=10)
    _refused(topo, "group", cls=BatchedDeepRMSAEnv, gn_gate=g, step_kernel="group")
    _refused(topo, "thresholds_db has 3 entries", gn_gate=dict(g, thresholds_db=g["thresholds_db"][:3]))
    for name in osnr.RMSA_GN_GATE_SCALARS:
        for bad in (0.0, -1.0, np.nan, np.inf):
            _refused(topo, name, gn_gate=dict(g, **{name: bad}))
    _refused(topo, "shape", gn_gate=dict(g, link_num_spans=g["link_num_spans"][:-1]))
    _refused(topo, "link_num_spans", gn_gate=dict(g, link_num_spans=np.zeros_like(g["link_num_spans"])))
    _refused(topo, "link_num_spans", gn_gate=dict(g, link_span_length_km=-g["link_span_length_km"]))
    _refused(topo, "thresholds_db", gn_gate=dict(g, thresholds_db=[np.nan] * 6))


@pytest.mark.parametrize("case", list(ref.CASES))
def test_case_is_meaningful(case):
    """Asserted from the gated oracle alone: the gate refuses between 2 % and 50 % of what it checks, and no GSNR lies within
    1e-4 dB of its threshold (the device sums the interferers in another order: ~1e-15 relative).

    The cases of more than 64 links, seed 7, as this test prints them (checks / refused / most running services / closest [dB]):
    ring34_s100_l60_sapff 407 / 25 / 47 / 0.076; ring34_s320_l300_llpff 460 / 49 / 178 / 0.010;
    ring36_s512_l500_sapff 347 / 62 / 158 / 0.014."""
    tr, final, fig = ref.run_case(case)
    print(case, fig)
    assert fig["checks"] > 0
    assert 0.02 * fig["checks"] <= fig["rejects"] <= 0.5 * fig["checks"]
    assert fig["closest"] > 1e-4
    assert int(np.isfinite(tr["gsnr"]).sum()) == fig["checks"]
    assert int(tr["accepted"].sum()) == fig["checks"] - fig["rejects"]


def test_ring34_cases_hold_services_on_every_range_of_64_links():
    """Above 64 links the device keeps a running service's link set in four mask words and selects one by link >> 6: in each
    ring34 case some check sees running services on links of [0, 64), [64, 128), [128, 192) and [192, 238) at once (ring36, 108
    links: both of its ranges).  Without that the words beyond the first are not exercised."""
    for case, c in ref.CASES.items():
        if c["topology"].startswith("ring"):
            E = load_topology(c["topology"]).num_links
            assert E > 64 and ref.run_case(case)[2]["link_ranges"] == (E + 63) // 64, case


def test_cases_reach_the_second_chunk_of_lanes():
    """Two cases hold more than 64 running services at a check: the second chunk of 64 lanes of the device's check."""
    assert sum(ref.run_case(case)[2]["max_running"] > 64 for case in ref.CASES) >= 2
