"""The group kernel's long launches with full statistics release a service in ONE pass per hop (group_release_links): the links'
statistics follow from a per-link summary in LDS and the free runs that border the window, instead of a rescan of the link.
Held byte for byte against the wave-per-environment kernel and against the oracle: per-step outputs, counters, link statistics
and save_state, at slot counts of 1, 2, 5 and 8 words per link (S = 400: slot S - 1 is not in the last word), with links that
fill up and links that become completely free, in whole-launch tickets and in 7 forced chunks (the summaries rebuilt at every
chunk start), with the link logs replayed inside the launch (load 300: a link collects 40 updates within a launch)."""
import numpy as np
import pytest

from gpu_support import against_oracle, device_log_fixture, drive, rmsa_env, same_bytes  # noqa: F401

pytestmark = pytest.mark.gpu

OUTS = ("act_path", "act_slot", "accepted", "reward", "done", "network_compactness", "network_compactness_difference")
LAUNCHES = (700, 333)

# (slots, load, policy, what the occupancy must show at some launch's end: a full link -- at most one free slot: the first-fit
# policies never start a window at S - n or above, so slot S - 1 stays free under them -- or a completely free one)
CASES = [
    (64, 300, "sap_ff", "full"),
    (64, 2, "sap_ff", "free"),
    (100, 300, "deeprmsa_sap_ff", "full"),
    (320, 50, "sap_ff", None),
    (320, 1, "deeprmsa_sp_ff", "free"),
    (400, 600, "deeprmsa_sp_ff", None),
    (512, 150, "sap_ff", None),
    (512, 2, "llp_ff", "free"),
]


@pytest.mark.parametrize("chunks", [None, "7"])
@pytest.mark.parametrize("S,load,policy,shows", CASES)
def test_release_pass_vs_wave_kernel_and_oracle(S, load, policy, shows, chunks, device_log_in_oracle):
    name = "nsfnet_chen_5-paths_6-modulations"
    kw = dict(num_spectrum_resources=S, load=load, mean_service_holding_time=25, episode_length=300, seed=23)
    B = 10
    run = lambda kernel, env_vars: drive(lambda: rmsa_env(name, B, kernel, **kw), LAUNCHES, OUTS, env_vars=env_vars, policy=policy,
                                         each=lambda env: env.available_slots().copy())
    grp = run("group", {"ORLG_GROUP_CHUNKS": chunks} if chunks else {})
    for said in grp["said"]:
        assert said.startswith("orlg_rmsa_group_kernel<") and ",2,false,true>" in said, said
        if chunks:
            assert "chunks=7" in said, said
    wav = run("wave", {})
    same_bytes(grp["tr"], wav["tr"], "outputs")
    same_bytes(grp["snap"], wav["snap"], "state")
    for a, b in zip(grp["each"], wav["each"]):
        assert np.array_equal(a, b)
    if shows == "full":
        assert any((o.sum(axis=2) <= 1).any() for o in grp["each"]), min(int(o.sum(axis=2).min()) for o in grp["each"])
    if shows == "free":
        assert any((o.sum(axis=2) == S).any() for o in grp["each"])
    assert (grp["tr"]["act_slot"][grp["tr"]["accepted"] != 0] == 0).any()   # windows at slot 0
    # (these launches ask for neither arrival nor holding)
    against_oracle(name, kw, grp, policy, LAUNCHES, (0, 5, B - 1), "full", fields=("act_path", "act_slot", "accepted"))
