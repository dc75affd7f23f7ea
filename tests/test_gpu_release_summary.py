"""The group kernel's long launches with full statistics release a service in ONE pass per hop (group_release_links): the links'
statistics follow from a per-link summary in LDS and the free runs that border the window, instead of a rescan of the link.
Held byte for byte against the wave-per-environment kernel and against the oracle: per-step outputs, counters, link statistics
and save_state, at slot counts of 1, 2, 5 and 8 words per link (S = 400: slot S - 1 is not in the last word), with links that
fill up and links that become completely free, in whole-launch tickets and in 7 forced chunks (the summaries rebuilt at every
chunk start), with the link logs replayed inside the launch (load 300: a link collects 40 updates within a launch)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_topology, oracle_env_from_kwargs

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


@pytest.fixture()
def device_log_in_oracle():
    import oracle as orc
    from optical_rl_gym_amd import _lib
    orc.set_log_fn(C.cast(_lib.load().orlg_host_log, C.c_void_p).value)
    yield
    orc.set_log_fn(None)


def _drive(topo, kw, B, kernel, policy, env_vars):
    from optical_rl_gym_amd import BatchedRMSAEnv
    old = {k: os.environ.get(k) for k in ("ORLG_GROUP_CHUNKS", "ORLG_NO_DEFER")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env_vars)
    try:
        env = BatchedRMSAEnv(topo, B, step_kernel=kernel, **kw)
        runs, names, occ = [], [], []
        for n in LAUNCHES:
            runs.append(env.run(policy, n, outputs=OUTS, auto_reset=True))
            names.append(env.last_kernel())
            occ.append(env.available_slots().copy())
        res = dict(runs=runs, names=names, occ=occ, state=env.save_state().copy(),
                   counters={k: v.copy() for k, v in env.counters().items()},
                   links={k: v.copy() for k, v in env.link_stats().items()})
        env.close()
        return res
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("chunks", [None, "7"])
@pytest.mark.parametrize("S,load,policy,shows", CASES)
def test_release_pass_vs_wave_kernel_and_oracle(S, load, policy, shows, chunks, device_log_in_oracle):
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    kw = dict(num_spectrum_resources=S, load=load, mean_service_holding_time=25, episode_length=300, seed=23)
    B = 10
    grp = _drive(topo, kw, B, "group", policy, {"ORLG_GROUP_CHUNKS": chunks} if chunks else {})
    for name in grp["names"]:
        assert name.startswith("orlg_rmsa_group_kernel<") and ",2,false,true>" in name, name
        if chunks:
            assert "chunks=7" in name, name
    wav = _drive(topo, kw, B, "wave", policy, {})
    for x, y in zip(grp["runs"], wav["runs"]):
        for k in OUTS:
            assert np.array_equal(x[k], y[k]), k
    assert np.array_equal(grp["state"], wav["state"])
    for k in wav["counters"]:
        assert np.array_equal(grp["counters"][k], wav["counters"][k]), k
    for k in wav["links"]:
        assert np.array_equal(grp["links"][k], wav["links"][k]), k
    for a, b in zip(grp["occ"], wav["occ"]):
        assert np.array_equal(a, b)
    if shows == "full":
        assert any((o.sum(axis=2) <= 1).any() for o in grp["occ"]), min(int(o.sum(axis=2).min()) for o in grp["occ"])
    if shows == "free":
        assert any((o.sum(axis=2) == S).any() for o in grp["occ"])
    assert (np.concatenate([r["act_slot"][r["accepted"] != 0] for r in grp["runs"]]) == 0).any()   # windows at slot 0
    for i in (0, 5, B - 1):
        o = oracle_env_from_kwargs(topo, kw, seed=23 + i)
        tr = o.run(policy, sum(LAUNCHES), reset_on_done=True)
        for f in ("act_path", "act_slot", "accepted"):
            assert np.array_equal(np.concatenate([r[f][:, i] for r in grp["runs"]]), tr[f]), (f, i)
        assert np.array_equal(grp["occ"][-1][i], o.available_slots()), i
        ols = o.link_stats()
        for name in ols:
            assert np.array_equal(grp["links"][name][i], ols[name]), (name, i)
        o.close()
