"""The Python side without a device: the handle base both batched environments derive from may call only functions that
exist under both symbol prefixes, the prototype table is the header's list of functions, the shared blocking-rate arithmetic
is the four expressions of the info dict written out, and a wrong-shaped ``seeds=`` is a ``ValueError`` on both kinds."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_phy_tables, load_topology


def test_shared_methods_name_only_functions_both_kinds_have():
    from optical_rl_gym_amd import BatchedPhyRMSAEnv, BatchedRMSAEnv, _lib
    from optical_rl_gym_amd._handle import BatchedHandle
    shared = set(BatchedHandle.SHARED_CALLS)
    assert len(shared) == len(BatchedHandle.SHARED_CALLS)
    prefixes = [cls.PREFIX for cls in (BatchedRMSAEnv, BatchedPhyRMSAEnv)]
    assert prefixes == ["orlg_", "orlg_phy_"] and BatchedHandle.PREFIX is None
    # the binding of BatchedHandle._open, done here for both prefixes against the loaded library: every shared name resolves
    L = _lib.load()
    for p in prefixes:
        for name in BatchedHandle.SHARED_CALLS:
            assert getattr(L, p + name).argtypes == _lib.PROTOTYPES[p + name][1], p + name
    # a tripwire over the source: whatever a method of the three classes calls through the bound namespace is declared shared
    # (and an entry that nothing calls is dead)
    used = set()
    for cls in (BatchedHandle, BatchedRMSAEnv, BatchedPhyRMSAEnv):
        used |= set(re.findall(r"\bself\._c\.([A-Za-z_0-9]+)", inspect.getsource(cls)))
    assert used == shared, used ^ shared
    # the base reaches the library through that namespace alone (self.L belongs to the variants)
    assert not re.findall(r"\bself\.L\.", inspect.getsource(BatchedHandle))
    for name in sorted(shared):
        rmsa, phy = (_lib.PROTOTYPES[p + name] for p in prefixes)   # KeyError: one kind lacks it
        assert rmsa[0] == phy[0], name
        if name.startswith("create"):   # the config struct is the variant's own
            assert [a for i, a in enumerate(rmsa[1]) if i != 1] == [a for i, a in enumerate(phy[1]) if i != 1], name
        else:
            assert rmsa[1] == phy[1] and rmsa[1] is not None, name
    # functions of one kind stay out of the base
    assert "launch_info" not in shared and "orlg_phy_launch_info" not in _lib.PROTOTYPES
    for name in ("launch_info", "episode_stats", "run", "occupancy_words", "available_channels"):
        assert not hasattr(BatchedHandle, name), name


def test_prototype_table_is_the_header():
    from optical_rl_gym_amd import _lib
    header = open(os.path.join(ROOT, "include", "orlg.h")).read()
    declared = sorted(set(re.findall(r"\b(orlg_[a-z_0-9]+)\s*\(", header)))
    assert declared
    assert sorted(_lib.PROTOTYPES) == declared
    assert sorted(_lib.EXPORTED_SYMBOLS) == declared and len(_lib.EXPORTED_SYMBOLS) == len(declared)
    L = _lib.load()
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        f = getattr(L, name)
        if restype is not None:
            assert f.restype is restype, name
        if name != "orlg_gn_osnr":   # (osnr.py sets its argtypes next to its struct)
            assert f.argtypes == argtypes, name


def _by_hand(c, nxt):
    """The four rates written out as the gym views' info dicts state them (``rmsa_env.py:293-332`` after taking the pending
    request out of the request-side counters): ints in, Python's true division."""
    c = dict(c)
    c["services_processed"] -= 1
    c["episode_services_processed"] -= 1
    c["bit_rate_requested"] -= nxt
    c["episode_bit_rate_requested"] -= nxt
    return {
        "service_blocking_rate": (c["services_processed"] - c["services_accepted"]) / c["services_processed"],
        "episode_service_blocking_rate": (c["episode_services_processed"] - c["episode_services_accepted"])
        / c["episode_services_processed"],
        "bit_rate_blocking_rate": (c["bit_rate_requested"] - c["bit_rate_provisioned"]) / c["bit_rate_requested"],
        "episode_bit_rate_blocking_rate": (c["episode_bit_rate_requested"] - c["episode_bit_rate_provisioned"])
        / c["episode_bit_rate_requested"],
    }


# (counters, pending bit rate): ordinary; nothing blocked -- the pending rate makes every numerator 0; all blocked
COUNTER_CASES = [
    (dict(services_processed=8, services_accepted=5, episode_services_processed=4, episode_services_accepted=2,
          bit_rate_requested=2100, bit_rate_provisioned=1300, episode_bit_rate_requested=1000,
          episode_bit_rate_provisioned=450), 300),
    (dict(services_processed=4, services_accepted=3, episode_services_processed=2, episode_services_accepted=1,
          bit_rate_requested=900, bit_rate_provisioned=700, episode_bit_rate_requested=350,
          episode_bit_rate_provisioned=150), 200),
    (dict(services_processed=3, services_accepted=0, episode_services_processed=3, episode_services_accepted=0,
          bit_rate_requested=75, bit_rate_provisioned=0, episode_bit_rate_requested=75, episode_bit_rate_provisioned=0), 25),
]


@pytest.mark.parametrize("c,nxt", COUNTER_CASES)
def test_blocking_rates_scalars(c, nxt):
    from optical_rl_gym_amd import traffic
    before = dict(c)
    got = traffic.blocking_rates(c, nxt)
    want = _by_hand(c, nxt)
    assert c == before                                   # (the caller's dict is left alone)
    assert list(got) == list(want)                       # the info dict's key order
    for k in want:
        assert type(got[k]) is float and got[k] == want[k], k
    if nxt == 200:
        assert set(got.values()) == {0.0}
    if nxt == 25:
        assert set(got.values()) == {1.0}
    assert traffic.blocking_rates(COUNTER_CASES[0][0], 300)["bit_rate_blocking_rate"] == (1800 - 1300) / 1800


def test_blocking_rates_arrays():
    """int64 arrays, as the evaluate functions of monitor.py pass them: element by element the scalar result."""
    from optical_rl_gym_amd import traffic
    c = {k: np.array([case[k] for case, _ in COUNTER_CASES], np.int64) for k in COUNTER_CASES[0][0]}
    nxt = np.array([n for _, n in COUNTER_CASES], np.int64)
    got = traffic.blocking_rates(c, nxt)
    # the same on arrays, as the Monitor rows of a whole batch are formed
    proc, eproc = c["services_processed"] - 1, c["episode_services_processed"] - 1
    req, ereq = c["bit_rate_requested"] - nxt, c["episode_bit_rate_requested"] - nxt
    want = {"service_blocking_rate": (proc - c["services_accepted"]) / proc,
            "episode_service_blocking_rate": (eproc - c["episode_services_accepted"]) / eproc,
            "bit_rate_blocking_rate": (req - c["bit_rate_provisioned"]) / req,
            "episode_bit_rate_blocking_rate": (ereq - c["episode_bit_rate_provisioned"]) / ereq}
    for k in want:
        assert got[k].dtype == np.float64 and got[k].shape == (3,) and np.array_equal(got[k], want[k]), k
        for i, (case, n) in enumerate(COUNTER_CASES):
            assert got[k][i] == _by_hand(case, n)[k], (k, i)


@pytest.mark.parametrize("seeds", [[1, 2, 3], np.arange(8).reshape(4, 2), list(range(5))])
def test_wrong_shaped_seeds_are_a_value_error_on_both_kinds(nsfnet, seeds):
    """The check runs after the library is loaded (the order it always had) and before anything is created, so it needs no
    device."""
    from optical_rl_gym_amd import BatchedDeepRMSAEnv, BatchedPhyRMSAEnv, BatchedRMSAEnv
    shape = np.shape(seeds)
    with pytest.raises(ValueError, match=re.escape(f"seeds: shape {shape}, expected (4,)")):
        BatchedRMSAEnv(nsfnet, 4, num_spectrum_resources=320, load=50, mean_service_holding_time=25, seeds=seeds)
    with pytest.raises(ValueError, match=re.escape(f"seeds: shape {shape}, expected (4,)")):
        BatchedDeepRMSAEnv(nsfnet, 4, num_spectrum_resources=320, seeds=seeds)
    us14, tables = load_topology("us14_3-paths_6-modulations"), load_phy_tables("us14_k3")
    with pytest.raises(ValueError, match=re.escape(f"seeds: shape {shape}, expected (4,)")):
        BatchedPhyRMSAEnv(us14, 4, modulation_level=tables[1], connections_detail=tables[0], gsnr=tables[2], load=1400,
                          mean_service_holding_time=25, seeds=seeds)
