"""The GPU tests' support module (gpu_support.py) on the CPU: the byte comparison is as strict as it says, the tooling environment
comes back, the instantiation names are the strings the tests used to write out, the external actions are the arrays the group
tests have always drawn."""
import hashlib
import os
import types

import numpy as np
import pytest

from gpu_support import TOOLING_VARS, external_actions, kernel_name, same_bytes, tooling_env


@pytest.mark.parametrize("a,b", [(np.array([0.0, 1.0]), np.array([-0.0, 1.0])),
                                 (np.arange(3, dtype=np.int32), np.arange(3, dtype=np.int64)),
                                 (np.zeros(3), np.zeros((3, 1)))], ids=["minus-zero", "dtype", "shape"])
def test_same_bytes_tells_apart(a, b):
    assert np.array_equal(a.ravel(), b.ravel())   # (what a looser comparison lets through)
    with pytest.raises(AssertionError):
        same_bytes({"x": a}, {"x": b}, "strict")


def test_same_bytes_wants_the_same_keys_and_names_the_difference():
    with pytest.raises(AssertionError):
        same_bytes({"x": np.zeros(2), "y": np.zeros(2)}, {"x": np.zeros(2)}, "keys")
    a = np.zeros((4, 3))
    b = a.copy()
    b[2, 1] = 5.0
    with pytest.raises(AssertionError, match=r"run: y differs, first at \(2, 1\)"):
        same_bytes({"x": a, "y": a}, {"x": a, "y": b}, "run")


def test_same_bytes_takes_equal_nans_as_equal():
    a = np.array([np.nan, 1.0, np.nan])
    assert not np.array_equal(a, a.copy())
    same_bytes({"x": a, "n": np.zeros(0), "s": np.float64(2.0)}, {"x": a.copy(), "n": np.zeros(0), "s": np.float64(2.0)}, "nan")


def test_tooling_env_restores_the_environment(monkeypatch):
    monkeypatch.setenv("ORLG_NO_DEFER", "before")
    monkeypatch.setenv("ORLG_NO_LEAN", "1")
    monkeypatch.delenv("ORLG_GROUP_CHUNKS", raising=False)
    before = dict(os.environ)
    with pytest.raises(RuntimeError):
        with tooling_env(ORLG_NO_DEFER="1", ORLG_GROUP_CHUNKS="7"):
            # only what was asked for is set inside: a variable of the caller's shell does not leak into a launch
            assert {k: os.environ[k] for k in TOOLING_VARS if k in os.environ} == {"ORLG_NO_DEFER": "1", "ORLG_GROUP_CHUNKS": "7"}
            raise RuntimeError("the body raises")
    assert dict(os.environ) == before
    with pytest.raises(AssertionError):
        with tooling_env(ORLG_NOT_A_VARIABLE="1"):
            pass
    assert dict(os.environ) == before


# (arguments -> the literal the GPU tests asserted before kernel_name existed)
NAMES = [
    # test_gpu_kernel_selection.py: NSFNET-320, launches of 1, 8 and 20 steps, per kind of handle and statistics level
    (("group", 320, "counters", dict(hbmq=True)), "orlg_rmsa_group_kernel<5,0,true>"),
    (("group", 320, "counters", {}), "orlg_rmsa_group_kernel<5,0>"),
    (("group", 320, "network", dict(hbmq=True)), "orlg_rmsa_group_kernel<5,1,true>"),
    (("group", 320, "network", {}), "orlg_rmsa_group_kernel<5,1>"),
    (("group", 320, "full", dict(hbmq=True)), "orlg_rmsa_group_kernel<5,2,true>"),
    (("group", 320, "full", {}), "orlg_rmsa_group_kernel<5,2>"),
    (("group", 320, "full", dict(defer=True)), "orlg_rmsa_group_kernel<5,2,false,true>"),
    (("group", 320, "counters", dict(hbmq=True, traffic=True)), "orlg_rmsa_group_kernel<5,0,true,false,true>"),
    (("group", 320, "counters", dict(traffic=True)), "orlg_rmsa_group_kernel<5,0,false,false,true>"),
    (("group", 320, "network", dict(hbmq=True, traffic=True)), "orlg_rmsa_group_kernel<5,1,true,false,true>"),
    (("group", 320, "network", dict(traffic=True)), "orlg_rmsa_group_kernel<5,1,false,false,true>"),
    (("group", 320, "full", dict(hbmq=True, traffic=True)), "orlg_rmsa_group_kernel<5,2,true,false,true>"),
    (("group", 320, "full", dict(traffic=True)), "orlg_rmsa_group_kernel<5,2,false,false,true>"),
    (("group", 320, "full", dict(defer=True, traffic=True)), "orlg_rmsa_group_kernel<5,2,false,true,true>"),
    (("group", 320, "counters", dict(hbmq=True, trace=True)), "orlg_rmsa_group_kernel<5,0,true,false,false,true>"),
    (("group", 320, "counters", dict(trace=True)), "orlg_rmsa_group_kernel<5,0,false,false,false,true>"),
    (("group", 320, "network", dict(hbmq=True, trace=True)), "orlg_rmsa_group_kernel<5,1,true,false,false,true>"),
    (("group", 320, "network", dict(trace=True)), "orlg_rmsa_group_kernel<5,1,false,false,false,true>"),
    (("group", 320, "full", dict(hbmq=True, trace=True)), "orlg_rmsa_group_kernel<5,2,true,false,false,true>"),
    (("group", 320, "full", dict(trace=True)), "orlg_rmsa_group_kernel<5,2,false,false,false,true>"),
    (("group", 320, "full", dict(defer=True, trace=True)), "orlg_rmsa_group_kernel<5,2,false,true,false,true>"),
    (("wave", 320, "counters", dict(ff=True)), "orlg_rmsa_kernel_ff<5,0>"),
    (("wave", 320, "network", dict(ff=True)), "orlg_rmsa_kernel_ff<5,1>"),
    (("wave", 320, "full", dict(ff=True)), "orlg_rmsa_kernel_ff<5,2>"),
    (("wave", 320, "full", dict(ff=True, defer=True)), "orlg_rmsa_kernel_ff<5,2,true>"),
    (("wave", 320, "counters", {}), "orlg_rmsa_kernel<5,0>"),
    (("wave", 320, "network", {}), "orlg_rmsa_kernel<5,1>"),
    (("wave", 320, "full", {}), "orlg_rmsa_kernel<5,2>"),
    (("wave", 320, "full", dict(defer=True)), "orlg_rmsa_kernel<5,2,true>"),
    # test_gpu_group_chain.py: W from the slot count, seven words of slots on the eight-word layout; the level by number
    (("group", 64, "full", dict(defer=True)), "orlg_rmsa_group_kernel<1,2,false,true>"),
    (("group", 100, 1, {}), "orlg_rmsa_group_kernel<2,1>"),
    (("group", 400, "full", dict(defer=True)), "orlg_rmsa_group_kernel<8,2,false,true>"),
    (("group", 400, "network", {}), "orlg_rmsa_group_kernel<8,1>"),
    (("group", 512, 0, {}), "orlg_rmsa_group_kernel<8,0>"),
    # test_gpu_rmsa.py and test_gpu_many_links.py: words per link given as such
    (("group", 2, "full", {}), "orlg_rmsa_group_kernel<2,2>"),
    (("group", 2, "full", dict(defer=True)), "orlg_rmsa_group_kernel<2,2,false,true>"),
    (("wave", 2, "full", dict(ff=True)), "orlg_rmsa_kernel_ff<2,2>"),
    (("wave", 2, "full", dict(ff=True, defer=True)), "orlg_rmsa_kernel_ff<2,2,true>"),
    (("wave", 5, 0, dict(ff=True)), "orlg_rmsa_kernel_ff<5,0>"),
    (("group", 5, 1, dict(hbmq=True)), "orlg_rmsa_group_kernel<5,1,true>"),
    # test_gpu_rmsa_gn_gate.py: the general wave kernel with the GN-model admission check
    (("wave", 5, "full", dict(gn=True)), "orlg_rmsa_kernel<5,2,false,true>"),
    (("wave", 2, 0, dict(gn=True)), "orlg_rmsa_kernel<2,0,false,true>"),
    (("wave", 8, 1, dict(gn=True)), "orlg_rmsa_kernel<8,1,false,true>"),
]


@pytest.mark.parametrize("args,literal", NAMES, ids=[n for _, n in NAMES])
def test_kernel_name_is_the_written_out_literal(args, literal):
    family, w_or_s, stats, flags = args
    assert kernel_name(family, w_or_s, stats, **flags) == literal


# sha256 (first 16 hex digits) of the arrays the two functions this one replaced returned, recorded from them: test_gpu_group_chain's
# (seed 123, a third of the steps // 8) and test_gpu_group_lean's (seed 5; every slot // 4, or the paths alone)
ACTIONS = [
    ((5, 64, 200, 10, 123, "third_low"), (200, 10, 2), "a0b1acb403ecae15", [[0, 1], [2, 41], [0, 4], [0, 3]]),
    ((3, 100, 200, 10, 123, "third_low"), (200, 10, 2), "d0f215ae539e1df2", [[0, 1], [1, 63], [0, 6], [0, 5]]),
    ((5, 320, 200, 10, 123, "third_low"), (200, 10, 2), "a8b7d64404dc9841", [[0, 5], [2, 202], [0, 21], [0, 18]]),
    ((5, 320, 40, 5, 5, "quarter"), (40, 5, 2), "b3af41645f39add0", [[4, 15], [3, 11], [1, 44]]),
    ((3, 100, 40, 64, 5, "quarter"), (40, 64, 2), "75b1d9921f716c9d", [[2, 1], [0, 15], [2, 18]]),
    ((5, 320, 40, 5, 5, "paths"), (40, 5), "d1fc1b4db760971c", [4, 3, 1]),
    ((3, 100, 40, 64, 5, "paths"), (40, 64), "1a035d04da42b684", [2, 0, 2]),
]


@pytest.mark.parametrize("args,shape,digest,first", ACTIONS, ids=[f"K{a[0]}-S{a[1]}-{a[5]}" for a, *_ in ACTIONS])
def test_external_actions_are_the_arrays_they_were(args, shape, digest, first):
    K, S, n, batch, seed, kind = args
    a = external_actions(types.SimpleNamespace(k_paths=K), S, n, batch, seed=seed, kind=kind)
    assert a.shape == shape and a.dtype == np.int32
    assert a[:len(first), 0].tolist() == first
    assert hashlib.sha256(a.tobytes()).hexdigest()[:16] == digest
    if kind == "third_low":
        assert external_actions(types.SimpleNamespace(k_paths=K), S, n, batch).tobytes() == a.tobytes()   # the defaults


@pytest.mark.parametrize("K,S", [(9, 64), (10, 384), (32, 100)])
def test_external_actions_aimed_at_the_high_paths(K, S):
    """kind "high_paths": more than half of the actions name a path 8 .. K - 1, both components go out of range, a third of the
    steps aim low as "third_low" does, and the actions left alone are the ones "third_low" gives."""
    topo = types.SimpleNamespace(k_paths=K)
    a, low = external_actions(topo, S, 150, 6, kind="high_paths"), external_actions(topo, S, 150, 6)
    assert a.shape == (150, 6, 2) and a.dtype == np.int32
    high = (a[..., 0] >= 8) & (a[..., 0] < K)
    assert high.mean() > 0.55
    assert (a[..., 0] == K).any() and (a[..., 1] == S).any() and a.min() == 0 and a[..., 0].max() == K and a[..., 1].max() == S
    assert np.array_equal(a[..., 1], low[..., 1]) and np.array_equal(a[~high], low[~high])
    assert (a[..., 0] != low[..., 0]).mean() > 0.4
    with pytest.raises(AssertionError):
        external_actions(types.SimpleNamespace(k_paths=8), S, 4, 2, kind="high_paths")
