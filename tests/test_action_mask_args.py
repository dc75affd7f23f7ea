"""Valid-action masks, the part that needs no GPU: the entry points are declared, exported and bound, and a buffer of the wrong
shape or dtype or an unknown mask kind is refused before the library is called."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from optical_rl_gym_amd import BatchedPhyRMSAEnv, BatchedRMSAEnv, _lib

NEW = ["orlg_deeprmsa_observation_masked", "orlg_deeprmsa_mask_dim", "orlg_action_masks", "orlg_phy_channel_masks"]


def test_new_symbols_in_a_fresh_library():
    assert set(NEW) <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.load()
    assert L.orlg_abi_version() == 3
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW) <= names
    header = open(os.path.join(ROOT, "include", "orlg.h")).read()
    assert "#define ORLG_ABI_VERSION 3" in header
    for s in NEW:
        assert s + "(" in header
        assert hasattr(L, s) and getattr(L, s).argtypes is not None   # bound with argument types in _lib.load


class _NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although the arguments are wrong")


def _rmsa_shell(B=3, k=5, j=2, S=320, reject=1, N=14):
    env = BatchedRMSAEnv.__new__(BatchedRMSAEnv)
    env.L, env.h = _NoLibrary(), None
    env.batch_size, env.k_paths, env.j, env.num_spectrum_resources, env.reject_action = B, k, j, S, reject
    env.words_per_link = (S + 63) // 64
    env.obs_dim = 1 + 2 * N + (2 * j + 3) * k
    env.mask_dim = k * j + reject
    return env


def test_mask_shapes():
    env = _rmsa_shell()
    assert env.action_mask_shape("deeprmsa") == ((3, 11), np.uint8)
    assert env.action_mask_shape("path_ff") == ((3, 6), np.uint8)
    assert env.action_mask_shape("slots") == ((3, 5, 5), np.uint64)
    env = _rmsa_shell(reject=0, j=1)
    assert env.action_mask_shape("deeprmsa") == ((3, 5), np.uint8)
    assert env.action_mask_shape("path_ff") == ((3, 5), np.uint8)


@pytest.mark.parametrize("kind", ["deep", "", None, "channels", "DEEPRMSA"])
def test_unknown_kind(kind):
    with pytest.raises(ValueError, match="kind"):
        _rmsa_shell().action_masks(kind)


@pytest.mark.parametrize("kind,shape,dtype,err", [
    ("deeprmsa", (3, 10), np.uint8, ValueError),      # the rejection column is missing
    ("deeprmsa", (11, 3), np.uint8, ValueError),
    ("deeprmsa", (3, 11), np.bool_, TypeError),
    ("deeprmsa", (3, 11), np.int8, TypeError),
    ("path_ff", (3, 5), np.uint8, ValueError),
    ("path_ff", (3, 6), np.int32, TypeError),
    ("slots", (3, 5, 4), np.uint64, ValueError),
    ("slots", (3, 5, 320), np.uint64, ValueError),
    ("slots", (3, 5, 5), np.int64, TypeError),
    ("slots", (3, 5, 5), np.uint8, TypeError),
])
def test_action_masks_refuses_a_wrong_buffer(kind, shape, dtype, err):
    with pytest.raises(err, match="out"):
        _rmsa_shell().action_masks(kind, out=np.zeros(shape, dtype))


def test_action_masks_refuses_a_strided_or_read_only_buffer():
    env = _rmsa_shell()
    with pytest.raises(ValueError, match="contiguous"):
        env.action_masks("deeprmsa", out=np.zeros((3, 22), np.uint8)[:, ::2])
    ro = np.zeros((3, 6), np.uint8)
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="read-only"):
        env.action_masks("path_ff", out=ro)


@pytest.mark.parametrize("shape,dtype,err", [((3, 10), np.uint8, ValueError), ((3, 11), np.bool_, TypeError),
                                             ((3, 11), np.float32, TypeError), ((33,), np.uint8, ValueError)])
def test_observation_refuses_a_wrong_mask_buffer(shape, dtype, err):
    env = _rmsa_shell()
    with pytest.raises(err, match="mask_out"):
        env.observation(mask_out=np.zeros(shape, dtype))
    with pytest.raises(err, match="mask_out"):
        env.observation(out=np.zeros((3, env.obs_dim), np.float32), mask_out=np.zeros(shape, dtype))


def test_observation_checks_the_observation_buffer_before_the_mask_call():
    env = _rmsa_shell()
    good_mask = np.zeros((3, 11), np.uint8)
    with pytest.raises(ValueError, match="out"):
        env.observation(out=np.zeros((3, env.obs_dim + 1)), mask_out=good_mask)
    with pytest.raises(TypeError, match="out"):
        env.observation(out=np.zeros((3, env.obs_dim), np.float16), mask_out=good_mask)


@pytest.mark.parametrize("shape,dtype,err", [((2, 3, 4), np.uint64, ValueError), ((2, 3, 5), np.int64, TypeError),
                                             ((2, 3, 268), np.uint8, ValueError), ((2, 15), np.uint64, ValueError)])
def test_channel_masks_refuses_a_wrong_buffer(shape, dtype, err):
    env = BatchedPhyRMSAEnv.__new__(BatchedPhyRMSAEnv)
    env.L, env.h = _NoLibrary(), None
    env.batch_size, env.k_paths, env.num_channels, env.words_per_link = 2, 3, 268, 5
    with pytest.raises(err, match="out"):
        env.channel_masks(out=np.zeros(shape, dtype))


def test_action_index_division_in_the_observation_kernel():
    """The kernel turns action a into (route, block) = (a // j, a % j) with a multiply and a shift; exact for every a it sees:
    a < k * j + 1 with k * W <= 64 and j <= 16 (the observation row of 2j + 3 values per path has the same bound)."""
    for j in range(1, 17):
        inv = (65536 + j - 1) // j
        a = np.arange(64 * j + 1, dtype=np.uint32)
        assert np.array_equal((a * np.uint32(inv)) >> np.uint32(16), a // j), j
