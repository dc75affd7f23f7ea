"""Blocking cause and fit levels (``include/orlg.h`` ``ORLG_CAUSE_*`` / ``ORLG_FIT_*``), what needs no GPU: the numpy
restatement of the definitions (``block_cause_reference.py``) against brute force on the oracle's own queries, what the
definitions imply for the first-fit policies, that every code the GPU comparison of ``test_gpu_block_cause.py`` is meant to see
does occur on its shapes, the entry points and their prototypes, the refusals that come before the library is called, the
per-group helper, and that the new key lists resolve to their kernels."""
import os
import subprocess

import numpy as np
import pytest

import block_cause_reference as ref
from conftest import ROOT, load_topology, oracle_env_from_kwargs
from gpu_support import device_log_in_oracle
from optical_rl_gym_amd import BLOCK_CAUSES, FIT_LEVELS, BatchedPhyRMSAEnv, BatchedRMSAEnv, _lib, traffic

NEW = ["orlg_step_diag", "orlg_path_fit_levels"]
FF_POLICIES = ("sp_ff", "sap_ff", "llp_ff")


# ---------------------------------------------------------------------------------------- the reference against brute force
@pytest.mark.parametrize("S,load", [(64, 10), (100, 20)])
def test_reference_levels_against_the_oracle_queries(S, load):
    """level 4 <=> some is_path_free(p, s, n) with s < S - n; level >= 3 <=> some s <= S - n; below 3 the link questions by
    brute force on the availability rows."""
    topo = load_topology(ref.NSFNET)
    kw = ref.shape_kwargs(S, load)
    seen = set()
    with device_log_in_oracle():
        o = oracle_env_from_kwargs(topo, kw, seed=ref.SEED0)
        for _ in range(ref.N_STEPS):
            r, avail = o.request(), o.available_slots()
            lv = ref.path_levels(avail, topo, r.src, r.dst, r.bit_rate)
            base = int(topo.pair_path_base[r.src * topo.num_nodes + r.dst])
            for p in range(topo.k_paths):
                n = o.number_slots(p)
                assert n == ref.number_slots(r.bit_rate, int(topo.path_se[base + p]))
                free = [s for s in range(S) if o.is_path_free(p, s, n)]
                assert (lv[p] == ref.FIT) == any(s < S - n for s in free), (p, lv[p], free)
                assert (lv[p] >= ref.LAST_WINDOW) == any(s <= S - n for s in free), (p, lv[p], free)
                if lv[p] < ref.LAST_WINDOW:
                    links = topo.path_links[topo.path_link_off[base + p]:topo.path_link_off[base + p + 1]]
                    runs = [any(avail[l, s:s + n].all() for s in range(S - n + 1)) for l in links]
                    room = [int(avail[l].sum()) >= n for l in links]
                    assert lv[p] == (ref.ALIGNMENT if all(runs) else ref.CONTIGUITY if all(room) else ref.CAPACITY), (p, lv[p])
                seen.add(int(lv[p]))
            o.run("sap_ff", 1, reset_on_done=True, fields=[])
        o.close()
    assert seen == set(range(5)), seen   # every level was compared


def test_reference_edge_cases():
    avail = np.ones((2, 10), np.uint8)
    assert ref.path_level(avail, [0, 1], 10) == ref.LAST_WINDOW     # the only window starts at S - n = 0
    assert ref.path_level(avail, [0, 1], 11) == ref.CAPACITY        # n > S
    assert ref.path_level(avail, [0, 1], 9) == ref.FIT
    avail[0, 0] = 0
    assert ref.path_level(avail, [0, 1], 9) == ref.LAST_WINDOW
    avail[1, 9] = 0
    assert ref.path_level(avail, [0, 1], 9) == ref.ALIGNMENT        # [1, 10) on link 0, [0, 9) on link 1
    avail[1, 4] = 0
    assert ref.path_level(avail, [0, 1], 8) == ref.CONTIGUITY       # link 1 has 8 free slots in runs of 4
    assert ref.path_level(avail, [0, 1], 9) == ref.CAPACITY
    assert ref.block_cause([0, 4, 2], True) == ref.ACCEPTED and ref.block_cause([0, 4, 2], False) == ref.C_POLICY
    assert ref.block_cause([0, 4, 2], False, gn_refused=True) == ref.C_GN and ref.block_cause([0, 1], False) == ref.C_CONTIGUITY


# ---------------------------------------------------------------------------------------- what the definitions imply; occurrence
@pytest.mark.parametrize("S,load", ref.SHAPES[:3])
@pytest.mark.parametrize("policy", FF_POLICIES)
def test_first_fit_policies_on_the_issue_shapes(S, load, policy):
    """Accepted implies L = 4 for the first-fit policies; sap_ff and llp_ff never yield POLICY; and each code 0..4 (sp_ff: 0..5)
    occurs on every shape the GPU tests compare, so that none of their comparisons is vacuous."""
    runs = [ref.nsfnet_steps(S, load, policy, i) for i in range(ref.N_ENVS)]
    cause = np.stack([r["cause"] for r in runs], axis=1)
    top = np.stack([r["levels"].max(axis=1) for r in runs], axis=1)
    acc = np.stack([r["accepted"] for r in runs], axis=1)
    assert (top[acc == 1] == ref.FIT).all()
    assert ((cause == ref.ACCEPTED) == (acc == 1)).all()
    if policy != "sp_ff":
        assert not (cause == ref.C_POLICY).any()
        assert ((top == ref.FIT) == (acc == 1)).all()
    counts = np.bincount(cause.ravel(), minlength=ref.NUM_CAUSES)
    want = range(6) if policy == "sp_ff" else range(5)
    assert all(counts[c] > 0 for c in want), (S, load, policy, counts)
    assert counts[6] == 0 and counts[7] == 0 and counts.sum() == ref.N_ENVS * ref.N_STEPS


def test_counts_of_the_issue_table():
    """The table of the issue, one row: NSFNET-320 at load 50 under sap_ff."""
    cause = np.stack([ref.nsfnet_steps(320, 50, "sap_ff", i)["cause"] for i in range(ref.N_ENVS)], axis=1)
    assert list(np.bincount(cause.ravel(), minlength=8)) == [1312, 12, 128, 143, 5, 0, 0, 0]
    assert ref.counts_of(cause).sum(axis=1).tolist() == [ref.N_STEPS] * ref.N_ENVS


# ---------------------------------------------------------------------------------------- ABI, prototypes, exports
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
        assert hasattr(L, s) and getattr(L, s).argtypes is not None
    for i, name in enumerate(BLOCK_CAUSES):
        assert "ORLG_CAUSE_%s = %d" % (name.upper(), i) in header
    for i, name in enumerate(FIT_LEVELS):
        assert "ORLG_FIT_%s = %d" % (name.upper(), i) in header
    assert "ORLG_NUM_CAUSES = 8" in header and _lib.NUM_CAUSES == 8
    assert [n for n, _ in _lib.StepDiag._fields_] == ["block_cause", "cause_counts", "gn_gsnr_db"]
    assert BLOCK_CAUSES == ("accepted", "capacity", "contiguity", "alignment", "last_window", "policy", "gn")
    assert FIT_LEVELS == ("capacity", "contiguity", "alignment", "last_window", "fit")


def test_cause_key_lists_resolve_to_their_kernels():
    from host_programs import variant_names
    from optical_rl_gym_amd import build
    counts = variant_names().counts
    # per word count: 3 statistics levels x {no gate, GN} wave keys, 3 x {plain, traffic, trace} group keys; the query kernel is one
    # of the single-kernel lookups the program walks
    assert (counts["ORLG_WAVE_CAUSE_KEYS"], counts["ORLG_GROUP_CAUSE_KEYS"]) == (6 * len(build.WAVE_W), 9 * len(build.WAVE_W))
    assert counts["ORLG_WAVE_QUERIES"] == 12 * len(build.WAVE_W) + 2   # (orlg_fit_levels_kernel among them)


# ---------------------------------------------------------------------------------------- refusals before the library is called
class _NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although the arguments are wrong")


def _rmsa_shell(B=3, k=5):
    env = BatchedRMSAEnv.__new__(BatchedRMSAEnv)
    env.L, env.h = _NoLibrary(), None
    env.batch_size, env.k_paths = B, k
    return env


@pytest.mark.parametrize("buf,error", [(np.zeros((3, 8), np.int64), TypeError), (np.zeros((3, 7), np.int32), ValueError),
                                       (np.zeros((4, 8), np.int32), ValueError), (np.zeros((8, 3), np.int32).T, ValueError),
                                       (np.zeros(24, np.int32), ValueError)])
def test_cause_counts_buffer_is_checked(buf, error):
    with pytest.raises(error, match="cause_counts"):
        _rmsa_shell().run("sap_ff", 10, cause_counts=buf)


def test_cause_counts_read_only_buffer():
    buf = np.zeros((3, 8), np.int32)
    buf.setflags(write=False)
    with pytest.raises(ValueError, match="read-only"):
        _rmsa_shell().run("sap_ff", 10, cause_counts=buf)


@pytest.mark.parametrize("buf,error", [(np.zeros((10, 3), np.int8), TypeError), (np.zeros((10, 4), np.uint8), ValueError),
                                       (np.zeros((9, 3), np.uint8), ValueError)])
def test_block_cause_buffer_is_checked(buf, error):
    with pytest.raises(error, match="block_cause"):
        _rmsa_shell().run("sap_ff", 10, out={"block_cause": buf})


@pytest.mark.parametrize("buf,error", [(np.zeros((3, 5), np.int32), TypeError), (np.zeros((3, 4), np.uint8), ValueError),
                                       (np.zeros((5, 3), np.uint8).T, ValueError)])
def test_path_fit_levels_buffer_is_checked(buf, error):
    with pytest.raises(error, match="out"):
        _rmsa_shell().path_fit_levels(out=buf)


@pytest.mark.parametrize("kw", [dict(cause_counts=True), dict(cause_counts=np.zeros((3, 8), np.int32)),
                                dict(outputs=("block_cause",)), dict(out={"block_cause": np.zeros((10, 3), np.uint8)})])
def test_qot_aware_handle_has_no_blocking_cause(kw):
    env = BatchedPhyRMSAEnv.__new__(BatchedPhyRMSAEnv)
    env.L, env.h, env.batch_size = _NoLibrary(), None, 3
    with pytest.raises(ValueError, match="blocking cause"):
        env.run("bmfa", 10, **kw)


# ---------------------------------------------------------------------------------------- blocking by cause versus load
def test_blocking_shares_by_group():
    counts = np.array([[8, 1, 1, 0, 0, 0, 0, 0], [6, 0, 2, 2, 0, 0, 0, 0], [10, 0, 0, 0, 0, 0, 0, 0], [5, 0, 0, 0, 1, 4, 0, 0]], np.int32)
    r = traffic.blocking_shares_by_group(counts, [0, 0, 1, 2], num_groups=4, loads=[10, 10, 20, 30])
    assert r["counts"].tolist() == [[14, 1, 3, 2, 0, 0, 0, 0], [10, 0, 0, 0, 0, 0, 0, 0], [5, 0, 0, 0, 1, 4, 0, 0], [0] * 8]
    assert r["steps"].tolist() == [20, 10, 10, 0]
    assert np.array_equal(r["shares"][0], np.array([14, 1, 3, 2, 0, 0, 0, 0]) / 20) and r["shares"][1, 0] == 1.0
    assert np.isnan(r["shares"][3]).all() and np.isnan(r["loads"][3]) and r["loads"][:3].tolist() == [10.0, 20.0, 30.0]
    assert "loads" not in traffic.blocking_shares_by_group(counts, [0, 0, 1, 2])
    with pytest.raises(ValueError, match="different loads"):
        traffic.blocking_shares_by_group(counts, [0, 0, 1, 1], loads=[10, 10, 20, 30])
    with pytest.raises(ValueError, match="cause_counts"):
        traffic.blocking_shares_by_group(counts[:, :7], [0, 0, 1, 2])
    with pytest.raises(TypeError, match="cause_counts"):
        traffic.blocking_shares_by_group(counts.astype(np.float64), [0, 0, 1, 2])
    with pytest.raises(ValueError, match="groups"):
        traffic.blocking_shares_by_group(counts, [0, 0, 1])
