"""Adaptive modulation behind the GN gate (``include/orlg.h`` ``orlg_set_gn_modulation``, ``orlg_step_modulation``,
``orlg_gn_modulation_windows``) without a GPU: the symbols, the unit and the names of its kernels, every refusal before
the library is called, the descriptor's decode, and -- from the reference alone, every case of ``test_gpu_gn_modulation.py`` stepped by
its own choices -- what those cases exercise, and what the shapes of ``test_gpu_gn_modulation_shapes.py`` reach."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gn_gate_reference as ref
import gn_modulation_reference as am
from conftest import ROOT, load_topology, oracle_env_from_kwargs
from gpu_support import device_log_in_oracle
from optical_rl_gym_amd import BatchedDeepRMSAEnv, BatchedRMSAEnv, _lib, rmsa_gn_gate_parameters

NEW = ("orlg_set_gn_modulation", "orlg_step_modulation", "orlg_gn_modulation_windows", "orlg_get_running_services_se")


# ---------------------------------------------------------------------------------------- the entry points and their unit
def test_prototypes_exports_and_abi():
    import optical_rl_gym_amd as orlg
    header = open(os.path.join(ROOT, "include", "orlg.h")).read()
    declared = set(re.findall(r"\b(orlg_[a-z_0-9]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.PROTOTYPES and name in _lib.EXPORTED_SYMBOLS
    assert "#define ORLG_ABI_VERSION 3" in header
    assert orlg.ADAPTIVE_POLICIES is _lib.ADAPTIVE_POLICIES == ("sp_ff_am", "sap_ff_am", "path_am_external", "external_am")
    assert not set(_lib.ADAPTIVE_POLICIES) & (set(_lib.POLICIES) | set(_lib.ASSIGN_POLICIES) | set(_lib.CUT_POLICIES) |
                                              set(_lib.WINDOW_POLICIES) | set(_lib.MAX_MARGIN_POLICIES))
    for name, value in _lib.ADAPTIVE_POLICY_IDS.items():
        c_name = {"sp_ff_am": "ORLG_AM_SP_FF", "sap_ff_am": "ORLG_AM_SAP_FF", "path_am_external": "ORLG_AM_PATH_EXTERNAL",
                  "external_am": "ORLG_AM_EXTERNAL"}[name]
        assert re.search(r"\b%s = %d\b" % (c_name, value), header), name
    L = _lib.load()   # (a fresh library: the loader rebuilds a stale one)
    assert L.orlg_abi_version() == 3
    assert L.orlg_set_gn_modulation(None, 1) == -1 and b"null handle" in L.orlg_last_error()
    assert L.orlg_step_modulation(None, 201, 1, None, 0, None, None, None) == -1
    assert L.orlg_gn_modulation_windows(None, None, None, None, None) == -1
    assert L.orlg_get_running_services_se(None, None, None, None, None, None, None, None, None) == -1
    # the existing step entries accept no new policy value
    out = (C.c_int32 * 2)()
    for policy in (10, 11, 12, 13, 200, 201, 202, 203):
        assert L.orlg_debug_step_call((C.c_int32 * 7)(0, policy, 0, 0, 1, 1, 0), 7, out) == -1 and b"unknown policy" in L.orlg_last_error()


def test_the_kernels_are_a_unit_of_their_own():
    from optical_rl_gym_amd import build
    units = build.units()
    mine = [(n, s, x) for n, s, x in units if s == "orlg_inst_gnam.hip"]
    assert [n for n, _, _ in mine] == [f"orlg_inst_gnam_w{w}" for w in sorted(build.WAVE_W, reverse=True)]
    assert all(x == [f"-DORLG_INST_W={n.rsplit('w', 1)[1]}"] for n, _, x in mine)
    assert len({n for n, _, _ in units}) == len(units)
    for other in ("orlg_inst_wave.hip", "orlg_inst_gnrules.hip", "orlg_inst_gnprotect.hip", "orlg_inst_gnadmit.hip", "orlg_inst_gnslots.hip",
                  "orlg_inst_gnmm.hip", "orlg_inst_group.hip"):
        text = open(os.path.join(build.CSRC, other)).read()
        assert "am_kernel" not in text and "GN_AM" not in text and "modulation" not in text, other
    for new in ("orlg_qdesc.h", "orlg_rmsa_gn_am.h", "orlg_gn_modulation_kernels.hip", "orlg_inst_gnam.hip"):
        assert "asm" not in open(os.path.join(build.CSRC, new)).read(), new   # no inline assembly
    variants = open(os.path.join(build.CSRC, "orlg_variants.h")).read()
    assert "ORLG_WAVE_GN_AM_KEYS(X) X(1) X(2) X(0)" in variants
    # ... and orlg_pick(W, OrlgAmKey) returns, per key, the kernel of that name with the parameters (OrlgParams, OrlgAmArgs), the one
    # the unit's own lookup returns (tests/variant_names.cpp); the list ends with <W,0>
    from host_programs import variant_names
    run = variant_names()
    assert run.counts["ORLG_WAVE_GN_AM_KEYS"] == 3 * len(build.WAVE_W)
    assert any(line.startswith("W=5 ") and line.endswith(" orlg_rmsa_am_kernel<5,0>") for line in run.lines)
    assert variants.index("ORLG_WAVE_GN_AM_KEYS") > variants.index("ORLG_WAVE_GN_MM_KEYS")   # behind the existing lists
    # the level-aware decode is written once: its readers name the header's functions, none masks a descriptor's path field itself
    for user in ("orlg_rmsa_gn_am.h", "orlg_gn_modulation_kernels.hip"):
        text = open(os.path.join(build.CSRC, user)).read()
        assert "0x7ffu" not in text and "0x3fff" not in text and ">> 11" not in text, user
    assert "orlg_qdesc_gid" in open(os.path.join(build.CSRC, "orlg_rmsa_gn_am.h")).read()
    assert "orlg_qdesc_gid" in open(os.path.join(build.CSRC, "orlg_gn_audit_kernels.hip")).read()
    assert "orlg_qdesc_gid" in open(os.path.join(build.CSRC, "orlg_rmsa_gn_audit.h")).read()


def test_the_descriptor_keeps_its_level():
    """orlg_qdesc.h restated: 11 bits of path record, 3 of level, 10 of slot, 8 of rate; level 0 reads as the plain layout"""
    make = lambda gid, level, slot, rate: gid | level << 11 | slot << 14 | rate << 24
    for gid, level, slot, rate in ((0, 0, 0, 0), (2047, 6, 1023, 255), (454, 3, 319, 20), (454, 0, 319, 20)):
        d = make(gid, level, slot, rate)
        assert d < 1 << 32
        assert (d & 0x7ff, (d >> 11) & 7, (d >> 14) & 0x3ff, d >> 24) == (gid, level, slot, rate)
        if level == 0:
            assert d & 0x3fff == gid   # a state without levels reads the same on every handle
        else:
            assert d & 0x3fff >= 2048   # ... and a level names no path record of a handle that may be adaptive


# ---------------------------------------------------------------------------------------- the gate's mode, before the library is loaded
def test_gate_parameters_and_their_refusals(nsfnet):
    plain = rmsa_gn_gate_parameters(nsfnet)
    assert "modulation" not in plain and len(plain) == 8
    g = rmsa_gn_gate_parameters(nsfnet, modulation="adaptive")
    assert g["modulation"] == "adaptive" and len(g) == 9
    with pytest.raises(ValueError, match="modulation"):
        rmsa_gn_gate_parameters(nsfnet, modulation="best")
    from optical_rl_gym_amd.osnr import check_rmsa_gn_gate
    assert check_rmsa_gn_gate(g, nsfnet)["modulation"] == "adaptive" and "modulation" not in check_rmsa_gn_gate(plain, nsfnet)
    with pytest.raises(ValueError, match="modulation"):
        check_rmsa_gn_gate(dict(plain, modulation="best"), nsfnet)
    with pytest.raises(ValueError, match="protect_running"):
        check_rmsa_gn_gate(dict(g, protect_running=True), nsfnet)
    with pytest.raises(ValueError, match="7 thresholds"):
        check_rmsa_gn_gate(dict(g, thresholds_db=np.arange(7.0)), nsfnet)
    with pytest.raises(ValueError, match="group"):
        check_rmsa_gn_gate(g, nsfnet, "group")
    big = am.expanded(nsfnet, 6)   # 2730 path records
    assert big.num_paths >= _lib.MAX_ADAPTIVE_PATHS
    with pytest.raises(ValueError, match="path records"):
        check_rmsa_gn_gate(rmsa_gn_gate_parameters(big, modulation="adaptive"), big)
    for cls in (BatchedRMSAEnv, BatchedDeepRMSAEnv):   # refused by the constructor before the library is touched
        with pytest.raises(ValueError, match="protect_running"):
            cls(nsfnet, 2, gn_gate=dict(g, protect_running=True), seed=1)
        with pytest.raises(ValueError, match="group"):
            cls(nsfnet, 2, gn_gate=g, step_kernel="group", seed=1)


class _NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although the arguments are wrong")


NB, K, S, W = 3, 5, 320, 5


def _shell(gn_gate, cls=BatchedRMSAEnv):
    env = cls.__new__(cls)
    env.L, env.h = _NoLibrary(), None
    env.batch_size, env.k_paths, env.j, env.reject_action, env.words_per_link, env.num_spectrum_resources = NB, K, 1, 0, W, S
    env.gn_gate = gn_gate
    return env


@pytest.mark.parametrize("cls", [BatchedRMSAEnv, BatchedDeepRMSAEnv])
def test_refused_before_the_library_is_called(cls, nsfnet):
    plain, adaptive = rmsa_gn_gate_parameters(nsfnet), rmsa_gn_gate_parameters(nsfnet, modulation="adaptive")
    path_acts, ext_acts = np.zeros(NB, np.int32), np.zeros((NB, 3), np.int32)
    for name in _lib.ADAPTIVE_POLICIES:
        acts = ext_acts if name == "external_am" else path_acts if name == "path_am_external" else None
        for gate in (None, plain):   # the names need the mode
            with pytest.raises(ValueError, match="adaptive"):
                _shell(gate, cls).run(name, 1, actions=acts)
        env = _shell(adaptive, cls)
        assert env.gn_adaptive and env.modulation_levels == 6 and not env.gn_protect
        with pytest.raises(ValueError, match="gn_rule"):
            env.run(name, 1, actions=acts, gn_rule="check")
        with pytest.raises(ValueError, match="block_cause"):
            env.run(name, 1, actions=acts, outputs=("block_cause",))
        with pytest.raises(ValueError, match="block_cause"):
            env.run(name, 1, actions=acts, cause_counts=True)
        with pytest.raises(ValueError, match="gn_window_margin_db"):
            env.run(name, 1, actions=acts, outputs=("gn_window_margin_db",))
        with pytest.raises(ValueError, match="n_steps"):
            env.run(name, 0, actions=acts)
    env = _shell(adaptive, cls)
    with pytest.raises(ValueError, match="actions"):
        env.run("external_am", 1)
    with pytest.raises(ValueError, match="n_steps must be 1"):
        env.run("path_am_external", 2, actions=path_acts)
    with pytest.raises(ValueError):
        env.run("external_am", 1, actions=np.zeros((NB, 2), np.int32))   # (path, slot) without the level
    with pytest.raises(TypeError):
        env.run("external_am", 1, actions=np.zeros((NB, 3)))
    # what an adaptive handle does not serve yet
    for name in _lib.MAX_MARGIN_POLICIES:
        with pytest.raises(ValueError, match="modulation='adaptive'"):
            env.run(name, 1, actions=path_acts if name.endswith("external") else None)
    with pytest.raises(ValueError, match="modulation='adaptive'"):
        env.run("sap_lf", 1, gn_rule="check")
    with pytest.raises(ValueError, match="modulation='adaptive'"):
        env.run("sap_ff", 1, outputs=("block_cause",))
    with pytest.raises(ValueError, match="modulation='adaptive'"):
        env.run("sap_ff", 1, cause_counts=True)
    for kind in BatchedRMSAEnv.GN_MASK_KINDS:
        with pytest.raises(ValueError, match="modulation='adaptive'"):
            env.action_masks(kind)
    for call in (lambda: env.path_rule_windows("first"), lambda: env.admission_masks("path_ff"), lambda: env.admission_windows("first"),
                 env.admission_slot_masks, env.max_margin_windows):
        with pytest.raises(ValueError, match="modulation='adaptive'"):
            call()
    # gn_se and the query belong to the mode
    with pytest.raises(ValueError, match="ADAPTIVE_POLICIES"):
        env.run("sap_ff", 1, outputs=("gn_se",))
    for gate in (None, plain):
        with pytest.raises(ValueError, match="adaptive"):
            _shell(gate, cls).modulation_windows()
    with pytest.raises(ValueError):
        env.modulation_windows(slot_out=np.zeros((NB, K, 5), np.int16))


def test_the_views_know_the_level():
    from optical_rl_gym_amd import adaptive_modulation_heuristic
    with pytest.raises(ValueError, match="route"):
        adaptive_modulation_heuristic("llp")
    assert adaptive_modulation_heuristic("sap").__name__ == "sap_adaptive_modulation"


# ---------------------------------------------------------------------------------------- what the GPU cases exercise, from the reference alone
@pytest.mark.parametrize("case", list(am.CASES))
def test_the_case_exercises_the_levels(case):
    fig = [am.run_case(case, i)[2] for i in range(am.B)]
    accepted, other = sum(f["accepted"] for f in fig), sum(f["other_level"] for f in fig)
    closest = min(f["closest"] for f in fig)
    print(case, "accepted", accepted, "at another level", other, "refused after", max(f["refused_after"] for f in fig), "levels; most running",
          max(f["max_running"] for f in fig), "closest", closest, "mean checks", np.mean([f["mean_checks"] for f in fig]), "max checks",
          max(f["max_checks"] for f in fig))
    assert other >= 0.05 * accepted > 0                      # at least 5 % of the accepted services take a level other than their path's
    assert max(f["refused_after"] for f in fig) >= 2          # a gate refusal after several levels
    assert closest > 1e-6                                     # no compared GSNR within 1e-6 dB of its threshold
    assert min(f["min_admitted_margin"] for f in fig) >= 0
    topo = load_topology(am.CASES[case]["topology"])
    assert max(f["max_checks"] for f in fig) <= topo.k_paths * 6
    if "l150" in case and "nsfnet" in case:
        assert max(f["max_running"] for f in fig) > 64        # more than one chunk of interferers
    if "ring34" in case:
        assert max(f["link_ranges"] for f in fig) == 4        # link masks of four words


def test_thresholds_nobody_misses_give_the_ungated_oracle(nsfnet):
    """With all thresholds at -100 dB the adaptive reference is sap_ff on a topology whose every path has spectral efficiency M"""
    kw = ref.case_kwargs("nsfnet_s320_l150_sapff")
    gate = am.case_gate(nsfnet, 6.0, thresholds_db=[-100.0] * 6)
    with device_log_in_oracle():
        ao = am.AdaptiveOracle(nsfnet, kw, gate, seed=11)
        got = ao.run_route("sap", 300)
        ao_final = ao.final()
        ao.close()
        o = oracle_env_from_kwargs(am.expanded(nsfnet, 6, only_se=6), kw, seed=11)
        want = o.run("sap_ff", 300, reset_on_done=True)
        for f in ("act_path", "act_slot", "accepted"):
            assert np.array_equal(got[f], want[f]), f
        assert (got["gn_se"][got["accepted"] == 1] == 6).all()
        assert np.array_equal(ao_final["available_slots"], o.available_slots()) and ao_final["counters"] == o.counters()
        assert ao_final["current_time"] == o.current_time()
        o.close()


# ---------------------------------------------------------------------------------------- what the shapes of test_gpu_gn_modulation_shapes.py reach
STATS_CASES = ("nsfnet_s128_l25_6dbm", "nsfnet_s320_l150_0dbm")


def _figures(shape, n_envs, **kw):
    fig = [am.run_shape(shape, i, **kw)[2] for i in range(n_envs)]
    print(shape, "accepted", [f["accepted"] for f in fig], "at another level", [f["other_level"] for f in fig], "refusals",
          [f["rejects"] for f in fig], "peak", [f["max_running"] for f in fig], "closest", min(f["closest"] for f in fig), "max checks",
          max(f["max_checks"] for f in fig), "released", [f["released"] for f in fig])
    assert min(f["closest"] for f in fig) > 1e-6   # no compared GSNR within 1e-6 dB of its threshold
    return fig


@pytest.mark.parametrize("case", STATS_CASES + ("mixed",))
def test_the_statistics_cases_release_services_at_another_level(case):
    """sum_sh, the link statistics and the compactness of a release take the slots of the LEVEL: in every environment a service whose
    level is not its path's own is released before the last step, so a release that took the path's own would show"""
    for i in range(am.B):
        fig = (am.run_mixed(i) if case == "mixed" else am.run_case(case, i))[2]
        assert fig["released_other"] >= 1 and fig["closest"] > 1e-6, (case, i, fig)


def test_the_mixed_plan_interleaves_releases_with_and_without_a_level():
    for i in range(am.B):
        tr, _, fig, services = am.run_mixed(i)
        assert 1 <= fig["released_other"] < fig["released"], (i, fig)


@pytest.mark.parametrize("M", [3, 1])
def test_fewer_levels(M, nsfnet):
    topo = am.clipped(nsfnet, M)
    assert int(topo.path_se.max()) == M and np.array_equal(topo.path_se, np.minimum(nsfnet.path_se, M))
    assert np.array_equal(topo.path_links, nsfnet.path_links) and np.array_equal(topo.path_hops, nsfnet.path_hops)
    gate = am.shape_gate(topo, 6.0, M)
    assert len(gate["thresholds_db"]) == M and np.array_equal(gate["thresholds_db"], am.case_gate(nsfnet, 6.0)["thresholds_db"][:M])
    from optical_rl_gym_amd.osnr import check_rmsa_gn_gate
    assert len(check_rmsa_gn_gate(gate, topo)["thresholds_db"]) == M
    if M == 3:
        # the unclipped topology is refused; the message names the highest spectral efficiency of a path (NSFNET's paths end at 5)
        assert int(nsfnet.path_se.max()) == 5
        with pytest.raises(ValueError, match="a path has spectral efficiency 5, thresholds_db has 3 entries"):
            check_rmsa_gn_gate(am.shape_gate(nsfnet, 6.0, M), nsfnet)
    hot, cold = _figures("m%d_6dbm" % M, am.B), _figures("m%d_0dbm" % M, am.B)
    f0 = hot[0]
    assert (f0["accepted"], f0["rejects"]) == ((96, 34) if M == 3 else (69, 4))   # the figures of seed 21
    if M == 3:
        assert (f0["other_level"], f0["max_checks"]) == (11, 12)
        assert all(f["other_level"] >= 1 and f["refused_after"] >= 2 for f in hot)
    else:
        assert all(f["other_level"] == 0 and f["max_checks"] <= nsfnet.k_paths for f in hot)   # the walk has one level
    assert all(f["rejects"] >= 1 and f["accepted"] >= 1 for f in hot)
    assert all(f["rejects"] == 0 for f in cold)   # 0 dBm: the all-admitted arm


def test_three_chunks_of_interferers():
    c = am.SHAPES["chunks3"]
    fig = _figures("chunks3", c["B"])
    assert all(f["max_running"] > 128 for f in fig)   # a third chunk of 64 in every environment
    assert all(f["rejects"] >= 1 and f["max_checks"] >= 2 for f in fig)
    f0 = fig[0]
    assert (f0["max_running"], f0["rejects"], f0["max_checks"]) == (147, 25, 10) and abs(f0["closest"] - 2.7e-4) < 1e-5   # seed 11
    for i, f in enumerate(fig):   # the step of the peak has more than 128 running: where the query is compared
        assert f["peak_step"] < c["n"] and f["max_running"] > 128


def test_the_ring_laps():
    c = am.SHAPES["lap"]
    fig = _figures("lap", am.B)
    peak = max(f["max_running"] for f in fig)
    Q = am.ring_capacity(peak, c["queue_margin"])
    assert (peak, Q) == (23, 64) and fig[0]["max_running"] == 19
    assert all(f["released"] >= 2 * Q for f in fig)   # the head passes Q twice in every environment
    assert all(f["max_running"] < Q for f in fig)


@pytest.mark.parametrize("shape", list(am.MANY))
def test_the_many_path_shapes_reach_the_high_paths(shape, tmp_path):
    from gpu_support import MANY_PATHS, many_paths_topology
    topo = many_paths_topology(shape, tmp_path)
    c = MANY_PATHS[shape]
    assert topo.k_paths == c["k"] > 8 and topo.num_paths < _lib.MAX_ADAPTIVE_PATHS
    assert topo.num_paths == {"g3x3_k9_s64": 324, "g4x4_k16_s200": 1920, "g3x4_k10_s384": 660}[shape]
    fig = _figures(shape, am.B, topo=topo)
    high = 0
    for i in range(am.B):
        tr = am.run_shape(shape, i, topo=topo)[0]
        acc = tr["accepted"].astype(bool)
        high += int((tr["act_path"][acc] >= 8).sum())
    print(shape, "accepted on paths >= 8:", high)
    assert high >= 10
    assert sum(f["other_level"] for f in fig) >= 1 and sum(f["rejects"] for f in fig) >= 1


def test_too_many_path_records_are_refused(tmp_path):
    from gpu_support import many_paths_topology
    from optical_rl_gym_amd.osnr import check_rmsa_gn_gate
    topo = many_paths_topology(am.MANY_REFUSED, tmp_path)
    assert topo.num_paths == 2520
    with pytest.raises(ValueError, match="path records"):
        check_rmsa_gn_gate(am.case_gate(topo, 6.0), topo)


def test_the_query_cases_at_the_other_word_counts():
    """ring34 (link masks of four words), one and eight words per link: after the warm-up the query sees levels with and without a
    window, admitted and refused"""
    for case in ("ring34_s100_l60_6dbm", "nsfnet_s64_l12_6dbm", "nsfnet_s512_l100_6dbm"):
        for i in (0, 1):
            fig = am.run_case(case, i, n_steps=110)[2]
            assert fig["rejects"] >= 1 and fig["other_level"] >= 1 and fig["closest"] > 1e-6, (case, i, fig)


def test_the_sweep_and_the_deeprmsa_handle():
    c = am.SWEEP
    for i in range(len(c["loads"]) * c["seeds_per_load"]):
        fig = am.run_sweep(i)[2]
        assert fig["closest"] > 1e-6 and fig["other_level"] >= 1 and fig["rejects"] >= 1, (i, fig)
    low, high = (sum(am.run_sweep(g * c["seeds_per_load"] + r)[2]["max_running"] for r in range(c["seeds_per_load"])) for g in (0, 1))
    assert high > low   # the environments do run their own loads
    for i in range(am.DEEP["B"]):
        tr, own, _, fig, _ = am.run_deep(i)
        assert fig["closest"] > 1e-6 and fig["other_level"] >= 1 and fig["rejects"] >= 1, (i, fig)
        assert set(np.unique(tr["reward"])) == {-1.0, 1.0} and np.array_equal(tr["reward"], np.where(tr["accepted"] == 1, 1.0, -1.0))
        assert own["accepted"].any() and (own["gn_se"] == 0).all()
