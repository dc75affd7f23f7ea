"""Assignment rules behind the GN-model admission check (``include/orlg.h`` ``orlg_step_rule_gn`` / ``orlg_gn_path_windows``,
DESIGN 2.26), what needs no GPU: the refusals of ``run(..., gn_rule=)`` and ``path_rule_windows`` before the library is called,
with everything that existed before unchanged; the entry points, their prototypes and constants; the new key lists and the
objects they live in; and, from the oracle alone, the conditions the comparisons of ``test_gpu_gn_rules.py`` rest on -- for every
(case, route, rule, mode) it uses, over the environments it uses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gn_rules_reference as gref
from conftest import ROOT
from optical_rl_gym_amd import BatchedDeepRMSAEnv, BatchedRMSAEnv, _lib, assignment_heuristic, min_cut_heuristic

NEW = {"orlg_step_rule_gn": 9, "orlg_gn_path_windows": 5}
GATE = {"any": 1}


# ---------------------------------------------------------------------------------------- refusals before the library is called
class _NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although the arguments are wrong")


def _rmsa_shell(B=3, k=5, gn_gate=None, cls=BatchedRMSAEnv):
    env = cls.__new__(cls)
    env.L, env.h = _NoLibrary(), None
    env.batch_size, env.k_paths, env.gn_gate = B, k, gn_gate
    return env


RULE_NAMES = sorted(set(_lib.ASSIGN_POLICIES) | set(_lib.CUT_POLICIES))


@pytest.mark.parametrize("cls", [BatchedRMSAEnv, BatchedDeepRMSAEnv])
@pytest.mark.parametrize("mode", gref.MODES)
def test_an_ungated_handle_is_refused(mode, cls):
    for name in RULE_NAMES:
        with pytest.raises(ValueError, match="gn_gate"):
            _rmsa_shell(cls=cls).run(name, 10, actions=np.zeros(3, np.int32), gn_rule=mode)


@pytest.mark.parametrize("mode", gref.MODES)
@pytest.mark.parametrize("name", sorted(_lib.POLICIES) + sorted(_lib.WINDOW_POLICIES))
def test_first_fit_deeprmsa_and_window_names_are_refused(name, mode):
    """... on a gated and on an ungated shell: the name is looked at first"""
    for gate in (GATE, None):
        with pytest.raises(ValueError, match="gn_rule"):
            _rmsa_shell(gn_gate=gate).run(name, 10, actions=np.zeros(3, np.int32), gn_rule=mode)
    if name in _lib.WINDOW_POLICIES:
        with pytest.raises(ValueError, match="most-used rule and the any_"):
            _rmsa_shell(gn_gate=GATE).run(name, 10, actions=np.zeros(3, np.int32), gn_rule=mode)


@pytest.mark.parametrize("name", [n for n in RULE_NAMES if not n.startswith("sap_")])
def test_next_path_needs_a_sap_name(name):
    with pytest.raises(ValueError, match="next_path"):
        _rmsa_shell(gn_gate=GATE).run(name, 1, actions=np.zeros(3, np.int32), gn_rule="next_path")


@pytest.mark.parametrize("mode", ["", "Check", "next", 0, 1, True, "retry"])
def test_unknown_modes(mode):
    with pytest.raises(ValueError, match="gn_rule"):
        _rmsa_shell(gn_gate=GATE).run("sap_bf", 10, gn_rule=mode)


@pytest.mark.parametrize("name", RULE_NAMES + sorted(_lib.WINDOW_POLICIES))
def test_without_the_keyword_a_gated_handle_refuses_as_before(name):
    for kw in ({}, {"gn_rule": None}):
        with pytest.raises(ValueError, match="does not run on a handle with a GN-model admission check"):
            _rmsa_shell(gn_gate=GATE).run(name, 10, actions=np.zeros(3, np.int32), **kw)


@pytest.mark.parametrize("name", ["sap_mc_gn", "sap_mu_gn", "sap_ff_gn_lf", "sap_bf_gn", "min_cut_gn", "sap_lf_next_path"])
def test_the_feature_has_no_policy_names(name):
    for gate in (GATE, None):
        with pytest.raises(KeyError):
            _rmsa_shell(gn_gate=gate).run(name, 10)
    assert name not in _lib.POLICIES and name not in _lib.ASSIGN_POLICIES and name not in _lib.CUT_POLICIES and name not in _lib.WINDOW_POLICIES


def test_the_arguments_behind_the_keyword_are_checked_as_before():
    shell = _rmsa_shell(gn_gate=GATE)
    with pytest.raises(ValueError, match="actions"):
        shell.run("path_bf_external", 1, gn_rule="check")
    with pytest.raises(ValueError, match="actions"):
        shell.run("path_mc_external", 1, actions=np.zeros((3, 2), np.int32), gn_rule="check")
    with pytest.raises(ValueError, match="cause_counts"):
        shell.run("sap_mc", 10, cause_counts=np.zeros((3, 7), np.int32), gn_rule="next_path")


def test_path_rule_windows_arguments():
    for rule in ("", "most_used", "ff", "mc", 3, None):
        with pytest.raises(ValueError, match="rule"):
            _rmsa_shell(gn_gate=GATE).path_rule_windows(rule)
    for rule in _lib.GN_PATH_WINDOW_RULES:
        with pytest.raises(ValueError, match="gn_gate"):
            _rmsa_shell().path_rule_windows(rule)
    shell = _rmsa_shell(gn_gate=GATE)
    with pytest.raises(ValueError, match="slots_out"):
        shell.path_rule_windows("best", slots_out=np.zeros((3, 4), np.int16))
    with pytest.raises((ValueError, TypeError), match="gsnr_out"):
        shell.path_rule_windows("best", gsnr_out=np.zeros((3, 5), np.float32))
    with pytest.raises((ValueError, TypeError), match="admitted_out"):
        shell.path_rule_windows("best", admitted_out=np.zeros((3, 5), np.int8))


def test_heuristic_arguments():
    for gn in ("", "next", True, 1):
        with pytest.raises(ValueError, match="gn"):
            assignment_heuristic("sap", "best", gn=gn)
        with pytest.raises(ValueError, match="gn"):
            min_cut_heuristic("sap", gn=gn)
    for route in ("sp", "llp"):
        with pytest.raises(ValueError, match="next_path"):
            assignment_heuristic(route, "best", gn="next_path")
    for route in ("sp", "llp", "min_cut"):
        with pytest.raises(ValueError, match="next_path"):
            min_cut_heuristic(route, gn="next_path")
    for gn in ("check", "next_path"):
        with pytest.raises(ValueError, match="first"):
            assignment_heuristic("sap", "first", gn=gn)
    assert assignment_heuristic("sap", "best").__name__ == assignment_heuristic("sap", "best", gn="next_path").__name__ == "sap_best"
    assert min_cut_heuristic("min_cut", gn="check").__name__ == "min_cut_min_cut"


# ---------------------------------------------------------------------------------------- ABI, prototypes, constants, tables
def test_new_symbols_in_a_fresh_library():
    assert set(NEW) <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.load()
    assert L.orlg_abi_version() == 3
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW) <= names
    header = open(os.path.join(ROOT, "include", "orlg.h")).read()
    assert "#define ORLG_ABI_VERSION 3" in header
    for s, nargs in NEW.items():
        assert "int " + s + "(orlg_env *env" in header and hasattr(L, s) and len(getattr(L, s).argtypes) == nargs
    assert "#define ORLG_RULE_FEWEST_CUTS %d" % _lib.RULE_FEWEST_CUTS in header
    assert "#define ORLG_GN_MODE_CHECK %d" % _lib.GN_RULE_MODES["check"] in header
    assert "#define ORLG_GN_MODE_NEXT_PATH %d" % _lib.GN_RULE_MODES["next_path"] in header
    assert header.count("DESIGN 2.26") >= 1
    # the public rules and policies are what they were; the device's own values stay out of the header
    assert "ORLG_NUM_ASSIGN_RULES = 5" in header and "ORLG_ASSIGN_MIN_CUT" not in header and "ORLG_POLICY_SAP_GN" not in header
    assert _lib.RULE_FEWEST_CUTS not in (_lib.RULE_MOST_USED, _lib.ROUTE_BEST_WINDOW, _lib.ROUTE_FEWEST_CUTS)
    assert _lib.RULE_FEWEST_CUTS >= 100 and _lib.RULE_FEWEST_CUTS not in _lib.POLICIES.values()


def test_the_old_tables_are_what_they_were():
    assert BatchedRMSAEnv.MASK_KINDS == ("deeprmsa", "path_ff", "slots", "path_ff_gn", "deeprmsa_gn")
    assert BatchedRMSAEnv.GN_MASK_KINDS == ("path_ff_gn", "deeprmsa_gn")
    assert len(_lib.ASSIGN_POLICIES) == 16 and len(_lib.CUT_POLICIES) == 5 and len(_lib.WINDOW_POLICIES) == 9
    assert _lib.ASSIGN_RULES == ("first", "first_full", "last", "best", "exact")
    assert tuple(_lib.GN_PATH_WINDOW_RULES) == gref.RULES
    assert [_lib.GN_PATH_WINDOW_RULES[r] for r in _lib.ASSIGN_RULES] == list(range(5))
    assert _lib.GN_PATH_WINDOW_RULES["min_cut"] == _lib.RULE_FEWEST_CUTS
    for route in ("sp", "sap", "llp", "path"):
        for rule in gref.RULES[1:]:
            name = gref.policy_name(route, rule)
            assert name in _lib.ASSIGN_POLICIES or name in _lib.CUT_POLICIES, name
    assert gref.policy_name("min_cut", "min_cut") == "min_cut"


def test_a_null_handle_answers_first():
    L = _lib.load()
    for route, rule, mode in ((1, 3, 0), (1, 3, 1), (99, 3, 0), (1, 99, 0), (1, 3, 7), (_lib.ROUTE_FEWEST_CUTS, 1, 0)):
        assert L.orlg_step_rule_gn(None, route, rule, mode, 10, None, 1, None, None) == -1 and b"null handle" in L.orlg_last_error()
    out = np.zeros(8, np.int16)
    for rule in (0, 3, _lib.RULE_FEWEST_CUTS, 99):
        assert L.orlg_gn_path_windows(None, rule, out.ctypes.data_as(C.c_void_p), None, None) == -1 and b"null handle" in L.orlg_last_error()


# ---------------------------------------------------------------------------------------- the key lists and their objects
def test_gn_rule_key_lists_resolve_to_their_kernels():
    from host_programs import variant_names
    from optical_rl_gym_amd import build
    counts = variant_names().counts
    # per word count: 3 statistics levels x {no cause, CAUSE} x {a rule, the fewest-cuts window}
    assert (counts["ORLG_WAVE_GN_ASSIGN_KEYS"], counts["ORLG_WAVE_GN_CUT_KEYS"]) == (6 * len(build.WAVE_W), 6 * len(build.WAVE_W))


def test_the_new_instantiations_are_objects_of_their_own():
    from optical_rl_gym_amd import build
    build.build(verbose=False)
    names = [n for n, _, _ in build.units()]
    new = [n for n in names if n.startswith("orlg_inst_gnrules_w")]
    assert new == [f"orlg_inst_gnrules_w{w}" for w in sorted(build.WAVE_W, reverse=True)]
    assert len([n for n in names if n.startswith("orlg_inst_wave_w")]) == 7 and len(set(names)) == len(names)
    for n in new:
        deps = {os.path.basename(d) for d in build._deps(os.path.join(build.OBJ, n + ".d"))}
        assert {"orlg_kernels.hip", "orlg_gn_rule_kernels.hip", "orlg_inst_gnrules.hip"} <= deps, n
        assert not [d for d in deps if d.startswith("orlg_group_") or d.startswith("orlg_phy_")], n
    for w in build.WAVE_W:   # ... and the wave objects do not parse the new query
        deps = {os.path.basename(d) for d in build._deps(os.path.join(build.OBJ, f"orlg_inst_wave_w{w}.d"))}
        assert "orlg_gn_rule_kernels.hip" not in deps and "orlg_inst_gnrules.hip" not in deps


# ---------------------------------------------------------------------------------------- what the GPU comparisons rest on
@pytest.mark.parametrize("name", sorted(gref.GPU_CASES))
def test_the_oracle_meets_the_conditions_of_the_gpu_comparisons(name):
    """From the oracle alone, summed over the environments test_gpu_gn_rules.py uses: no candidate within 1e-5 dB of its
    threshold (the comparison is rtol 1e-9 on about 20 dB: a margin of about 500); >= 10 steps refused by the gate; under
    next_path >= 5 steps that take a later path; >= 10 steps with a window other than the chosen path's first fit for best, last
    and min_cut, >= 1 for first_full and exact; both values of every admitted column."""
    c = gref.GPU_CASES[name]
    fig = gref.summed(gref.run_batch(gref.gpu_case(name), c["route"], c["rule"], c["mode"], n_steps=c["n"], gate_items=c["gate"]))
    print(name, fig)
    assert fig["closest"] >= 1e-5, fig
    assert fig["refused"] >= 10, fig
    if c["mode"] == "next_path":
        assert fig["later"] >= 5, fig
    assert fig["other_window"] >= (10 if c["rule"] in ("best", "last", "min_cut") else 1), fig
    assert fig["admitted_values"] == (0, 1), fig


@pytest.mark.parametrize("name,rule", gref.PATH_CASES)
def test_the_oracle_meets_the_conditions_of_the_path_comparisons(name, rule):
    """The agent's path under mode check: the margin, gate refusals and provisions; out-of-range paths occur on both sides."""
    fig = gref.summed(gref.run_path_case(name, rule))
    print(name, rule, fig)
    assert fig["closest"] >= 1e-5 and fig["refused"] >= 10 and fig["provisions"] >= 10, fig
    k = 5 if not name.startswith("ring") else 3
    assert {-1, k, k + 1} <= set(gref.path_actions(k).ravel().tolist())


def test_the_gpu_cases_cover_every_rule_mode_and_word_count():
    cases = gref.GPU_CASES.values()
    assert {c["rule"] for c in cases} == set(gref.RULES[1:]) and {c["mode"] for c in cases} == set(gref.MODES)
    assert {c["W"] for c in cases} == {1, 2, 5, 8}
    assert {c["route"] for c in cases} >= {"sp", "sap", "llp", "min_cut"}
