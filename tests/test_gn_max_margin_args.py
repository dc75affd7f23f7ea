"""Max-margin assignment inside the step (``include/orlg.h`` ``orlg_step_max_margin``) without a GPU: the symbol, the
unit and the names of its kernels, every refusal before the library is called, the proposal rules on hand-made rows, and -- from the
reference alone, every batch of ``test_gpu_gn_max_margin.py`` and every shape of ``test_gpu_gn_max_margin_shapes.py`` stepped by its own
max-margin choices -- what those batches and shapes exercise, so that no comparison on the device passes with its target idle."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gn_max_margin_reference as mm
import gn_slots_reference as sl
from conftest import ROOT
from optical_rl_gym_amd import BatchedDeepRMSAEnv, BatchedRMSAEnv, _lib

NEW = ("orlg_step_max_margin", "orlg_step_max_margin_protect")


# ---------------------------------------------------------------------------------------- the entry point and its unit
def test_prototype_export_and_abi():
    import optical_rl_gym_amd as orlg
    header = open(os.path.join(ROOT, "include", "orlg.h")).read()
    declared = set(re.findall(r"\b(orlg_[a-z_0-9]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.PROTOTYPES and name in _lib.EXPORTED_SYMBOLS
    assert _lib.PROTOTYPES[NEW[0]][1][-1] == C.c_void_p and len(_lib.PROTOTYPES[NEW[0]][1]) == 8 and len(_lib.PROTOTYPES[NEW[1]][1]) == 9
    assert "#define ORLG_ABI_VERSION 3" in header
    assert _lib.MAX_MARGIN_POLICIES == ("sap_mm", "any_mm", "path_mm_external") and orlg.MAX_MARGIN_POLICIES is _lib.MAX_MARGIN_POLICIES
    assert not set(_lib.MAX_MARGIN_POLICIES) & (set(_lib.POLICIES) | set(_lib.ASSIGN_POLICIES) | set(_lib.CUT_POLICIES) | set(_lib.WINDOW_POLICIES))
    L = _lib.load()   # (a fresh library: the loader rebuilds a stale one)
    assert L.orlg_abi_version() == 3
    assert L.orlg_step_max_margin(None, 1, 1, None, 0, None, None, None) == -1 and b"null handle" in L.orlg_last_error()
    assert L.orlg_step_max_margin_protect(None, 1, 1, None, 0, None, None, None, None) == -1


def test_the_kernels_are_a_unit_of_their_own():
    from optical_rl_gym_amd import build
    units = build.units()
    mine = [(n, s, x) for n, s, x in units if s == "orlg_inst_gnmm.hip"]
    assert [n for n, _, _ in mine] == [f"orlg_inst_gnmm_w{w}" for w in sorted(build.WAVE_W, reverse=True)]
    assert all(x == [f"-DORLG_INST_W={n.rsplit('w', 1)[1]}"] for n, _, x in mine)
    assert len({n for n, _, _ in units}) == len(units) and "-ffp-contract=off" in build.FLAGS
    for other in ("orlg_inst_wave.hip", "orlg_inst_gnrules.hip", "orlg_inst_gnprotect.hip", "orlg_inst_gnadmit.hip", "orlg_inst_gnslots.hip",
                  "orlg_inst_group.hip", "orlg_gn_audit_kernels.hip"):
        text = open(os.path.join(build.CSRC, other)).read()
        assert "mm_kernel" not in text and "GN_MM" not in text, other
    for new in ("orlg_gn_max_margin.h", "orlg_gn_slots_path.h", "orlg_inst_gnmm.hip"):
        assert "asm" not in open(os.path.join(build.CSRC, new)).read(), new   # no inline assembly
    # the per-path evaluation is written once: both kernels call the header's function, neither holds its loops
    for user in ("orlg_gn_slots_kernels.hip", "orlg_gn_max_margin.h"):
        text = open(os.path.join(build.CSRC, user)).read()
        assert "gn_slots_path<W" in text and "gn_slots_finish<W>" in text and "asinh" not in text, user
    variants = open(os.path.join(build.CSRC, "orlg_variants.h")).read()
    assert "ORLG_WAVE_GN_MM_KEYS(X) X(1) X(2) X(0) X(1, true) X(2, true) X(0, true)" in variants
    # the unit exports its lookup per word count, and for no other
    exported = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    assert sorted(re.findall(r"orlg_gnmm_kernel_W(\d)9OrlgMmKey", exported)) == sorted(str(w) for w in build.WAVE_W)


def test_reported_names_are_the_kernels():
    """through tests/variant_names.cpp: orlg_pick(W, OrlgMmKey) returns, per key, the kernel of that name with the parameters
    (OrlgParams, OrlgMmArgs) -- the kernel the unit's own lookup returns -- and the list ends with <W,0,true>"""
    from host_programs import variant_names
    from optical_rl_gym_amd import build
    run = variant_names()
    assert run.counts["ORLG_WAVE_GN_MM_KEYS"] == 6 * len(build.WAVE_W)
    assert any(line.startswith("W=5 orlg_rmsa_mm_kernel<5,0,true> ") for line in run.lines)


def test_the_existing_entries_keep_their_domain():
    """No OrlgStepEntry was added and no entry accepts a new policy value: what tests/test_step_calls.py pins, asked again here."""
    L = _lib.load()
    out = (C.c_int32 * 2)()
    call = lambda *v: L.orlg_debug_step_call((C.c_int32 * 7)(*v), 7, out)
    assert call(5, 1, 0, 0, 1, 1, 0) == -1 and b"unknown step entry" in L.orlg_last_error()
    for entry in (0, 1):
        for policy in (8, 9, 10):
            for gated in (0, 1):
                assert call(entry, policy, 0, 0, 1, gated, 0) == -1 and b"unknown policy" in L.orlg_last_error(), (entry, policy)
    assert call(0, 7, 0, 0, 1, 1, 0) == 0 and tuple(out) == (7, 0)


# ---------------------------------------------------------------------------------------- refusals before the library is called
class _NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although the arguments are wrong")


B, K, S, W = 3, 5, 320, 5


def _shell(gn_gate, cls=BatchedRMSAEnv):
    env = cls.__new__(cls)
    env.L, env.h = _NoLibrary(), None
    env.batch_size, env.k_paths, env.j, env.reject_action, env.words_per_link, env.num_spectrum_resources = B, K, 1, 0, W, S
    env.gn_gate = gn_gate
    return env


@pytest.mark.parametrize("cls", [BatchedRMSAEnv, BatchedDeepRMSAEnv])
@pytest.mark.parametrize("name", _lib.MAX_MARGIN_POLICIES)
def test_refused_before_the_library_is_called(cls, name):
    actions = np.zeros(B, np.int32) if name == "path_mm_external" else None
    with pytest.raises(ValueError, match="gn_gate"):
        _shell(None, cls).run(name, 1, actions=actions)
    for gate in ({"protect_running": True}, {"any": 1}):
        env = _shell(gate, cls)
        for mode in ("check", "next_path"):
            with pytest.raises(ValueError, match="gn_rule"):
                env.run(name, 1, actions=actions, gn_rule=mode)
        with pytest.raises(ValueError, match="n_steps"):
            env.run(name, 0, actions=actions)
    env = _shell({"any": 1}, cls)
    if name == "path_mm_external":
        with pytest.raises(ValueError, match="actions"):
            env.run(name, 1)
        with pytest.raises(ValueError, match="n_steps must be 1"):
            env.run(name, 2, actions=actions)
        with pytest.raises(ValueError, match="shape"):
            env.run(name, 1, actions=np.zeros((B, 2), np.int32))
        with pytest.raises(TypeError, match="integer"):
            env.run(name, 1, actions=np.zeros(B))
    with pytest.raises(ValueError, match="shape"):
        env.run(name, 1, actions=actions, out={"gn_window_margin_db": np.zeros((2, B))})
    with pytest.raises(TypeError, match="dtype"):
        env.run(name, 1, actions=actions, out={"gn_window_margin_db": np.zeros((1, B), np.float32)})


def test_the_window_margin_is_an_output_of_these_names_only():
    for policy in ("sap_ff", "sap_ff_gn", "external", "sap_lf", "sap_mc", "any_mu"):
        with pytest.raises(ValueError, match="MAX_MARGIN_POLICIES"):
            _shell({"any": 1}).run(policy, 1, outputs=("gn_window_margin_db",))


# ---------------------------------------------------------------------------------------- the rules on hand-made rows
def test_the_rules_on_hand_made_rows():
    nan, S = np.nan, 8
    # path 0: no window; path 1: free, none admitted; path 2 and 3: admitted, the same best margin; path 4: admitted, smaller
    best_slot = np.array([S, S, 5, 2, 1])
    best_margin = np.array([nan, nan, 1.5, 1.5, 0.5])
    first_free = np.array([S, 3, 4, 0, 1])
    assert mm.proposal(best_slot, best_margin, first_free, S, "sap") == (2, 5, 1.5, "admitted")
    assert mm.proposal(best_slot, best_margin, first_free, S, "any") == (2, 5, 1.5, "admitted")       # a tie between paths: the lowest index
    best_margin[4] = 1.5000001
    assert mm.proposal(best_slot, best_margin, first_free, S, "any") == (4, 1, 1.5000001, "admitted")  # strictly greater wins
    assert mm.proposal(best_slot, best_margin, first_free, S, "path", 3) == (3, 2, 1.5, "admitted")
    got = mm.proposal(best_slot, best_margin, first_free, S, "path", 1)                                # a fallback: refused by the step
    assert got[:2] == (1, 3) and np.isnan(got[2]) and got[3] == "fallback"
    for given in (0, 5, -1, 1 << 20):                                                                  # no window, or out of range
        got = mm.proposal(best_slot, best_margin, first_free, S, "path", given)
        assert got[:2] == (5, S) and np.isnan(got[2]) and got[3] == "rejection", given
    none = np.full(5, S)
    for route in ("sap", "any"):
        got = mm.proposal(none, np.full(5, nan), first_free, S, route)                                 # the first path with a free window
        assert got[:2] == (1, 3) and got[3] == "fallback"
        assert mm.proposal(none, np.full(5, nan), none, S, route)[:2] == (5, S)
    # a tie between slots is the query's: the lowest start with the largest w (gn_slots_reference.slots: nanargmax)
    w = np.array([[nan, 0.25, 0.75, 0.75, nan, 0.5, nan, nan]])
    assert int(np.nanargmax(w[0])) == 2
    rows = dict(window=~np.isnan(w) | np.array([[True] + [False] * 7]), mask=~np.isnan(w), near=np.zeros((1, 8), bool), w=w)
    assert mm.check_choice(rows, "sap", 0, 2) == "admitted" and mm.check_choice(rows, "any", 0, 3) == "admitted"   # inside BEST_TOL_DB
    with pytest.raises(AssertionError, match="best window"):
        mm.check_choice(rows, "sap", 0, 5)
    with pytest.raises(AssertionError, match="fallback although"):
        mm.check_choice(rows, "sap", 0, 0)
    with pytest.raises(AssertionError, match="rejection although"):
        mm.check_choice(rows, "sap", 1, 8)
    acts, ws, kinds = mm.proposals(best_slot[None], best_margin[None], first_free[None], S, "sap")
    assert acts.dtype == np.int32 and acts.tolist() == [[2, 5]] and ws.tolist() == [1.5] and kinds == ["admitted"]
    assert mm.first_free_of(rows["window"]).tolist() == [0]


# ---------------------------------------------------------------------------------------- what the batches exercise
@pytest.mark.parametrize("route", ["sap", "any"])
@pytest.mark.parametrize("batch", list(sl.BATCHES))
def test_what_a_batch_exercises(batch, route, tmp_path):
    c = mm.self_run(batch, route, tmp_path)
    print(batch, route, c)
    assert c["steps"] == sl.BATCHES[batch]["B"] * sl.BATCHES[batch]["n"]
    assert c["near"] <= mm.MAX_NEAR * c["steps"], c
    if batch in mm.COUNTED:
        assert c["best_not_first"] >= mm.MIN_COUNT and c["fallback"] >= mm.MIN_COUNT, c
        if route == "sap":
            assert c["later_path"] >= mm.MIN_COUNT, c
        assert c["neighbour_decided"] >= mm.MIN_COUNT, c   # (the counted batches all protect)
    if batch in sl.WORDS:   # there for their word count: a fallback, best windows that are not the first free one, and under the route
        # that looks at every path a proposal on a path from 8 up (sap_mm proposes there 0 .. 2 times per batch; path_mm_external is
        # given such paths by the device test: below)
        assert c["fallback"] >= 1 and c["best_not_first"] >= mm.MIN_COUNT, c
        if route == "any":
            assert c["high_path"] >= 1, c


def test_the_word_count_batches_are_given_high_paths(tmp_path):
    """path_mm_external in test_gpu_gn_max_margin.py draws its paths from default_rng(32): at every new word count some of them lie at
    8 or above (k = 9 has one such path: about one draw in nine)"""
    from gpu_support import MANY_PATHS
    assert [MANY_PATHS[b]["W"] for b in sl.WORDS] == [1, 3, 4, 6]
    for batch in sl.WORDS:
        c, k = sl.BATCHES[batch], MANY_PATHS[batch]["k"]
        assert (c["B"], c["n"], c["warmup"], c["protect"]) == (2, 40, 60, True) and batch not in mm.COUNTED
        given = np.random.default_rng(32).integers(0, k, size=(c["n"], c["B"]))
        assert (given >= 8).sum() >= 1, batch


# ---------------------------------------------------------------------------------------- what the shapes of test_gpu_gn_max_margin_shapes.py reach
@pytest.mark.parametrize("W", sorted(mm.WORD_CASES))
def test_what_a_word_count_case_reaches(W, tmp_path):
    """the first SHAPE_B environments of the batch, SHAPE_N steps of sap_mm: admitted proposals and a fallback (the classifier's "gn")
    at every word count; at one and two words also rejections (k, S), whose cause the classifier takes from the fit levels"""
    batch = mm.WORD_CASES[W]
    topo, kw, _ = sl.batch_case(batch, tmp_path)
    assert (kw["num_spectrum_resources"] + 63) // 64 == W and sorted(mm.WORD_CASES) == [1, 2, 3, 4, 5, 6, 8]
    steps = [s for i in range(mm.SHAPE_B) for s in mm.word_case_run(W, i, tmp_path)]
    kinds = [s[0] for s in steps]
    print(batch, {k: kinds.count(k) for k in ("admitted", "fallback", "rejection")}, "most running", max(s[2] for s in steps))
    assert len(steps) == mm.SHAPE_B * mm.SHAPE_N and kinds.count("admitted") >= mm.MIN_COUNT and kinds.count("fallback") >= 1
    if W <= 2:
        assert kinds.count("rejection") >= 1


def test_what_the_chunks_case_reaches(tmp_path):
    """every environment has more than 192 services in progress (four chunks of the ring) and more than 128 that share a link with one
    path (three chunks of the compacted list) at the first step the device evaluates -- whatever the max-margin steps then choose;
    nothing overflows a ring of 256"""
    c, kw = mm.CHUNKS, mm.chunks_kwargs()
    topo = sl.tri_topology(tmp_path)
    for i in range(c["B"]):
        (kind, _, running, sharing, pops), = mm.own_run(topo, kw, kw["seed"] + i, c["policy"], c["warmup"], (("sap", 1),))
        print("chunks", i, kind, "running", running, "sharing a link with one path", sharing, "released", pops)
        assert 192 < running < c["queue_capacity"] - sum(n for _, n in c["plan"]) and sharing > 128, (i, running, sharing)


def test_what_the_lapping_ring_reaches(tmp_path):
    """every environment releases at least 2 Q services, the ring's live entries wrap at Q at ten or more evaluated steps, and the ring
    never fills"""
    c = mm.LAP
    Q = c["queue_capacity"]
    for i in range(c["B"]):
        steps = mm.lap_run(i, tmp_path)
        wrapped = sum(1 for _, _, running, _, pops in steps if pops % Q + running > Q)
        print("lap", i, "released before the last step", steps[-1][4], "steps with a wrapped ring", wrapped, "most running", max(s[2] for s in steps))
        assert len(steps) == c["n"] and steps[-1][4] >= 2 * Q and wrapped >= mm.MIN_COUNT and max(s[2] for s in steps) < Q - 1, i


def test_the_plan_of_the_launch_of_fewer_waves():
    """NSFNET with 320 slots and a ring of 1024 (tests/test_wave_plan.py GEOMETRY): the handle's eight waves per workgroup become six, 14
    environments three workgroups; at the ring's cap of 4096 slots the handle has two waves and the launch keeps both"""
    from gpu_support import wave_plan
    c = mm.FEWER
    wave_bytes = lambda Q: 6112 + 12 * Q
    up16 = lambda n: (n + 15) & ~15
    Q = c["queue_capacity"]
    p = wave_plan(gated=1, protect=1, max_margin=1, n_steps=c["n"], wave_bytes=wave_bytes(Q), extra_per_wave=up16(4 * Q), wpb=8, B=c["B"])
    assert (p["family"], p["wpu"], p["nblocks"], p["lds"]) == ("MM", 6, 3, 14320 + 6 * (wave_bytes(Q) + 4 * Q)) and c["B"] % 6
    p = wave_plan(gated=1, protect=1, max_margin=1, wave_bytes=wave_bytes(4096), extra_per_wave=up16(4 * 4096), wpb=2, B=c["B"])
    assert p["wpu"] == 2
