"""Action masks and rule windows that know both halves of the GN-model admission check (``include/orlg.h``
``orlg_gn_admission_masks`` / ``orlg_gn_admission_windows``), what needs no GPU: the entry points, the shapes, the
refusals that come before the library is called, and -- from the admission oracle alone (``gn_admission_reference.py``, the
device's logarithm in it) -- the conditions that make the comparison of ``test_gpu_gn_admission.py`` meaningful."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gn_admission_reference as adm
import gn_protect_reference as pref
import gn_shapes_reference as sh
from conftest import load_topology
from optical_rl_gym_amd import BatchedDeepRMSAEnv, BatchedRMSAEnv, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("orlg_gn_admission_masks", "orlg_gn_admission_windows")


# ---------------------------------------------------------------------------------------- the entry points
def test_prototypes_exports_and_abi():
    header = open(os.path.join(ROOT, "include", "orlg.h")).read()
    declared = set(re.findall(r"\b(orlg_[a-z_0-9]+)\s*\(", header))
    vp = C.c_void_p
    for name in NEW:
        assert name in declared and name in _lib.PROTOTYPES and name in _lib.EXPORTED_SYMBOLS
    assert _lib.PROTOTYPES["orlg_gn_admission_masks"][1] == [vp] * 7
    assert _lib.PROTOTYPES["orlg_gn_admission_windows"][1] == [vp, C.c_int32, vp, vp, vp, vp]
    assert "#define ORLG_ABI_VERSION 3" in header
    L = _lib.load()
    assert L.orlg_abi_version() == 3
    # null handles are refused, not dereferenced (no device needed)
    assert L.orlg_gn_admission_masks(None, None, None, None, None, None, None) == -1
    assert L.orlg_gn_admission_windows(None, 0, None, None, None, None) == -1


def test_the_names_the_old_entries_are_pinned_to_stay():
    assert BatchedRMSAEnv.MASK_KINDS == ("deeprmsa", "path_ff", "slots", "path_ff_gn", "deeprmsa_gn")
    assert BatchedRMSAEnv.GN_MASK_KINDS == ("path_ff_gn", "deeprmsa_gn")
    assert BatchedRMSAEnv.ADMISSION_MASK_KINDS == ("path_ff", "deeprmsa") == BatchedDeepRMSAEnv.ADMISSION_MASK_KINDS
    assert tuple(_lib.GN_RULE_MODES) == ("check", "next_path")
    assert tuple(_lib.GN_PATH_WINDOW_RULES) == ("first", "first_full", "last", "best", "exact", "min_cut")


def test_the_kernels_are_a_unit_of_their_own():
    from optical_rl_gym_amd import build
    units = build.units()
    mine = [(n, s, x) for n, s, x in units if s == "orlg_inst_gnadmit.hip"]
    assert [n for n, _, _ in mine] == [f"orlg_inst_gnadmit_w{w}" for w in sorted(build.WAVE_W, reverse=True)]
    assert all(x == [f"-DORLG_INST_W={n.rsplit('w', 1)[1]}"] for n, _, x in mine)
    assert len({n for n, _, _ in units}) == len(units)
    inst = open(os.path.join(build.CSRC, "orlg_inst_gnadmit.hip")).read()
    assert '#include "orlg_gn_admission_kernels.hip"' in inst and "orlg_kernels.hip" not in inst
    for other in ("orlg_inst_wave.hip", "orlg_inst_gnrules.hip", "orlg_inst_gnprotect.hip", "orlg_inst_group.hip", "orlg_gn_audit_kernels.hip"):
        assert "gn_admission" not in open(os.path.join(build.CSRC, other)).read(), other
    variants = open(os.path.join(build.CSRC, "orlg_variants.h")).read()
    assert "orlg_pick_gn_admission_masks" in variants and "orlg_pick_gn_admission_windows" in variants


# ---------------------------------------------------------------------------------------- refusals before the library is called
class _NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although the arguments are wrong")


class _Recorder:
    """Stands where the loaded library would and keeps the calls: every entry returns ORLG_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _shell(gn_gate, cls=BatchedRMSAEnv, B=3, k=5, j=1, reject=0, lib=None):
    env = cls.__new__(cls)
    env.L, env.h = lib or _NoLibrary(), None
    env.batch_size, env.k_paths, env.j, env.reject_action, env.words_per_link = B, k, j, reject, 5
    env.gn_gate = gn_gate
    return env


PROTECTING, GATED = {"protect_running": True}, {"any": 1}


@pytest.mark.parametrize("cls", [BatchedRMSAEnv, BatchedDeepRMSAEnv])
def test_a_handle_without_a_gate_is_refused(cls):
    env = _shell(None, cls)
    for kind in cls.ADMISSION_MASK_KINDS:
        with pytest.raises(ValueError, match="gn_gate"):
            env.admission_masks(kind)
    for rule in _lib.GN_PATH_WINDOW_RULES:
        with pytest.raises(ValueError, match="gn_gate"):
            env.admission_windows(rule)


@pytest.mark.parametrize("gate", [PROTECTING, GATED])
def test_unknown_kinds_and_rules(gate):
    env = _shell(gate)
    for kind in ("slots", "path_ff_gn", "deeprmsa_gn", "best", None):
        with pytest.raises(ValueError, match="expected one of"):
            env.admission_masks(kind)
    for rule in ("most_used", "path_ff", 3, None):
        with pytest.raises(ValueError, match="expected one of"):
            env.admission_windows(rule)


@pytest.mark.parametrize("gate", [PROTECTING, GATED])
def test_wrong_and_read_only_buffers(gate):
    B, k, j = 3, 5, 2
    env = _shell(gate, B=B, k=k, j=j, reject=1)
    ro = lambda shape, dt: np.zeros(shape, dt).view()
    for kind, cols in (("path_ff", k), ("deeprmsa", k * j)):
        with pytest.raises(ValueError, match="shape"):
            env.admission_masks(kind, out=np.zeros((B, cols), np.uint8))        # the rejection's column is missing
        with pytest.raises(TypeError, match="dtype"):
            env.admission_masks(kind, out=np.zeros((B, cols + 1), np.int8))
        with pytest.raises(ValueError, match="shape"):
            env.admission_masks(kind, gsnr_out=np.zeros((B, cols + 1)))         # no rejection column in the rows
        with pytest.raises(ValueError, match="shape"):
            env.admission_masks(kind, margin_out=np.zeros((B, cols + 1)))
        with pytest.raises(TypeError, match="dtype"):
            env.admission_masks(kind, margin_out=np.zeros((B, cols), np.float32))
        with pytest.raises(ValueError, match="contiguous"):
            env.admission_masks(kind, gsnr_out=np.zeros((cols, B)).T)
        for name, shape, dt in (("out", (B, cols + 1), np.uint8), ("gsnr_out", (B, cols), np.float64), ("margin_out", (B, cols), np.float64)):
            a = ro(shape, dt)
            a.setflags(write=False)
            with pytest.raises(ValueError, match="read-only"):
                env.admission_masks(kind, **{name: a})
    for name, dt in (("slots_out", np.int16), ("gsnr_out", np.float64), ("margin_out", np.float64), ("admitted_out", np.uint8)):
        with pytest.raises(ValueError, match="shape"):
            env.admission_windows("best", **{name: np.zeros((B, k + 1), dt)})
        with pytest.raises(TypeError, match="dtype"):
            env.admission_windows("best", **{name: np.zeros((B, k), np.int64)})
        a = np.zeros((B, k), dt)
        a.setflags(write=False)
        with pytest.raises(ValueError, match="read-only"):
            env.admission_windows("best", **{name: a})


@pytest.mark.parametrize("gate", [PROTECTING, GATED])
def test_shapes_dtypes_and_what_is_returned(gate):
    B, k, j = 3, 5, 2
    lib = _Recorder()
    env = _shell(gate, B=B, k=k, j=j, reject=1, lib=lib)
    for kind, cols, where in (("path_ff", k, 1), ("deeprmsa", k * j, 4)):
        m = env.admission_masks(kind)
        assert isinstance(m, np.ndarray) and m.shape == (B, cols + 1) and m.dtype == np.uint8
        name, args = lib.calls[-1]
        assert name == "orlg_gn_admission_masks" and len(args) == 7
        assert [a is not None for a in args[1:]] == [i == where for i in range(1, 7)]   # the mask alone, in its kind's place
        m, g = env.admission_masks(kind, gsnr_out=True)
        assert g.shape == (B, cols) and g.dtype == np.float64
        m, mg = env.admission_masks(kind, margin_out=True)
        assert mg.shape == (B, cols) and mg.dtype == np.float64
        assert [a is not None for a in lib.calls[-1][1][1:]] == [i in (where, where + 2) for i in range(1, 7)]
        mine, rows, marg = np.zeros((B, cols + 1), np.uint8), np.zeros((B, cols)), np.zeros((B, cols))
        got = env.admission_masks(kind, out=mine, gsnr_out=rows, margin_out=marg)
        assert got[0] is mine and got[1] is rows and got[2] is marg
        assert [a is not None for a in lib.calls[-1][1][1:]] == [where <= i < where + 3 for i in range(1, 7)]
        assert env.admission_masks(kind, out=mine, gsnr_out=False, margin_out=None) is mine
    for rule, code in _lib.GN_PATH_WINDOW_RULES.items():
        slots, gsnr, margin, admitted = env.admission_windows(rule)
        assert [a.shape for a in (slots, gsnr, margin, admitted)] == [(B, k)] * 4
        assert [a.dtype for a in (slots, gsnr, margin, admitted)] == [np.int16, np.float64, np.float64, np.uint8]
        name, args = lib.calls[-1]
        assert name == "orlg_gn_admission_windows" and args[1] == code and all(a is not None for a in args[2:])
    mine = np.zeros((B, k))
    assert env.admission_windows("first", margin_out=mine)[2] is mine


@pytest.mark.parametrize("cls", [BatchedRMSAEnv, BatchedDeepRMSAEnv])
def test_the_old_names_still_refuse_and_name_the_new_entry(cls):
    env = _shell(PROTECTING, cls)
    for kind in cls.GN_MASK_KINDS:
        with pytest.raises(ValueError, match="protects its running lightpaths.*admission_masks"):
            env.action_masks(kind)
    with pytest.raises(ValueError, match="protects its running lightpaths.*admission_windows"):
        env.path_rule_windows("best")
    with pytest.raises(ValueError, match="protects its running lightpaths"):
        env.run("sap_bf", 10, gn_rule="check")


def test_the_views_choose_the_entry_by_the_handle():
    """DeepRMSAEnv.action_masks(gn=True) and PathOnlyFirstFitAction.action_masks(gn=True): admission_masks on a protecting handle,
    the call they always made otherwise; RMSAEnv.action_masks(gn=True) stays refused."""
    from optical_rl_gym_amd import DeepRMSAEnv, PathOnlyFirstFitAction, RMSAEnv

    class _Batched:
        def __init__(self, protect):
            self.gn_protect, self.said = protect, []

        def action_masks(self, kind):
            self.said.append(("action_masks", kind))
            return np.ones((1, 4), np.uint8)

        def admission_masks(self, kind):
            self.said.append(("admission_masks", kind))
            return np.ones((1, 4), np.uint8)

    for protect in (True, False):
        deep = DeepRMSAEnv.__new__(DeepRMSAEnv)
        deep._batched, deep._index = _Batched(protect), 0
        assert deep.action_masks(gn=True).dtype == bool and deep.action_masks().dtype == bool
        assert deep._batched.said == [("admission_masks", "deeprmsa") if protect else ("action_masks", "deeprmsa_gn"), ("action_masks", "deeprmsa")]
        inner = RMSAEnv.__new__(RMSAEnv)
        inner._batched, inner._index = _Batched(protect), 0
        view = PathOnlyFirstFitAction.__new__(PathOnlyFirstFitAction)
        view._inner, view.assign = inner, "first"
        view.action_masks(gn=True), view.action_masks()
        assert inner._batched.said == [("admission_masks", "path_ff") if protect else ("action_masks", "path_ff_gn"), ("action_masks", "path_ff")]
        with pytest.raises(ValueError, match="slot matrix"):
            inner.action_masks(gn=True)


# ---------------------------------------------------------------------------------------- the batches, from the oracle alone
@pytest.mark.parametrize("case", list(adm.BATCHES) + list(adm.COUNTED))
def test_batch_is_meaningful(case):
    """Per batch (the case's seed + 0 .. 7, 150 steps, 100 at S = 512), over the first fits and the blocks: at least 10 candidates
    the neighbour check alone refuses, 10 their own check refuses and 10 admitted with no affected service; and over every
    candidate, the rules' windows included, no own or neighbour margin within gn_shapes_reference.MARGIN_DB of zero."""
    runs = adm.parity_batch(case)
    fig, ff = adm.counts(runs, kinds=adm.KINDS), adm.counts(runs, kinds=("path_ff",))
    print(case, fig, "first fits: %d of %d neighbour-refused among those that pass their own check"
          % (ff["neighbour_refused"], ff["windows"] - ff["own_refused"]))
    assert fig["closest"] > sh.MARGIN_DB, fig["closest"]
    for name in ("neighbour_refused", "own_refused", "admitted_unaffected"):
        assert fig[name] >= adm.MIN_COUNT and ff[name] >= adm.MIN_COUNT, (name, fig[name], ff[name])
    for tr, _, _ in runs:
        for kind in adm.KINDS + adm.RULES:
            mask, gsnr, margin, affected = (tr[f"{kind}_{k}"] for k in ("mask", "gsnr", "margin", "affected"))
            assert not (np.isfinite(margin) & np.isnan(gsnr)).any() and not (mask[np.isnan(gsnr)]).any()
            assert np.array_equal(np.isfinite(margin), affected > 0)
            assert not (mask[margin < 0]).any() and (mask[np.isfinite(margin) & ~(margin < 0)] == 1).all()
        # rule "first" is the first fit of the mask: the same windows, the same verdicts
        for k in ("mask", "gsnr", "margin"):
            assert np.array_equal(tr[f"first_{k}"], tr[f"path_ff_{k}"], equal_nan=True)
        # the step's own candidate is one of the rows: its outcome is the row's
        for t in np.flatnonzero(np.isfinite(tr["gsnr"])):
            p = int(tr["act_path"][t])
            if int(tr["act_slot"][t]) == int(tr["path_ff_slots"][t, p]):
                assert int(tr["accepted"][t]) == int(tr["path_ff_mask"][t, p]), (t, p)


def test_the_issues_table():
    """The neighbour-refused first fits among those that pass their own check, as counted when the feature was asked for."""
    for case, want in (("nsfnet_s320_l50_sapff", (376, 2730)), ("jpn12_s320_l150_sapff", (2207, 4207)), ("ring36_s512_l500_sapff", (765, 2030)),
                       ("nsfnet_s100_l20_spff", (24, None)), ("ring34_s100_l60_sapff", (61, None))):
        ff = adm.counts(adm.parity_batch(case), kinds=("path_ff",))
        assert ff["neighbour_refused"] == want[0], (case, ff)
        if want[1] is not None:
            assert ff["windows"] - ff["own_refused"] == want[1], (case, ff)


def test_one_batch_holds_more_than_64_running_services_and_the_rings_light_every_range():
    fig = adm.counts(adm.parity_batch("ring34_s320_l300_llpff"))
    assert fig["max_running"] > 64, fig
    for case in ("ring34_s320_l300_llpff", "ring36_s512_l500_sapff"):
        E = load_topology(pref.CASES[case]["topology"]).num_links
        assert E > 64 and max(f["link_ranges"] for _, _, f in adm.parity_batch(case)) == (E + 63) // 64, case
