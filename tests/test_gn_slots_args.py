"""The GN-model admission check over the whole spectrum (``include/orlg.h`` ``orlg_gn_admission_slots``), what needs no
GPU: the entry point, the shapes, the refusals that come before the library is called, the view and the heuristic on a fake batched
object, and -- from the reference alone (``gn_slots_reference.py``, the device's logarithm in it) -- the conditions that make the
comparison of ``test_gpu_gn_slots.py`` meaningful."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gn_slots_reference as sl
from optical_rl_gym_amd import BatchedDeepRMSAEnv, BatchedRMSAEnv, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "orlg_gn_admission_slots"


# ---------------------------------------------------------------------------------------- the entry point
def test_prototype_export_and_abi():
    header = open(os.path.join(ROOT, "include", "orlg.h")).read()
    declared = set(re.findall(r"\b(orlg_[a-z_0-9]+)\s*\(", header))
    assert NEW in declared and NEW in _lib.PROTOTYPES and NEW in _lib.EXPORTED_SYMBOLS
    assert _lib.PROTOTYPES[NEW][1] == [C.c_void_p] * 6
    assert "#define ORLG_ABI_VERSION 3" in header
    L = _lib.load()   # (a fresh library: the loader rebuilds a stale one)
    assert L.orlg_abi_version() == 3
    assert L.orlg_gn_admission_slots(None, None, None, None, None, None) == -1   # a null handle is refused, not dereferenced


def test_the_kernel_is_a_unit_of_its_own():
    from optical_rl_gym_amd import build
    units = build.units()
    mine = [(n, s, x) for n, s, x in units if s == "orlg_inst_gnslots.hip"]
    assert [n for n, _, _ in mine] == [f"orlg_inst_gnslots_w{w}" for w in sorted(build.WAVE_W, reverse=True)]
    assert all(x == [f"-DORLG_INST_W={n.rsplit('w', 1)[1]}"] for n, _, x in mine)
    assert len({n for n, _, _ in units}) == len(units)
    assert "-ffp-contract=off" in build.FLAGS
    inst = open(os.path.join(build.CSRC, "orlg_inst_gnslots.hip")).read()
    assert '#include "orlg_gn_slots_kernels.hip"' in inst and "orlg_kernels.hip" not in inst
    for other in ("orlg_inst_wave.hip", "orlg_inst_gnrules.hip", "orlg_inst_gnprotect.hip", "orlg_inst_gnadmit.hip", "orlg_inst_group.hip",
                  "orlg_gn_audit_kernels.hip"):
        assert "gn_slots" not in open(os.path.join(build.CSRC, other)).read(), other
    assert "asm" not in open(os.path.join(build.CSRC, "orlg_gn_slots_kernels.hip")).read()   # no inline assembly in the new unit


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


B, K, S, W = 3, 5, 320, 5


def _shell(gn_gate, cls=BatchedRMSAEnv, lib=None):
    env = cls.__new__(cls)
    env.L, env.h = lib or _NoLibrary(), None
    env.batch_size, env.k_paths, env.j, env.reject_action, env.words_per_link, env.num_spectrum_resources = B, K, 1, 0, W, S
    env.gn_gate = gn_gate
    return env


PROTECTING, GATED = {"protect_running": True}, {"any": 1}


@pytest.mark.parametrize("cls", [BatchedRMSAEnv, BatchedDeepRMSAEnv])
def test_a_handle_without_a_gate_is_refused(cls):
    env = _shell(None, cls)
    with pytest.raises(ValueError, match="gn_gate"):
        env.admission_slot_masks()
    with pytest.raises(ValueError, match="gn_gate"):
        env.max_margin_windows()


@pytest.mark.parametrize("gate", [PROTECTING, GATED])
def test_wrong_and_read_only_buffers(gate):
    env = _shell(gate)
    with pytest.raises(ValueError, match="shape"):
        env.admission_slot_masks(out=np.zeros((B, K, W + 1), np.uint64))
    with pytest.raises(TypeError, match="dtype"):
        env.admission_slot_masks(out=np.zeros((B, K, W), np.int64))
    for name in ("gsnr_out", "margin_out"):
        with pytest.raises(ValueError, match="shape"):
            env.admission_slot_masks(**{name: np.zeros((B, K, S + 1))})
        with pytest.raises(TypeError, match="dtype"):
            env.admission_slot_masks(**{name: np.zeros((B, K, S), np.float32)})
        with pytest.raises(ValueError, match="contiguous"):
            env.admission_slot_masks(**{name: np.zeros((B, S, K)).transpose(0, 2, 1)})
    for name, shape, dt in (("out", (B, K, W), np.uint64), ("gsnr_out", (B, K, S), np.float64), ("margin_out", (B, K, S), np.float64)):
        a = np.zeros(shape, dt)
        a.setflags(write=False)
        with pytest.raises(ValueError, match="read-only"):
            env.admission_slot_masks(**{name: a})
    for name, dt in (("slots_out", np.int16), ("margin_out", np.float64)):
        with pytest.raises(ValueError, match="shape"):
            env.max_margin_windows(**{name: np.zeros((B, K + 1), dt)})
        with pytest.raises(TypeError, match="dtype"):
            env.max_margin_windows(**{name: np.zeros((B, K), np.int32)})
        a = np.zeros((B, K), dt)
        a.setflags(write=False)
        with pytest.raises(ValueError, match="read-only"):
            env.max_margin_windows(**{name: a})


@pytest.mark.parametrize("gate", [PROTECTING, GATED])
def test_shapes_dtypes_and_what_is_returned(gate):
    lib = _Recorder()
    env = _shell(gate, lib=lib)
    m = env.admission_slot_masks()
    assert isinstance(m, np.ndarray) and m.shape == (B, K, W) and m.dtype == np.uint64
    name, args = lib.calls[-1]
    assert name == NEW and len(args) == 6 and [a is not None for a in args[1:]] == [True, False, False, False, False]
    m, g = env.admission_slot_masks(gsnr_out=True)
    assert g.shape == (B, K, S) and g.dtype == np.float64
    assert [a is not None for a in lib.calls[-1][1][1:]] == [True, True, False, False, False]
    m, mg = env.admission_slot_masks(margin_out=True)
    assert mg.shape == (B, K, S) and mg.dtype == np.float64
    assert [a is not None for a in lib.calls[-1][1][1:]] == [True, False, True, False, False]
    mine, rows, marg = np.zeros((B, K, W), np.uint64), np.zeros((B, K, S)), np.zeros((B, K, S))
    got = env.admission_slot_masks(out=mine, gsnr_out=rows, margin_out=marg)
    assert got[0] is mine and got[1] is rows and got[2] is marg
    assert env.admission_slot_masks(out=mine, gsnr_out=False, margin_out=None) is mine
    slots, margin = env.max_margin_windows()
    assert slots.shape == margin.shape == (B, K) and slots.dtype == np.int16 and margin.dtype == np.float64
    name, args = lib.calls[-1]
    assert name == NEW and [a is not None for a in args[1:]] == [False, False, False, True, True]
    mine = np.zeros((B, K))
    assert env.max_margin_windows(margin_out=mine)[1] is mine


def test_torch_tensors_are_taken():
    torch = pytest.importorskip("torch")
    lib = _Recorder()
    env = _shell(GATED, lib=lib)
    g, mg = torch.zeros((B, K, S), dtype=torch.float64), torch.zeros((B, K, S), dtype=torch.float64)
    got = env.admission_slot_masks(gsnr_out=g, margin_out=mg)
    assert got[1] is g and got[2] is mg
    assert lib.calls[-1][1][2].value == g.data_ptr() and lib.calls[-1][1][3].value == mg.data_ptr()
    with pytest.raises(ValueError, match="shape"):
        env.admission_slot_masks(gsnr_out=torch.zeros((B, K, S + 1), dtype=torch.float64))
    with pytest.raises(TypeError, match="dtype"):
        env.admission_slot_masks(out=torch.zeros((B, K, W), dtype=torch.int64))   # the mask is unsigned
    s, bm = torch.zeros((B, K), dtype=torch.int16), torch.zeros((B, K), dtype=torch.float64)
    got = env.max_margin_windows(slots_out=s, margin_out=bm)
    assert got[0] is s and got[1] is bm and lib.calls[-1][0] == NEW


# ---------------------------------------------------------------------------------------- the view and the heuristic
class _Topology:
    graph = {"num_spectrum_resources": 8, "k_paths": 3}


class _Batched:
    """two environments, k = 3, S = 8"""

    def __init__(self, slots, margin, words=None):
        self.slots, self.margin, self.words, self.said = slots, margin, words, []

    def max_margin_windows(self):
        self.said.append("max_margin_windows")
        return self.slots, self.margin

    def admission_slot_masks(self):
        self.said.append("admission_slot_masks")
        return self.words

    def action_masks(self, kind):
        raise AssertionError("the gated view reads admission_slot_masks only")


def _view(batched, index, reject=0):
    from optical_rl_gym_amd import RMSAEnv
    v = RMSAEnv.__new__(RMSAEnv)
    v._batched, v._index, v.topology = batched, index, _Topology()
    v.k_paths, v.num_spectrum_resources, v.reject_action = 3, 8, reject
    return v


def test_the_heuristic_on_a_fake_batched_object():
    from optical_rl_gym_amd import max_margin_heuristic
    nan = np.nan
    b = _Batched(np.array([[8, 5, 2], [8, 8, 8], [3, 4, 1], [0, 7, 6]], np.int16), np.array([[nan, 1.5, 2.5], [nan, nan, nan], [0.5, 0.5, 0.25], [-0.0, 0.0, 0.0]]))
    for i, (sap, best) in enumerate([((1, 5), (2, 2)), ((3, 8), (3, 8)), ((0, 3), (0, 3)), ((0, 0), (0, 0))]):
        assert max_margin_heuristic("sap")(_view(b, i)) == sap, i
        assert max_margin_heuristic("any")(_view(b, i)) == best, i   # the lowest index on ties
    assert b.said == ["max_margin_windows"] * 8
    assert max_margin_heuristic("any").__name__ == "any_max_margin"
    for route in ("llp", "path", None):
        with pytest.raises(ValueError, match="expected one of"):
            max_margin_heuristic(route)


def test_the_view_on_a_fake_batched_object():
    words = np.zeros((2, 3, 1), np.uint64)
    words[1, 0, 0], words[1, 2, 0] = 0b10000001, 0b00011000
    b = _Batched(None, None, words)
    m = _view(b, 1).admission_slot_masks()
    assert m.dtype == bool and m.shape == (3, 8)
    assert np.array_equal(np.argwhere(m), [[0, 0], [0, 7], [2, 3], [2, 4]])
    m = _view(b, 1, reject=1).admission_slot_masks()
    assert m.shape == (4, 9) and m[3, 8] and not m[3, :8].any() and not m[:3, 8].any() and m[:3, :8].sum() == 4
    assert not _view(b, 0).admission_slot_masks().any()
    with pytest.raises(ValueError, match="slot matrix"):   # the refusal stays, with its message
        _view(b, 0).action_masks(gn=True)


# ---------------------------------------------------------------------------------------- the batches, from the reference alone
@pytest.mark.parametrize("batch", list(sl.BATCHES))
def test_batch_is_meaningful(batch, tmp_path):
    """Per batch: the windows the mask comparison leaves out (a deciding margin inside MARGIN_DB) are at most 0.01 % of its free
    windows; the rows are consistent; on the counted batches at least MIN_COUNT windows of each kind and MIN_COUNT paths whose best
    window is not their first free window; the shape with k > 8 admits and refuses windows on paths >= 8; the gated batch has no
    margin at all."""
    c = sl.BATCHES[batch]
    runs = sl.run_batch(batch, tmp_path)
    fig = sl.counts(runs)
    print(batch, fig)
    assert fig["windows"] > 0 and fig["near"] <= sl.MAX_LEFT_OUT * fig["windows"], fig
    for tr, _ in runs:
        window, gsnr, margin, mask, w = (tr[k] for k in ("window", "gsnr", "margin", "mask", "w"))
        assert np.array_equal(np.isfinite(gsnr), window) and not (np.isfinite(margin) & ~window).any()
        assert np.array_equal(np.isfinite(margin), tr["affected"] > 0)
        assert not mask[~window].any() and np.array_equal(np.isfinite(w), mask)
        S = window.shape[-1]
        for t in range(len(window)):
            for p in range(window.shape[1]):
                n = int(tr["n_slots"][t, p])
                assert not window[t, p, S - n + 1:].any()
                if mask[t, p].any():
                    assert tr["best_margin"][t, p] == np.nanmax(w[t, p]) and tr["best_slot"][t, p] == np.flatnonzero(w[t, p] == np.nanmax(w[t, p]))[0]
                else:
                    assert tr["best_slot"][t, p] == S and np.isnan(tr["best_margin"][t, p])
        # the step's own candidate is one of the windows: its outcome is the bit, its values are the rows'
        for t in np.flatnonzero(np.isfinite(tr["step_gsnr"])):
            p, s = int(tr["step_act_path"][t]), int(tr["step_act_slot"][t])
            assert window[t, p, s] and bool(tr["step_accepted"][t]) == bool(mask[t, p, s]), (t, p, s)
            assert tr["step_gsnr"][t] == gsnr[t, p, s] and np.array_equal(tr["step_margin"][t], margin[t, p, s], equal_nan=True), (t, p, s)
    if batch in sl.COUNTED:
        for name in ("own_refused", "neighbour_refused", "admitted_unaffected", "admitted_checked", "best_not_first"):
            assert fig[name] >= sl.MIN_COUNT, (name, fig)
    if batch == sl.K32:
        high_adm = sum(int(tr["mask"][:, 8:].sum()) for tr, _ in runs)
        high_ref = sum(int((tr["window"][:, 8:] & ~tr["mask"][:, 8:]).sum()) for tr, _ in runs)
        assert high_adm >= sl.MIN_COUNT and high_ref >= sl.MIN_COUNT, (high_adm, high_ref)
    if batch in sl.WORDS:   # one, three, four and six words per link with k > 8: windows admitted and refused on the paths from 8 up, and
        # best windows in the last word of the row (the end of the select chains over the chunks)
        S = runs[0][0]["window"].shape[-1]
        last = 64 * ((S + 63) // 64 - 1)
        high_adm = sum(int(tr["mask"][:, 8:].sum()) for tr, _ in runs)
        high_ref = sum(int((tr["window"][:, 8:] & ~tr["mask"][:, 8:]).sum()) for tr, _ in runs)
        best_last = sum(int(((tr["best_slot"] >= last) & (tr["best_slot"] < S)).sum()) for tr, _ in runs)
        assert (S + 63) // 64 in (1, 3, 4, 6) and min(high_adm, high_ref, best_last, fig["best_not_first"]) >= sl.MIN_COUNT, (high_adm, high_ref, best_last, fig)
    if batch == sl.TRI:   # more than 64 services share a link with one path, more than 64 run
        assert max(int(tr["affected"].max()) for tr, _ in runs) > 64 and fig["max_running"] > 64 and fig["admitted_checked"] >= sl.MIN_COUNT, fig
    if not c["protect"]:
        assert fig["neighbour_refused"] == 0 and fig["admitted_checked"] == 0 and fig["own_refused"] >= sl.MIN_COUNT, fig
        assert all(np.isnan(tr["margin"]).all() for tr, _ in runs)


@pytest.mark.parametrize("batch,steps", [("nsfnet_s100_l20_spff", (0, 25, 60)), ("jpn12_s320_l150_sapff", (30,)), ("gated:nsfnet_s320_l150_sapff", (35,))])
def test_the_rows_are_evaluate_window_by_window(batch, steps, tmp_path):
    """slots() sends the windows of a path through the oracle in one batch per check: the values are those of evaluate(p, s)"""
    assert sl.cross_check(batch, tmp_path, steps) >= 200


def test_the_shapes_the_batches_are_there_for(tmp_path):
    """nsfnet_s100: two start chunks, the second partial; jpn12: the neighbour check is busy; ring34: four mask words and more
    than 64 running services; ring36: eight words and 14 hops."""
    from conftest import load_topology
    import gn_protect_reference as pref
    assert pref.CASES["nsfnet_s100_l20_spff"]["S"] == 100
    jpn = sl.counts(sl.run_batch("jpn12_s320_l150_sapff", tmp_path))
    assert jpn["neighbour_refused"] > jpn["own_refused"] > 0, jpn
    ring34 = load_topology(pref.CASES["ring34_s320_l300_llpff"]["topology"])
    assert (ring34.num_links + 63) // 64 == 4
    assert sl.counts(sl.run_batch("ring34_s320_l300_llpff", tmp_path))["max_running"] > 64
    ring36 = load_topology(pref.CASES["ring36_s512_l500_sapff"]["topology"])
    assert pref.CASES["ring36_s512_l500_sapff"]["S"] == 512 and int(np.max(np.diff(ring36.path_link_off))) == 14
