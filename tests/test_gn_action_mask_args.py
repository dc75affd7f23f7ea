"""Action masks that know the GN-model admission check, and the policy ``sap_ff_gn``: the part that needs no GPU.  Shapes and
dtypes of the new mask kinds, every refusal raised before the library is called, the policy's number -- and, from the CPU oracle
alone (``gn_candidates_reference.py``), the conditions the comparisons of ``test_gpu_gn_action_masks.py`` rest on."""
import os

import numpy as np
import pytest

import gn_candidates_reference as cref
from conftest import ROOT
from optical_rl_gym_amd import BatchedRMSAEnv, DeepRMSAEnv, PathOnlyFirstFitAction, RMSAEnv, _lib

MARGIN_DB = 1e-4   # the margin of test_rmsa_gn_gate_args.py: no candidate's GSNR lies this close to its threshold
# (case, j) of the oracle-parity runs: 300 steps, environments on the seeds case seed + 0 .. 7
CASES = (("nsfnet_s320_l50_sapff", 1), ("nsfnet_s100_l20_spff", 2), ("jpn12_s320_l150_sapff", 1), ("ring34_s100_l60_sapff", 1))


class _NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although the arguments are wrong")


def _rmsa_shell(B=3, k=5, j=2, S=320, reject=1, gate=True):
    env = BatchedRMSAEnv.__new__(BatchedRMSAEnv)
    env.L, env.h = _NoLibrary(), None
    env.batch_size, env.k_paths, env.j, env.num_spectrum_resources, env.reject_action = B, k, j, S, reject
    env.words_per_link = (S + 63) // 64
    env.mask_dim = k * j + reject
    env.gn_gate = dict(thresholds_db=[0.0] * 6) if gate else None
    return env


def test_symbol_policy_and_kinds():
    assert _lib.POLICIES["sap_ff_gn"] == 7
    assert "orlg_gn_action_masks" in _lib.EXPORTED_SYMBOLS
    assert BatchedRMSAEnv.MASK_KINDS == ("deeprmsa", "path_ff", "slots", "path_ff_gn", "deeprmsa_gn")
    header = open(os.path.join(ROOT, "include", "orlg.h")).read()
    assert "#define ORLG_ABI_VERSION 3" in header and "orlg_gn_action_masks(" in header and "ORLG_POLICY_SAP_FF_GN = 7" in header
    L = _lib.load()
    assert L.orlg_abi_version() == 3 and L.orlg_gn_action_masks.argtypes is not None


def test_shapes_and_dtypes():
    env = _rmsa_shell()
    assert env.action_mask_shape("path_ff_gn") == ((3, 6), np.uint8)
    assert env.action_mask_shape("deeprmsa_gn") == ((3, 11), np.uint8)
    assert env.action_mask_gsnr_shape("path_ff_gn") == ((3, 5), np.float64)     # no column for the rejection
    assert env.action_mask_gsnr_shape("deeprmsa_gn") == ((3, 10), np.float64)
    env = _rmsa_shell(reject=0, j=1)
    assert env.action_mask_shape("path_ff_gn") == ((3, 5), np.uint8)
    assert env.action_mask_shape("deeprmsa_gn") == ((3, 5), np.uint8)
    assert env.action_mask_gsnr_shape("deeprmsa_gn") == ((3, 5), np.float64)
    # the old kinds as they were
    assert env.action_mask_shape("deeprmsa") == ((3, 5), np.uint8) and env.action_mask_shape("slots") == ((3, 5, 5), np.uint64)


@pytest.mark.parametrize("kind", ["path_ff_gn", "deeprmsa_gn"])
def test_a_handle_without_a_gate_refuses_the_new_kinds(kind):
    env = _rmsa_shell(gate=False)
    with pytest.raises(ValueError, match="gn_gate"):
        env.action_masks(kind)
    with pytest.raises(ValueError, match="gn_gate"):
        env.action_masks(kind, gsnr_out=True)


@pytest.mark.parametrize("kind", ["deeprmsa", "path_ff", "slots"])
def test_gsnr_out_with_an_old_kind(kind):
    for env in (_rmsa_shell(), _rmsa_shell(gate=False)):
        with pytest.raises(ValueError, match="gsnr_out"):
            env.action_masks(kind, gsnr_out=True)
        with pytest.raises(ValueError, match="gsnr_out"):
            env.action_masks(kind, gsnr_out=np.zeros((3, 5)))


@pytest.mark.parametrize("kind", ["path_ff_gnn", "gn", "PATH_FF_GN", "slots_gn"])
def test_unknown_kind(kind):
    with pytest.raises(ValueError, match="kind"):
        _rmsa_shell().action_masks(kind)
    with pytest.raises(ValueError, match="kind"):
        _rmsa_shell().action_mask_gsnr_shape(kind)


@pytest.mark.parametrize("kind,shape,dtype,err", [
    ("path_ff_gn", (3, 5), np.uint8, ValueError),        # the rejection column is missing
    ("path_ff_gn", (3, 6), np.bool_, TypeError),
    ("deeprmsa_gn", (3, 10), np.uint8, ValueError),
    ("deeprmsa_gn", (11, 3), np.uint8, ValueError),
    ("deeprmsa_gn", (3, 11), np.int8, TypeError),
])
def test_refuses_a_wrong_mask_buffer(kind, shape, dtype, err):
    with pytest.raises(err, match="out"):
        _rmsa_shell().action_masks(kind, out=np.zeros(shape, dtype))


@pytest.mark.parametrize("kind,shape,dtype,err", [
    ("path_ff_gn", (3, 6), np.float64, ValueError),      # the GSNR rows have no rejection column
    ("path_ff_gn", (3, 5), np.float32, TypeError),
    ("deeprmsa_gn", (3, 11), np.float64, ValueError),
    ("deeprmsa_gn", (3, 5), np.float64, ValueError),
    ("deeprmsa_gn", (3, 10), np.uint8, TypeError),
])
def test_refuses_a_wrong_gsnr_buffer(kind, shape, dtype, err):
    with pytest.raises(err, match="gsnr_out"):
        _rmsa_shell().action_masks(kind, gsnr_out=np.zeros(shape, dtype))
    ro = np.zeros(_rmsa_shell().action_mask_gsnr_shape(kind)[0])
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="read-only"):
        _rmsa_shell().action_masks(kind, gsnr_out=ro)


def test_views():
    """RMSAEnv's slot matrix has no gated form (k S checks per environment); the two views that have one ask the batched handle
    for the _gn kind, which a handle without a gate refuses before the library is called."""
    view = RMSAEnv.__new__(RMSAEnv)
    view._batched, view._index = _rmsa_shell(B=1), 0
    with pytest.raises(ValueError, match="slot matrix"):
        view.action_masks(gn=True)
    deep = DeepRMSAEnv.__new__(DeepRMSAEnv)
    deep._batched, deep._index = _rmsa_shell(B=1, gate=False), 0
    with pytest.raises(ValueError, match="gn_gate"):
        deep.action_masks(gn=True)
    path = PathOnlyFirstFitAction.__new__(PathOnlyFirstFitAction)
    path.__dict__.update(env=deep, _inner=deep)
    with pytest.raises(ValueError, match="gn_gate"):
        path.action_masks(gn=True)


# ---------------------------------------------------------------------------------------- what the GPU comparisons rest on
@pytest.mark.parametrize("case,j", CASES)
def test_oracle_conditions(case, j):
    """Over the 300 steps of the case on eight seeds: no candidate within 1e-4 dB of its threshold (so that a GSNR that differs in
    its last bits decides alike); every path_ff_gn column holds at least 5 % of both values in every environment; the gated and
    the window-free path_ff masks differ in at least 5 % of the steps, in environment 0 and over the eight together (a single
    environment of the 34-node ring lies at 4 - 9 %)."""
    runs = cref.run_batch(case, j=j)
    differ = []
    for i, (tr, _, fig) in enumerate(runs):
        assert tr["margin"].min() > MARGIN_DB, (case, i, tr["margin"].min())
        share = tr["path_ff_gn"].mean(axis=0)
        assert share.min() >= 0.05 and share.max() <= 0.95, (case, i, share)
        assert not (tr["path_ff_gn"] > tr["path_ff"]).any() and not (tr["deeprmsa_gn"] > tr["deeprmsa"]).any()
        assert np.array_equal(np.isfinite(tr["path_ff_gsnr"]), tr["path_ff"] == 1)
        assert np.array_equal(np.isfinite(tr["deeprmsa_gsnr"]), tr["deeprmsa"] == 1)
        differ.append((tr["path_ff_gn"] != tr["path_ff"]).any(axis=1).mean())
        assert fig["checks"] > 100
    assert differ[0] >= 0.05 and np.mean(differ) >= 0.05, (case, differ)
    if j == 2:
        # second blocks are rare at S = 100 (0 - 8 % of the steps): at least one set and at least one refused over the eight
        second, plain = (np.concatenate([tr[k][:, 1::2] for tr, _, _ in runs]) for k in ("deeprmsa_gn", "deeprmsa"))
        assert second.any() and ((plain == 1) & (second == 0)).any(), (int(second.sum()), int(plain.sum()))


def test_sap_ff_gn_goes_on_to_a_later_path():
    """sap_ff_gn on JPN12-320 at load 150: at least 10 steps where the first candidate is refused and a later one is taken, and
    the run keeps the margin."""
    for i, (tr, _, fig) in enumerate(cref.run_batch("jpn12_s320_l150_sapff", policy="sap_ff_gn")):
        assert fig["later_taken"] >= 10, (i, fig)
        assert tr["margin"].min() > MARGIN_DB, (i, tr["margin"].min())
    for i, (tr, _, fig) in enumerate(cref.run_batch("nsfnet_s320_l50_sapff", policy="sap_ff_gn")):
        assert tr["margin"].min() > MARGIN_DB, (i, tr["margin"].min())


def test_sap_ff_gn_accepts_iff_a_column_is_set():
    tr, _, _ = cref.run_case("jpn12_s320_l150_sapff", seed=3, policy="sap_ff_gn")
    assert np.array_equal(tr["accepted"] != 0, tr["path_ff_gn"].any(axis=1))
    acc = tr["accepted"] != 0
    assert np.array_equal(tr["act_path"][acc], tr["path_ff_gn"][acc].argmax(axis=1))
    assert np.array_equal(tr["gsnr"][acc], tr["path_ff_gsnr"][acc, tr["act_path"][acc]])
