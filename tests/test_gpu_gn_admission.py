"""Action masks and rule windows that know both halves of the GN-model admission check (``include/orlg.h``
``orlg_gn_admission_masks`` / ``orlg_gn_admission_windows``) on the device, held to the admission oracle of
``gn_admission_reference.py`` and to the step they describe: masks, ``admitted`` and ``slots`` exact; GSNR to rtol 1e-9 (the
tolerance of the gate); the neighbour margin to atol = 1e-9 x the largest |GSNR| the oracle computed in the batch (the
tolerance of ``test_gpu_gn_protect.py``); NaN in the same places; against the step itself, bit for bit.  ``test_gn_admission_args.py``
pins from the oracle alone what each batch exercises.  Every test here needs ``admission_masks`` / ``admission_windows``."""
import ctypes as C

import numpy as np
import pytest

import gn_admission_reference as adm
import gn_protect_reference as pref
import gn_shapes_reference as sh
from conftest import load_topology
from gpu_support import MANY_PATHS, many_paths_kwargs, many_paths_topology, rmsa_env

pytestmark = pytest.mark.gpu

RTOL = 1e-9
STEP_OUTS = ("act_path", "act_slot", "accepted", "gn_gsnr_db", "gn_neighbour_margin_db")


def _handle(case, B, protect=True, gate_over=None, **over):
    c = pref.CASES[case]
    topo = load_topology(c["topology"])
    return rmsa_env(topo, B, gn_gate=pref.case_gate(topo, protect=protect, **(gate_over or {})), **pref.case_kwargs(case, **over)), topo, c


def _query(env, rules):
    """every row of both entries for the pending requests: {kind: dict(mask, gsnr, margin[, slots])}"""
    out = {}
    for kind in env.ADMISSION_MASK_KINDS:
        m, g, mg = env.admission_masks(kind, gsnr_out=True, margin_out=True)
        out[kind] = dict(mask=m, gsnr=g, margin=mg)
    for rule in rules:
        s, g, mg, a = env.admission_windows(rule)
        out[rule] = dict(mask=a, gsnr=g, margin=mg, slots=s)
    return out


def _rows_match(dev, tr, t, i, reject, atol, what):
    """the device's rows of environment i before step t against the oracle's"""
    for kind, rows in dev.items():
        want = {k: tr[f"{kind}_{k}"][t] for k in ("mask", "gsnr", "margin", "slots")}
        cols = len(want["mask"])
        mask = rows["mask"][i]
        if "slots" in rows:
            assert np.array_equal(rows["slots"][i], want["slots"]), (what, kind, "slots")
        else:
            assert mask.shape == (cols + reject,) and (not reject or mask[cols] == 1), (what, kind, "the rejection's column")
        assert np.array_equal(mask[:cols], want["mask"]), (what, kind, "mask", mask[:cols], want["mask"])
        for name, tol in (("gsnr", dict(rtol=RTOL, atol=0)), ("margin", dict(rtol=0, atol=atol))):
            d, w = rows[name][i], want[name]
            assert np.array_equal(np.isnan(d), np.isnan(w)), (what, kind, name, d, w)
            ok = ~np.isnan(w)
            assert np.allclose(d[ok], w[ok], **tol), (what, kind, name, float(np.max(np.abs(d[ok] - w[ok]))))


def _parity(env, runs, policy, n, rules, reject, what, each=None):
    """n launches of one step, every query before each, against the batch's oracle runs"""
    atol = RTOL * max(fig["max_abs_gsnr"] for _, _, fig in runs)
    for t in range(n):
        dev = _query(env, rules)
        if each:
            each(env)
        step = env.run(policy, 1, outputs=STEP_OUTS, auto_reset=True)
        for i, (tr, _, _) in enumerate(runs):
            _rows_match(dev, tr, t, i, reject, atol, (what, t, i))
            assert step["act_path"][0, i] == tr["act_path"][t] and step["accepted"][0, i] == tr["accepted"][t], (what, t, i)


# ---------------------------------------------------------------------------------------- 1. oracle parity
def _ring_watch(env, seen):
    """per query: does the live part of some environment's release ring cross the ring's end?"""
    Q = env.queue_capacity

    def each(e):
        rs = e.running_services()
        seen.append(bool(((rs["head"] + rs["count"]) > Q).any()))
    return each


@pytest.mark.parametrize("case", list(adm.BATCHES))
def test_case_against_the_admission_oracle(case):
    """B = 8 on the case's seed + 0 .. 7, one launch per step; both masks with their rows and the windows of three rules before
    each.  jpn12 runs on a release ring of 128 slots: its environments provision 51 to 83 services in the 150 steps, so that ring
    does not reach its end -- test_the_live_ring_crosses_its_end runs the batch on 64 slots."""
    c = adm.BATCHES[case]
    env, topo, pc = _handle(case, adm.B, j=c["j"], **c["handle"])
    assert env.gn_protect and env.j == c["j"]
    if "queue_capacity" in c["handle"]:
        assert env.queue_capacity == c["handle"]["queue_capacity"]
    runs = adm.parity_batch(case)
    _parity(env, runs, pc["policy"], c["n"], adm.RULES, int(bool(c["handle"].get("allow_rejection"))), case)
    if case == "ring34_s320_l300_llpff":
        assert env.num_running().max() > 64
    env.close()


def test_the_live_ring_crosses_its_end():
    """The jpn12 batch on a release ring of 64 slots (at most 48 services run at once): the head advances with every release, and
    from about the 65th provisioned service on the live entries lie across the ring's end, where the kernel's copy to LDS
    straightens them out."""
    case = "jpn12_s320_l150_sapff"
    c = adm.BATCHES[case]
    env, topo, pc = _handle(case, adm.B, j=c["j"], queue_capacity=64)
    assert env.queue_capacity == 64
    crossed = []
    _parity(env, adm.parity_batch(case), pc["policy"], c["n"], adm.RULES, 0, case, _ring_watch(env, crossed))
    assert sum(crossed) >= 20, sum(crossed)
    env.close()


# ---------------------------------------------------------------------------------------- 2. mask = step, bit for bit
def test_the_rows_are_the_steps_outcome_bit_for_bit():
    """B = 64, NSFNET-320, load 50, j = 2, after 150 steps of sap_ff: for every DeepRMSA action, every path and every [p, slots[p]]
    of rule best -- load_state, one step: accepted is the bit, gn_gsnr_db and gn_neighbour_margin_db have the bytes of the rows."""
    B = 64
    env, topo, _ = _handle("nsfnet_s320_l50_sapff", B, j=2)
    K, J = topo.k_paths, 2
    env.run("sap_ff", 150, auto_reset=True)
    state = env.save_state()
    dev = _query(env, ("best",))
    own = neighbour = admitted = 0

    def one(policy, actions, mask, gsnr, margin, what):
        nonlocal own, neighbour, admitted
        env.load_state(state)
        r = env.run(policy, 1, actions=actions, outputs=STEP_OUTS)
        assert np.array_equal(r["accepted"][0] != 0, mask != 0), what
        assert r["gn_gsnr_db"][0].tobytes() == np.ascontiguousarray(gsnr).tobytes(), what
        assert r["gn_neighbour_margin_db"][0].tobytes() == np.ascontiguousarray(margin).tobytes(), what
        own += int((np.isfinite(gsnr) & np.isnan(margin) & (mask == 0)).sum())
        neighbour += int((margin < 0).sum())
        admitted += int((mask != 0).sum())

    for a in range(K * J):
        d = dev["deeprmsa"]
        one("deeprmsa_external", np.full(B, a, np.int32), d["mask"][:, a], d["gsnr"][:, a], d["margin"][:, a], ("deeprmsa", a))
    for p in range(K):
        d = dev["path_ff"]
        one("path_ff_external", np.full(B, p, np.int32), d["mask"][:, p], d["gsnr"][:, p], d["margin"][:, p], ("path_ff", p))
        d = dev["best"]
        acts = np.stack([np.full(B, p, np.int32), d["slots"][:, p].astype(np.int32)], axis=1)
        one("external", np.ascontiguousarray(acts), d["mask"][:, p], d["gsnr"][:, p], d["margin"][:, p], ("best", p))
    assert own > 0 and neighbour > 0 and admitted > 0, (own, neighbour, admitted)   # both kinds of refusal occur
    env.close()


# ---------------------------------------------------------------------------------------- 3. a handle that does not protect
def test_a_gated_handle_gets_the_bytes_of_the_old_entries():
    case = "nsfnet_s320_l150_sapff"
    B = 16
    env, topo, c = _handle(case, B, protect=False, j=2, allow_rejection=True)
    assert not env.gn_protect
    env.run("sap_ff", 200, auto_reset=True)
    for kind in env.ADMISSION_MASK_KINDS:
        m, g, mg = env.admission_masks(kind, gsnr_out=True, margin_out=True)
        m0, g0 = env.action_masks(kind + "_gn", gsnr_out=True)
        assert m.tobytes() == m0.tobytes() and g.tobytes() == g0.tobytes() and np.isnan(mg).all(), kind
        assert (m0[:, :-1] == 0).any() and (m0 == 1).any()
    from optical_rl_gym_amd import _lib
    for rule in _lib.GN_PATH_WINDOW_RULES:
        s, g, mg, a = env.admission_windows(rule)
        s0, g0, a0 = env.path_rule_windows(rule)
        assert s.tobytes() == s0.tobytes() and g.tobytes() == g0.tobytes() and a.tobytes() == a0.tobytes() and np.isnan(mg).all(), rule
    env.close()
    # protection that refuses nothing (0 dBm per 50 GHz on NSFNET): the masks of the gated handle, and the second check ran
    over = dict(launch_power_dbm_per_50ghz=0.0)
    prot, _, _ = _handle(case, B, gate_over=over)
    gated, _, _ = _handle(case, B, protect=False, gate_over=over)
    for e in (prot, gated):
        e.run("sap_ff", 200, auto_reset=True)
    assert prot.save_state().tobytes() == gated.save_state().tobytes()
    for kind in prot.ADMISSION_MASK_KINDS:
        m, g, mg = prot.admission_masks(kind, gsnr_out=True, margin_out=True)
        m0, g0 = gated.action_masks(kind + "_gn", gsnr_out=True)
        assert m.tobytes() == m0.tobytes() and g.tobytes() == g0.tobytes(), kind
        assert np.isfinite(mg).any() and not (mg < 0).any() and not (np.isfinite(mg) & np.isnan(g)).any()
    prot.close(); gated.close()


# ---------------------------------------------------------------------------------------- 4. sap_ff_gn under protection
@pytest.mark.parametrize("case", pref.SAP_GN_CASES)
def test_sap_ff_gn_takes_the_first_column_that_is_set(case):
    env, topo, c = _handle(case, pref.B)
    K = topo.k_paths
    taken_later = 0
    for t in range(150):
        m, g, mg = env.admission_masks("path_ff", gsnr_out=True, margin_out=True)
        r = env.run("sap_ff_gn", 1, outputs=STEP_OUTS, auto_reset=True)
        for i in range(pref.B):
            cols, has = np.flatnonzero(m[i, :K]), np.flatnonzero(~np.isnan(g[i]))
            assert bool(r["accepted"][0, i]) == bool(cols.size), (t, i)
            if has.size == 0:   # no path has a first fit: the rejection, no check
                assert np.isnan(r["gn_gsnr_db"][0, i]) and not r["accepted"][0, i]
                continue
            p = int(cols[0] if cols.size else has[0])   # the first admitted column; none: the refusal shows the first candidate
            assert r["act_path"][0, i] == p, (t, i)
            assert r["gn_gsnr_db"][0, i].tobytes() == g[i, p].tobytes() and r["gn_neighbour_margin_db"][0, i].tobytes() == mg[i, p].tobytes(), (t, i)
            taken_later += int(cols.size and p != has[0])
    assert taken_later >= 5, taken_later
    env.close()


# ---------------------------------------------------------------------------------------- 5. every word count, more than eight paths
@pytest.mark.parametrize("name", list(MANY_PATHS))
def test_every_word_count_above_eight_paths(name, tmp_path):
    """W = 1 .. 6, k = 9 .. 32, B = 4, 60 steps: rule first reads the candidates W lanes apart, best and min_cut scan eight paths per
    pass; columns >= 8 are both admitted and refused by the neighbour check."""
    c = MANY_PATHS[name]
    topo, kw = many_paths_topology(name, tmp_path), many_paths_kwargs(name)
    B, n = 4, 60
    runs = adm.run_batch((topo, kw), n_steps=n, policy=c["policy"], batch=B)
    high = adm.counts(runs, first_col=8)
    assert high["admitted_checked"] >= 10 and high["admitted_unaffected"] >= 10 and high["neighbour_refused"] >= 5 and high["own_refused"] >= 10, high
    assert high["closest"] > sh.MARGIN_DB
    env = rmsa_env(topo, B, gn_gate=pref.case_gate(topo), **kw)
    assert env.gn_protect and env.words_per_link == c["W"] and env.k_paths == c["k"] > 8
    _parity(env, runs, c["policy"], n, adm.RULES, 0, name)
    env.close()


# ---------------------------------------------------------------------------------------- 6. a batch larger than the grid
def test_a_batch_larger_than_the_grid():
    """B = 20 000: every wave strides over several environments.  The first and the last eight against the oracle after 100 steps."""
    case = "nsfnet_s320_l50_sapff"
    B, n = 20000, 100
    env, topo, c = _handle(case, B)
    env.run(c["policy"], n, auto_reset=True)
    dev = _query(env, ("best",))
    for i in list(range(8)) + list(range(B - 8, B)):
        tr, _, fig = adm.run_case(case, seed=c["seed"] + i, n_steps=n + 1, rules=("best",))
        one = {kind: {k: v[i:i + 1] for k, v in rows.items()} for kind, rows in dev.items()}
        _rows_match(one, tr, n, 0, 0, RTOL * fig["max_abs_gsnr"], (case, i))
    env.close()


# ---------------------------------------------------------------------------------------- 7. views, refusals
def test_views_serve_the_protecting_handle():
    from optical_rl_gym_amd import DeepRMSAEnv, PathOnlyFirstFitAction, RMSAEnv, shortest_available_path_first_fit
    topo = load_topology(pref.NSF)
    g = pref.case_gate(topo)
    env = RMSAEnv(topology=topo, num_spectrum_resources=100, load=20, mean_service_holding_time=25, seed=13, gn_gate=g)
    view = PathOnlyFirstFitAction(env)
    zeros = 0
    for _ in range(80):
        m = view.action_masks(gn=True)
        assert m.dtype == bool and np.array_equal(m, env._batched.admission_masks("path_ff")[0].astype(bool))
        zeros += int((~m).sum())
        env.step(shortest_available_path_first_fit(env))
    assert zeros > 0
    with pytest.raises(ValueError, match="slot matrix"):
        env.action_masks(gn=True)
    with pytest.raises(ValueError, match="protects its running lightpaths"):
        env._batched.action_masks("path_ff_gn")
    env.close()
    env = DeepRMSAEnv(topology=topo, num_spectrum_resources=100, seed=13, j=2, gn_gate=g)
    for a in (0, 1, 2, 3):
        m = env.action_masks(gn=True)
        assert m.dtype == bool and np.array_equal(m, env._batched.admission_masks("deeprmsa")[0].astype(bool))
        env.step(a)
    env.close()
    # a gated view makes the call it always made
    env = DeepRMSAEnv(topology=topo, num_spectrum_resources=100, seed=13, gn_gate=pref.case_gate(topo, protect=False))
    assert np.array_equal(env.action_masks(gn=True), env._batched.action_masks("deeprmsa_gn")[0].astype(bool))
    env.close()


def test_c_level_refusals_and_null_pointers():
    from optical_rl_gym_amd import BatchedRMSAEnv
    topo = load_topology(pref.NSF)
    kw = dict(num_spectrum_resources=100, load=20, mean_service_holding_time=25, seed=1)
    B, K = 4, topo.k_paths
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    m, f, s16 = np.zeros((B, K), np.uint8), np.zeros((B, K)), np.zeros((B, K), np.int16)
    env = BatchedRMSAEnv(topo, B, **kw)   # no gate
    L = env.L
    assert L.orlg_gn_admission_masks(env.h, ptr(m), None, None, None, None, None) == -1 and b"gn_gate" in L.orlg_last_error()
    assert L.orlg_gn_admission_windows(env.h, 0, ptr(s16), None, None, None) == -1 and b"gn_gate" in L.orlg_last_error()
    env.close()
    env = BatchedRMSAEnv(topo, B, gn_gate=pref.case_gate(topo), **kw)
    env.run("sap_ff", 40)
    before = env.save_state().tobytes()
    assert L.orlg_gn_admission_masks(env.h, None, None, None, None, None, None) == -1 and b"null argument" in L.orlg_last_error()
    assert L.orlg_gn_admission_windows(env.h, 0, None, None, None, None) == -1 and b"null argument" in L.orlg_last_error()
    for rule in (-1, 5, 101, 103):
        assert L.orlg_gn_admission_windows(env.h, rule, ptr(s16), None, None, None) == -1 and b"unknown rule" in L.orlg_last_error()
    # any single pointer is served, and has the bytes of the full call
    full = env.admission_masks("path_ff", gsnr_out=True, margin_out=True)
    deep = env.admission_masks("deeprmsa", gsnr_out=True, margin_out=True)
    for pos, want in enumerate(full + deep):
        buf = np.zeros_like(want)
        args = [None] * 6
        args[pos] = ptr(buf)
        assert L.orlg_gn_admission_masks(env.h, *args) == 0 and buf.tobytes() == want.tobytes(), pos
    win = env.admission_windows("min_cut")
    for pos, want in enumerate(win):
        buf = np.zeros_like(want)
        args = [None] * 4
        args[pos] = ptr(buf)
        assert L.orlg_gn_admission_windows(env.h, 102, *args) == 0 and buf.tobytes() == want.tobytes(), pos
    assert env.save_state().tobytes() == before   # they read state only
    # the old names still refuse on the protecting handle, and name the new entries
    assert L.orlg_gn_action_masks(env.h, ptr(m), ptr(f), None, None) == -1
    assert b"protects its running lightpaths" in L.orlg_last_error() and b"orlg_gn_admission_masks" in L.orlg_last_error()
    assert L.orlg_gn_path_windows(env.h, 0, ptr(s16), None, None) == -1
    assert b"protects its running lightpaths" in L.orlg_last_error() and b"orlg_gn_admission_windows" in L.orlg_last_error()
    with pytest.raises(ValueError, match="protects its running lightpaths"):
        env.action_masks("deeprmsa_gn")
    with pytest.raises(ValueError, match="protects its running lightpaths"):
        env.path_rule_windows("best")
    with pytest.raises(ValueError, match="protects its running lightpaths"):
        env.run("sap_bf", 2, gn_rule="check")
    env.close()
