"""Spectrum-assignment rules beyond the reference's first fit (``include/orlg.h`` ``ORLG_ASSIGN_*`` / ``orlg_step_assign``,
DESIGN 2.23), what needs no GPU: the numpy restatement of the definitions (``assign_reference.py``) against brute force on the
oracle's own queries; that the rules really differ from the reference's first fit on the shapes ``test_gpu_assign_rules.py``
compares, so that none of its comparisons is vacuous; the causes a new policy can produce; the entry point, its prototype and
the policy-name table; the refusals that come before the library is called; the new key lists; and the drop-in heuristic on a
stub view.

Measured with the oracle (8 environments x 200 steps; starts that differ from the reference's first fit / of them at the last
window S - n), ``sap`` route:   S = 64: last 917 / 603, best 21 / 14, exact 15 / 15, first_full 13 / 13;   S = 100: 951 / 429,
56 / 16, 18 / 18, 12 / 12;   S = 320: 1300 / 301, 318 / 12, 25 / 17, 6 / 6.  Minimum over the three routes: last 839, best 20,
exact 11, first_full (S <= 100) 6."""
import os
import subprocess

import numpy as np
import pytest

import assign_reference as ref
import block_cause_reference as bcr
from conftest import ROOT, load_topology, oracle_env_from_kwargs
from gpu_support import device_log_in_oracle
from optical_rl_gym_amd import ASSIGN_RULES, BatchedRMSAEnv, PathOnlyFirstFitAction, _lib, assignment_heuristic

NEW = ["orlg_step_assign"]


# ---------------------------------------------------------------------------------------- the reference against brute force
@pytest.mark.parametrize("S,load", [(64, 10), (100, 20)])
def test_reference_against_the_oracle_queries(S, load):
    """Slot by slot with is_path_free: the windows; first / first_full / last as the lowest / highest of them.  With
    available_blocks (j = 64: every block of these shapes): best = the shortest block, exact = the lowest block of exactly n else first_full."""
    topo = load_topology(ref.NSFNET)
    kw = bcr.shape_kwargs(S, load)
    seen = {r: 0 for r in ref.RULES}
    with device_log_in_oracle():
        o = oracle_env_from_kwargs(topo, kw, seed=ref.SEED0, j=64)
        for _ in range(ref.N_STEPS):
            r, avail = o.request(), o.available_slots()
            cand = ref.candidates(avail, topo, r.src, r.dst, r.bit_rate)
            for p, (A, n) in enumerate(cand):
                assert n == o.number_slots(p)
                free = [s for s in range(S) if o.is_path_free(p, s, n)]
                assert free == list(ref.windows(A, n))
                got = {rule: ref.rule_slot(A, n, rule) for rule in ref.RULES}
                below = [s for s in free if s < S - n]
                assert got["first"] == (below[0] if below else None)
                assert got["first_full"] == (free[0] if free else None) and got["last"] == (free[-1] if free else None)
                starts, lengths = (np.asarray(v) for v in o.available_blocks(p))
                assert list(starts) == [s for s, l in zip(*ref.blocks(A)) if l >= n]
                if not free:
                    assert len(starts) == 0 and got["best"] is None and got["exact"] is None
                    continue
                assert got["best"] == min(zip(lengths, starts))[1]
                same = [s for s, l in zip(starts, lengths) if l == n]
                assert got["exact"] == (same[0] if same else free[0])
                for rule in ref.NEW_RULES:
                    seen[rule] += got[rule] != got["first"]
            o.run("sap_ff", 1, reset_on_done=True, fields=[])
        o.close()
    assert all(seen[rule] > 0 for rule in ref.NEW_RULES), seen


def test_reference_edge_cases():
    A = np.array([1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1], np.uint8)   # blocks (0, 2) (3, 3) (7, 4) (12, 2)
    assert [ref.rule_slot(A, 2, r) for r in ref.RULES] == [0, 0, 12, 0, 0]
    assert [ref.rule_slot(A, 3, r) for r in ref.RULES] == [3, 3, 8, 3, 3]
    assert [ref.rule_slot(A, 4, r) for r in ref.RULES] == [7, 7, 7, 7, 7]
    assert [ref.rule_slot(A, 5, r) for r in ref.RULES] == [None] * 5
    A[0] = 0                                                            # blocks (1, 1) (3, 3) (7, 4) (12, 2)
    assert [ref.rule_slot(A, 2, r) for r in ref.RULES] == [3, 3, 12, 12, 12]   # best and exact: the block of exactly 2 at the end
    A[:] = 0
    A[12:] = 1
    assert [ref.rule_slot(A, 2, r) for r in ref.RULES] == [None, 12, 12, 12, 12]   # only the window at S - n
    assert ref.rule_slot(np.ones(4, np.uint8), 5, "last") is None                  # n > S


# ---------------------------------------------------------------------------------------- the rules differ; the causes
@pytest.mark.parametrize("route", ref.ROUTES)
@pytest.mark.parametrize("S,load", ref.SHAPES)
def test_rules_differ_from_first_fit_and_cause_bounds(S, load, route):
    for rule in ref.NEW_RULES:
        tr = ref.stacked(S, load, route, rule)
        differs = (tr["act_path"] != tr["first_path"]) | (tr["act_slot"] != tr["first_slot"])
        chosen = tr["act_path"] < 5
        at_last = differs & chosen & (tr["act_slot"] == S - tr["n_slots"])
        print(S, route, rule, "differing starts", int(differs.sum()), "at the last window", int(at_last.sum()),
              "blocking", 1 - tr["accepted"].mean())
        if rule != "first_full":
            assert differs.sum() >= 10, (S, route, rule, differs.sum())
        elif S <= 100:
            assert differs.sum() >= 5, (S, route, rule, differs.sum())
        # a proposed window is a free window: accepted iff a path was chosen
        assert np.array_equal(tr["accepted"] == 1, chosen)
        assert np.array_equal(tr["cause"] == bcr.ACCEPTED, tr["accepted"] == 1)
        # sap / llp take any window of any path: they refuse only where no path has one; sp may leave one on another path
        if route == "sp":
            assert tr["cause"].max() <= bcr.C_POLICY
        else:
            assert tr["cause"].max() <= bcr.C_ALIGNMENT, (S, route, rule, np.bincount(tr["cause"].ravel()))
        if rule == "exact" and S == 320:
            other = chosen & (tr["act_slot"] != tr["lowest_block"])
            print(S, route, "exact took a block that is not the path's first:", int(other.sum()))
            assert other.sum() >= 10, (route, other.sum())


def test_sp_can_refuse_with_the_last_window_or_policy_cause():
    seen = set()
    for S, load in ref.SHAPES:
        for rule in ref.NEW_RULES:
            seen |= set(np.unique(ref.stacked(S, load, "sp", rule)["cause"]).tolist())
    assert bcr.C_LAST_WINDOW in seen or bcr.C_POLICY in seen, seen


# ---------------------------------------------------------------------------------------- ABI, prototypes, exports, names
def test_new_symbol_in_a_fresh_library():
    assert set(NEW) <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.load()
    assert L.orlg_abi_version() == 3
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW) <= names
    header = open(os.path.join(ROOT, "include", "orlg.h")).read()
    assert "#define ORLG_ABI_VERSION 3" in header
    for s in NEW:
        assert s + "(" in header and hasattr(L, s) and len(getattr(L, s).argtypes) == 8
    for i, name in enumerate(ASSIGN_RULES):
        assert "ORLG_ASSIGN_%s = %d" % (name.upper(), i) in header
    assert "ORLG_NUM_ASSIGN_RULES = %d" % len(ASSIGN_RULES) in header
    assert ASSIGN_RULES == ("first", "first_full", "last", "best", "exact") == ref.RULES


def test_policy_name_table():
    P = _lib.POLICIES
    want = {}
    for rule, suffix in (("first_full", "ff_full"), ("last", "lf"), ("best", "bf"), ("exact", "ef")):
        for route in ("sp", "sap", "llp"):
            want[f"{route}_{suffix}"] = (P[route + "_ff"], ASSIGN_RULES.index(rule))
        want[f"path_{suffix}_external"] = (P["path_ff_external"], ASSIGN_RULES.index(rule))
    assert _lib.ASSIGN_POLICIES == want and len(want) == 16
    assert not set(want) & set(P)
    for name, ids in want.items():
        assert _lib.policy_ids(name) == ids
    for name, pid in P.items():
        assert _lib.policy_ids(name) == (pid, 0)
    with pytest.raises(KeyError):
        _lib.policy_ids("sap_rf")
    for route in ref.ROUTES + ("path",):
        for rule in ref.NEW_RULES:
            assert ref.policy_name(route, rule) in want


def test_assign_key_lists_resolve_to_their_kernels():
    from host_programs import variant_names
    from optical_rl_gym_amd import build
    counts = variant_names().counts
    # per word count: 3 statistics levels x {no cause, CAUSE} wave keys, 3 x {plain, traffic, trace} x {no cause, CAUSE} group keys
    assert (counts["ORLG_WAVE_ASSIGN_KEYS"], counts["ORLG_GROUP_ASSIGN_KEYS"]) == (6 * len(build.WAVE_W), 18 * len(build.WAVE_W))


# ---------------------------------------------------------------------------------------- refusals before the library is called
class _NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although the arguments are wrong")


def _rmsa_shell(B=3, k=5, gn_gate=None):
    env = BatchedRMSAEnv.__new__(BatchedRMSAEnv)
    env.L, env.h = _NoLibrary(), None
    env.batch_size, env.k_paths, env.gn_gate = B, k, gn_gate
    return env


@pytest.mark.parametrize("policy", sorted(_lib.ASSIGN_POLICIES))
def test_gated_handle_refuses_in_python(policy):
    with pytest.raises(ValueError, match="gn_gate"):
        _rmsa_shell(gn_gate={"any": 1}).run(policy, 10, actions=np.zeros(3, np.int32))


@pytest.mark.parametrize("policy", ["sap_rf", "external_lf", "deeprmsa_sap_bf", "sap_ff_gn_lf", "path_external_lf"])
def test_unknown_combinations_have_no_name(policy):
    """external names its own slot, the DeepRMSA policies index blocks, sap_ff_gn asks the gate: none of them has a rule."""
    with pytest.raises(KeyError):
        _rmsa_shell().run(policy, 10)


def test_path_actions_are_checked():
    for policy in ("path_lf_external", "path_bf_external"):
        with pytest.raises(ValueError, match="actions"):
            _rmsa_shell().run(policy, 1)
        with pytest.raises(ValueError, match="actions"):
            _rmsa_shell().run(policy, 1, actions=np.zeros((3, 2), np.int32))
        with pytest.raises(TypeError, match="actions"):
            _rmsa_shell().run(policy, 1, actions=np.zeros(3, np.float64))


def test_cause_buffers_are_checked_under_a_rule():
    with pytest.raises(ValueError, match="cause_counts"):
        _rmsa_shell().run("sap_bf", 10, cause_counts=np.zeros((3, 7), np.int32))


# ---------------------------------------------------------------------------------------- the drop-in heuristic on a stub view
class _StubPath:
    def __init__(self, A, n):
        self.A, self.n = np.asarray(A), n


class _StubView:
    """What a heuristic reads of RMSA-v0: the topology's two sizes, the candidates of the pending request, the two queries."""

    def __init__(self, cand):
        self.k_shortest_paths = {(0, 1): [_StubPath(A, n) for A, n in cand]}
        self.current_service = type("S", (), dict(source=0, destination=1))()
        self.topology = type("T", (), dict(graph=dict(num_spectrum_resources=len(cand[0][0]), k_paths=len(cand))))()
        self.k_paths, self.reject_action = len(cand), 0

    def get_available_slots(self, path):
        return path.A.copy()

    def get_number_slots(self, path):
        return path.n


def test_assignment_heuristic_equals_the_reference_on_a_stub_view():
    topo = load_topology(ref.NSFNET)
    checked = 0
    with device_log_in_oracle():
        o = oracle_env_from_kwargs(topo, bcr.shape_kwargs(64, 10), seed=ref.SEED0)
        for _ in range(120):
            r, avail = o.request(), o.available_slots()
            view = _StubView(ref.candidates(avail, topo, r.src, r.dst, r.bit_rate))
            for rule in ref.RULES:
                for route in ref.ROUTES:
                    got = assignment_heuristic(route, rule)(view)
                    assert tuple(got) == ref.propose(avail, topo, r.src, r.dst, r.bit_rate, route, rule), (route, rule)
                    checked += 1
                wrapped = PathOnlyFirstFitAction.__new__(PathOnlyFirstFitAction)
                wrapped.assign, wrapped._inner = rule, view
                if rule != "first":
                    for a in (-1, 0, 2, 4, 5, 9):
                        assert wrapped.action(a) == ref.propose(avail, topo, r.src, r.dst, r.bit_rate, "path", rule, a), (rule, a)
            o.run("sap_ff", 1, reset_on_done=True, fields=[])
        o.close()
    assert checked == 120 * 15
    with pytest.raises(ValueError, match="route"):
        assignment_heuristic("path", "best")
    with pytest.raises(ValueError, match="rule"):
        assignment_heuristic("sap", "random")
    with pytest.raises(ValueError, match="assign"):
        PathOnlyFirstFitAction(None, assign="random")
