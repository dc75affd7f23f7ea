"""The fewest-cuts window (``include/orlg.h`` ``orlg_step_min_cut`` / ``orlg_path_min_cuts``), what needs no GPU: the
numpy restatement of the definitions (``cut_reference.py``) against brute force -- slot by slot on random availability arrays and
with the oracle's ``is_path_free``; that the rule really differs from first fit and best fit on the shapes
``test_gpu_cut_rules.py`` compares, so that none of its comparisons is vacuous; the causes a route can produce; the entry
points, their prototypes and the policy-name table; the new key lists; the refusals that come before the library is called; and the drop-in
heuristic on a stub view.

Measured with the oracle under the device logarithm (8 environments x 200 steps, minimum over the environments; the printed
lines of test_rule_differs_and_cause_bounds): decisions that differ from both first_full and best 17 .. 68 over the routes and
shapes; chosen windows with cuts > 0 at S = 320: 35 .. 46; fewest-cuts path other than sap's path: S = 320 13, S = 100 2,
S = 64 0 (nothing asserted there)."""
import os
import subprocess

import numpy as np
import pytest

import block_cause_reference as bcr
import cut_reference as ref
from conftest import ROOT, load_topology, oracle_env_from_kwargs
from gpu_support import device_log_in_oracle
from optical_rl_gym_amd import CUT_POLICIES, BatchedRMSAEnv, _lib, min_cut_heuristic

NEW = {"orlg_step_min_cut": 7, "orlg_path_min_cuts": 3}


# ---------------------------------------------------------------------------------------- the reference against brute force
def _brute(rows, n):
    """every window with its cuts, slot by slot"""
    h, S = rows.shape
    out = []
    for s in range(0, S - n + 1):
        if all(rows[l][t] for l in range(h) for t in range(s, s + n)):
            cuts = 0
            for l in range(h):
                left = rows[l][s - 1] if s - 1 >= 0 else 0
                right = rows[l][s + n] if s + n < S else 0
                cuts += 1 if left and right else 0
            out.append((s, cuts))
    return out


@pytest.mark.parametrize("S", [64, 100, 130, 320])
def test_reference_against_brute_force_on_random_arrays(S):
    rng = np.random.default_rng(S)
    seen = dict(at0=0, at_end=0, long=0, cut_gt0=0, not_lowest=0, none=0)
    for trial in range(150):
        h = int(rng.integers(1, 6))
        n = int(rng.integers(64, 90)) if trial % 5 == 0 and S > 100 else int(rng.integers(1, 12))
        # long free runs with a few used slots per link, so that windows exist and their neighbours vary
        rows = (rng.random((h, S)) > rng.choice([0.01, 0.03, 0.08])).astype(np.uint8)
        if trial % 3 == 0:
            rows[:, :n] = 1          # a window at slot 0
        if trial % 4 == 0:
            rows[:, S - n:] = 1      # a window at S - n
        want = _brute(rows, n)
        starts, cuts = ref.window_cuts(rows, n)
        assert list(zip(starts.tolist(), cuts.tolist())) == want
        got = ref.min_cut_window(rows, n)
        if not want:
            assert got is None
            seen["none"] += 1
            continue
        best = min(want, key=lambda sc: (sc[1], sc[0]))
        assert got == (best[1], best[0])
        seen["at0"] += want[0][0] == 0
        seen["at_end"] += want[-1][0] == S - n
        seen["long"] += n >= 64
        seen["cut_gt0"] += best[1] > 0
        seen["not_lowest"] += best[0] != want[0][0]
    print(S, seen)
    assert seen["at0"] and seen["at_end"] and seen["not_lowest"] and seen["none"]
    if S > 100:
        assert seen["long"]


def test_reference_edge_cases():
    one = lambda *rows: np.array(rows, np.uint8)
    # a window in the middle of a block cuts it; at either end of the block it does not; the spectrum's ends are not free
    assert ref.min_cut_window(one([1, 1, 1, 1]), 4) == (0, 0)
    assert ref.min_cut_window(one([1, 1, 1, 1, 1]), 3) == (0, 0)
    starts, cuts = ref.window_cuts(one([1, 1, 1, 1, 1]), 3)
    assert starts.tolist() == [0, 1, 2] and cuts.tolist() == [0, 1, 0]
    # two links: the lowest window cuts both, a later one cuts one, the window at S - n cuts none
    rows = one([1, 1, 1, 1, 0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1, 1, 1, 1])
    starts, cuts = ref.window_cuts(rows, 2)
    assert starts.tolist() == [0, 1, 2, 5, 6, 7, 8] and cuts.tolist() == [0, 2, 1, 1, 2, 2, 0]
    assert ref.min_cut_window(rows, 2) == (0, 0)
    rows[:, 0] = 0
    rows[:, 9] = 0
    assert ref.min_cut_window(rows, 2) == (0, 1)        # [1, 3): left neighbour used on both links
    rows[0, 3] = 0                                       # link 0: blocks [1, 3) [5, 9); link 1: [1, 9), cut by [5, 7)
    starts, cuts = ref.window_cuts(rows, 2)
    assert starts.tolist() == [1, 5, 6, 7] and cuts.tolist() == [0, 1, 2, 0]
    assert ref.min_cut_window(one([1, 1, 0, 1]), 3) is None and ref.min_cut_window(one([1, 1]), 3) is None   # none, n > S


@pytest.mark.parametrize("S,load", [(64, 10), (100, 20)])
def test_reference_against_the_oracle_queries(S, load):
    """Slot by slot with is_path_free: the windows; with the links' own rows: the neighbours.  path_min_cuts and propose on top."""
    topo = load_topology(ref.NSFNET)
    kw = bcr.shape_kwargs(S, load)
    with device_log_in_oracle():
        o = oracle_env_from_kwargs(topo, kw, seed=ref.SEED0)
        for _ in range(ref.N_STEPS):
            r, avail = o.request(), o.available_slots()
            base = int(topo.pair_path_base[r.src * topo.num_nodes + r.dst])
            cuts, slots = ref.path_min_cuts(avail, topo, r.src, r.dst, r.bit_rate)
            per_path = []
            for p, (rows, n) in enumerate(ref.candidates(avail, topo, r.src, r.dst, r.bit_rate)):
                assert n == o.number_slots(p)
                links = ref.path_links(topo, base + p)
                assert len(links) == topo.path_hops[base + p] and np.array_equal(rows, avail[links])
                free = [s for s in range(S) if o.is_path_free(p, s, n)]
                want = [(s, sum(1 for l in links if s > 0 and avail[l][s - 1] and s + n < S and avail[l][s + n])) for s in free]
                starts, c = ref.window_cuts(rows, n)
                assert list(zip(starts.tolist(), c.tolist())) == want
                best = min(want, key=lambda sc: (sc[1], sc[0])) if want else None
                assert (cuts[p], slots[p]) == ((best[1], best[0]) if best else (-1, S))
                per_path.append(best)
            have = [p for p, b in enumerate(per_path) if b]
            rej = (topo.k_paths, S, -1)
            assert ref.propose(avail, topo, r.src, r.dst, r.bit_rate, "sp") == ((0, per_path[0][0], per_path[0][1]) if per_path[0] else rej)
            assert ref.propose(avail, topo, r.src, r.dst, r.bit_rate, "sap") == ((have[0], per_path[have[0]][0], per_path[have[0]][1]) if have else rej)
            p_mc = min(have, key=lambda p: (per_path[p][1], p)) if have else None
            assert ref.propose(avail, topo, r.src, r.dst, r.bit_rate, "min_cut") == ((p_mc, per_path[p_mc][0], per_path[p_mc][1]) if have else rej)
            free_of = lambda p: int(avail[ref.path_links(topo, base + p)].min(axis=0).sum())
            p_ll = min(have, key=lambda p: (-free_of(p), p)) if have else None
            assert ref.propose(avail, topo, r.src, r.dst, r.bit_rate, "llp") == ((p_ll, per_path[p_ll][0], per_path[p_ll][1]) if have else rej)
            for a in (-1, 0, 3, 5, 8):
                ok = 0 <= a < topo.k_paths and per_path[a]
                assert ref.propose(avail, topo, r.src, r.dst, r.bit_rate, "path", a) == ((a, per_path[a][0], per_path[a][1]) if ok else rej)
            o.run("sap_ff", 1, reset_on_done=True, fields=[])
        o.close()


# ---------------------------------------------------------------------------------------- the rule differs; the causes
@pytest.mark.parametrize("route", ref.ROUTES)
@pytest.mark.parametrize("S,load", ref.SHAPES)
def test_rule_differs_and_cause_bounds(S, load, route):
    tr = ref.stacked(S, load, route)
    k = 5
    chosen = tr["act_path"] < k
    d_ff = (tr["act_path"] != tr["ff_path"]) | (tr["act_slot"] != tr["ff_slot"])
    d_bf = (tr["act_path"] != tr["bf_path"]) | (tr["act_slot"] != tr["bf_slot"])
    both = (d_ff & d_bf).sum(axis=0)            # per environment
    cut_gt0 = (tr["cuts"] > 0).sum(axis=0)
    other_path = (chosen & (tr["act_path"] != tr["sap_path"])).sum(axis=0)
    print(S, route, "differs from first_full and best: min", int(both.min()), "max", int(both.max()), "| cuts > 0: min", int(cut_gt0.min()),
          "| path other than sap's: min", int(other_path.min()), "| blocking", 1 - tr["accepted"].mean())
    assert both.min() >= 10, (S, route, both)
    if S == 320:
        assert cut_gt0.min() >= 20, (route, cut_gt0)
    if route == "min_cut":
        if S == 320:
            assert other_path.min() >= 5, other_path
        if S == 100:
            assert other_path.min() >= 1, other_path
    # a proposed window is a free window: accepted iff a path was chosen; the cuts are in 0 .. hops
    assert np.array_equal(tr["accepted"] == 1, chosen)
    assert np.array_equal(tr["cause"] == bcr.ACCEPTED, tr["accepted"] == 1)
    assert np.array_equal(tr["cuts"] >= 0, chosen) and (tr["cuts"] <= tr["hops"]).all() and (tr["cuts"] <= tr["lowest_cuts"]).all()
    # sap / llp / fewest-cuts take any window of any path: they refuse only where no path has one; sp may leave one on another path
    if route == "sp":
        assert tr["cause"].max() <= bcr.C_POLICY
    else:
        assert tr["cause"].max() <= bcr.C_ALIGNMENT, (S, route, np.bincount(tr["cause"].ravel()))
        assert np.array_equal(chosen, tr["sap_path"] < k)


def test_sp_can_refuse_with_the_last_window_or_policy_cause():
    seen = set()
    for S, load in ref.SHAPES:
        seen |= set(np.unique(ref.stacked(S, load, "sp")["cause"]).tolist())
    assert bcr.C_LAST_WINDOW in seen or bcr.C_POLICY in seen, seen


# ---------------------------------------------------------------------------------------- ABI, prototypes, exports, names
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
    # the public rules and policies are what they were: the new rule and route are not among them
    assert "ORLG_NUM_ASSIGN_RULES = 5" in header and "ORLG_ASSIGN_MIN_CUT" not in header and "ORLG_POLICY_MIN_CUT" not in header
    assert "#define ORLG_ROUTE_FEWEST_CUTS %d" % _lib.ROUTE_FEWEST_CUTS in header
    assert _lib.ROUTE_FEWEST_CUTS not in _lib.POLICIES.values()
    device = open(os.path.join(ROOT, "optical-rl-gym-qot-aware_amd", "csrc", "orlg_device.h")).read()
    assert "ORLG_ASSIGN_MIN_CUT = 5" in device and "ORLG_POLICY_MIN_CUT = 8" in device
    assert _lib.ASSIGN_RULES == ("first", "first_full", "last", "best", "exact")


def test_a_null_handle_answers_first():
    """orlg_step_assign keeps the order of its answers: the handle before the rule; the new entry points check the handle too."""
    L = _lib.load()
    for rule in (0, 3, 5, 99):
        assert L.orlg_step_assign(None, 1, rule, 10, None, 1, None, None) == -1 and b"null handle" in L.orlg_last_error()
    for route in (1, _lib.ROUTE_FEWEST_CUTS, 99):
        assert L.orlg_step_min_cut(None, route, 10, None, 1, None, None) == -1 and b"null handle" in L.orlg_last_error()
    assert L.orlg_path_min_cuts(None, None, None) == -1 and b"null handle" in L.orlg_last_error()


def test_policy_name_table():
    P = _lib.POLICIES
    assert _lib.CUT_POLICIES is CUT_POLICIES
    assert CUT_POLICIES == {"sp_mc": P["sp_ff"], "sap_mc": P["sap_ff"], "llp_mc": P["llp_ff"], "min_cut": _lib.ROUTE_FEWEST_CUTS,
                            "path_mc_external": P["path_ff_external"]}
    assert not set(CUT_POLICIES) & set(P) and not set(CUT_POLICIES) & set(_lib.ASSIGN_POLICIES)
    assert len(_lib.ASSIGN_POLICIES) == 16
    for name in CUT_POLICIES:       # policy_ids answers for the names it always answered for
        with pytest.raises(KeyError):
            _lib.policy_ids(name)
    for name, pid in P.items():
        assert _lib.policy_ids(name) == (pid, 0)
    assert set(ref.POLICY.values()) == set(CUT_POLICIES)


def test_cut_key_lists_resolve_to_their_kernels():
    from host_programs import variant_names
    from optical_rl_gym_amd import build
    counts = variant_names().counts
    # per word count: 3 statistics levels x {no cause, CAUSE} wave keys, 3 x {plain, traffic, trace} x {no cause, CAUSE} group keys
    assert (counts["ORLG_WAVE_CUT_KEYS"], counts["ORLG_GROUP_CUT_KEYS"]) == (6 * len(build.WAVE_W), 18 * len(build.WAVE_W))


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


@pytest.mark.parametrize("policy", sorted(CUT_POLICIES))
def test_gated_handle_refuses_in_python(policy):
    with pytest.raises(ValueError, match="gn_gate"):
        _rmsa_shell(gn_gate={"any": 1}).run(policy, 10, actions=np.zeros(3, np.int32))


@pytest.mark.parametrize("policy", ["min_cut_external", "external_mc", "deeprmsa_sap_mc", "sap_ff_gn_mc", "sap_mc_gn", "mc"])
def test_unknown_combinations_have_no_name(policy):
    with pytest.raises(KeyError):
        _rmsa_shell().run(policy, 10)


def test_path_actions_are_checked():
    with pytest.raises(ValueError, match="actions"):
        _rmsa_shell().run("path_mc_external", 1)
    with pytest.raises(ValueError, match="actions"):
        _rmsa_shell().run("path_mc_external", 1, actions=np.zeros((3, 2), np.int32))
    with pytest.raises(TypeError, match="actions"):
        _rmsa_shell().run("path_mc_external", 1, actions=np.zeros(3, np.float64))


def test_buffers_are_checked():
    with pytest.raises(ValueError, match="cause_counts"):
        _rmsa_shell().run("sap_mc", 10, cause_counts=np.zeros((3, 7), np.int32))
    with pytest.raises(ValueError, match="cuts_out"):
        _rmsa_shell().path_min_cuts(cuts_out=np.zeros((3, 4), np.int16))
    with pytest.raises((ValueError, TypeError), match="slots_out"):
        _rmsa_shell().path_min_cuts(slots_out=np.zeros((3, 5), np.int32))


# ---------------------------------------------------------------------------------------- the drop-in heuristic on a stub view
class _StubPath:
    def __init__(self, idp, hops, n):
        self.node_list, self.n = [(idp, i) for i in range(hops + 1)], n


class _StubView:
    """What min_cut_heuristic reads of RMSA-v0: the topology's sizes, its available_slots rows, the link index of an edge, the
    candidates of the pending request with their node lists, get_number_slots."""

    def __init__(self, avail, links_of, ns):
        edges = {}
        self.k_shortest_paths = {(0, 1): [_StubPath(p, len(l), n) for p, (l, n) in enumerate(zip(links_of, ns))]}
        for p, links in enumerate(links_of):
            for i, l in enumerate(links):
                edges.setdefault((p, i), {})[(p, i + 1)] = {"index": int(l)}
        graph = dict(num_spectrum_resources=avail.shape[1], k_paths=len(ns), available_slots=avail)
        self.topology = type("T", (), dict(graph=graph, __getitem__=lambda s, node: edges[node]))()
        self.current_service = type("S", (), dict(source=0, destination=1))()

    def get_number_slots(self, path):
        return path.n


def test_min_cut_heuristic_equals_the_reference_on_a_stub_view():
    topo = load_topology(ref.NSFNET)
    checked = 0
    with device_log_in_oracle():
        o = oracle_env_from_kwargs(topo, bcr.shape_kwargs(100, 20), seed=ref.SEED0)
        for _ in range(120):
            r, avail = o.request(), o.available_slots().copy()
            base = int(topo.pair_path_base[r.src * topo.num_nodes + r.dst])
            links_of = [ref.path_links(topo, base + p) for p in range(topo.k_paths)]
            ns = [bcr.number_slots(r.bit_rate, int(topo.path_se[base + p])) for p in range(topo.k_paths)]
            view = _StubView(avail, links_of, ns)
            for route in ref.ROUTES:
                got = min_cut_heuristic(route)(view)
                assert tuple(got) == ref.propose(avail, topo, r.src, r.dst, r.bit_rate, route)[:2], route
                checked += 1
            o.run("sap_ff", 1, reset_on_done=True, fields=[])
        o.close()
    assert checked == 120 * 4
    with pytest.raises(ValueError, match="route"):
        min_cut_heuristic("path")
