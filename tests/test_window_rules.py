"""Most-used assignment and the best-window-over-all-paths route (``include/orlg.h`` ``orlg_step_window``, ``orlg_slot_usage``,
``orlg_path_most_used``), what needs no GPU: the numpy restatement of the definitions (``usage_reference.py``)
against a brute force over every (start, link, slot); that MOST_USED really differs from first fit and the route from sap on the
shapes ``test_gpu_window_rules.py`` compares, so that none of its comparisons is vacuous; the entry points, their prototypes
and the name table; that the pinned tables are what they were; the new key lists; the refusals that come before the library is
called; and the drop-in heuristic on a stub view.

Measured with the oracle under the device logarithm (8 environments x 200 steps, minimum over the environments; the printed
lines of test_the_new_names_differ): accepted steps on which MOST_USED's slot differs from first_full's on the same route --
sap_mu 50 / 68 / 95 at S = 64 / 100 / 320, sp_mu 32 / 37 / 74, llp_mu 43 / 54 / 102, any_mu 42 / 67 / 92; steps on which
any_ff_full's path differs from sap_ff_full's -- 11 / 13 / 35."""
import os
import subprocess

import numpy as np
import pytest

import block_cause_reference as bcr
import usage_reference as ref
from conftest import ROOT, load_topology, oracle_env_from_kwargs
from gpu_support import device_log_in_oracle
from optical_rl_gym_amd import WINDOW_POLICIES, BatchedRMSAEnv, _lib, window_heuristic

NEW = {"orlg_step_window": 8, "orlg_slot_usage": 2, "orlg_path_most_used": 3}


# ---------------------------------------------------------------------------------------- the reference against brute force
def _brute_usage(avail):
    E, S = avail.shape
    return [sum(1 for l in range(E) if not avail[l][t]) for t in range(S)]


def _brute_windows(avail, links, n):
    """every window of the path with its usage and the bounds of the block around it, slot by slot"""
    E, S = avail.shape
    free = lambda t: all(avail[l][t] for l in links)
    out = []
    for s in range(0, S - n + 1):
        if all(free(t) for t in range(s, s + n)):
            usage = sum(1 for t in range(s, s + n) for l in range(E) if not avail[l][t])
            lo, hi = s, s + n
            while lo > 0 and free(lo - 1):
                lo -= 1
            while hi < S and free(hi):
                hi += 1
            out.append((s, usage, lo, hi - lo))
    return out


def _brute_proposal(wins, n, rule):
    if not wins:
        return None
    key = {"first_full": lambda w: (w[0],), "last": lambda w: (-w[0],), "best": lambda w: (w[3], w[2]),
           "exact": lambda w: (int(w[3] != n), w[2]), "most_used": lambda w: (-w[1], w[0])}[rule]
    w = min(wins, key=key)
    return key(w), (w[0] if rule in ("first_full", "last", "most_used") else w[2])


@pytest.mark.parametrize("S", [64, 100, 130, 320])
def test_reference_against_brute_force_on_random_arrays(S):
    rng = np.random.default_rng(S)
    seen = dict(at0=0, at_end=0, long=0, mu_not_lowest=0, none=0, tie=0, any_not_first=0)
    for trial in range(60):
        E, k = int(rng.integers(3, 9)), 3
        n_of = [int(rng.integers(64, 90)) if trial % 5 == 0 and S > 100 else int(rng.integers(1, 10)) for _ in range(k)]
        avail = (rng.random((E, S)) > rng.choice([0.02, 0.06, 0.15])).astype(np.uint8)
        paths = [sorted(rng.choice(E, int(rng.integers(1, 4)), replace=False).tolist()) for _ in range(k)]
        if trial % 3 == 0:
            avail[paths[0], :n_of[0]] = 1
        if trial % 4 == 0:
            avail[paths[0], S - n_of[0]:] = 1
            if trial % 8 == 0:   # ... and used on every other link there: the most-used window of the path
                avail[[l for l in range(E) if l not in paths[0]], S - n_of[0]:] = 0
        if trial % 7 == 0:
            avail[:] = 1      # an empty network: every usage 0
        U = ref.slot_usage(avail)
        assert U.tolist() == _brute_usage(avail)
        per_rule = {rule: [] for rule in ref.RULES}
        for links, n in zip(paths, n_of):
            A = avail[links].min(axis=0)
            wins = _brute_windows(avail, links, n)
            assert ref.window_usage(U, [w[0] for w in wins], n).tolist() == [w[1] for w in wins]
            for rule in ref.RULES:
                want = _brute_proposal(wins, n, rule)
                assert ref.proposal(A, U, n, rule) == want, (rule, n)
                per_rule[rule].append(want)
            if not wins:
                seen["none"] += 1
                continue
            mu = _brute_proposal(wins, n, "most_used")
            seen["at0"] += mu[1] == 0
            seen["at_end"] += mu[1] == S - n
            seen["long"] += n >= 64
            seen["mu_not_lowest"] += mu[1] != wins[0][0]
            seen["tie"] += sum(1 for w in wins if w[1] == -mu[0][0]) > 1
        for rule in ref.RULES:   # the route: the best rank, ties to the lowest path
            have = [p for p in range(k) if per_rule[rule][p]]
            if have:
                seen["any_not_first"] += min(have, key=lambda p: (per_rule[rule][p][0], p)) != have[0]
    print(S, seen)
    assert all(seen[c] for c in ("at0", "at_end", "mu_not_lowest", "none", "tie", "any_not_first")), seen
    if S > 100:
        assert seen["long"]


def test_reference_edge_cases():
    one = lambda *rows: np.array(rows, np.uint8)
    # two links; the path is link 0.  Slot 2 is used on link 1 only: a slot occupied on every link but the path's counts
    avail = one([1, 1, 1, 1, 1, 1], [1, 1, 0, 1, 1, 1])
    U = ref.slot_usage(avail)
    assert U.tolist() == [0, 0, 1, 0, 0, 0]
    assert ref.proposal(avail[0], U, 2, "most_used") == ((-1, 1), 1)       # [1, 3) and [2, 4) tie at 1: the lower start
    assert ref.proposal(avail[0], U, 2, "first_full") == ((0,), 0) and ref.proposal(avail[0], U, 2, "last") == ((-4,), 4)
    assert ref.proposal(avail[0], ref.slot_usage(one([1] * 6, [1] * 6)), 2, "most_used") == ((0, 0), 0)   # an empty network: the first window
    assert ref.proposal(one([1, 0, 1])[0], U[:3], 2, "most_used") is None and ref.proposal(one([1, 1])[0], U[:2], 3, "best") is None
    # exact: a block of exactly n before any other; best: the shortest block
    A = one([1, 1, 1, 0, 1, 1, 0, 1, 1, 1])[0]
    Z = np.zeros(10, np.int64)
    assert ref.proposal(A, Z, 2, "exact") == ((0, 4), 4) and ref.proposal(A, Z, 3, "exact") == ((0, 0), 0)
    assert ref.proposal(A, Z, 1, "exact") == ((1, 0), 0) and ref.proposal(A, Z, 1, "best") == ((2, 4), 4)


@pytest.mark.parametrize("S,load", [(64, 10), (100, 20)])
def test_reference_against_the_oracle_queries(S, load):
    """Windows slot by slot with is_path_free; the usage from the links' own rows; path_most_used and propose on top."""
    topo = load_topology(ref.NSFNET)
    kw = bcr.shape_kwargs(S, load)
    with device_log_in_oracle():
        o = oracle_env_from_kwargs(topo, kw, seed=ref.SEED0)
        for _ in range(ref.N_STEPS):
            r, avail = o.request(), o.available_slots()
            E = avail.shape[0]
            usage, slots = ref.path_most_used(avail, topo, r.src, r.dst, r.bit_rate)
            per_path = []
            for p, (A, n) in enumerate(ref.candidates(avail, topo, r.src, r.dst, r.bit_rate)):
                assert n == o.number_slots(p)
                free = [s for s in range(S) if o.is_path_free(p, s, n)]
                want = [(s, sum(1 for t in range(s, s + n) for l in range(E) if not avail[l][t])) for s in free]
                best = min(want, key=lambda su: (-su[1], su[0])) if want else None
                assert (usage[p], slots[p]) == ((best[1], best[0]) if best else (-1, S))
                per_path.append(best)
            have = [p for p, b in enumerate(per_path) if b]
            rej = (topo.k_paths, S)
            assert ref.propose(avail, topo, r.src, r.dst, r.bit_rate, "sp", "most_used") == ((0, per_path[0][0]) if per_path[0] else rej)
            assert ref.propose(avail, topo, r.src, r.dst, r.bit_rate, "sap", "most_used") == ((have[0], per_path[have[0]][0]) if have else rej)
            p_any = min(have, key=lambda p: (-per_path[p][1], per_path[p][0], p)) if have else None
            assert ref.propose(avail, topo, r.src, r.dst, r.bit_rate, "any", "most_used") == ((p_any, per_path[p_any][0]) if have else rej)
            for a in (-1, 0, 3, 5, 8):
                ok = 0 <= a < topo.k_paths and per_path[a]
                assert ref.propose(avail, topo, r.src, r.dst, r.bit_rate, "path", "most_used", a) == ((a, per_path[a][0]) if ok else rej)
            o.run("sap_ff", 1, reset_on_done=True, fields=[])
        o.close()


# ---------------------------------------------------------------------------------------- the new names differ; the causes
@pytest.mark.parametrize("name", ref.LAUNCHED)
@pytest.mark.parametrize("S,load", ref.SHAPES)
def test_the_new_names_differ(S, load, name):
    tr = ref.stacked(S, load, name)
    route, rule = ref.NAMES[name]
    k = 5
    chosen = tr["act_path"] < k
    acc = tr["accepted"] == 1
    slot_differs = (acc & (tr["act_slot"] != tr["ff_slot"])).sum(axis=0)      # per environment
    path_differs = (tr["act_path"] != tr["sap_path"]).sum(axis=0)
    print(S, name, "slot differs from first_full's: min", int(slot_differs.min()), "| path differs from sap's: min", int(path_differs.min()),
          "| blocking", 1 - tr["accepted"].mean())
    if rule == "most_used":
        assert slot_differs.min() >= 1, (S, name, slot_differs)
    if name == "any_ff_full":
        assert path_differs.min() >= 1, (S, path_differs)
    # a proposed window is a free window: accepted iff a path was chosen
    assert np.array_equal(acc, chosen) and np.array_equal(tr["cause"] == bcr.ACCEPTED, acc)
    assert np.array_equal(tr["usage"] >= 0, chosen)
    if route == "sp":
        assert tr["cause"].max() <= bcr.C_POLICY
    else:   # sap / llp / any take any window of any path: they refuse only where no path has one
        assert tr["cause"].max() <= bcr.C_ALIGNMENT, (S, name, np.bincount(tr["cause"].ravel()))


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
    assert "#define ORLG_ROUTE_BEST_WINDOW 101" in header and "#define ORLG_RULE_MOST_USED 100" in header
    assert (_lib.ROUTE_BEST_WINDOW, _lib.RULE_MOST_USED) == (101, 100)


def test_the_pinned_tables_are_what_they_were():
    header = open(os.path.join(ROOT, "include", "orlg.h")).read()
    assert "ORLG_NUM_ASSIGN_RULES = 5" in header and "ORLG_ASSIGN_MOST_USED" not in header and "ORLG_POLICY_BEST_WINDOW" not in header
    assert "#define ORLG_ROUTE_FEWEST_CUTS 100" in header
    device = open(os.path.join(ROOT, "optical-rl-gym-qot-aware_amd", "csrc", "orlg_device.h")).read()
    assert "ORLG_ASSIGN_MIN_CUT = 5" in device and "ORLG_POLICY_MIN_CUT = 8" in device
    assert device.index("ORLG_POLICY_MIN_CUT = 8") < device.index("ORLG_POLICY_BEST_WINDOW = 9")
    assert device.index("ORLG_ASSIGN_MIN_CUT = 5") < device.index("ORLG_ASSIGN_MOST_USED = 6")
    P = _lib.POLICIES
    assert _lib.ASSIGN_RULES == ("first", "first_full", "last", "best", "exact")
    assert len(_lib.ASSIGN_POLICIES) == 16
    assert _lib.CUT_POLICIES == {"sp_mc": P["sp_ff"], "sap_mc": P["sap_ff"], "llp_mc": P["llp_ff"], "min_cut": 100,
                                 "path_mc_external": P["path_ff_external"]}
    assert P == {"external": -1, "sp_ff": 0, "sap_ff": 1, "llp_ff": 2, "deeprmsa_sp_ff": 3, "deeprmsa_sap_ff": 4, "deeprmsa_external": 5,
                 "path_ff_external": 6, "sap_ff_gn": 7}


def test_a_null_handle_answers_first():
    L = _lib.load()
    for route, rule in ((1, 2), (_lib.ROUTE_BEST_WINDOW, _lib.RULE_MOST_USED), (99, 1), (1, 0), (1, 99)):
        assert L.orlg_step_window(None, route, rule, 10, None, 1, None, None) == -1 and b"null handle" in L.orlg_last_error()
    assert L.orlg_slot_usage(None, None) == -1 and b"null handle" in L.orlg_last_error()
    assert L.orlg_path_most_used(None, None, None) == -1 and b"null handle" in L.orlg_last_error()


def test_policy_name_table():
    P, R = _lib.POLICIES, _lib.ASSIGN_RULES
    assert _lib.WINDOW_POLICIES is WINDOW_POLICIES
    mu, bw = _lib.RULE_MOST_USED, _lib.ROUTE_BEST_WINDOW
    assert WINDOW_POLICIES == {"sp_mu": (P["sp_ff"], mu), "sap_mu": (P["sap_ff"], mu), "llp_mu": (P["llp_ff"], mu),
                               "path_mu_external": (P["path_ff_external"], mu), "any_ff_full": (bw, R.index("first_full")),
                               "any_lf": (bw, R.index("last")), "any_bf": (bw, R.index("best")), "any_ef": (bw, R.index("exact")),
                               "any_mu": (bw, mu)}
    assert not set(WINDOW_POLICIES) & (set(P) | set(_lib.ASSIGN_POLICIES) | set(_lib.CUT_POLICIES))
    for name in WINDOW_POLICIES:       # policy_ids answers for the names it always answered for
        with pytest.raises(KeyError):
            _lib.policy_ids(name)
    for name, pid in P.items():
        assert _lib.policy_ids(name) == (pid, 0)
    assert set(ref.NAMES) == set(WINDOW_POLICIES)
    assert bw not in P.values() and mu not in range(len(R))


def test_window_key_lists_resolve_to_their_kernels():
    from host_programs import variant_names
    from optical_rl_gym_amd import build
    counts = variant_names().counts
    # per word count: 3 statistics levels x {no cause, CAUSE} wave keys, 3 x {plain, traffic, trace} x {no cause, CAUSE} group keys
    assert (counts["ORLG_WAVE_USAGE_KEYS"], counts["ORLG_GROUP_USAGE_KEYS"]) == (6 * len(build.WAVE_W), 18 * len(build.WAVE_W))


# ---------------------------------------------------------------------------------------- refusals before the library is called
class _NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although the arguments are wrong")


def _rmsa_shell(B=3, k=5, S=100, gn_gate=None):
    env = BatchedRMSAEnv.__new__(BatchedRMSAEnv)
    env.L, env.h = _NoLibrary(), None
    env.batch_size, env.k_paths, env.num_spectrum_resources, env.gn_gate = B, k, S, gn_gate
    return env


@pytest.mark.parametrize("policy", sorted(WINDOW_POLICIES))
def test_gated_handle_refuses_in_python(policy):
    with pytest.raises(ValueError, match="gn_gate"):
        _rmsa_shell(gn_gate={"any": 1}).run(policy, 10, actions=np.zeros(3, np.int32))


@pytest.mark.parametrize("policy", ["any_mu_external", "external_mu", "deeprmsa_sap_mu", "sap_ff_gn_mu", "sap_mu_gn", "mu", "any_ff",
                                    "any_mc", "path_any_external"])
def test_unknown_combinations_have_no_name(policy):
    with pytest.raises(KeyError):
        _rmsa_shell().run(policy, 10)


def test_path_actions_are_checked():
    with pytest.raises(ValueError, match="actions"):
        _rmsa_shell().run("path_mu_external", 1)
    with pytest.raises(ValueError, match="actions"):
        _rmsa_shell().run("path_mu_external", 1, actions=np.zeros((3, 2), np.int32))
    with pytest.raises(TypeError, match="actions"):
        _rmsa_shell().run("path_mu_external", 1, actions=np.zeros(3, np.float64))


def test_buffers_are_checked():
    with pytest.raises(ValueError, match="cause_counts"):
        _rmsa_shell().run("any_mu", 10, cause_counts=np.zeros((3, 7), np.int32))
    with pytest.raises(ValueError, match="out"):
        _rmsa_shell().slot_usage(out=np.zeros((3, 99), np.uint8))
    with pytest.raises((ValueError, TypeError), match="out"):
        _rmsa_shell().slot_usage(out=np.zeros((3, 100), np.int32))
    with pytest.raises(ValueError, match="usage_out"):
        _rmsa_shell().path_most_used(usage_out=np.zeros((3, 4), np.int32))
    with pytest.raises((ValueError, TypeError), match="usage_out"):
        _rmsa_shell().path_most_used(usage_out=np.zeros((3, 5), np.int16))
    with pytest.raises((ValueError, TypeError), match="slots_out"):
        _rmsa_shell().path_most_used(slots_out=np.zeros((3, 5), np.int32))


# ---------------------------------------------------------------------------------------- the drop-in heuristic on a stub view
class _StubPath:
    def __init__(self, idp, links, n):
        self.idp, self.links, self.n = idp, links, n


class _StubView:
    """What window_heuristic reads of RMSA-v0: the topology's sizes and its available_slots rows, the candidates of the pending
    request, get_available_slots, get_number_slots."""

    def __init__(self, avail, links_of, ns):
        self.k_shortest_paths = {(0, 1): [_StubPath(p, l, n) for p, (l, n) in enumerate(zip(links_of, ns))]}
        graph = dict(num_spectrum_resources=avail.shape[1], k_paths=len(ns), available_slots=avail)
        self.topology = type("T", (), dict(graph=graph))()
        self.current_service = type("S", (), dict(source=0, destination=1))()
        self.avail = avail

    def get_number_slots(self, path):
        return path.n

    def get_available_slots(self, path):
        return self.avail[path.links].min(axis=0)


def test_window_heuristic_equals_the_reference_on_a_stub_view():
    topo = load_topology(ref.NSFNET)
    checked = 0
    with device_log_in_oracle():
        o = oracle_env_from_kwargs(topo, bcr.shape_kwargs(100, 20), seed=ref.SEED0)
        for _ in range(80):
            r, avail = o.request(), o.available_slots().copy()
            base = int(topo.pair_path_base[r.src * topo.num_nodes + r.dst])
            links_of = [np.asarray(topo.path_links[topo.path_link_off[base + p]:topo.path_link_off[base + p + 1]], np.int64)
                        for p in range(topo.k_paths)]
            ns = [bcr.number_slots(r.bit_rate, int(topo.path_se[base + p])) for p in range(topo.k_paths)]
            view = _StubView(avail, links_of, ns)
            for route in ref.ROUTES:
                for rule in ref.RULES:
                    got = window_heuristic(route, rule)(view)
                    assert tuple(got) == ref.propose(avail, topo, r.src, r.dst, r.bit_rate, route, rule), (route, rule)
                    checked += 1
            o.run("sap_ff", 1, reset_on_done=True, fields=[])
        o.close()
    assert checked == 80 * 20
    with pytest.raises(ValueError, match="route"):
        window_heuristic("path", "most_used")
    with pytest.raises(ValueError, match="rule"):
        window_heuristic("any", "first")
