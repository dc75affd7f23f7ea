"""The batches of ``test_gn_shapes_args.py`` and ``test_gpu_gn_shapes.py``: the GN gate's rule launches and the
protection of the running lightpaths on the six shapes of ``gpu_support.MANY_PATHS`` -- more than eight candidate
paths at one to six words per link --, with continuous bit rates, with per-environment loads and on a replayed trace.  Each batch
once: its seeds, its steps, its oracle run (``gn_protect_reference`` / ``gn_rules_reference`` on a (topology, kwargs) pair) and the
figures the CPU module asserts and the GPU module relies on.  Nothing here touches a GPU.
"""
import functools

import numpy as np

import gn_gate_reference as ref
import gn_protect_reference as pref
import gn_rules_reference as gref
from gpu_support import MANY_PATHS, device_log_in_oracle, external_actions, many_paths_kwargs, many_paths_topology, topology

SHAPES = list(MANY_PATHS)
K9, K32, K21, K16, K12, K10 = SHAPES
N_STEPS = 150
MARGIN_DB = 1e-6   # the floor of test_many_paths.py: the GSNR is held to rtol 1e-9, about 2e-8 dB at 20 dB

# ---------------------------------------------------------------------------------------- protection, many paths
# every shape under sap_ff_gn; the three llp_ff shapes under llp_ff too.  Seeds 3 .. 10 (the kwargs' seed onwards), 150 steps
PROTECT_B = 8
PROTECT_BATCHES = [(name, "sap_ff_gn") for name in SHAPES] + [(name, "llp_ff") for name in (K32, K12, K10)]
PROTECT_SEEDS = {}   # (shape, policy) -> the seeds of a batch that had to move off a margin inside MARGIN_DB (none had to)


def protect_seeds(name, policy):
    return list(PROTECT_SEEDS.get((name, policy), range(many_paths_kwargs(name)["seed"], many_paths_kwargs(name)["seed"] + PROTECT_B)))


def protect_runs(case, seeds, policy, n_steps=N_STEPS):
    """pref.run_case of a (topology, kwargs) pair for each seed"""
    return [pref.run_case(case, seed=s, n_steps=n_steps, policy=policy) for s in seeds]


def protect_batch(name, policy, tmp_path):
    topo, kw = many_paths_topology(name, tmp_path), many_paths_kwargs(name)
    return topo, kw, protect_runs((topo, kw), protect_seeds(name, policy), policy)


def protect_figures(runs):
    """Summed over a batch: own checks and refusals, neighbour checks and refusals, steps that took a later path (sap_ff_gn),
    accepted steps on a path >= 8 after a neighbour check, candidates on a path >= 8 the neighbour check refused, the most running
    services at a neighbour check, the own or neighbour margin closest to zero, the largest |GSNR|."""
    out = {k: sum(fig[k] for _, _, fig in runs) for k in ("checks", "rejects", "n_checks", "n_rejects", "later_taken")}
    out["high_accepted_after_check"] = sum(int(((tr["accepted"] != 0) & (tr["act_path"] >= 8) & np.isfinite(tr["margin"])).sum())
                                           for tr, _, _ in runs)
    out["high_neighbour_refused"] = sum(int(((tr["act_path"] >= 8) & (tr["margin"] < 0)).sum()) for tr, _, _ in runs)
    out["n_max_running"] = max(fig["n_max_running"] for _, _, fig in runs)
    out["closest"] = min(fig["any_closest"] for _, _, fig in runs)
    out["max_abs_gsnr"] = max(fig["max_abs_gsnr"] for _, _, fig in runs)
    return out


# ---------------------------------------------------------------------------------------- rule launches, many paths
COMBOS = (("sap", "best", "next_path"), ("sap", "min_cut", "next_path"), ("llp", "last", "check"), ("min_cut", "min_cut", "check"))
RULE_B = 4        # seeds 3 .. 6
# (shape, route, rule, mode) -> (environments, steps) where 4 x 150 gives fewer than 10 later paths or fewer than 2 on a path >= 8
# under next_path (at most 8 seeds or 300 steps)
RULE_SIZES = {
    (K10, "sap", "best", "next_path"): (8, N_STEPS),      # 4 x 150: 1 later path on a path >= 8; 8 x 150: 4
    (K10, "sap", "min_cut", "next_path"): (4, 300),       # 4 x 150: 3, none far_behind; 4 x 300: 6, one far_behind
    (K16, "sap", "best", "next_path"): (8, N_STEPS),      # 4 x 150: none far_behind; 8 x 150: one
}
RULE_BATCHES = [(name,) + combo for name in SHAPES for combo in COMBOS]
QUERY_SHAPES = (K32, K21, K10)   # path_rule_windows before every one-step launch: W = 2, 3 and 6


def rule_size(name, route, rule, mode):
    return RULE_SIZES.get((name, route, rule, mode), (RULE_B, N_STEPS))


def rule_batch(name, route, rule, mode, tmp_path):
    topo, kw = many_paths_topology(name, tmp_path), many_paths_kwargs(name)
    batch, n = rule_size(name, route, rule, mode)
    return topo, kw, gref.run_batch((topo, kw), route, rule, mode, n_steps=n, batch=batch)


# the next_path batches (shape, rule) in which some step takes a path eight or more behind the one it last started over from
# (at the sizes above; k = 12 has none at 8 x 150 nor at 4 x 300 under either rule, k = 10 none under best, k = 9 cannot have one)
FAR_BEHIND = ((K32, "best"), (K32, "min_cut"), (K21, "best"), (K21, "min_cut"), (K16, "best"), (K16, "min_cut"), (K10, "min_cut"))


def far_behind(tr, S):
    """Steps of a next_path run whose taken path lies eight or more behind the path the step last started over from (the path
    behind the last refused one): the rule's scan of the remaining paths reaches its second pass of eight with a start other
    than 0.  [n] bool."""
    out = np.zeros(len(tr["act_path"]), bool)
    for t in np.flatnonzero(tr["later"]):
        p = int(tr["act_path"][t])
        refused = np.flatnonzero(tr["q_slots"][t][:p] < S)   # every path with a window below the taken one was refused
        out[t] = p - (int(refused[-1]) + 1) >= 8
    return out


def rule_figures(runs, S, K):
    """Summed over a batch: checks, steps the gate refused, accepted steps on a path >= 8, query rows with a refused window in a
    column >= 8, later paths taken, later paths on a path >= 8, far_behind steps, the margin closest to zero."""
    out = dict(gref.summed(runs))
    trs = [tr for tr, _, _ in runs]
    out["high_accepted"] = sum(int(((tr["accepted"] != 0) & (tr["act_path"] >= 8) & (tr["act_path"] < K)).sum()) for tr in trs)
    out["high_refused_rows"] = sum(int(((tr["q_slots"][:, 8:] < S) & (tr["q_admitted"][:, 8:] == 0)).any(axis=1).sum()) for tr in trs)
    out["later_high"] = sum(int((tr["later"] & (tr["act_path"] >= 8)).sum()) for tr in trs)
    out["far_behind"] = sum(int(far_behind(tr, S).sum()) for tr in trs)
    return out


# ---------------------------------------------------------------------------------------- the query of rule "first", many paths
# path_rule_windows("first") is the one rule whose query reads the candidates W lanes apart above eight paths (the other rules scan
# eight paths per pass): every shape, RULE_B environments stepped with llp_lf under check, the query before each of N_STEPS steps
class _FirstToo(gref.RuleOracle):
    """A rule oracle that also keeps, per step, the rows of rule "first" (taken just before the step's own rows)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.first = []

    def rows(self, rule):
        self.first.append(super().rows("first"))
        return super().rows(rule)


@functools.lru_cache(maxsize=None)
def _first_query_run(key, seed, n_steps):
    topo, kw = key[0], dict(key[1])
    with device_log_in_oracle():
        go = _FirstToo(topo, kw, ref.case_gate(topo), seed=seed)
        tr = gref._run(go, "llp", "last", "check", n_steps, None)
    o = go.o
    final = dict(available_slots=o.available_slots(), counters=o.counters(), num_running=o.num_running(), current_time=o.current_time())
    go.close()
    tr.update({"f_" + k: np.array([r[k] for r in go.first]) for k in ("slots", "gsnr", "admitted", "margin")})
    for a in tr.values():
        a.setflags(write=False)
    return tr, final


def first_query_batch(name, tmp_path):
    """(topology, kwargs, [(per-step arrays of gn_rules_reference with f_slots, f_gsnr, f_admitted, f_margin added, final state)])"""
    topo, kw = many_paths_topology(name, tmp_path), many_paths_kwargs(name)
    return topo, kw, [_first_query_run(ref.cache_key((topo, kw)), kw["seed"] + i, N_STEPS) for i in range(RULE_B)]


# the agent's path under mode check, aimed at the paths 8 .. K - 1: (shape, rule); RULE_B environments, N_STEPS launches of one step
PATH_CASES = ((K32, "best"), (K16, "min_cut"), (K10, "last"))


def path_batch(name, rule, tmp_path):
    """(topology, kwargs, paths [N_STEPS, RULE_B] -- the path column of external_actions(kind="high_paths") --, the reference's runs)"""
    topo, kw = many_paths_topology(name, tmp_path), many_paths_kwargs(name)
    paths = np.ascontiguousarray(external_actions(topo, MANY_PATHS[name]["S"], N_STEPS, RULE_B, kind="high_paths")[..., 0])
    return topo, kw, paths, gref.run_batch((topo, kw), "path", rule, "check", n_steps=N_STEPS, batch=RULE_B, paths=paths)


# ---------------------------------------------------------------------------------------- continuous bit rates
# NSFNET, S = 320, load 150, rates 100 .. 350 (251 rate indices; the reference's 25 .. 100 refuse nothing at +6 dBm)
CONT_KW = dict(num_spectrum_resources=320, load=150, mean_service_holding_time=ref.HOLDING_TIME, episode_length=ref.EPISODE_LENGTH, seed=2,
               bit_rate_selection="continuous", bit_rate_lower_bound=100, bit_rate_higher_bound=350)
CONT_B, CONT_STEPS, CONT_POLICY = 4, 300, "sap_ff"   # seeds 2 .. 5
CONT_WARMUP, CONT_QUERY_STEPS = 200, 100   # the query run: 200 steps of sap_ff fill the network, then 100 steps with the queries


def continuous_case():
    return topology(pref.NSF), CONT_KW


def continuous_protect_runs():
    return pref.run_batch(continuous_case(), n_steps=CONT_STEPS, policy=CONT_POLICY, batch=CONT_B)


def continuous_gated_runs():
    return [ref.run_case(continuous_case(), seed=CONT_KW["seed"] + i, n_steps=CONT_STEPS, policy=CONT_POLICY) for i in range(CONT_B)]


@functools.lru_cache(maxsize=None)
def continuous_query_run(seed, n_steps=CONT_QUERY_STEPS):
    """One gated environment, after CONT_WARMUP steps of sap_ff, stepped with sap_bf under next_path; before every step the path_ff_gn mask with its GSNR row
    (gn_candidates_reference) and the rows of path_rule_windows("best").  Per-step arrays as gn_rules_reference.run_case gives
    them, with path_ff_gn / path_ff_gsnr added, and the final state.  Read-only by agreement."""
    topo, kw = continuous_case()
    with device_log_in_oracle():
        go = gref.RuleOracle(topo, dict(kw), ref.case_gate(topo), seed=seed)
        masks = {"path_ff_gn": [], "path_ff_gsnr": [], "mask_margin": []}
        cols = {k: [] for k in gref.STEP_FIELDS + ("request", "later") + tuple("q_" + k for k in gref.ROW_FIELDS)}
        for _ in range(CONT_WARMUP):
            go.step(*go.propose(CONT_POLICY))
        for _ in range(n_steps):
            go._known = {}   # (the rows of the step before: the shadow has changed since)
            c = go.candidates()
            masks["path_ff_gn"].append(c["path_ff_gn"]); masks["path_ff_gsnr"].append(c["path_ff_gsnr"]); masks["mask_margin"].append(c["margin"])
            rows = go.rows("best")
            p, s, _, later = go.propose_rule("sap", "best", "next_path", rows)
            row = go.step(p, s)
            for k in gref.STEP_FIELDS + ("request",):
                cols[k].append(row[k])
            cols["later"].append(bool(later and row["accepted"]))
            for k in gref.ROW_FIELDS:
                cols["q_" + k].append(rows[k])
    o = go.o
    final = dict(available_slots=o.available_slots(), counters=o.counters(), num_running=o.num_running(), current_time=o.current_time())
    go.close()
    tr = {k: np.array(v) for k, v in dict(cols, **masks).items()}
    for a in tr.values():
        a.setflags(write=False)
    return tr, final


# ---------------------------------------------------------------------------------------- per-environment loads, trace
SWEEP_LOADS, SWEEP_SEEDS, SWEEP_SEED0, SWEEP_STEPS = (50, 150), 4, 2, 300
SWEEP_KW = dict(num_spectrum_resources=320, mean_service_holding_time=ref.HOLDING_TIME, episode_length=ref.EPISODE_LENGTH)
SWEEP_POLICY = "sap_ff"


def sweep_case(load):
    return topology(pref.NSF), dict(SWEEP_KW, load=load, seed=SWEEP_SEED0)


def sweep_runs(protect):
    """The oracle of every environment of the sweep handle, group-major: load 50 on seeds 2 .. 5, then load 150 on the same"""
    run = pref.run_case if protect else ref.run_case
    return [run(sweep_case(load), seed=SWEEP_SEED0 + i, n_steps=SWEEP_STEPS, policy=SWEEP_POLICY) for load in SWEEP_LOADS for i in range(SWEEP_SEEDS)]


TRACE_CASE, TRACE_B, TRACE_STEPS = "nsfnet_s320_l150_sapff", 4, 300   # a case of gn_protect_reference.CASES, held to the oracle there
