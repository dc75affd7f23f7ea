"""The CPU reference of the assignment rules behind the GN-model admission check (``include/orlg.h`` ``orlg_step_rule_gn`` /
``orlg_gn_path_windows``): the candidate oracle of ``gn_candidates_reference.py`` driven with the proposals of
``assign_reference.propose`` and ``cut_reference.propose``, in both modes.  Helper module of ``test_gn_rules_args.py`` and
``test_gpu_gn_rules.py``; nothing here touches a GPU.

Per step, before anything changes: the query's three rows -- the rule's window of every candidate path, its GSNR against the
shadow, admitted or not --, all of a step's checks evaluated by ONE ``oracle.gn_osnr`` call; then the proposal: mode ``check`` the
route's and the rule's (exactly what they propose without a gate), mode ``next_path`` the first path whose window is admitted,
else the first path that has a window (the step refuses it), else the rejection.  ``GatedOracle.step`` then runs the check on the
proposal (the value comes from the step's rows) and steps the oracle.
"""
import functools

import numpy as np

import assign_reference as ar
import cut_reference as cr
import gn_candidates_reference as gc
import gn_gate_reference as ref
import oracle as orc
from gpu_support import device_log_in_oracle

RULES = ("first", "first_full", "last", "best", "exact", "min_cut")   # the query's; the step's: all but "first"
MODES = ("check", "next_path")
SUFFIX = dict(ar.SUFFIX, min_cut="mc")
B = 4           # environments per case: seeds case seed + 0 .. 3
N_STEPS = 300   # (100 at S = 512)


def policy_name(route, rule):
    """The name run(..., gn_rule=) takes for a route (sp, sap, llp, min_cut, path) and a rule"""
    if rule == "min_cut":
        return cr.POLICY[route]
    return ar.policy_name(route, rule)


class RuleOracle(gc.CandidateOracle):
    """A candidate oracle that answers, before a step, for the rule's window of every candidate path."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._known = {}   # (links, s, n) -> GSNR of this step's rows

    def gsnr(self, links, s, n):
        key = (tuple(links), s, n)
        return self._known[key] if key in self._known else super().gsnr(links, s, n)

    def _gsnr_many(self, checks):
        """GSNR [dB] of the windows [(links, s, n)] against the shadow, one call of the oracle's routine"""
        g = self.gate
        by_link = {}
        for (_, ls, f_i, b_i, se_i) in self.shadow:   # provision order
            for l in ls:
                by_link.setdefault(l, []).append((b_i, f_i, se_i))
        link_off, span_off, svc_off, lengths, sb, sf, sse, bw, fc = [0], [0], [0], [], [], [], [], [], []
        for links, s, n in checks:
            b, f = self._window(s, n)
            bw.append(b); fc.append(f)
            for l in links:
                ns = int(g["link_num_spans"][l])
                lengths += [float(g["link_span_length_km"][l])] * ns
                span_off.append(len(lengths))
                for b_i, f_i, se_i in by_link.get(l, ()):
                    sb.append(b_i); sf.append(f_i); sse.append(se_i)
                svc_off.append(len(sb))
            link_off.append(len(span_off) - 1)
        n_sp = len(lengths)
        batch = dict(check_link_off=link_off, link_span_off=span_off, link_svc_off=svc_off, bandwidth=bw, center_frequency=fc,
                     launch_power=[g["launch_power_density_w_hz"] * b for b in bw], span_length_km=lengths,
                     span_attenuation=[g["attenuation_normalized"]] * n_sp, span_noise_figure=[g["noise_figure"]] * n_sp,
                     svc_bandwidth=sb, svc_center_frequency=sf, svc_se=sse, svc_is_self=[0] * len(sb))
        return orc.gn_osnr(batch)

    def rows(self, rule):
        """The pending request against what is lit now: dict of slots [K] int16 (S = the path has no window), gsnr [K] float64
        (NaN there), admitted [K] uint8, margin (the smallest |GSNR - threshold| of the step, inf without a window), ff_slots [K]
        (the reference's first fit of the path, -1 = none).  Keeps the step's values for GatedOracle.step."""
        o, K, S = self.o, self.K, self.S
        now = o.current_time()
        self.shadow = [e for e in self.shadow if not e[0] <= now]   # what step() drops first: the services due by now
        r, avail = o.request(), o.available_slots()
        cand = cr.candidates(avail, self.topo, r.src, r.dst, r.bit_rate)
        out = dict(slots=np.full(K, S, np.int16), gsnr=np.full(K, np.nan), admitted=np.zeros(K, np.uint8), margin=np.inf,
                   ff_slots=np.full(K, -1, np.int32))
        checks, thr = [], []
        for p, (rws, n) in enumerate(cand):
            assert n == o.number_slots(p)
            A = rws.min(axis=0)
            if rule == "min_cut":
                got = cr.min_cut_window(rws, n)
                s = None if got is None else got[1]
            else:
                s = ar.rule_slot(A, n, rule)
            ff = ar.rule_slot(A, n, "first")
            out["ff_slots"][p] = -1 if ff is None else ff
            if s is None:
                continue
            assert o.is_path_free(p, s, n)
            links, se = self._path(p)
            out["slots"][p] = s
            checks.append((p, links, s, n))
            thr.append(float(self.gate["thresholds_db"][se - 1]))
        self._known = {}
        if checks:
            g = self._gsnr_many([c[1:] for c in checks])
            for (p, links, s, n), v, t in zip(checks, g, thr):
                out["gsnr"][p], out["admitted"][p] = v, v >= t
                out["margin"] = min(out["margin"], abs(float(v) - t))
                self._known[(tuple(links), s, n)] = float(v)
        return out

    def propose_rule(self, route, rule, mode, rows, given=None):
        """(path, slot, checks the step runs, a later path taken?)"""
        o, K, S = self.o, self.K, self.S
        r, avail = o.request(), o.available_slots()
        if mode == "check":
            if rule == "min_cut":
                p, s = cr.propose(avail, self.topo, r.src, r.dst, r.bit_rate, route, given)[:2]
            else:
                p, s = ar.propose(avail, self.topo, r.src, r.dst, r.bit_rate, route, rule, given)
            assert p == K or int(rows["slots"][p]) == s   # the route takes the rule's window of its path
            return int(p), int(s), int(p < K), False
        assert mode == "next_path" and route == "sap"
        has, ok = np.flatnonzero(rows["slots"] < S), np.flatnonzero(rows["admitted"])
        if has.size == 0:
            return K, S, 0, False
        if ok.size == 0:
            return int(has[0]), int(rows["slots"][has[0]]), int(has.size), False
        p = int(ok[0])
        return p, int(rows["slots"][p]), int(np.sum(has <= p)), p != int(has[0])


STEP_FIELDS = ("act_path", "act_slot", "accepted", "done", "gsnr", "reward")
ROW_FIELDS = ("slots", "gsnr", "admitted", "margin", "ff_slots")


def _run(go, route, rule, mode, n_steps, paths):
    cols = {k: [] for k in STEP_FIELDS + ("checks", "later", "ff_slot", "request") + tuple("q_" + k for k in ROW_FIELDS)}
    for t in range(n_steps):
        rows = go.rows(rule)
        p, s, checks, later = go.propose_rule(route, rule, mode, rows, None if paths is None else int(paths[t]))
        row = go.step(p, s)
        if mode == "next_path" and checks and not row["accepted"]:
            assert not rows["admitted"].any()
        for k in STEP_FIELDS + ("request",):
            cols[k].append(row[k])
        cols["checks"].append(checks)
        cols["later"].append(bool(later and row["accepted"]))
        cols["ff_slot"].append(int(rows["ff_slots"][p]) if p < go.K else -1)
        for k in ROW_FIELDS:
            cols["q_" + k].append(rows[k])
    return {k: np.array(v) for k, v in cols.items()}


def run_case(case, route, rule, mode, seed=None, n_steps=N_STEPS, gate_items=(), paths=None, policy=None):
    """One environment of a case -- a name of gn_gate_reference.CASES (seed: the case's own by default) or a (topology, kwargs)
    pair -- under route, rule and mode, run once per process and shared: (per-step arrays -- STEP_FIELDS, checks, later, ff_slot
    (the reference's first fit of the chosen path, -1 = none or rejected), request, and the query's rows of the request pending
    BEFORE the step as q_slots, q_gsnr, q_admitted, q_margin, q_ff_slots --, final state, figures).  paths: the agent's path per step
    for route "path" (a tuple).  Read-only by agreement."""
    return _run_case(ref.cache_key(case), route, rule, mode, seed, n_steps, tuple(gate_items), None if paths is None else tuple(int(x) for x in paths))


@functools.lru_cache(maxsize=None)
def _run_case(key, route, rule, mode, seed, n_steps, gate_items, paths):
    topo, kw, _ = ref.resolve_case(key if isinstance(key, str) else (key[0], dict(key[1])), "unused")
    with device_log_in_oracle():
        go = RuleOracle(topo, kw, ref.case_gate(topo, **dict(gate_items)), seed=seed)
        tr = _run(go, route, rule, mode, n_steps, paths)
    o = go.o
    final = dict(available_slots=o.available_slots(), counters=o.counters(), num_running=o.num_running(), current_time=o.current_time())
    checked = ~np.isnan(tr["gsnr"])
    figures = dict(checks=int(tr["checks"].sum()), refused=int(np.sum(checked & (tr["accepted"] == 0))), later=int(tr["later"].sum()),
                   other_window=int(np.sum((tr["act_path"] < topo.k_paths) & (tr["act_slot"] != tr["ff_slot"]))),
                   closest=float(np.min(tr["q_margin"])), provisions=int(tr["accepted"].sum()),
                   admitted_values=tuple(sorted(set(np.unique(tr["q_admitted"][tr["q_slots"] < int(kw["num_spectrum_resources"])]).tolist()))))
    go.close()
    for a in tr.values():
        a.setflags(write=False)
    return tr, final, figures


def case_seed(case):
    return ref.CASES[case]["seed"] if isinstance(case, str) else case[1]["seed"]


def run_batch(case, route, rule, mode, n_steps=N_STEPS, batch=B, paths=None, **kw):
    """run_case for the seeds of the case + 0 .. batch - 1: a list of its results.  paths [n, batch] for route "path"."""
    seed = case_seed(case)
    return [run_case(case, route, rule, mode, seed=seed + i, n_steps=n_steps, paths=None if paths is None else paths[:, i], **kw)
            for i in range(batch)]


def summed(results):
    """The figures of run_batch summed over its environments (closest: the minimum; admitted_values: the union)"""
    figs = [r[2] for r in results]
    out = {k: sum(f[k] for f in figs) for k in ("checks", "refused", "later", "other_window", "provisions")}
    out["closest"] = min(f["closest"] for f in figs)
    out["admitted_values"] = tuple(sorted(set().union(*[f["admitted_values"] for f in figs])))
    return out


# ---------------------------------------------------------------------------------------- the cases of test_gpu_gn_rules.py
# name -> case (a name of gn_gate_reference.CASES, or None = the W = 1 shape below), route, rule, mode, steps, words per link, and
# the gate's keywords beyond gn_gate_reference.GATE_KWARGS.  test_gn_rules_args.py holds the oracle alone to the conditions the GPU
# comparisons rest on, for each of them; every rule, both modes and the word counts 1, 2, 5 and 8 occur
W1_KWARGS = dict(num_spectrum_resources=64, load=10, mean_service_holding_time=ref.HOLDING_TIME, episode_length=ref.EPISODE_LENGTH, seed=10)
GPU_CASES = {}


def gpu_case(name):
    """What run_case / resolve_case take for a name of GPU_CASES"""
    from gpu_support import topology
    c = GPU_CASES[name]
    return c["case"] if c["case"] is not None else (topology(ar.NSFNET), W1_KWARGS)


def _case(case, route, rule, mode, W, n=N_STEPS, levels=False, **gate):
    return dict(case=case, route=route, rule=rule, mode=mode, n=n, W=W, levels=levels, gate=tuple(sorted(gate.items())))


GPU_CASES.update({
    # nsfnet, S = 100: two words per link, the last one not full
    "w2_sap_last_check": _case("nsfnet_s100_l20_spff", "sap", "last", "check", 2, levels=True),
    "w2_llp_exact_check": _case("nsfnet_s100_l20_spff", "llp", "exact", "check", 2),
    "w2_sp_best_check": _case("nsfnet_s100_l20_spff", "sp", "best", "check", 2),
    # nsfnet, S = 320: five words
    "w5_l150_sap_best_next": _case("nsfnet_s320_l150_sapff", "sap", "best", "next_path", 5, levels=True),
    "w5_l150_mincut_route_check": _case("nsfnet_s320_l150_sapff", "min_cut", "min_cut", "check", 5),
    "w5_l50_sap_mincut_next": _case("nsfnet_s320_l50_sapff", "sap", "min_cut", "next_path", 5, levels=True),
    # jpn12, S = 320: the later paths
    "jpn12_sap_last_next": _case("jpn12_s320_l150_sapff", "sap", "last", "next_path", 5),
    "jpn12_sap_first_full_next": _case("jpn12_s320_l150_sapff", "sap", "first_full", "next_path", 5),
    # ring34, S = 100: 238 links, link sets of four mask words
    "ring34_sap_best_check": _case("ring34_s100_l60_sapff", "sap", "best", "check", 2),
    "ring34_llp_mincut_check": _case("ring34_s100_l60_sapff", "llp", "min_cut", "check", 2),
    # ring36, S = 512: eight words, candidates of up to 14 hops
    "ring36_w8_check": _case("ring36_s512_l500_sapff", "sap", "min_cut", "check", 8, n=100),
    "ring36_w8_next": _case("ring36_s512_l500_sapff", "sap", "exact", "next_path", 8, n=100),
    # nsfnet, S = 64: one word
    "w1_sap_last_check": _case(None, "sap", "last", "check", 1),
})

# the agent's path under mode check (test_the_agents_path_under_check): case name -> rule; 200 steps, paths drawn as path_actions draws them
PATH_CASES = (("w5_l150_sap_best_next", "exact"), ("ring34_sap_best_check", "min_cut"), ("w2_sap_last_check", "last"))
PATH_STEPS = 200


def path_actions(k):
    """[PATH_STEPS, B] int32 in -1 .. k + 1: k and the values on both sides of the range are rejections"""
    return np.random.default_rng(5).integers(-1, k + 2, (PATH_STEPS, B)).astype(np.int32)


def run_path_case(name, rule):
    from gpu_support import topology
    c = GPU_CASES[name]
    topo = ref.resolve_case(gpu_case(name), "unused")[0]
    return run_batch(gpu_case(name), "path", rule, "check", n_steps=PATH_STEPS, gate_items=c["gate"], paths=path_actions(topo.k_paths))
