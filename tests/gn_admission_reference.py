"""The CPU reference of the action masks and rule windows that know BOTH halves of the GN-model admission check (``include/orlg.h``
``orlg_gn_admission_masks`` / ``orlg_gn_admission_windows``): a candidate oracle on the protecting oracle of
``gn_protect_reference.py``.  Before each step, after the services due by now are dropped, every candidate window of the pending
request -- the first fit of every path, the first ``n`` slots of every block ``b < j``, the window of every rule asked for
(``assign_reference.rule_slot``, ``cut_reference.min_cut_window``) -- goes through ``ProtectingOracle.evaluate(p, s)``: mask bit,
GSNR, neighbour margin, affected services.  Then the case's policy, or ``sap_ff_gn``, steps.  Helper module of
``test_gn_admission_args.py`` and ``test_gpu_gn_admission.py``; nothing here touches a GPU.
"""
import functools

import numpy as np

import assign_reference as ar
import cut_reference as cr
import gn_gate_reference as ref
import gn_protect_reference as pref
from gpu_support import device_log_in_oracle

RULES = ("first", "best", "min_cut")   # the rules of the parity cases
B = 8                                  # environments per batch: seeds case seed + 0 .. 7
N_STEPS = 150                          # (100 at S = 512)
MIN_COUNT = 10                         # of each kind of candidate per batch

# the parity batches of test_gpu_gn_admission.py: case of gn_protect_reference.CASES -> steps, j, and the handle's keywords beyond the
# case's (the oracle knows neither an explicit rejection nor a ring: both are the device's)
BATCHES = {
    "nsfnet_s100_l20_spff": dict(n=N_STEPS, j=2, handle=dict(allow_rejection=True)),
    "nsfnet_s320_l50_sapff": dict(n=N_STEPS, j=1, handle={}),
    "jpn12_s320_l150_sapff": dict(n=N_STEPS, j=1, handle=dict(queue_capacity=128)),
    "ring34_s320_l300_llpff": dict(n=N_STEPS, j=1, handle={}),
    "ring36_s512_l500_sapff": dict(n=100, j=1, handle={}),
}
# the further batches the issue counts: conditions only (test_gn_admission_args.py)
COUNTED = {"ring34_s100_l60_sapff": dict(n=N_STEPS, j=1, handle={})}
SEEDS = {}   # case -> the first seed of its batch where it had to move off a margin inside gn_shapes_reference.MARGIN_DB (none had to)


class AdmissionOracle(pref.ProtectingOracle):
    """A protecting oracle that also answers, before a step, what every candidate window of the pending request would meet."""

    def candidates(self, rules=RULES):
        """The pending request against what is lit now.  dict of, per kind in ("path_ff", "deeprmsa") + rules: <kind>_mask uint8,
        <kind>_gsnr, <kind>_margin float64 (NaN as the entries write them), <kind>_affected int32, <kind>_slots int32 (-1 = no
        window; the rules': S, as the query writes them) -- [K], deeprmsa [K j].  running: the services lit now."""
        o, K, S, j = self.o, self.K, self.S, self.j
        self._drop_due()
        seen = {}

        def verdict(p, s):
            if (p, s) not in seen:
                gsnr, own, margin, affected = self.evaluate(p, s)
                seen[(p, s)] = (int(own and not margin < 0), gsnr, margin, affected)
            return seen[(p, s)]

        def rows(n_cols, none):
            return dict(mask=np.zeros(n_cols, np.uint8), gsnr=np.full(n_cols, np.nan), margin=np.full(n_cols, np.nan),
                        affected=np.zeros(n_cols, np.int32), slots=np.full(n_cols, none, np.int32))

        out = {"path_ff": rows(K, -1), "deeprmsa": rows(K * j, -1)}
        out.update({rule: rows(K, S) for rule in rules})

        def put(kind, col, p, s):
            r = out[kind]
            r["mask"][col], r["gsnr"][col], r["margin"][col], r["affected"][col] = verdict(p, s)
            r["slots"][col] = s

        r, avail = o.request(), o.available_slots()
        cand = cr.candidates(avail, self.topo, r.src, r.dst, r.bit_rate)
        for p in range(K):
            n = o.number_slots(p)
            starts, _ = o.available_blocks(p)   # the first j free runs of at least n slots (rmsa_env.py:774-804)
            if len(starts) and starts[0] < S - n:   # PathOnlyFirstFitAction: range(0, S - n) does not try the start S - n
                put("path_ff", p, p, int(starts[0]))
            for b in range(min(j, len(starts))):
                put("deeprmsa", p * j + b, p, int(starts[b]))
            rws, n_c = cand[p]
            assert n_c == n
            for rule in rules:
                if rule == "min_cut":
                    got = cr.min_cut_window(rws, n)
                    s = None if got is None else int(got[1])
                else:
                    s = ar.rule_slot(rws.min(axis=0), n, rule)
                if s is not None:
                    assert o.is_path_free(p, int(s), n)
                    put(rule, p, p, int(s))
        flat = {f"{kind}_{k}": v for kind, r in out.items() for k, v in r.items()}
        flat["running"] = len(self.shadow)
        return flat


def _run(go, policy, n_steps, rules):
    cols, rows = {}, []
    for _ in range(n_steps):
        c = go.candidates(rules)
        for k, v in c.items():
            cols.setdefault(k, []).append(v)
        if policy == "sap_ff_gn":
            p, s, _ = go.propose_sap_ff_gn()
        else:
            p, s = go.propose(policy)
        rows.append(go.step(p, s))
    tr = {k: np.array([row[k] for row in rows]) for k in rows[0]}
    tr.update({k: np.array(v) for k, v in cols.items()})
    return tr


def run_case(case, seed=None, j=1, policy=None, n_steps=N_STEPS, rules=RULES, gate_items=()):
    """One environment of a case -- a name of gn_protect_reference.CASES (seed, policy: the case's own by default) or a (topology,
    kwargs) pair with its `policy` -- on the admission oracle, run once per process and shared: (per-step arrays -- the protecting
    oracle's and the candidates' rows taken BEFORE the step --, final state, figures).  Read-only by agreement."""
    if isinstance(case, str):
        seed, policy = pref.CASES[case]["seed"] if seed is None else seed, policy or pref.CASES[case]["policy"]
    else:
        assert policy is not None, "a (topology, kwargs) case has no policy of its own"
        seed = case[1]["seed"] if seed is None else seed
    return _run_case(ref.cache_key(case), seed, j, policy, n_steps, tuple(rules), tuple(gate_items))


@functools.lru_cache(maxsize=None)
def _run_case(key, seed, j, policy, n_steps, rules, gate_items):
    if isinstance(key, str):
        from conftest import load_topology
        topo, kw = load_topology(pref.CASES[key]["topology"]), pref.case_kwargs(key)
    else:
        topo, kw = key[0], dict(key[1])
    with device_log_in_oracle():
        go = AdmissionOracle(topo, kw, pref.case_gate(topo, **dict(gate_items)), seed=seed, j=j)
        tr = _run(go, policy, n_steps, rules)
    final, fig = pref.final_state(go.o), go.figures()
    go.close()
    for a in tr.values():
        a.setflags(write=False)
    return tr, final, fig


def batch_seed(case):
    return SEEDS.get(case, pref.CASES[case]["seed"]) if isinstance(case, str) else case[1]["seed"]


def run_batch(case, n_steps=N_STEPS, j=1, policy=None, batch=B, rules=RULES, gate_items=()):
    """run_case for the seeds of the batch: a list of its results"""
    seed = batch_seed(case)
    return [run_case(case, seed=seed + i, j=j, policy=policy, n_steps=n_steps, rules=rules, gate_items=gate_items) for i in range(batch)]


def parity_batch(case):
    c = dict(BATCHES, **COUNTED)[case]
    return run_batch(case, n_steps=c["n"], j=c["j"])


KINDS = ("path_ff", "deeprmsa")


def counts(runs, kinds=KINDS + RULES, first_col=0):
    """Summed over a batch and the kinds of candidate (columns first_col onwards): candidates with a window, refused by their own
    check, refused by the neighbour check alone, admitted with no affected service (margin NaN, bit 1), admitted behind a neighbour
    check; the most running services, the own or neighbour margin closest to zero, the largest |GSNR|."""
    out = dict(windows=0, own_refused=0, neighbour_refused=0, admitted_unaffected=0, admitted_checked=0)
    for tr, _, _ in runs:
        for kind in kinds:
            mask, gsnr, margin = (tr[f"{kind}_{k}"][:, first_col:] for k in ("mask", "gsnr", "margin"))
            affected = tr[f"{kind}_affected"][:, first_col:]
            has = ~np.isnan(gsnr)
            out["windows"] += int(has.sum())
            out["neighbour_refused"] += int((margin < 0).sum())
            out["own_refused"] += int((has & (mask == 0) & ~(margin < 0)).sum())
            out["admitted_unaffected"] += int(((mask == 1) & (affected == 0)).sum())
            out["admitted_checked"] += int(((mask == 1) & (affected > 0)).sum())
    out["max_running"] = max(int(tr["running"].max()) for tr, _, _ in runs)
    out["closest"] = min(fig["any_closest"] for _, _, fig in runs)
    out["max_abs_gsnr"] = max(fig["max_abs_gsnr"] for _, _, fig in runs)
    return out
