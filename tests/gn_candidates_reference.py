"""The CPU reference of the action masks that know the GN-model admission check and of the policy ``sap_ff_gn`` (``include/orlg.h``
``orlg_gn_action_masks``, ``ORLG_POLICY_SAP_FF_GN``), on top of the gated oracle of ``gn_gate_reference.py``: per step
and environment the ``path_ff_gn`` / ``deeprmsa_gn`` masks with their GSNR rows -- from the oracle's ``available_blocks`` and
``number_slots``, ``GatedOracle.gsnr`` and the gate's thresholds -- and the ``sap_ff_gn`` proposal.  Helper module of
``test_gn_action_mask_args.py`` and ``test_gpu_gn_action_masks.py``; nothing here touches a GPU.
"""
import functools

import numpy as np

import gn_gate_reference as ref
from gpu_support import device_log_in_oracle

N_STEPS = 300
B = 8   # environments per case: seeds case seed + 0 .. 7


class CandidateOracle(ref.GatedOracle):
    """A gated oracle that also answers, before a step, what every candidate window of the pending request would meet."""

    def candidates(self):
        """The pending request against what is lit now: dict of
        path_ff [K], path_ff_gn [K] uint8, path_ff_gsnr [K] float64 (NaN where path_ff is 0), path_ff_slot [K] (-1: no fit),
        deeprmsa [K j], deeprmsa_gn [K j] uint8, deeprmsa_gsnr [K j] (NaN where the block does not exist), margin: the smallest
        |GSNR - threshold| over the candidates (inf without one)."""
        o, K, S, j = self.o, self.K, self.S, self.j
        now = o.current_time()
        self.shadow = [e for e in self.shadow if not e[0] <= now]   # what step() drops first: the services due by now
        c = dict(path_ff=np.zeros(K, np.uint8), path_ff_gn=np.zeros(K, np.uint8), path_ff_gsnr=np.full(K, np.nan),
                 path_ff_slot=np.full(K, -1), deeprmsa=np.zeros(K * j, np.uint8), deeprmsa_gn=np.zeros(K * j, np.uint8),
                 deeprmsa_gsnr=np.full(K * j, np.nan), margin=np.inf)
        for p in range(K):
            n = o.number_slots(p)
            links, se = self._path(p)
            thr = float(self.gate["thresholds_db"][se - 1])
            starts, _ = o.available_blocks(p)   # the first j free runs of at least n slots (rmsa_env.py:774-804)
            seen = {}

            def gsnr(s):
                if s not in seen:
                    seen[s] = self.gsnr(links, s, n)
                    c["margin"] = min(c["margin"], abs(seen[s] - thr))
                return seen[s]

            # PathOnlyFirstFitAction (rmsa_env.py:974-1008): the lowest free window is the first block's start; range(0, S - n)
            # does not try the start S - n
            if len(starts) and starts[0] < S - n:
                s = int(starts[0])
                assert o.is_path_free(p, s, n) and not any(o.is_path_free(p, q, n) for q in range(max(0, s - 2), s))
                c["path_ff"][p], c["path_ff_slot"][p], c["path_ff_gsnr"][p] = 1, s, gsnr(s)
                c["path_ff_gn"][p] = c["path_ff_gsnr"][p] >= thr
            for b in range(min(j, len(starts))):   # deeprmsa_env.py:48-58: the block's first n slots
                a = p * j + b
                c["deeprmsa"][a], c["deeprmsa_gsnr"][a] = 1, gsnr(int(starts[b]))
                c["deeprmsa_gn"][a] = c["deeprmsa_gsnr"][a] >= thr
        return c

    def propose_sap_ff_gn(self, c=None):
        """(path, slot) of the policy sap_ff_gn: the first path whose first fit passes the gate; none passes: the first path with a
        fit (the step refuses it); no path has a fit: the rejection."""
        c = c or self.candidates()
        admitted, fits = np.flatnonzero(c["path_ff_gn"]), np.flatnonzero(c["path_ff"])
        if fits.size == 0:
            return self.K, self.S
        p = int(admitted[0] if admitted.size else fits[0])
        return p, int(c["path_ff_slot"][p])


MASK_FIELDS = ("path_ff", "path_ff_gn", "path_ff_gsnr", "deeprmsa", "deeprmsa_gn", "deeprmsa_gsnr", "margin")


def _run(go, policy, n_steps):
    masks, rows, later = {k: [] for k in MASK_FIELDS}, [], 0
    for _ in range(n_steps):
        c = go.candidates()
        for k in MASK_FIELDS:
            masks[k].append(c[k])
        p, s = go.propose_sap_ff_gn(c) if policy == "sap_ff_gn" else go.propose(policy)
        rows.append(go.step(p, s))
        if policy == "sap_ff_gn" and rows[-1]["accepted"] and p != int(np.flatnonzero(c["path_ff"])[0]):
            later += 1   # the first candidate was refused and a later one taken
    tr = {k: np.array([row[k] for row in rows]) for k in rows[0]}
    tr.update({k: np.array(v) for k, v in masks.items()})
    return tr, later


def run_case(case, seed=None, j=1, policy=None, n_steps=N_STEPS, gate_items=(), kw_items=()):
    """One environment of a case -- a name of gn_gate_reference.CASES (seed, policy: the case's own by default) or a (topology,
    kwargs) pair with its `policy` -- on the candidate oracle, run once per process and shared: (per-step arrays -- the gated
    oracle's and MASK_FIELDS, the masks taken BEFORE the step --, final state, figures).  Read-only by agreement."""
    return _run_case(ref.cache_key(case), seed, j, policy, n_steps, tuple(gate_items), tuple(kw_items))


@functools.lru_cache(maxsize=None)
def _run_case(key, seed, j, policy, n_steps, gate_items, kw_items):
    topo, kw, policy = ref.resolve_case(key if isinstance(key, str) else (key[0], dict(key[1])), policy)
    kw.update(dict(kw_items))
    with device_log_in_oracle():
        go = CandidateOracle(topo, kw, ref.case_gate(topo, **dict(gate_items)), seed=seed, j=j)
        tr, later = _run(go, policy, n_steps)
    o = go.o
    final = dict(available_slots=o.available_slots(), counters=o.counters(), num_running=o.num_running(),
                 current_time=o.current_time())
    figures = dict(checks=go.checks, rejects=go.rejects, max_running=go.max_running, later_taken=later,
                   provisions=int(tr["accepted"].sum()), closest=float(np.min(tr["margin"])))
    go.close()
    for a in tr.values():
        a.setflags(write=False)
    return tr, final, figures


def run_batch(case, j=1, policy=None, n_steps=N_STEPS, batch=B, seed=None, **kw):
    """run_case for the seeds seed + 0 .. batch - 1 (seed: the case's own; a (topology, kwargs) pair's is its kwargs'): a list of
    its results"""
    if seed is None:
        seed = ref.CASES[case]["seed"] if isinstance(case, str) else case[1]["seed"]
    return [run_case(case, seed=seed + i, j=j, policy=policy, n_steps=n_steps, **kw) for i in range(batch)]
