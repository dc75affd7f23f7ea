"""The spectrum-assignment rules (``include/orlg.h`` ``ORLG_ASSIGN_*``) restated in numpy, and the oracle stepped one
request at a time with the ``external`` action the definitions propose.  Support module of ``test_assign_rules.py`` and
``test_gpu_assign_rules.py``; nothing here touches a GPU or the library's kernels.

The reference has no counterpart (its heuristics are first fit only, ``rmsa_env.py:854-937``), so the definitions are the
project's: ``propose`` works from the ``[E, S]`` availability array the step met, the topology tables and the pending request,
and shares no code with the package or the oracle's queries -- ``test_assign_rules.py`` holds it to ``is_path_free`` and
``available_blocks`` by brute force."""
import functools

import numpy as np

import block_cause_reference as bcr

RULES = ("first", "first_full", "last", "best", "exact")   # ORLG_ASSIGN_*
NEW_RULES = RULES[1:]
ROUTES = ("sp", "sap", "llp")
SUFFIX = {"first": "ff", "first_full": "ff_full", "last": "lf", "best": "bf", "exact": "ef"}
SHAPES = ((64, 10), (100, 20), (320, 50))   # W = 1, 2 (a last word that is not full) and 5
NSFNET, N_ENVS, N_STEPS, SEED0 = bcr.NSFNET, bcr.N_ENVS, bcr.N_STEPS, bcr.SEED0


def policy_name(route, rule):
    return f"path_{SUFFIX[rule]}_external" if route == "path" else f"{route}_{SUFFIX[rule]}"


def blocks(A):
    """(starts, lengths) of the maximal runs of free slots of A [S] (a block may touch slot S - 1)"""
    padded = np.concatenate(([0], np.asarray(A, np.int64), [0]))
    edges = np.flatnonzero(np.diff(padded))
    return edges[::2], edges[1::2] - edges[::2]


def windows(A, n):
    """the starts s in 0 .. S - n INCLUSIVE with [s, s + n) free, ascending"""
    S = len(A)
    if not 1 <= n <= S:
        return np.zeros(0, np.int64)
    c = np.concatenate(([0], np.cumsum(np.asarray(A, np.int64))))
    return np.flatnonzero(c[n:] - c[:S - n + 1] == n)


def rule_slot(A, n, rule):
    """The start slot of `rule` on a path with availability A [S] for n slots, or None: the path has no candidate."""
    S = len(A)
    w = windows(A, n)
    if rule == "first":                     # the reference's: range(0, S - n)
        w = w[w < S - n]
        return int(w[0]) if w.size else None
    if w.size == 0:
        return None
    if rule == "first_full":
        return int(w[0])
    if rule == "last":
        return int(w[-1])
    starts, lengths = blocks(A)
    fits = lengths >= n
    starts, lengths = starts[fits], lengths[fits]
    if rule == "best":                      # the shortest block, ties to the lowest start
        order = sorted(range(len(starts)), key=lambda b: (lengths[b], starts[b]))
        return int(starts[order[0]])
    if rule == "exact":                     # the lowest block of exactly n, else first_full
        same = starts[lengths == n]
        return int(same[0]) if same.size else int(w[0])
    raise ValueError(rule)


def candidates(avail, topo, src, dst, bit_rate):
    """[(A [S], n)] of the k candidate paths of the request"""
    base = int(topo.pair_path_base[src * topo.num_nodes + dst])
    out = []
    for p in range(topo.k_paths):
        gid = base + p
        links = np.asarray(topo.path_links[topo.path_link_off[gid]:topo.path_link_off[gid + 1]], np.int64)
        out.append((avail[links].min(axis=0), bcr.number_slots(bit_rate, int(topo.path_se[gid]))))
    return out


def propose(avail, topo, src, dst, bit_rate, route, rule, given=None):
    """(path, slot) the route and the rule propose on avail [E, S], (k, S) = the rejection.  route "path": `given` names the path."""
    k, S = topo.k_paths, avail.shape[1]
    cand = candidates(avail, topo, src, dst, bit_rate)
    if route == "path":
        if not 0 <= given < k:
            return k, S
        s = rule_slot(*cand[given], rule)
        return (k, S) if s is None else (int(given), s)
    best, action = 0, (k, S)
    for p, (A, n) in enumerate(cand[:1] if route == "sp" else cand):
        s = rule_slot(A, n, rule)
        if s is None:
            continue
        if route != "llp":
            return p, s
        if int(A.sum()) > best:             # strict >: ties go to the first
            best, action = int(A.sum()), (p, s)
    return action


def oracle_steps(topo, kw, seed, route, rule, n_steps, paths=None):
    """One oracle environment stepped n_steps times with auto-reset under external actions = propose(...).  Arrays [n]: act_path,
    act_slot, accepted, cause (the state-based blocking cause, block_cause_reference), n_slots of the chosen path (0 = rejected),
    first_path / first_slot (what the reference's first fit proposes on the same route and state), lowest_block (the start of the
    chosen path's lowest block of >= n slots, -1 = rejected); levels [n, k] where the step was refused (else 255).
    paths [n]: the agent's path per step for route "path"."""
    from conftest import oracle_env_from_kwargs
    from gpu_support import device_log_in_oracle
    cols = {c: [] for c in ("act_path", "act_slot", "accepted", "cause", "n_slots", "first_path", "first_slot", "lowest_block")}
    levels = np.full((n_steps, topo.k_paths), 255, np.uint8)
    with device_log_in_oracle():
        o = oracle_env_from_kwargs(topo, kw, seed=seed)
        for t in range(n_steps):
            r, avail = o.request(), o.available_slots().copy()
            given = None if paths is None else int(paths[t])
            p, s = propose(avail, topo, r.src, r.dst, r.bit_rate, route, rule, given)
            fp, fs = propose(avail, topo, r.src, r.dst, r.bit_rate, route, "first", given)
            acc = int(o.run("external", 1, reset_on_done=True, actions=np.array([[p, s]], np.int32), fields=["accepted"])["accepted"][0])
            cause = bcr.ACCEPTED
            if not acc:
                levels[t] = bcr.path_levels(avail, topo, r.src, r.dst, r.bit_rate)
                cause = bcr.block_cause(levels[t], False)
            n, low = 0, -1
            if p < topo.k_paths:
                A, n = candidates(avail, topo, r.src, r.dst, r.bit_rate)[p]
                low = rule_slot(A, n, "first_full")
            for c, v in zip(cols, (p, s, acc, cause, n, fp, fs, low)):
                cols[c].append(v)
        o.close()
    out = {c: np.array(v, np.uint8 if c in ("accepted", "cause") else np.int32) for c, v in cols.items()}
    out["levels"] = levels
    return out


@functools.lru_cache(maxsize=None)
def nsfnet_steps(S, load, route, rule, i, n_steps=N_STEPS):
    """Environment i (seed 10 + i) of a shape, once per process; read-only by agreement."""
    from gpu_support import topology
    return oracle_steps(topology(NSFNET), bcr.shape_kwargs(S, load), SEED0 + i, route, rule, n_steps)


def stacked(S, load, route, rule, envs=range(N_ENVS), n_steps=N_STEPS):
    """the columns of nsfnet_steps as [n, B] arrays"""
    runs = [nsfnet_steps(S, load, route, rule, i, n_steps) for i in envs]
    return {c: np.stack([r[c] for r in runs], axis=1) for c in runs[0]}
