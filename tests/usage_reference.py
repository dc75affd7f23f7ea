"""Most-used assignment and the route that takes the best window over all candidate paths (``include/orlg.h`` ``orlg_step_window``,
``orlg_slot_usage``, ``orlg_path_most_used``) restated in numpy, and the oracle stepped one request at a time with
the ``external`` action the definitions propose.  Support module of ``test_window_rules.py`` and ``test_gpu_window_rules.py``;
nothing here touches a GPU or the library's kernels.

The reference has no counterpart, so the definitions are the project's: everything works from the ``[E, S]`` availability array
the step met, the topology tables and the pending request, and shares no code with the package -- ``test_window_rules.py`` holds
it to a brute force over every (start, link, slot)."""
import functools

import numpy as np

import assign_reference as ar
import block_cause_reference as bcr

RULES = ("first_full", "last", "best", "exact", "most_used")
ROUTES = ("sp", "sap", "llp", "any")   # and "path": the agent's
# policy name -> (route, rule): the names of _lib.WINDOW_POLICIES
NAMES = {"sp_mu": ("sp", "most_used"), "sap_mu": ("sap", "most_used"), "llp_mu": ("llp", "most_used"),
         "path_mu_external": ("path", "most_used"), "any_ff_full": ("any", "first_full"), "any_lf": ("any", "last"),
         "any_bf": ("any", "best"), "any_ef": ("any", "exact"), "any_mu": ("any", "most_used")}
LAUNCHED = tuple(n for n in NAMES if n != "path_mu_external")   # the names a launch of many steps runs
SHAPES = ar.SHAPES
NSFNET, N_ENVS, N_STEPS, SEED0 = bcr.NSFNET, bcr.N_ENVS, bcr.N_STEPS, bcr.SEED0


def slot_usage(avail):
    """U [S]: the links of the whole topology on which the slot is occupied"""
    avail = np.asarray(avail, np.int64)
    return avail.shape[0] - avail.sum(axis=0)


def window_usage(U, starts, n):
    """usage of the windows [s, s + n) for s in starts"""
    c = np.concatenate(([0], np.cumsum(np.asarray(U, np.int64))))
    starts = np.asarray(starts, np.int64)
    return c[starts + n] - c[starts]


def proposal(A, U, n, rule):
    """(rank, start) of the rule's window on a path with availability A [S] for n slots -- rank: a tuple, smaller = the better
    proposal by the rule's own order -- or None: the path has no window."""
    w = ar.windows(A, n)
    if w.size == 0:
        return None
    if rule == "first_full":
        return (int(w[0]),), int(w[0])
    if rule == "last":
        return (-int(w[-1]),), int(w[-1])
    if rule == "most_used":
        u = window_usage(U, w, n)
        i = int(np.argmax(u))   # the first of equal sums: the lowest start
        return (-int(u[i]), int(w[i])), int(w[i])
    starts, lengths = ar.blocks(A)
    fits = lengths >= n
    starts, lengths = starts[fits], lengths[fits]
    if rule == "best":
        b = min(range(len(starts)), key=lambda b: (lengths[b], starts[b]))
        return (int(lengths[b]), int(starts[b])), int(starts[b])
    if rule == "exact":
        same = starts[lengths == n]
        return ((0, int(same[0])), int(same[0])) if same.size else ((1, int(w[0])), int(w[0]))
    raise ValueError(rule)


def candidates(avail, topo, src, dst, bit_rate, channel_width=bcr.CHANNEL_WIDTH):
    """[(A [S], n)] of the k candidate paths of the request"""
    base = int(topo.pair_path_base[src * topo.num_nodes + dst])
    out = []
    for p in range(topo.k_paths):
        gid = base + p
        links = np.asarray(topo.path_links[topo.path_link_off[gid]:topo.path_link_off[gid + 1]], np.int64)
        out.append((avail[links].min(axis=0), bcr.number_slots(bit_rate, int(topo.path_se[gid]), channel_width)))
    return out


def path_most_used(avail, topo, src, dst, bit_rate, channel_width=bcr.CHANNEL_WIDTH):
    """(usage [k] int32, slots [k] int16) of orlg_path_most_used: -1 and S where the path has no window"""
    k, S = topo.k_paths, avail.shape[1]
    U = slot_usage(avail)
    usage, slots = np.full(k, -1, np.int32), np.full(k, S, np.int16)
    for p, (A, n) in enumerate(candidates(avail, topo, src, dst, bit_rate, channel_width)):
        got = proposal(A, U, n, "most_used")
        if got is not None:
            usage[p], slots[p] = -got[0][0], got[1]
    return usage, slots


def propose(avail, topo, src, dst, bit_rate, route, rule, given=None, channel_width=bcr.CHANNEL_WIDTH):
    """(path, slot) the route proposes under the rule on avail [E, S]; (k, S) = the rejection."""
    k, S = topo.k_paths, avail.shape[1]
    U = slot_usage(avail)
    cand = candidates(avail, topo, src, dst, bit_rate, channel_width)
    if route == "path":
        got = proposal(cand[given][0], U, cand[given][1], rule) if 0 <= given < k else None
        return (k, S) if got is None else (int(given), got[1])
    best, action = None, (k, S)
    for p, (A, n) in enumerate(cand[:1] if route == "sp" else cand):
        got = proposal(A, U, n, rule)
        if got is None:
            continue
        if route in ("sp", "sap"):
            return p, got[1]
        rank = (-int(A.sum()),) if route == "llp" else got[0]   # most free slots / the rule's own order
        if best is None or rank < best:                           # strict <: ties go to the first
            best, action = rank, (p, got[1])
    return action


def oracle_steps(topo, kw, seed, name, n_steps, paths=None):
    """One oracle environment stepped n_steps times with auto-reset under external actions = propose(...) of policy `name`.
    Arrays [n]: act_path, act_slot, accepted, cause (the state-based blocking cause), n_slots of the chosen path (0 = rejected),
    usage of the chosen window (-1 = rejected), ff_path / ff_slot (what first_full proposes on the same route and state) and
    sap_path / sap_slot (what the same rule proposes on route sap); slot_usage [n + 1, S] uint8, mu_usage / mu_slots [n + 1, k]:
    the queries on the state before step t (row n: after the last step).  paths [n]: the agent's path per step for route "path"."""
    from conftest import oracle_env_from_kwargs
    from gpu_support import device_log_in_oracle
    route, rule = NAMES[name]
    names = ("act_path", "act_slot", "accepted", "cause", "n_slots", "usage", "ff_path", "ff_slot", "sap_path", "sap_slot")
    cols = {c: [] for c in names}
    su, mu, ms = [], [], []
    cw = kw.get("channel_width", bcr.CHANNEL_WIDTH)
    with device_log_in_oracle():
        o = oracle_env_from_kwargs(topo, kw, seed=seed)
        for t in range(n_steps + 1):
            r, avail = o.request(), o.available_slots().copy()
            su.append(slot_usage(avail).astype(np.uint8))
            u, s = path_most_used(avail, topo, r.src, r.dst, r.bit_rate, cw)
            mu.append(u); ms.append(s)
            if t == n_steps:
                break
            given = None if paths is None else int(paths[t])
            p, s = propose(avail, topo, r.src, r.dst, r.bit_rate, route, rule, given, cw)
            fp, fs = propose(avail, topo, r.src, r.dst, r.bit_rate, route, "first_full", given, cw)
            sp_, ss = propose(avail, topo, r.src, r.dst, r.bit_rate, "sap", rule, None, cw)
            acc = int(o.run("external", 1, reset_on_done=True, actions=np.array([[p, s]], np.int32), fields=["accepted"])["accepted"][0])
            cause = bcr.ACCEPTED
            if not acc:
                cause = bcr.block_cause(bcr.path_levels(avail, topo, r.src, r.dst, r.bit_rate, cw), False)
            n, usage = 0, -1
            if p < topo.k_paths:
                n = candidates(avail, topo, r.src, r.dst, r.bit_rate, cw)[p][1]
                usage = int(window_usage(slot_usage(avail), [s], n)[0])
            for c, v in zip(names, (p, s, acc, cause, n, usage, fp, fs, sp_, ss)):
                cols[c].append(v)
        o.close()
    out = {c: np.array(v, np.uint8 if c in ("accepted", "cause") else np.int32) for c, v in cols.items()}
    out.update(slot_usage=np.stack(su), mu_usage=np.stack(mu), mu_slots=np.stack(ms))
    return out


@functools.lru_cache(maxsize=None)
def nsfnet_steps(S, load, name, i, n_steps=N_STEPS):
    """Environment i (seed 10 + i) of a shape, once per process; read-only by agreement."""
    from gpu_support import topology
    return oracle_steps(topology(NSFNET), bcr.shape_kwargs(S, load), SEED0 + i, name, n_steps)


def stacked(S, load, name, envs=range(N_ENVS), n_steps=N_STEPS):
    """the columns of nsfnet_steps as [n, B(, ..)] arrays"""
    runs = [nsfnet_steps(S, load, name, i, n_steps) for i in envs]
    return {c: np.stack([r[c] for r in runs], axis=1) for c in runs[0]}
