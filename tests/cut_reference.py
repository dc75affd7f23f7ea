"""The fewest-cuts window (``include/orlg.h`` ``orlg_step_min_cut`` / ``orlg_path_min_cuts``) restated in numpy, and
the oracle stepped one request at a time with the ``external`` action the definitions propose.  Support module of
``test_cut_rules.py`` and ``test_gpu_cut_rules.py``; nothing here touches a GPU or the library's kernels.

The reference has no counterpart for these environments (its ``calculate_r_cut`` belongs to the QoT-aware one), so the
definitions are the project's: everything works from the ``[E, S]`` availability array the step met, the topology tables and
the pending request, and shares no code with the package -- ``test_cut_rules.py`` holds it to ``is_path_free`` and the links'
own neighbouring slots by brute force."""
import functools

import numpy as np

import assign_reference as ar
import block_cause_reference as bcr

ROUTES = ("sp", "sap", "llp", "min_cut")   # and "path": the agent's
POLICY = {"sp": "sp_mc", "sap": "sap_mc", "llp": "llp_mc", "min_cut": "min_cut", "path": "path_mc_external"}
SHAPES = ar.SHAPES
NSFNET, N_ENVS, N_STEPS, SEED0 = bcr.NSFNET, bcr.N_ENVS, bcr.N_STEPS, bcr.SEED0


def path_links(topo, gid):
    return np.asarray(topo.path_links[topo.path_link_off[gid]:topo.path_link_off[gid + 1]], np.int64)


def window_cuts(rows, n):
    """(starts, cuts) of the windows of n slots on a path whose links have the availability rows [hops, S]: starts = every s in
    0 .. S - n with [s, s + n) free on every link, ascending; cuts[i] = the links with slot starts[i] - 1 and slot starts[i] + n
    both free (slots -1 and S are not free)."""
    rows = np.asarray(rows, np.int64)
    S = rows.shape[1]
    starts = ar.windows(rows.min(axis=0), n)
    padded = np.concatenate((np.zeros((len(rows), 1), np.int64), rows, np.zeros((len(rows), 1), np.int64)), axis=1)   # slot t at t + 1
    cuts = (padded[:, starts] & padded[:, starts + n + 1]).sum(axis=0) if starts.size else np.zeros(0, np.int64)
    assert S == padded.shape[1] - 2
    return starts, cuts


def min_cut_window(rows, n):
    """(cuts, start) of the fewest-cuts window, ties to the lowest start; None: no window"""
    starts, cuts = window_cuts(rows, n)
    if starts.size == 0:
        return None
    i = int(np.argmin(cuts))   # the first of equal counts: the lowest start
    return int(cuts[i]), int(starts[i])


def candidates(avail, topo, src, dst, bit_rate, channel_width=bcr.CHANNEL_WIDTH):
    """[(rows [hops, S], n)] of the k candidate paths of the request"""
    base = int(topo.pair_path_base[src * topo.num_nodes + dst])
    return [(avail[path_links(topo, base + p)], bcr.number_slots(bit_rate, int(topo.path_se[base + p]), channel_width))
            for p in range(topo.k_paths)]


def path_min_cuts(avail, topo, src, dst, bit_rate, channel_width=bcr.CHANNEL_WIDTH):
    """(cuts [k], slots [k]) int16 of orlg_path_min_cuts: -1 and S where the path has no window"""
    k, S = topo.k_paths, avail.shape[1]
    cuts, slots = np.full(k, -1, np.int16), np.full(k, S, np.int16)
    for p, (rows, n) in enumerate(candidates(avail, topo, src, dst, bit_rate, channel_width)):
        got = min_cut_window(rows, n)
        if got is not None:
            cuts[p], slots[p] = got
    return cuts, slots


def propose(avail, topo, src, dst, bit_rate, route, given=None, channel_width=bcr.CHANNEL_WIDTH):
    """(path, slot, cuts) the route proposes under MIN_CUT on avail [E, S]; (k, S, -1) = the rejection."""
    k, S = topo.k_paths, avail.shape[1]
    cand = candidates(avail, topo, src, dst, bit_rate, channel_width)
    if route == "path":
        got = min_cut_window(*cand[given]) if 0 <= given < k else None
        return (k, S, -1) if got is None else (int(given), got[1], got[0])
    best, action = None, (k, S, -1)
    for p, (rows, n) in enumerate(cand[:1] if route == "sp" else cand):
        got = min_cut_window(rows, n)
        if got is None:
            continue
        if route in ("sp", "sap"):
            return p, got[1], got[0]
        rank = int(rows.min(axis=0).sum()) if route == "llp" else -got[0]   # most free slots / fewest cuts
        if best is None or rank > best:                                       # strict >: ties go to the first
            best, action = rank, (p, got[1], got[0])
    return action


def _other_route(route):
    return "sap" if route == "min_cut" else route   # the route the classic rules are asked on where they have no fewest-cuts route


def oracle_steps(topo, kw, seed, route, n_steps, paths=None):
    """One oracle environment stepped n_steps times with auto-reset under external actions = propose(...).  Arrays [n]: act_path,
    act_slot, accepted, cuts (of the chosen window, -1 = rejected), cause (the state-based blocking cause), n_slots and hops of the
    chosen path (0 = rejected), lowest_cuts (the cuts of the chosen path's lowest window, -1), ff_path / ff_slot and bf_path /
    bf_slot (what first_full and best propose on the same state; route min_cut: on route sap), sap_path (the first path that has
    a window, k = none); request [n, 3]; min_cuts / min_slots [n + 1, k]: path_min_cuts of the request pending before step t (row
    n: after the last step).  paths [n]: the agent's path per step for route "path"."""
    from conftest import oracle_env_from_kwargs
    from gpu_support import device_log_in_oracle
    names = ("act_path", "act_slot", "accepted", "cuts", "cause", "n_slots", "hops", "lowest_cuts", "ff_path", "ff_slot", "bf_path",
             "bf_slot", "sap_path")
    cols = {c: [] for c in names}
    reqs, mc, ms = [], [], []
    cw = kw.get("channel_width", bcr.CHANNEL_WIDTH)
    with device_log_in_oracle():
        o = oracle_env_from_kwargs(topo, kw, seed=seed)
        for t in range(n_steps + 1):
            r, avail = o.request(), o.available_slots().copy()
            c, s = path_min_cuts(avail, topo, r.src, r.dst, r.bit_rate, cw)
            mc.append(c); ms.append(s)
            if t == n_steps:
                break
            given = None if paths is None else int(paths[t])
            p, s, cuts = propose(avail, topo, r.src, r.dst, r.bit_rate, route, given, cw)
            other = _other_route(route)
            fp, fs = ar.propose(avail, topo, r.src, r.dst, r.bit_rate, other, "first_full", given)
            bp, bs = ar.propose(avail, topo, r.src, r.dst, r.bit_rate, other, "best", given)
            acc = int(o.run("external", 1, reset_on_done=True, actions=np.array([[p, s]], np.int32), fields=["accepted"])["accepted"][0])
            cause = bcr.ACCEPTED
            if not acc:
                cause = bcr.block_cause(bcr.path_levels(avail, topo, r.src, r.dst, r.bit_rate, cw), False)
            n, hops, low = 0, 0, -1
            if p < topo.k_paths:
                rows, n = candidates(avail, topo, r.src, r.dst, r.bit_rate, cw)[p]
                hops, low = len(rows), int(window_cuts(rows, n)[1][0])
            has = np.flatnonzero(c >= 0)
            for name, v in zip(names, (p, s, acc, cuts, cause, n, hops, low, fp, fs, bp, bs, int(has[0]) if has.size else topo.k_paths)):
                cols[name].append(v)
            reqs.append((r.src, r.dst, r.bit_rate))
        o.close()
    out = {c: np.array(v, np.uint8 if c in ("accepted", "cause") else np.int32) for c, v in cols.items()}
    out.update(request=np.array(reqs, np.int32), min_cuts=np.stack(mc), min_slots=np.stack(ms))
    return out


@functools.lru_cache(maxsize=None)
def nsfnet_steps(S, load, route, i, n_steps=N_STEPS):
    """Environment i (seed 10 + i) of a shape, once per process; read-only by agreement."""
    from gpu_support import topology
    return oracle_steps(topology(NSFNET), bcr.shape_kwargs(S, load), SEED0 + i, route, n_steps)


def stacked(S, load, route, envs=range(N_ENVS), n_steps=N_STEPS):
    """the columns of nsfnet_steps as [n, B(, ..)] arrays"""
    runs = [nsfnet_steps(S, load, route, i, n_steps) for i in envs]
    return {c: np.stack([r[c] for r in runs], axis=1) for c in runs[0]}


def stack_runs(runs):
    return {c: np.stack([r[c] for r in runs], axis=1) for c in runs[0]}
