"""The definitions of the blocking cause and of the fit levels (``include/orlg.h`` ``ORLG_CAUSE_*`` / ``ORLG_FIT_*``)
restated in numpy, and the oracle stepped one request at a time next to them.  Support module of ``test_block_cause.py`` and
``test_gpu_block_cause.py``; nothing here touches a GPU or the library's kernels.

``path_levels`` works from what the definition names and nothing else: the ``[E, S]`` availability array the step met, the
topology tables, the pending request.  It shares no code with the oracle's queries (``is_path_free``), which the CPU tests hold
it against by brute force."""
import functools
import math

import numpy as np

CAPACITY, CONTIGUITY, ALIGNMENT, LAST_WINDOW, FIT = range(5)                               # ORLG_FIT_*
ACCEPTED, C_CAPACITY, C_CONTIGUITY, C_ALIGNMENT, C_LAST_WINDOW, C_POLICY, C_GN = range(7)   # ORLG_CAUSE_*
NUM_CAUSES = 8

# the table of the issue: (S, load) on NSFNET, 8 environments on seeds 10 .. 17, 200 steps from an empty network
NSFNET = "nsfnet_chen_5-paths_6-modulations"
SHAPES = ((64, 10), (100, 20), (192, 35), (320, 50))
N_ENVS, N_STEPS, SEED0 = 8, 200, 10
CHANNEL_WIDTH = 12.5


def shape_kwargs(S, load, **over):
    return dict(dict(num_spectrum_resources=S, load=load, mean_service_holding_time=25, episode_length=50, seed=SEED0), **over)


def number_slots(bit_rate, se, channel_width=CHANNEL_WIDTH):
    """get_number_slots (rmsa_env.py:708-719)"""
    return math.ceil(bit_rate / (se * channel_width)) + 1


def longest_run(row):
    """length of the longest run of ones of a 0/1 vector"""
    padded = np.concatenate(([0], np.asarray(row, np.int64), [0]))
    edges = np.flatnonzero(np.diff(padded))
    return int((edges[1::2] - edges[::2]).max()) if edges.size else 0


def window_starts(avail, n):
    """[S] bool: [s, s + n) lies inside the spectrum and is free on every row of avail [h, S]"""
    h, S = avail.shape
    ok = np.zeros(S, bool)
    if 1 <= n <= S:
        c = np.concatenate((np.zeros((h, 1), np.int64), np.cumsum(avail.astype(np.int64), axis=1)), axis=1)
        ok[:S - n + 1] = ((c[:, n:] - c[:, :S - n + 1]) == n).all(axis=0)
    return ok


def path_level(avail, links, n):
    """The fit level of one path: avail [E, S] (1 = free), links = its link indices, n slots."""
    S = avail.shape[1]
    rows = avail[np.asarray(links, np.int64)]
    starts = window_starts(rows, n)
    if starts[:max(S - n, 0)].any():           # some s in range(0, S - n)
        return FIT
    if n <= S and starts[S - n]:
        return LAST_WINDOW
    if all(longest_run(r) >= n for r in rows):
        return ALIGNMENT
    if all(int(r.sum()) >= n for r in rows):
        return CONTIGUITY
    return CAPACITY


def path_levels(avail, topo, src, dst, bit_rate, channel_width=CHANNEL_WIDTH):
    """[k] uint8: the fit level of every candidate path of the request (src, dst, bit_rate) on avail [E, S]."""
    base = int(topo.pair_path_base[src * topo.num_nodes + dst])
    out = np.zeros(topo.k_paths, np.uint8)
    for p in range(topo.k_paths):
        gid = base + p
        links = topo.path_links[topo.path_link_off[gid]:topo.path_link_off[gid + 1]]
        out[p] = path_level(avail, links, number_slots(bit_rate, int(topo.path_se[gid]), channel_width))
    return out


def block_cause(levels, accepted, gn_refused=False):
    if accepted:
        return ACCEPTED
    if gn_refused:
        return C_GN
    return 1 + int(np.max(levels))


# ---------------------------------------------------------------------------------------- the oracle, one step at a time
def oracle_steps(topo, kw, seed, policy, n_steps, actions=None, j=1, reward_mode=0, keep=()):
    """One oracle environment stepped n_steps times with auto-reset, the definitions applied to what every step met: dict of
    levels [n, k], cause [n], accepted [n], request [n, 3] (src, dst, bit_rate).  actions: the external actions [n(, 2)].
    keep: steps after which (levels of the NEXT pending request, available_slots) are kept too, as "after"[t]."""
    from conftest import oracle_env_from_kwargs
    from gpu_support import device_log_in_oracle
    with device_log_in_oracle():
        o = oracle_env_from_kwargs(topo, kw, seed=seed, j=j, reward_mode=reward_mode)
        levels, cause, acc, reqs, after = [], [], [], [], {}

        def pending():
            r = o.request()
            return path_levels(o.available_slots(), topo, r.src, r.dst, r.bit_rate, kw.get("channel_width", CHANNEL_WIDTH)), r

        if 0 in keep:
            after[0] = pending()[0]
        for t in range(n_steps):
            lv, r = pending()
            a = None if actions is None else np.ascontiguousarray(actions[t:t + 1])
            tr = o.run(policy, 1, reset_on_done=True, actions=a, fields=["accepted"])
            levels.append(lv); acc.append(int(tr["accepted"][0])); reqs.append((r.src, r.dst, r.bit_rate))
            cause.append(block_cause(lv, acc[-1]))
            if t + 1 in keep:
                after[t + 1] = pending()[0]
        o.close()
    return dict(levels=np.array(levels, np.uint8), cause=np.array(cause, np.uint8), accepted=np.array(acc, np.uint8),
                request=np.array(reqs, np.int32), after=after)


@functools.lru_cache(maxsize=None)
def nsfnet_steps(S, load, policy, i, n_steps=N_STEPS, over=()):
    """Environment i (seed 10 + i) of a shape of the issue's table, once per process; read-only by agreement."""
    from gpu_support import topology
    j, reward_mode = (1, 1) if policy.startswith("deeprmsa") else (1, 0)
    return oracle_steps(topology(NSFNET), shape_kwargs(S, load, **dict(over)), SEED0 + i, policy, n_steps, j=j, reward_mode=reward_mode)


def counts_of(cause):
    """[n, B] causes -> [B, 8] int32 counts"""
    return np.stack([np.bincount(cause[:, i], minlength=NUM_CAUSES) for i in range(cause.shape[1])]).astype(np.int32)


def gated_steps(case, n_steps, policy=None, seed=None):
    """A case of gn_gate_reference.CASES behind its gate at +6 dBm, one step at a time: cause [n], accepted [n], gsnr [n]."""
    import gn_candidates_reference as gcr
    import gn_gate_reference as ggr
    from gpu_support import device_log_in_oracle
    topo, kw, policy = ggr.resolve_case(case, policy)
    with device_log_in_oracle():
        go = gcr.CandidateOracle(topo, kw, ggr.case_gate(topo), seed=seed)
        cause, acc, gsnr = [], [], []
        for _ in range(n_steps):
            r = go.o.request()
            lv = path_levels(go.o.available_slots(), topo, r.src, r.dst, r.bit_rate)
            row = go.step(*(go.propose_sap_ff_gn() if policy == "sap_ff_gn" else go.propose(policy)))
            acc.append(int(row["accepted"])); gsnr.append(row["gsnr"])
            cause.append(block_cause(lv, acc[-1], gn_refused=not acc[-1] and not np.isnan(row["gsnr"])))
        go.close()
    return dict(cause=np.array(cause, np.uint8), accepted=np.array(acc, np.uint8), gsnr=np.array(gsnr))
