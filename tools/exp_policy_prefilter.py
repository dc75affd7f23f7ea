#!/usr/bin/env python3
"""How many first-fit passes of the group kernel the links' longest free runs rule out -- on the CPU
oracle alone, no GPU.

The group kernel weighs PP = 16 // W candidate paths of a row's request per pass (W = 64-bit words per link) and runs a further
pass while any row of the wave -- four environments in lockstep, environments 4q .. 4q + 3 -- has found no window.  A path can
hold a window of n slots only if every one of its links has a longest free run ml >= n, and the DEFER instantiations keep ml of
every link in LDS (lsum_pack).  This tool steps the oracle one request at a time, evaluates that test on the occupancy every
step meets and counts, per quad-step, the passes of three schedules:

  today      a later pass runs while some row has found no window
  prefilter  ... and only if such a row has a candidate (ml >= n on every link) among that pass's paths
  compacted  every pass holds PP of the row's candidates (estimated and not built: DESIGN 3)

and the share of the later passes' paths whose tightest link decides the test by one slot (ml == n kept, ml == n - 1 dropped).
The functions are what tests/test_policy_prefilter.py pins its cases with.

usage: python tools/exp_policy_prefilter.py [--topology NAME] [--slots S] [--load L] [--seed0 10] [--envs 16] [--warmup 1000]
                                            [--steps 2500]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNEL_WIDTH = 12.5
RULED_OUT, KEPT_FOUND, KEPT_NONE = range(3)   # what a later pass is to a row that reaches it


def words_per_link(S):
    w = (S + 63) // 64
    return 8 if w == 7 else w


def longest_runs(avail):
    """[E] longest run of ones of every row of avail [E, S] (slots at and beyond S do not exist: a run ends at S)"""
    E = avail.shape[0]
    z = np.zeros((E, 1), np.int8)
    d = np.diff(np.concatenate((z, avail.astype(np.int8), z), axis=1), axis=1)
    out = np.zeros(E, np.int64)
    for e in range(E):
        up = np.flatnonzero(d[e] == 1)
        if up.size:
            out[e] = (np.flatnonzero(d[e] == -1) - up).max()
    return out


def first_fit(rows, n):
    """the lowest s in range(0, S - n) with [s, s + n) free on every row (rmsa_env.py:860-871); none: -1"""
    S = rows.shape[1]
    x = rows.min(axis=0).astype(np.int64)
    if not 1 <= n < S:
        return -1
    c = np.concatenate(([0], np.cumsum(x)))
    ok = np.flatnonzero((c[n:S] - c[:S - n]) == n)   # starts 0 .. S - n - 1
    return int(ok[0]) if ok.size else -1


def step_record(avail, topo, src, dst, bit_rate, channel_width=CHANNEL_WIDTH):
    """Per candidate path of the request on avail [E, S]: n (slots), ml (the longest free run of its tightest link), start (its
    first fit, -1: none) -- three [K] arrays."""
    K = topo.k_paths
    base = int(topo.pair_path_base[src * topo.num_nodes + dst])
    ml_link = longest_runs(avail)
    n, ml, start = (np.zeros(K, np.int64) for _ in range(3))
    for p in range(K):
        gid = base + p
        links = np.asarray(topo.path_links[topo.path_link_off[gid]:topo.path_link_off[gid + 1]], np.int64)
        n[p] = int(np.ceil(bit_rate / (int(topo.path_se[gid]) * channel_width))) + 1   # get_number_slots (rmsa_env.py:708-719)
        ml[p] = ml_link[links].min()
        start[p] = first_fit(avail[links], int(n[p]))
    return n, ml, start


def oracle_trace(topo, kw, seed, steps, warmup=0):
    """One oracle environment under sap_ff, `warmup` steps and then `steps` recorded ones: n, ml, start [steps, K] of what every
    step met.  The oracle's own decision is held to the record's: the first path with a fit and that fit, else a refusal."""
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from conftest import oracle_env_from_kwargs
    o = oracle_env_from_kwargs(topo, kw, seed=seed)
    if warmup:
        o.run("sap_ff", warmup, reset_on_done=True, fields=[])
    recs = []
    for _ in range(steps):
        r = o.request()
        n, ml, start = step_record(o.available_slots(), topo, r.src, r.dst, r.bit_rate, kw.get("channel_width", CHANNEL_WIDTH))
        tr = o.run("sap_ff", 1, reset_on_done=True, fields=["act_path", "act_slot", "accepted"])
        fits = np.flatnonzero(start >= 0)
        if fits.size:
            assert tr["accepted"][0] and tr["act_path"][0] == fits[0] and tr["act_slot"][0] == start[fits[0]], (seed, len(recs))
        else:
            assert not tr["accepted"][0], (seed, len(recs))
        recs.append((n, ml, start))
    o.close()
    return tuple(np.stack([r[i] for r in recs]) for i in range(3))


def row_passes(n, ml, start, PP):
    """One row's step: (classes of the later passes it reaches [RULED_OUT / KEPT_FOUND / KEPT_NONE per pass from the second on],
    the pass that finds its window or -1, per later pass whether a row that still looks has a candidate in it)."""
    K = len(n)
    cand, fit = ml >= n, start >= 0
    assert not (fit & ~cand).any(), "a path with a first fit fails the ml test"
    found_in = -1
    classes = []
    for j, p0 in enumerate(range(0, K, PP)):
        sl = slice(p0, min(p0 + PP, K))
        if j > 0:
            classes.append(RULED_OUT if not cand[sl].any() else (KEPT_FOUND if fit[sl].any() else KEPT_NONE))
        if fit[sl].any():
            found_in = j
            break
    return classes, found_in


def quad_passes(rows, PP):
    """rows: (n, ml, start) [K] each of a quad's rows at one step.  Passes the quad-step runs under (today, prefilter, compacted)."""
    K = len(rows[0][0])
    n_pass = -(-K // PP)
    info = [row_passes(*r, PP) for r in rows]
    last = [f if f >= 0 else n_pass - 1 for _, f in info]       # the last pass a row looks in
    today = 1 + max(last)
    pre = 1
    for j in range(1, n_pass):
        # a later pass runs if a row that reaches it has a candidate in it
        pre += any(j <= l and cls[j - 1] != RULED_OUT for (cls, _), l in zip(info, last))
    comp = 0
    for n, ml, start in rows:
        c = np.flatnonzero(ml >= n)
        hit = np.flatnonzero(start[c] >= 0)
        comp = max(comp, (int(hit[0]) // PP + 1) if hit.size else -(-len(c) // PP))
    return today, pre, comp


def summarize(traces, W, K):
    """traces: per environment (n, ml, start) [steps, K]; environments 4q .. 4q + 3 are a quad.  The table's figures."""
    PP = 16 // W
    steps = traces[0][0].shape[0]
    rows = later_row = blocked = kept_row = no_cand = 0
    tot = np.zeros(3, np.int64)
    second = np.zeros(2, np.int64)
    quads = 0
    tight = np.zeros(3, np.int64)   # later-pass paths a row examines: all, ml == n, ml == n - 1
    per_quad = []
    for q0 in range(0, len(traces) - len(traces) % 4, 4):
        qt = np.zeros(3, np.int64)
        for t in range(steps):
            quad = [tuple(a[t] for a in traces[q0 + i]) for i in range(4)]
            p = quad_passes(quad, PP)
            qt += p
            second += (p[0] > 1, p[1] > 1)
            for n, ml, start in quad:
                cls, found_in = row_passes(n, ml, start, PP)
                rows += 1
                later_row += len(cls) > 0
                blocked += found_in < 0
                kept_row += any(c != RULED_OUT for c in cls)
                no_cand += not (ml >= n).any()
                for j, _ in enumerate(cls, 1):
                    sl = slice(j * PP, min((j + 1) * PP, K))
                    tight += (sl.stop - sl.start, int((ml[sl] == n[sl]).sum()), int((ml[sl] == n[sl] - 1).sum()))
        quads += steps
        tot += qt
        per_quad.append((qt / steps).round(3).tolist())
    return dict(W=W, PP=PP, K=K, rows=rows, quad_steps=quads,
                rows_need_later_pass=later_row / rows, rows_blocked=blocked / rows, rows_fit_later=(later_row - blocked) / rows,
                rows_later_pass_kept=kept_row / rows, rows_without_candidate=no_cand / rows,
                passes_today=tot[0] / quads, passes_prefilter=tot[1] / quads, passes_compacted=tot[2] / quads,
                quad_steps_second_pass_today=second[0] / quads, quad_steps_second_pass_prefilter=second[1] / quads,
                per_quad=per_quad, later_paths=int(tight[0]), later_paths_ml_eq_n=tight[1] / max(tight[0], 1),
                later_paths_ml_eq_n_minus_1=tight[2] / max(tight[0], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--topology", default="nsfnet_chen_5-paths_6-modulations", help="a topology of tests/golden/topologies")
    ap.add_argument("--slots", type=int, default=320)
    ap.add_argument("--load", type=float, default=50)
    ap.add_argument("--seed0", type=int, default=10)
    ap.add_argument("--envs", type=int, default=16, help="environments (a multiple of four: quads)")
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=2500)
    args = ap.parse_args()
    for p in (ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    from conftest import load_topology
    topo = load_topology(args.topology)
    kw = dict(num_spectrum_resources=args.slots, load=args.load, mean_service_holding_time=25, episode_length=1000)
    traces = [oracle_trace(topo, kw, args.seed0 + i, args.steps, args.warmup) for i in range(args.envs)]
    s = summarize(traces, words_per_link(args.slots), topo.k_paths)
    print(json.dumps(dict(topology=args.topology, slots=args.slots, load=args.load, seeds=[args.seed0, args.seed0 + args.envs - 1],
                          warmup=args.warmup, steps=args.steps, **s)))
    print("                                              share of rows                       passes per quad-step")
    print(f"today: a pass while a row has no window       {100 * s['rows_need_later_pass']:.1f} % look further ({100 * s['rows_blocked']:.1f} % blocked, "
          f"{100 * s['rows_fit_later']:.1f} % fit later)   {s['passes_today']:.3f}")
    print(f"prefilter: ... and a candidate by ml >= n     {100 * s['rows_later_pass_kept']:.1f} %   {s['passes_prefilter']:.3f}")
    print(f"compacted: every pass over candidates only    {100 * s['rows_without_candidate']:.1f} % need no pass at all   {s['passes_compacted']:.3f}")
    print(f"quad-steps with a second pass: {100 * s['quad_steps_second_pass_today']:.1f} % -> {100 * s['quad_steps_second_pass_prefilter']:.1f} %")
    print(f"later-pass paths decided by one slot: ml == n {100 * s['later_paths_ml_eq_n']:.2f} %, ml == n - 1 "
          f"{100 * s['later_paths_ml_eq_n_minus_1']:.2f} % of {s['later_paths']}")


if __name__ == "__main__":
    main()
