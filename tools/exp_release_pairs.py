#!/usr/bin/env python3
"""Iteration model of the group kernel's release loop (csrc/orlg_group_body.h, SEC(9)-SEC(11)).  CPU only: the oracle's trace of
the headline workload (RMSA NSFNET-320, load 50, sap_ff) and three rules for how many due services one pass of the loop releases
per row.  It counts passes per env-step and per quad-step (four environments in step: the loop runs until the slowest row has
nothing due).  A model of iteration counts, not a measurement of the kernel.

    python tools/exp_release_pairs.py [--seeds 10 25] [--steps 10000] [--warmup 2000] [--load 50]

  one    the head only (the kernel before the paired release)
  two    the head and the entry behind it where that is due too, both paths have at most 8 hops and they share no link
  four   up to four consecutive due entries of at most 4 hops each that share no link pairwise

Under rule `two` it also counts the passes in which no row of the quad has a due entry behind its head (two_passes_b_free_share, and
those that are a quad-step's first pass per quad-step): the passes that need none of the pair's machinery."""
import argparse
import bisect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np

RULES = (("one", 1, 16), ("two", 2, 8), ("four", 4, 4))   # (name, services per pass, lanes = most hops per service)


def passes(due, width, max_hops):
    """How many passes release the due services `due` (link sets, in release order): each pass takes the head and, of the entries
    behind it in order, up to width - 1 more while all taken so far have at most max_hops links and share none.  A pass of one
    takes the head whatever its length."""
    n, i = 0, 0
    while i < len(due):
        taken, k = set(due[i]), 1
        while (k < width and i + k < len(due) and max(len(due[i]), len(due[i + k])) <= max_hops
               and not (taken & due[i + k])):
            taken |= due[i + k]
            k += 1
        i += k
        n += 1
    return n


def due_behind_head(due):
    """Rule `two`, pass by pass: whether the entry behind the head is due when the pass begins (what the row votes with)."""
    out, i = [], 0
    while i < len(due):
        out.append(i + 1 < len(due))
        pair = i + 1 < len(due) and max(len(due[i]), len(due[i + 1])) <= 8 and not (due[i] & due[i + 1])
        i += 2 if pair else 1
    return out


def b_free_share(votes):
    """votes[seed][step] = due_behind_head of that row and step.  The passes of a quad-step run to its slowest row; a pass is
    B-free where no row that still releases has a due entry behind its head.  Returns (passes, B-free passes, B-free FIRST
    passes) over whole quads of seeds."""
    n = nb = nb_first = 0
    for q in range(0, len(votes), 4):
        for rows in zip(*votes[q:q + 4]):
            for j in range(max(len(r) for r in rows)):
                free = not any(r[j] for r in rows if j < len(r))
                n, nb, nb_first = n + 1, nb + free, nb_first + (free and j == 0)
    return n, nb, nb_first


def replay(topo, tr, warmup):
    """Per step from `warmup` on: the passes of each rule, the step's consecutive due pairs as (pairs, link-disjoint pairs) and
    its votes under rule `two` (due_behind_head); the longest released path."""
    N = topo.num_nodes
    arrival, holding, accepted = np.asarray(tr["arrival"]), np.asarray(tr["holding"]), np.asarray(tr["accepted"]) != 0
    gid = topo.pair_path_base[np.asarray(tr["src"]) * N + np.asarray(tr["dst"])] + np.asarray(tr["act_path"])
    ring, sets = [], []   # release times in time order (ties in insert order), and each entry's links
    rows, pairs, votes, longest = [], [], [], 0
    for t in range(len(accepted)):
        if accepted[t]:
            k = bisect.bisect_right(ring, arrival[t] + holding[t])
            ring.insert(k, arrival[t] + holding[t])
            sets.insert(k, frozenset(topo.path_links[topo.path_link_off[gid[t]]:topo.path_link_off[gid[t] + 1]].tolist()))
        due = []
        if t + 1 < len(accepted):
            n = bisect.bisect_right(ring, arrival[t + 1])
            due, ring, sets = sets[:n], ring[n:], sets[n:]
        if t >= warmup:
            rows.append([passes(due, w, h) for _, w, h in RULES])
            pairs.append((max(len(due) - 1, 0), sum(1 for a, b in zip(due, due[1:]) if not (a & b))))
            votes.append(due_behind_head(due))
            longest = max([longest] + [len(d) for d in due])
    return np.array(rows), np.array(pairs), votes, longest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs=2, default=(10, 25), metavar=("FIRST", "LAST"))
    ap.add_argument("--steps", type=int, default=10000, help="steady-state steps per seed")
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--load", type=float, default=50)
    args = ap.parse_args()
    from conftest import load_topology, oracle_env_from_kwargs
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    n_seeds = args.seeds[1] - args.seeds[0] + 1
    assert n_seeds % 4 == 0, "whole quads of seeds"
    rows, pairs, votes, longest = [], [], [], 0
    for seed in range(args.seeds[0], args.seeds[1] + 1):
        kw = dict(num_spectrum_resources=320, load=args.load, mean_service_holding_time=25, episode_length=1000, seed=seed)
        o = oracle_env_from_kwargs(topo, kw, seed=seed)
        tr = o.run("sap_ff", args.warmup + args.steps, reset_on_done=True)
        o.close()
        r, p, v, h = replay(topo, tr, args.warmup)
        rows.append(r); pairs.append(p); votes.append(v); longest = max(longest, h)
    rows, pairs = np.stack(rows), np.concatenate(pairs)                       # [seed, step, rule], [seed x step, 2]
    quads = rows.reshape(n_seeds // 4, 4, rows.shape[1], len(RULES)).max(axis=1)   # the loop runs to the slowest of a wave's four rows
    n_pass, n_free, n_free_first = b_free_share(votes)
    names = [r[0] for r in RULES]
    rnd = lambda v: dict(zip(names, (round(float(x), 3) for x in v)))
    out = {"workload": f"RMSA NSFNET-320 load {args.load:g} sap_ff, seeds {args.seeds[0]}..{args.seeds[1]}, {args.steps} steps each "
                       f"after {args.warmup}",
           "releases_per_env_step": round(float(rows[..., 0].mean()), 3),
           "poisson_quad_step": round(float(poisson_max4(rows[..., 0].mean())), 3),
           "iterations_per_env_step": rnd(rows.mean(axis=(0, 1))),
           "iterations_per_quad_step": rnd(quads.mean(axis=(0, 1))),
           "p_quad_step_ge_2": rnd((quads >= 2).mean(axis=(0, 1))),
           "p_quad_step_ge_3": rnd((quads >= 3).mean(axis=(0, 1))),
           "two_passes_b_free_share": round(n_free / max(1, n_pass), 3),
           "two_passes_b_free_first_per_quad_step": round(n_free_first / quads.shape[1] / quads.shape[0], 3),
           "due_consecutive_pairs_link_disjoint": round(float(pairs[:, 1].sum() / max(1, pairs[:, 0].sum())), 3),
           "longest_released_path_hops": int(longest)}
    print(json.dumps(out, indent=1))


def poisson_max4(lam):
    """E[max of four independent Poisson(lam) counts]: what the releases per quad-step would be without their clustering."""
    from math import exp, factorial
    cdf, e, k = 0.0, 0.0, 0
    while cdf < 1.0 - 1e-12:
        cdf_next = cdf + exp(-lam) * lam ** k / factorial(k)
        e += k * (cdf_next ** 4 - cdf ** 4)
        cdf, k = cdf_next, k + 1
    return e


if __name__ == "__main__":
    main()
