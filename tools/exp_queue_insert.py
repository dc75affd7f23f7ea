#!/usr/bin/env python3
"""Iteration model of the group kernel's release-queue insert (csrc/orlg_group_body.h, SEC(5)).  CPU only: the oracle's trace of
the headline workload (RMSA NSFNET-320, load 50, sap_ff) and three scan rules over the sorted ring.  It counts 16-entry chunks
visited per insert -- one chunk is one dependent LDS round trip of the kernel's loop -- per accepted row and per quad-step (four
environments in step: the loop runs until the slowest row is done).  A model of iteration counts, not a measurement of the kernel.

    python tools/exp_queue_insert.py [--seeds 10 17] [--steps 10000] [--warmup 2000] [--load 50]

  aligned    chunks aligned to multiples of 16 above the head, from the top chunk down (the kernel before round 12)
  anchored   chunks anchored at the last entry: the first chunk is always 16 live entries
  nearer     anchored chunks from the nearer end: one compare with the middle entry, q_n // 2, picks the side"""
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

CH = 16


def chunks_visited(n, k):
    """(aligned, anchored, nearer) chunk visits of an insert at rank k (k entries stay below it) into a ring of n entries.  A
    scan stops in the first chunk that holds an entry which stays, or when it has run out of entries."""
    if n == 0:
        return 0, 0, 0
    top = (n - 1) // CH                                   # aligned: chunk c holds entries 16 c .. 16 c + 15
    aligned = top + 1 if k == 0 else top - (k - 1) // CH + 1
    up = -(-n // CH) if k == 0 else (n - k) // CH + 1     # anchored from the top: entry k - 1, which stays, is in chunk (n - k) // 16
    down = -(-n // CH) if k == n else k // CH + 1         # from the head: entry k is the first that stays
    # (bisect_right: the new entry is strictly earlier than entry n // 2 exactly when k <= n // 2; the read of that entry is one
    # more LDS round trip per insert, which the counts leave out)
    return aligned, up, down if k <= n // 2 else up


def replay(arrival, holding, accepted, warmup):
    """Per step from `warmup` on: (aligned, anchored, nearer) chunk visits of the step's insert (zeros where nothing was
    inserted), the ring's size at the insert, and the number of releases after it."""
    ring, rows, sizes, pops = [], [], [], []
    for t in range(len(accepted)):
        v = (0, 0, 0)
        if accepted[t]:
            rel, n = arrival[t] + holding[t], len(ring)
            k = bisect.bisect_right(ring, rel)
            v = chunks_visited(n, k)
            if t >= warmup:
                sizes.append(n)
            ring.insert(k, rel)
        n_pop = 0
        if t + 1 < len(accepted):
            while ring and ring[0] <= arrival[t + 1]:
                ring.pop(0)
                n_pop += 1
        if t >= warmup:
            rows.append(v)
            pops.append(n_pop)
    return np.array(rows), np.array(sizes), np.array(pops)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs=2, default=(10, 17), metavar=("FIRST", "LAST"))
    ap.add_argument("--steps", type=int, default=10000, help="steady-state steps per seed")
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--load", type=float, default=50)
    args = ap.parse_args()
    from conftest import load_topology, oracle_env_from_kwargs
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    n_seeds = args.seeds[1] - args.seeds[0] + 1
    assert n_seeds % 4 == 0, "whole quads of seeds"
    rows, sizes, pops, acc = [], [], [], []
    for seed in range(args.seeds[0], args.seeds[1] + 1):
        kw = dict(num_spectrum_resources=320, load=args.load, mean_service_holding_time=25, episode_length=1000, seed=seed)
        o = oracle_env_from_kwargs(topo, kw, seed=seed)
        tr = o.run("sap_ff", args.warmup + args.steps, reset_on_done=True)
        o.close()
        accepted = np.asarray(tr["accepted"]) != 0
        r, s, p = replay(np.asarray(tr["arrival"]), np.asarray(tr["holding"]), accepted, args.warmup)
        rows.append(r); sizes.append(s); pops.append(p); acc.append(accepted[args.warmup:])
    rows, acc = np.stack(rows), np.stack(acc)                        # [seed, step, rule], [seed, step]
    per_row = rows.sum(axis=(0, 1)) / acc.sum()
    quads = rows.reshape(n_seeds // 4, 4, rows.shape[1], 3).max(axis=1)   # the loop runs to the slowest of a wave's four rows
    per_quad = quads.mean(axis=(0, 1))
    out = {"workload": f"RMSA NSFNET-320 load {args.load:g} sap_ff, seeds {args.seeds[0]}..{args.seeds[1]}, {args.steps} steps each "
                       f"after {args.warmup}",
           "acceptance": float(acc.mean()), "mean_q_n_at_insert": float(np.concatenate(sizes).mean()),
           "releases_per_step": float(np.concatenate(pops).mean()),
           "iterations_per_accepted_row": dict(zip(("aligned", "anchored", "nearer"), (round(float(x), 3) for x in per_row))),
           "iterations_per_quad_step": dict(zip(("aligned", "anchored", "nearer"), (round(float(x), 3) for x in per_quad)))}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
