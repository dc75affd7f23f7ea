#!/usr/bin/env python3
"""What the assignment rules cost and what they do to blocking (include/orlg.h orlg_step_assign): NSFNET-320, load 50,
the `sap` route, 1000 steps per launch -- B = 4096 on the wave-per-environment kernel and B = 65 536 on the four-environments-per-wave
kernel.  Per kernel one handle per rule on the same seeds (`sap_ff`, `sap_ff_full`, `sap_lf`, `sap_bf`, `sap_ef`) and the yardstick
`plain_kind` (`sap_ff` under ORLG_NO_DEFER: the plain kind of instantiation a launch under a new rule runs, without the new code),
alternating launch by launch so that they share whatever else the machine does.  Prints one JSON line: env-steps/s of each (median of
the repeats, with their range), the kernel each ran, its rate relative to the yardstick, and from one more launch with cause_counts
the blocking probability and the blocking shares by cause in the steady state the timed launches ran in.
usage: python tools/bench_assign_rules.py [--kernels wave,group] [--steps K] [--repeats R] [--route sap]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCH = {"wave": 4096, "group": 65536}
SUFFIXES = ("ff", "ff_full", "lf", "bf", "ef")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", default="wave,group")
    ap.add_argument("--batch", type=int, default=0, help="0: 4096 on the wave kernel, 65536 on the group kernel")
    ap.add_argument("--steps", type=int, default=1000, help="steps per launch")
    ap.add_argument("--warmup", type=int, default=2, help="launches before the timed ones")
    ap.add_argument("--repeats", type=int, default=7, help="timed launches per handle")
    ap.add_argument("--load", type=float, default=50)
    ap.add_argument("--route", default="sap", choices=("sp", "sap", "llp"))
    args = ap.parse_args()
    import numpy as np
    from conftest import load_topology
    from optical_rl_gym_amd import BLOCK_CAUSES, BatchedRMSAEnv
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    kw = dict(num_spectrum_resources=320, load=args.load, mean_service_holding_time=25, episode_length=1000, seed=10)
    out = {"metric": f"env steps/s, RMSA NSFNET-320 load {args.load:g} route {args.route}, assignment rules",
           "steps_per_launch": args.steps, "repeats": args.repeats}
    policies = {s: f"{args.route}_{s}" for s in SUFFIXES}
    for kernel in args.kernels.split(","):
        batch = args.batch or BATCH[kernel]
        modes = ("plain_kind",) + SUFFIXES
        envs = {m: BatchedRMSAEnv(topo, batch, step_kernel=kernel, **kw) for m in modes}

        def launch(m, **run_kw):
            if m == "plain_kind":   # (the library reads its tooling variables at every launch)
                os.environ["ORLG_NO_DEFER"] = "1"
            try:
                r = envs[m].run(policies.get(m, policies["ff"]), args.steps, auto_reset=True, **run_kw)
                envs[m].synchronize()
                return r
            finally:
                os.environ.pop("ORLG_NO_DEFER", None)

        for _ in range(args.warmup):
            for m in modes:
                launch(m)
        times = {m: [] for m in modes}
        for _ in range(args.repeats):
            for m in modes:
                t0 = time.perf_counter()
                launch(m)
                times[m].append(time.perf_counter() - t0)
        work = batch * args.steps
        res = {"batch": batch}
        for m in modes:
            res[m] = {"value": work / statistics.median(times[m]), "min": work / max(times[m]), "max": work / min(times[m]),
                      "kernel": envs[m].last_kernel()}
        for m in modes:
            res[m]["relative_to_plain_kind"] = res[m]["value"] / res["plain_kind"]["value"]
            # (not timed) blocking by cause of one more launch
            counts = launch(m, cause_counts=True)["block_cause_counts"].astype(np.int64).sum(axis=0)
            res[m]["blocking_probability"] = float(1 - counts[0] / counts.sum())
            blocked = max(int(counts[1:].sum()), 1)
            res[m]["blocking_shares"] = {name: float(counts[c] / blocked) for c, name in enumerate(BLOCK_CAUSES) if c}
        for env in envs.values():
            env.close()
        out[kernel] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
