#!/usr/bin/env python3
"""What most-used assignment and the best-window-over-all-paths route cost and what they do to blocking (include/orlg.h
orlg_step_window): NSFNET-320, 1000 steps per launch -- B = 4096 on the wave-per-environment kernel and B = 65 536 on
the four-environments-per-wave kernel.  At the load of the throughput comparison (50) one handle per policy on the same seeds
(`sap_ff`, `sap_ff_full`, `sap_mc` as yardsticks; `sap_mu`, `any_ff_full`, `any_bf`, `any_mu`), alternating launch by launch so
that they share whatever else the machine does.  Prints one JSON line: env-steps/s of each (median of the repeats, with their
range), the kernel each ran, its rate relative to `sap_ff_full`, and per load (30 and 50) from one more launch with cause_counts
in the steady state the blocking probability and the blocking probability of either half of the batch -- two blocking figures
differ only by more than the halves do.
usage: python tools/bench_window_rules.py [--kernels wave,group] [--steps K] [--repeats R] [--loads 30,50] [--policies a,b,..]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCH = {"wave": 4096, "group": 65536}
POLICIES = ("sap_ff", "sap_ff_full", "sap_mc", "sap_mu", "any_ff_full", "any_bf", "any_mu")
TIMED_LOAD = 50.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", default="wave,group")
    ap.add_argument("--batch", type=int, default=0, help="0: 4096 on the wave kernel, 65536 on the group kernel")
    ap.add_argument("--steps", type=int, default=1000, help="steps per launch")
    ap.add_argument("--warmup", type=int, default=2, help="launches before the timed ones")
    ap.add_argument("--repeats", type=int, default=7, help="timed launches per handle")
    ap.add_argument("--loads", default="30,50", help="loads of the blocking table; the throughput comparison runs at 50 if listed")
    ap.add_argument("--policies", default=",".join(POLICIES), help="sap_ff_full must be among them")
    args = ap.parse_args()
    import numpy as np
    from conftest import load_topology
    from optical_rl_gym_amd import BatchedRMSAEnv
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    loads = [float(x) for x in args.loads.split(",")]
    modes = tuple(args.policies.split(","))
    out = {"metric": "env steps/s and blocking, RMSA NSFNET-320, most-used windows and the best window over all paths against first fit",
           "steps_per_launch": args.steps, "repeats": args.repeats}
    for kernel in args.kernels.split(","):
        batch = args.batch or BATCH[kernel]
        res = {"batch": batch}
        for load in loads:
            timed = load == TIMED_LOAD
            kw = dict(num_spectrum_resources=320, load=load, mean_service_holding_time=25, episode_length=1000, seed=10)
            envs = {m: BatchedRMSAEnv(topo, batch, step_kernel=kernel, **kw) for m in modes}

            def launch(m, **run_kw):
                r = envs[m].run(m, args.steps, auto_reset=True, **run_kw)
                envs[m].synchronize()
                return r

            for _ in range(args.warmup):
                for m in modes:
                    launch(m)
            at = {}
            if timed:
                times = {m: [] for m in modes}
                for _ in range(args.repeats):
                    for m in modes:
                        t0 = time.perf_counter()
                        launch(m)
                        times[m].append(time.perf_counter() - t0)
                work = batch * args.steps
                for m in modes:
                    at[m] = {"value": work / statistics.median(times[m]), "min": work / max(times[m]), "max": work / min(times[m]),
                             "kernel": envs[m].last_kernel()}
                for m in modes:
                    at[m]["relative_to_sap_ff_full"] = at[m]["value"] / at["sap_ff_full"]["value"]
            for m in modes:   # (not timed) blocking of one more launch, the whole batch and its two halves
                per_env = launch(m, cause_counts=True)["block_cause_counts"].astype(np.int64)
                counts = per_env.sum(axis=0)
                d = at.setdefault(m, {})
                d["blocking_probability"] = float(1 - counts[0] / counts.sum())
                halves = [per_env[:batch // 2].sum(axis=0), per_env[batch // 2:].sum(axis=0)]
                d["blocking_probability_halves"] = [float(1 - h[0] / h.sum()) for h in halves]
            for env in envs.values():
                env.close()
            res[f"load_{load:g}"] = at
        out[kernel] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
