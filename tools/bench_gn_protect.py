#!/usr/bin/env python3
"""What protecting the running lightpaths costs (include/orlg.h orlg_set_gn_protect): NSFNET-320, load 50, +6 dBm per
50 GHz, B = 4096, 1000 steps per launch -- a gated handle and a protecting handle, under sap_ff and under sap_ff_gn, in ONE run,
the handles alternating so that they share whatever else the machine does.  Prints one JSON line: env-steps/s of each (median of the
repeats, and their spread), the kernel each ran, and for the protecting handles the share of steps with a neighbour check and the
share that check refused.  usage: python tools/bench_gn_protect.py [--batch B] [--steps K] [--repeats R]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1000, help="steps per launch")
    ap.add_argument("--warmup", type=int, default=2, help="launches before the timed ones")
    ap.add_argument("--repeats", type=int, default=5, help="timed launches per handle")
    ap.add_argument("--load", type=float, default=50)
    ap.add_argument("--power", type=float, default=6.0, help="launch power, dBm per 50 GHz")
    args = ap.parse_args()
    import numpy as np
    from conftest import load_topology
    from optical_rl_gym_amd import BatchedRMSAEnv, rmsa_gn_gate_parameters
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    kw = dict(num_spectrum_resources=320, load=args.load, mean_service_holding_time=25, episode_length=1000, seed=10)
    runs = {}   # name -> (handle, policy): a handle per (kind, policy), so that every handle keeps the load its own decisions give
    for policy in ("sap_ff", "sap_ff_gn"):
        for kind, protect in (("gated", False), ("protecting", True)):
            gate = rmsa_gn_gate_parameters(topo, launch_power_dbm_per_50ghz=args.power, protect_running=protect)
            runs[f"{kind}_{policy}"] = (BatchedRMSAEnv(topo, args.batch, gn_gate=gate, **kw), policy)

    def launch(env, policy):
        env.run(policy, args.steps, auto_reset=True)
        env.synchronize()

    for _ in range(args.warmup):
        for env, policy in runs.values():
            launch(env, policy)
    times = {name: [] for name in runs}
    for _ in range(args.repeats):
        for name, (env, policy) in runs.items():
            t0 = time.perf_counter()
            launch(env, policy)
            times[name].append(time.perf_counter() - t0)
    out = {"metric": f"env steps/s, RMSA NSFNET-320 load {args.load:g} at {args.power:g} dBm per 50 GHz, gate that protects the running lightpaths",
           "batch": args.batch, "steps_per_launch": args.steps, "repeats": args.repeats}
    work = args.batch * args.steps
    for name, (env, policy) in runs.items():
        out[name] = {"value": work / statistics.median(times[name]), "min": work / max(times[name]), "max": work / min(times[name]),
                     "kernel": env.last_kernel(), "mean_running": float(env.num_running().mean())}
    # what the checks do, from one more launch each with the outputs (not timed)
    for name, (env, policy) in runs.items():
        r = env.run(policy, min(args.steps, 200), auto_reset=True, outputs=("gn_gsnr_db", "gn_neighbour_margin_db", "accepted"))
        checked, n_checked = np.isfinite(r["gn_gsnr_db"]), np.isfinite(r["gn_neighbour_margin_db"])
        n_refused = r["gn_neighbour_margin_db"] < 0
        out[name].update(share_checked=float(checked.mean()), share_rejected=float((checked & (r["accepted"] == 0)).mean()),
                         share_neighbour_checked=float(n_checked.mean()), share_neighbour_refused=float(n_refused.mean()),
                         share_neighbour_refused_of_checked=float(n_refused.sum() / max(int(n_checked.sum()), 1)))
    print(json.dumps(out))
    for env, _ in runs.values():
        env.close()


if __name__ == "__main__":
    main()
