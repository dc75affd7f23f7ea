#!/usr/bin/env python3
"""What the GN-model admission check of the slot-based step costs (include/orlg.h orlg_rmsa_gn_gate): NSFNET-320,
load 50, sap_ff, B = 4096, 1000 steps per launch -- ungated, gated at 0 dBm per 50 GHz (every check passes: the decisions are the
ungated ones) and gated at +6 dBm, in ONE run, the three handles alternating so that they share whatever else the machine does.
Prints one JSON line: env-steps/s of each (median of the repeats, and their spread), the kernel each ran, and the share of steps
the +6 dBm gate checked and refused.  usage: python tools/bench_rmsa_gn.py [--batch B] [--steps K] [--repeats R]"""
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
    ap.add_argument("--policy", default="sap_ff")
    args = ap.parse_args()
    import numpy as np
    from conftest import load_topology
    from optical_rl_gym_amd import BatchedRMSAEnv, rmsa_gn_gate_parameters
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    kw = dict(num_spectrum_resources=320, load=args.load, mean_service_holding_time=25, episode_length=1000, seed=10)
    envs = {"ungated": BatchedRMSAEnv(topo, args.batch, **kw),
            "gated_0dbm": BatchedRMSAEnv(topo, args.batch, gn_gate=rmsa_gn_gate_parameters(topo), **kw),
            "gated_6dbm": BatchedRMSAEnv(topo, args.batch, gn_gate=rmsa_gn_gate_parameters(topo, launch_power_dbm_per_50ghz=6.0), **kw)}

    def launch(env):
        env.run(args.policy, args.steps, auto_reset=True)
        env.synchronize()

    for _ in range(args.warmup):
        for env in envs.values():
            launch(env)
    times = {name: [] for name in envs}
    for _ in range(args.repeats):
        for name, env in envs.items():
            t0 = time.perf_counter()
            launch(env)
            times[name].append(time.perf_counter() - t0)
    out = {"metric": f"env steps/s, RMSA NSFNET-320 load {args.load:g} {args.policy}, GN-model admission check", "batch": args.batch,
           "steps_per_launch": args.steps, "repeats": args.repeats}
    work = args.batch * args.steps
    for name, env in envs.items():
        out[name] = {"value": work / statistics.median(times[name]), "min": work / max(times[name]), "max": work / min(times[name]),
                     "kernel": env.last_kernel(), "mean_running": float(env.num_running().mean())}
    # what the gates do, from one more launch each with the outputs (not timed)
    for name in ("gated_0dbm", "gated_6dbm"):
        r = envs[name].run(args.policy, min(args.steps, 200), auto_reset=True, outputs=("gn_gsnr_db", "accepted"))
        checked = np.isfinite(r["gn_gsnr_db"])
        refused = checked & (r["accepted"] == 0)
        out[name].update(share_checked=float(checked.mean()), share_rejected=float(refused.mean()),
                         share_rejected_of_checked=float(refused.sum() / max(int(checked.sum()), 1)))
    print(json.dumps(out))
    for env in envs.values():
        env.close()


if __name__ == "__main__":
    main()
