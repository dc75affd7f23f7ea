#!/usr/bin/env python3
"""What the GN-model audit of the running lightpaths costs, and what it finds (include/orlg.h orlg_gn_audit), in ONE
run with the calls alternating so that they share whatever else the machine does.  NSFNET-320 gated at +6 dBm per 50 GHz, B = 4096,
at load 50 and load 150, after --steps steps of sap_ff.  Per load, on the gated handle, the time of one call (median of the
repeats, the stream synchronised after each):
    qot_audit             the [B] summaries, read back to the host
    qot_audit+services    the summaries and the four [B, Q] per-service arrays, into device buffers
    path_ff_gn            action_masks("path_ff_gn") into a device buffer: the yardstick, one GSNR per candidate path
and the time of the --steps-step gated launch that built the state.  Beside them what the audit found on the gated and on a
protecting handle (protect_running=True) after the same number of steps: mean n_running and n_below per environment, the share
n_below / n_running, the smallest margin.  Prints one JSON line.
usage: python tools/bench_gn_audit.py [--repeats R] [--warmup W] [--steps K] [--batch B]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def found(env):
    import numpy as np
    a = env.qot_audit()
    n, below = int(a["n_running"].sum()), int(a["n_below"].sum())
    return {"mean_n_running": n / env.batch_size, "mean_n_below": below / env.batch_size, "share_below": below / max(n, 1),
            "envs_with_one_below": float((a["n_below"] > 0).mean()), "min_margin_db": float(np.nanmin(a["min_margin_db"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=25, help="timed calls of each kind")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1000, help="steps of sap_ff before the audit")
    ap.add_argument("--batch", type=int, default=4096)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")   # (torch creates its HIP context before the library does)
    from conftest import load_topology
    from optical_rl_gym_amd import BatchedRMSAEnv, rmsa_gn_gate_parameters
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    out = {"metric": "seconds per call (median), GN-model audit of the running lightpaths", "repeats": args.repeats,
           "batch": args.batch, "steps": args.steps}
    for load in (50, 150):
        make = lambda protect: BatchedRMSAEnv(topo, args.batch, num_spectrum_resources=320, load=load, mean_service_holding_time=25,
                                              episode_length=1000, seed=10,
                                              gn_gate=rmsa_gn_gate_parameters(topo, launch_power_dbm_per_50ghz=6.0, protect_running=protect))
        env = make(False)
        env.run("sap_ff", 10, auto_reset=True)   # (the first launch of a handle pays for loading the kernel)
        env.reset(only_episode_counters=False)
        env.synchronize()
        t0 = time.perf_counter()
        env.run("sap_ff", args.steps, auto_reset=True)
        env.synchronize()
        launch = time.perf_counter() - t0
        B, Q = env.batch_size, env.queue_capacity
        bufs = {k: torch.zeros((B, Q), dtype=torch.float64, device="cuda") for k in env.AUDIT_SERVICE_FIELDS}
        bufs["summary"] = torch.zeros((B, 24), dtype=torch.uint8, device="cuda")
        mask = torch.zeros(env.action_mask_shape("path_ff_gn")[0], dtype=torch.uint8, device="cuda")
        calls = {"qot_audit": lambda: env.qot_audit(),
                 "qot_audit+services": lambda: env.qot_audit(out=bufs),
                 "path_ff_gn": lambda: env.action_masks("path_ff_gn", out=mask)}
        times = {k: [] for k in calls}
        for rep in range(args.warmup + args.repeats):
            for k, call in calls.items():
                t0 = time.perf_counter()
                call()
                env.synchronize()
                if rep >= args.warmup:
                    times[k].append(time.perf_counter() - t0)
        rec = {"queue_capacity": Q, "kernel": env.last_kernel(), "gated_launch_seconds": launch,
               "seconds": {k: {"value": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}}
        rec["in_path_ff_gn_calls"] = {k: v["value"] / rec["seconds"]["path_ff_gn"]["value"] for k, v in rec["seconds"].items()}
        rec["in_gated_launches"] = {k: v["value"] / launch for k, v in rec["seconds"].items()}
        rec["found_gated"] = found(env)
        env.close()
        prot = make(True)
        prot.run("sap_ff", args.steps, auto_reset=True)
        rec["found_protecting"] = found(prot)
        prot.close()
        out["load_%d" % load] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
