#!/usr/bin/env python3
"""What max-margin assignment inside the step costs and what it buys (include/orlg.h orlg_step_max_margin), in ONE run.
NSFNET-320 at +6 dBm per 50 GHz, B = 4096, at load 50 and load 150, on a gated and on a protecting handle (protect_running=True),
from the state after --steps steps of sap_ff (every measurement starts from that saved state).  Per load, handle and route
(sap_mm, any_mm):
    fused   env-steps/s and seconds per step of ONE launch of --launch-steps steps (median of --repeats launches)
    loop    the loop it replaces, per step: max_margin_windows() into pinned buffers, the rule on the host, run("external", 1) with the
            actions in pinned memory -- code the library had before this entry -- over --loop-steps steps (median of --repeats)
path_mm_external is a launch per step by definition: its row is the fused step against the same loop with the path given.
Then what the rule buys: --quality-steps steps of sap_ff, sap_ff_gn, sap_mm and any_mm from a fresh handle of the same seeds -- the
share of requests accepted, qot_audit()'s n_below / n_running and min_margin_db, and the share of steps that were fallbacks.
Prints one JSON line.
usage: python tools/bench_gn_max_margin.py [--repeats R] [--steps K] [--launch-steps N] [--loop-steps M] [--quality-steps Q] [--batch B]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def host_rule(slots, margin, first_free, S, K, route, given=None):
    """the rule of the three routes on the query's rows, vectorised: actions [B, 2] int32"""
    import numpy as np
    B = slots.shape[0]
    has, free = slots < S, first_free < S
    if route == "path":
        rows = np.arange(B)
        ok = (given >= 0) & (given < K)
        g = np.where(ok, given, 0)
        p = np.where(ok & (has[rows, g] | free[rows, g]), g, K)
        s = np.where(p < K, np.where(has[rows, g], slots[rows, g], first_free[rows, g]), S)
        return np.stack([p, s], axis=1).astype(np.int32)
    if route == "any":
        best = np.argmax(np.where(has, margin, -np.inf), axis=1)   # the first of the largest: ties go to the lowest index
    else:
        best = np.argmax(has, axis=1)
    fb = np.argmax(free, axis=1)
    rows = np.arange(B)
    p = np.where(has.any(axis=1), best, np.where(free.any(axis=1), fb, K))
    q = np.minimum(p, K - 1)
    s = np.where(has.any(axis=1), slots[rows, q], np.where(free.any(axis=1), first_free[rows, q], S))
    return np.stack([p, s], axis=1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1000, help="steps of sap_ff before the measurements")
    ap.add_argument("--launch-steps", type=int, default=200)
    ap.add_argument("--loop-steps", type=int, default=20)
    ap.add_argument("--quality-steps", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--loads", type=int, nargs="+", default=[50, 150])
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.zeros(1, device="cuda")   # (torch creates its HIP context before the library does)
    from conftest import load_topology
    from optical_rl_gym_amd import BatchedRMSAEnv, rmsa_gn_gate_parameters
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    out = {"metric": "max-margin assignment: one fused launch against the query + host rule + external step loop", "batch": args.batch,
           "repeats": args.repeats, "steps": args.steps, "launch_steps": args.launch_steps, "loop_steps": args.loop_steps,
           "quality_steps": args.quality_steps}
    for load in args.loads:
        make = lambda protect: BatchedRMSAEnv(topo, args.batch, num_spectrum_resources=320, load=load, mean_service_holding_time=25,
                                              episode_length=1000, seed=10,
                                              gn_gate=rmsa_gn_gate_parameters(topo, launch_power_dbm_per_50ghz=6.0, protect_running=protect))
        rec = {}
        for kind, protect in (("gated", False), ("protecting", True)):
            env = make(protect)
            B, K, S = env.batch_size, env.k_paths, env.num_spectrum_resources
            env.run("sap_ff", args.steps, auto_reset=True)
            env.synchronize()
            state = env.save_state()
            pin = lambda shape, dt: torch.zeros(shape, dtype=dt).pin_memory()
            slots_t, margin_t, acts_t = pin((B, K), torch.int16), pin((B, K), torch.float64), pin((B, 2), torch.int32)
            given = np.random.default_rng(1).integers(0, K, size=B).astype(np.int32)
            given_t = pin((B,), torch.int32)
            given_t.numpy()[:] = given

            def loop(route, n):
                for _ in range(n):
                    env.max_margin_windows(slots_out=slots_t, margin_out=margin_t)
                    window = np.unpackbits(env.action_masks("slots").view(np.uint8), axis=-1, bitorder="little")[..., :S].astype(bool)
                    env.synchronize()
                    first_free = np.where(window.any(axis=-1), np.argmax(window, axis=-1), S)
                    acts_t.numpy()[:] = host_rule(slots_t.numpy(), margin_t.numpy(), first_free, S, K, route, given)
                    env.run("external", 1, actions=acts_t, auto_reset=True)
                env.synchronize()

            rows = {}
            for name, route in (("sap_mm", "sap"), ("any_mm", "any"), ("path_mm_external", "path")):
                fused, looped = [], []
                n_fused = args.launch_steps if route != "path" else args.loop_steps
                for rep in range(args.repeats + 1):   # (the first pair warms up)
                    env.load_state(state)
                    t0 = time.perf_counter()
                    if route != "path":
                        env.run(name, n_fused, auto_reset=True)
                    else:
                        for _ in range(n_fused):
                            env.run(name, 1, actions=given_t, auto_reset=True)
                    env.synchronize()
                    t1 = time.perf_counter()
                    kernel = env.last_kernel().split(" ")[0]
                    env.load_state(state)
                    t2 = time.perf_counter()
                    loop(route, args.loop_steps)
                    t3 = time.perf_counter()
                    if rep:
                        fused.append((t1 - t0) / n_fused)
                        looped.append((t3 - t2) / args.loop_steps)
                f, l = statistics.median(fused), statistics.median(looped)
                rows[name] = {"fused_seconds_per_step": f, "fused_env_steps_per_s": B / f, "fused_min": min(fused), "fused_max": max(fused),
                              "loop_seconds_per_step": l, "loop_env_steps_per_s": B / l, "loop_min": min(looped), "loop_max": max(looped),
                              "loop_over_fused": l / f, "kernel": kernel}
            env.close()
            rec[kind] = rows
            # what the rule buys: fresh handles of the same seeds
            quality = {}
            for policy in ("sap_ff", "sap_ff_gn", "sap_mm", "any_mm"):
                env = make(protect)
                outs = ("accepted", "gn_gsnr_db")
                acc = refused_by_gate = 0
                left = args.quality_steps
                while left:
                    n = min(left, 250)
                    r = env.run(policy, n, outputs=outs, auto_reset=True)
                    a = r["accepted"].astype(bool)
                    acc += int(a.sum())
                    refused_by_gate += int((~a & np.isfinite(r["gn_gsnr_db"])).sum())
                    left -= n
                audit = env.qot_audit()
                total = args.quality_steps * B
                quality[policy] = {"accepted_share": acc / total, "gate_refusal_share": refused_by_gate / total,
                                   "n_below_over_n_running": float(audit["n_below"].sum() / max(int(audit["n_running"].sum()), 1)),
                                   "min_margin_db": float(np.nanmin(audit["min_margin_db"])), "mean_n_running": float(audit["n_running"].mean())}
                env.close()
            rec[kind + "_quality"] = quality
        out["load_%d" % load] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
