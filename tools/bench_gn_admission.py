#!/usr/bin/env python3
"""What the action masks and rule windows that know both halves of the GN-model admission check cost (include/orlg.h
orlg_gn_admission_masks / orlg_gn_admission_windows), in ONE run with the calls alternating so that they share whatever
else the machine does.  NSFNET-320 at +6 dBm per 50 GHz, B = 4096, at load 50 and load 150, after --steps steps of sap_ff on a gated
and on a protecting handle (protect_running=True).  Per load the time of one call (median of the repeats, the stream synchronised
after each), every output into a device buffer:
    admission_path_ff     admission_masks("path_ff") with its GSNR and margin rows, protecting handle
    admission_deeprmsa    admission_masks("deeprmsa") with its rows, protecting handle
    admission_best        admission_windows("best"), protecting handle
    admission_path_ff_gated   admission_masks("path_ff") with its rows on the gated handle: the second check does not run
    path_ff_gn            action_masks("path_ff_gn") with its GSNR row on the gated handle: the first yardstick
    qot_audit             qot_audit() on the protecting handle, the [B] summaries read back: the second yardstick
and the ratios to the two yardsticks.  Beside them what the protected masks say: the share of first-fit candidates that pass their
own check and are refused by the neighbour check, and the share of environments whose protected mask differs from the mask of
the candidate's own check alone.  Prints one JSON line.
usage: python tools/bench_gn_admission.py [--repeats R] [--warmup W] [--steps K] [--batch B]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=25, help="timed calls of each kind")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1000, help="steps of sap_ff before the queries")
    ap.add_argument("--batch", type=int, default=4096)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")   # (torch creates its HIP context before the library does)
    from conftest import load_topology
    from optical_rl_gym_amd import BatchedRMSAEnv, rmsa_gn_gate_parameters
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    out = {"metric": "seconds per call (median), masks and rule windows behind both halves of the GN admission check",
           "repeats": args.repeats, "batch": args.batch, "steps": args.steps}
    for load in (50, 150):
        make = lambda protect: BatchedRMSAEnv(topo, args.batch, num_spectrum_resources=320, load=load, mean_service_holding_time=25,
                                              episode_length=1000, seed=10,
                                              gn_gate=rmsa_gn_gate_parameters(topo, launch_power_dbm_per_50ghz=6.0, protect_running=protect))
        gated, prot = make(False), make(True)
        for env in (gated, prot):
            env.run("sap_ff", args.steps, auto_reset=True)
            env.synchronize()
        B, K = prot.batch_size, prot.k_paths
        dev = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        ff = dict(out=dev((B, K + prot.reject_action), torch.uint8), gsnr_out=dev((B, K), torch.float64), margin_out=dev((B, K), torch.float64))
        deep = dict(out=dev((B, K * prot.j + prot.reject_action), torch.uint8), gsnr_out=dev((B, K * prot.j), torch.float64),
                    margin_out=dev((B, K * prot.j), torch.float64))
        win = dict(slots_out=dev((B, K), torch.int16), gsnr_out=dev((B, K), torch.float64), margin_out=dev((B, K), torch.float64),
                   admitted_out=dev((B, K), torch.uint8))
        old = dict(out=dev((B, K + gated.reject_action), torch.uint8), gsnr_out=dev((B, K), torch.float64))
        ffg = dict(out=dev((B, K + gated.reject_action), torch.uint8), gsnr_out=dev((B, K), torch.float64), margin_out=dev((B, K), torch.float64))
        calls = {"admission_path_ff": (prot, lambda: prot.admission_masks("path_ff", **ff)),
                 "admission_deeprmsa": (prot, lambda: prot.admission_masks("deeprmsa", **deep)),
                 "admission_best": (prot, lambda: prot.admission_windows("best", **win)),
                 "admission_path_ff_gated": (gated, lambda: gated.admission_masks("path_ff", **ffg)),
                 "path_ff_gn": (gated, lambda: gated.action_masks("path_ff_gn", **old)),
                 "qot_audit": (prot, lambda: prot.qot_audit())}
        times = {k: [] for k in calls}
        for rep in range(args.warmup + args.repeats):
            for k, (env, call) in calls.items():
                t0 = time.perf_counter()
                call()
                env.synchronize()
                if rep >= args.warmup:
                    times[k].append(time.perf_counter() - t0)
        rec = {"queue_capacity": prot.queue_capacity,
               "seconds": {k: {"value": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}}
        for yard in ("path_ff_gn", "qot_audit"):
            rec["in_%s_calls" % yard] = {k: v["value"] / rec["seconds"][yard]["value"] for k, v in rec["seconds"].items()}
        res = prot.admission_masks("path_ff", **ff)
        prot.synchronize()   # (the library's stream is not torch's)
        m, g, mg = (a.cpu().numpy() for a in res)
        own = (g >= 0) | (g < 0)   # a window exists
        thr_ok = own & ((m[:, :K] == 1) | (mg < 0))   # ... and passed its own check
        rec["found"] = {"mean_n_running": float(prot.num_running().mean()), "first_fit_windows": int(own.sum()),
                        "pass_own_check": int(thr_ok.sum()), "neighbour_refused": int((mg < 0).sum()),
                        "share_neighbour_refused": float((mg < 0).sum() / max(int(thr_ok.sum()), 1)),
                        "envs_whose_mask_differs": float((mg < 0).any(axis=1).mean())}
        gated.close()
        prot.close()
        out["load_%d" % load] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
