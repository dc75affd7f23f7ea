#!/usr/bin/env python3
"""What the GN-model admission check over the whole spectrum costs (include/orlg.h orlg_gn_admission_slots), in ONE run
with the calls alternating so that they share whatever else the machine does.  NSFNET-320 at +6 dBm per 50 GHz, B = 4096, at load
50 and load 150, after --steps steps of sap_ff on a gated and on a protecting handle (protect_running=True).  Per load the time of
one call (median of the repeats, the stream synchronised after each), every output into a device buffer:
    slots_mask            admission_slot_masks(), the mask alone, protecting handle
    slots_rows            admission_slot_masks() with its GSNR and margin rows, protecting handle
    max_margin            max_margin_windows(), protecting handle
    slots_mask_gated / slots_rows_gated / max_margin_gated   the same on the gated handle: the second check does not run
    admission_path_ff     admission_masks("path_ff") with its rows on the protecting handle: the first yardstick (k windows)
    qot_audit             qot_audit() on the protecting handle, the [B] summaries read back: the second yardstick
Beside them the free windows a call evaluates (hence ns per window), and what the rows say: the share of free windows refused by
their own check and by the neighbour check, and the share of paths with a window whose best window is not their first free one.
Prints one JSON line.
usage: python tools/bench_gn_admission_slots.py [--repeats R] [--warmup W] [--steps K] [--batch B]"""
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
    import numpy as np
    import torch
    torch.zeros(1, device="cuda")   # (torch creates its HIP context before the library does)
    from conftest import load_topology
    from optical_rl_gym_amd import BatchedRMSAEnv, rmsa_gn_gate_parameters
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    out = {"metric": "seconds per call (median), GN admission check over every start slot of every path",
           "repeats": args.repeats, "batch": args.batch, "steps": args.steps}
    for load in (50, 150):
        make = lambda protect: BatchedRMSAEnv(topo, args.batch, num_spectrum_resources=320, load=load, mean_service_holding_time=25,
                                              episode_length=1000, seed=10,
                                              gn_gate=rmsa_gn_gate_parameters(topo, launch_power_dbm_per_50ghz=6.0, protect_running=protect))
        gated, prot = make(False), make(True)
        for env in (gated, prot):
            env.run("sap_ff", args.steps, auto_reset=True)
            env.synchronize()
        B, K, S, W = prot.batch_size, prot.k_paths, prot.num_spectrum_resources, prot.words_per_link
        dev = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        bufs = lambda: dict(out=dev((B, K, W), torch.uint64), gsnr_out=dev((B, K, S), torch.float64), margin_out=dev((B, K, S), torch.float64))
        best = lambda: dict(slots_out=dev((B, K), torch.int16), margin_out=dev((B, K), torch.float64))
        rows_p, rows_g, best_p, best_g = bufs(), bufs(), best(), best()
        ff = dict(out=dev((B, K + prot.reject_action), torch.uint8), gsnr_out=dev((B, K), torch.float64), margin_out=dev((B, K), torch.float64))
        calls = {"slots_mask": (prot, lambda: prot.admission_slot_masks(out=rows_p["out"])),
                 "slots_rows": (prot, lambda: prot.admission_slot_masks(**rows_p)),
                 "max_margin": (prot, lambda: prot.max_margin_windows(**best_p)),
                 "slots_mask_gated": (gated, lambda: gated.admission_slot_masks(out=rows_g["out"])),
                 "slots_rows_gated": (gated, lambda: gated.admission_slot_masks(**rows_g)),
                 "max_margin_gated": (gated, lambda: gated.max_margin_windows(**best_g)),
                 "admission_path_ff": (prot, lambda: prot.admission_masks("path_ff", **ff)),
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
        for name, env, rows, bst in (("protecting", prot, rows_p, best_p), ("gated", gated, rows_g, best_g)):
            env.admission_slot_masks(**rows)
            env.max_margin_windows(**bst)
            env.synchronize()   # (the library's stream is not torch's)
            g, mg = rows["gsnr_out"].cpu().numpy(), rows["margin_out"].cpu().numpy()
            bits = np.unpackbits(rows["out"].cpu().numpy().view(np.uint8), axis=-1, bitorder="little")[..., :S].astype(bool)
            window = np.isfinite(g)
            n_win = int(window.sum())
            has = window.any(axis=-1)
            first = np.argmax(window, axis=-1)
            slots = bst["slots_out"].cpu().numpy()
            rec["found_" + name] = {
                "mean_n_running": float(env.num_running().mean()), "free_windows": n_win, "windows_per_env": n_win / B,
                "share_own_refused": float((window & ~bits & ~(mg < 0)).sum() / max(n_win, 1)),
                "share_neighbour_refused": float((mg < 0).sum() / max(n_win, 1)),
                "paths_with_an_admitted_window": int((slots < S).sum()),
                "share_best_not_first_free": float(((slots < S) & (slots != first)).sum() / max(int((slots < S).sum()), 1)),
                "paths_with_a_window_and_none_admitted": int((has & (slots == S)).sum())}
            for k in ("slots_mask", "slots_rows", "max_margin"):
                key = k if name == "protecting" else k + "_gated"
                rec["found_" + name]["ns_per_window_" + k] = 1e9 * rec["seconds"][key]["value"] / max(n_win, 1)
        gated.close()
        prot.close()
        out["load_%d" % load] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
