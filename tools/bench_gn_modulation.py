#!/usr/bin/env python3
"""What adaptive modulation behind the GN gate costs and what it buys (include/orlg.h orlg_step_modulation), in ONE run.
NSFNET-320, B = 4096, at loads 50 and 150 and at 0 and +6 dBm per 50 GHz, every measurement from the state after --steps steps of
sap_ff_am on an adaptive handle (saved once, loaded before every timed launch).  Per (load, power):
    fused   milliseconds per step of ONE launch of --launch-steps steps of sap_ff_am (median of --repeats launches)
    loop    the loop it replaces, per step: modulation_windows() into pinned buffers, the walk on the host (vectorised), and
            run("external_am", 1) with the actions in pinned memory, over --loop-steps steps (median of --repeats)
    gated   sap_ff_gn on a plain gated handle of the same seeds, from its own state after --steps steps, the same launch
    query   one modulation_windows() call beside one action_masks("path_ff_gn") call of the plain gated handle
    accepted share of both, and the mean number of candidates with a window per step of the adaptive rule's walk (from the query)
Prints one JSON line.
usage: python tools/bench_gn_modulation.py [--repeats R] [--steps K] [--launch-steps N] [--loop-steps M] [--batch B]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def host_walk(slot, admitted, S, K):
    """sap_ff_am on the query's rows, vectorised: (actions [B, 3] int32, candidates the walk checks [B])"""
    import numpy as np
    B, _, M = slot.shape
    has = (slot < S)[:, :, ::-1].reshape(B, K * M)          # candidates in walk order: path 0 levels M..1, path 1 ...
    adm = (admitted != 0)[:, :, ::-1].reshape(B, K * M) & has
    s = slot[:, :, ::-1].reshape(B, K * M)
    first_adm, first_has = np.argmax(adm, axis=1), np.argmax(has, axis=1)
    pick = np.where(adm.any(axis=1), first_adm, first_has)
    rows = np.arange(B)
    none = ~has.any(axis=1)
    acts = np.stack([np.where(none, K, pick // M), np.where(none, S, s[rows, pick]), np.where(none, 0, M - pick % M)], axis=1)
    # the walk checks every candidate with a window up to the admitted one (all of them when none is admitted)
    upto = np.where(adm.any(axis=1), first_adm + 1, K * M)
    checks = (np.cumsum(has, axis=1)[rows, upto - 1])
    return acts.astype(np.int32), checks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1000, help="steps before the measurements")
    ap.add_argument("--launch-steps", type=int, default=200)
    ap.add_argument("--loop-steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--loads", type=int, nargs="+", default=[50, 150])
    ap.add_argument("--powers", type=float, nargs="+", default=[0.0, 6.0])
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.zeros(1, device="cuda")   # (torch creates its HIP context before the library does)
    from conftest import load_topology
    from optical_rl_gym_amd import BatchedRMSAEnv, rmsa_gn_gate_parameters
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    out = {"metric": "adaptive modulation: one fused launch of sap_ff_am against the query + host walk + external_am loop", "batch": args.batch,
           "repeats": args.repeats, "steps": args.steps, "launch_steps": args.launch_steps, "loop_steps": args.loop_steps}
    med = statistics.median
    for load in args.loads:
        for dbm in args.powers:
            make = lambda mode: BatchedRMSAEnv(topo, args.batch, num_spectrum_resources=320, load=load, mean_service_holding_time=25,
                                               episode_length=1000, seed=10,
                                               gn_gate=rmsa_gn_gate_parameters(topo, launch_power_dbm_per_50ghz=dbm, modulation=mode))
            env, plain = make("adaptive"), make("path")
            B, K, S, M = env.batch_size, env.k_paths, env.num_spectrum_resources, env.modulation_levels
            acc_a = env.run("sap_ff_am", args.steps, outputs=("accepted",), auto_reset=True)["accepted"].mean()
            acc_p = plain.run("sap_ff_gn", args.steps, outputs=("accepted",), auto_reset=True)["accepted"].mean()
            env.synchronize(); plain.synchronize()
            state, pstate = env.save_state(), plain.save_state()
            pin = lambda shape, dt: torch.zeros(shape, dtype=dt).pin_memory()
            slot_t, gsnr_t, adm_t, best_t = pin((B, K, M), torch.int16), pin((B, K, M), torch.float64), pin((B, K, M), torch.uint8), pin((B, K), torch.uint8)
            acts_t = pin((B, 3), torch.int32)
            checks = []

            def loop(n):
                for _ in range(n):
                    env.modulation_windows(slot_out=slot_t, gsnr_out=gsnr_t, admitted_out=adm_t, best_se_out=best_t)
                    env.synchronize()
                    acts, c = host_walk(slot_t.numpy(), adm_t.numpy(), S, K)
                    checks.append(float(c.mean()))
                    acts_t.numpy()[:] = acts
                    env.run("external_am", 1, actions=acts_t, auto_reset=True)
                env.synchronize()

            fused, looped, gated, query, mask = [], [], [], [], []
            for rep in range(args.repeats + 1):   # (the first round warms up)
                env.load_state(state)
                t0 = time.perf_counter()
                env.run("sap_ff_am", args.launch_steps, auto_reset=True)
                env.synchronize()
                t1 = time.perf_counter()
                kernel = env.last_kernel().split(" ")[0]
                env.load_state(state)
                t2 = time.perf_counter()
                loop(args.loop_steps)
                t3 = time.perf_counter()
                plain.load_state(pstate)
                t4 = time.perf_counter()
                plain.run("sap_ff_gn", args.launch_steps, auto_reset=True)
                plain.synchronize()
                t5 = time.perf_counter()
                env.modulation_windows(slot_out=slot_t, gsnr_out=gsnr_t, admitted_out=adm_t, best_se_out=best_t)
                env.synchronize()
                t6 = time.perf_counter()
                plain.action_masks("path_ff_gn")
                plain.synchronize()
                t7 = time.perf_counter()
                if rep:
                    fused.append((t1 - t0) / args.launch_steps); looped.append((t3 - t2) / args.loop_steps)
                    gated.append((t5 - t4) / args.launch_steps); query.append(t6 - t5); mask.append(t7 - t6)
            out["load_%d_%+gdbm" % (load, dbm)] = {
                "fused_ms_per_step": 1e3 * med(fused), "fused_min_ms": 1e3 * min(fused), "fused_max_ms": 1e3 * max(fused),
                "loop_ms_per_step": 1e3 * med(looped), "loop_min_ms": 1e3 * min(looped), "loop_max_ms": 1e3 * max(looped),
                "loop_over_fused": med(looped) / med(fused), "sap_ff_gn_ms_per_step": 1e3 * med(gated),
                "modulation_windows_ms": 1e3 * med(query), "path_ff_gn_mask_ms": 1e3 * med(mask),
                "accepted_share_adaptive": float(acc_a), "accepted_share_sap_ff_gn": float(acc_p),
                "mean_checks_per_step": float(np.mean(checks)), "kernel": kernel}
            env.close(); plain.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
