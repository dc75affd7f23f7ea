#!/usr/bin/env python3
"""What the blocking cause costs (include/orlg.h orlg_step_diag): NSFNET-320, load 50, sap_ff, 1000 steps per launch --
B = 4096 on the wave-per-environment kernel and B = 65 536 on the four-environments-per-wave kernel.  Per kernel three handles on
the same seeds, alternating launch by launch so that they share whatever else the machine does: `plain` (no cause output: the
launch every user ran before), `plain_kind` (the same without the deferred link statistics, ORLG_NO_DEFER: the kind of
instantiation a cause launch runs, without the classifier -- what separates the classifier's cost from that of the optimisations a
cause launch does without), `counts` (cause_counts only), `per_step` (cause_counts and block_cause, into device buffers).
Prints one JSON line: env-steps/s of each (median of the repeats, with their range), the kernel each ran, and from one more
launch the share of steps that are refused and the share of wave-steps that run the classifier (a wave of the group kernel runs
it when any of its four environments refuses).  On a library without orlg_step_diag only `plain` is measured: the same command
gives the parent's figure.  usage: python tools/bench_block_cause.py [--kernels wave,group] [--steps K] [--repeats R]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCH = {"wave": 4096, "group": 65536}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", default="wave,group")
    ap.add_argument("--batch", type=int, default=0, help="0: 4096 on the wave kernel, 65536 on the group kernel")
    ap.add_argument("--steps", type=int, default=1000, help="steps per launch")
    ap.add_argument("--warmup", type=int, default=2, help="launches before the timed ones")
    ap.add_argument("--repeats", type=int, default=7, help="timed launches per handle")
    ap.add_argument("--load", type=float, default=50)
    ap.add_argument("--policy", default="sap_ff")
    args = ap.parse_args()
    import numpy as np
    import torch
    from conftest import load_topology
    from optical_rl_gym_amd import BatchedRMSAEnv, _lib
    has_cause = "orlg_step_diag" in _lib.EXPORTED_SYMBOLS
    topo = load_topology("nsfnet_chen_5-paths_6-modulations")
    kw = dict(num_spectrum_resources=320, load=args.load, mean_service_holding_time=25, episode_length=1000, seed=10)
    out = {"metric": f"env steps/s, RMSA NSFNET-320 load {args.load:g} {args.policy}, blocking cause", "steps_per_launch": args.steps,
           "repeats": args.repeats, "cause_outputs": has_cause}
    for kernel in args.kernels.split(","):
        batch = args.batch or BATCH[kernel]
        modes = ("plain", "plain_kind", "counts", "per_step") if has_cause else ("plain", "plain_kind")
        envs = {m: BatchedRMSAEnv(topo, batch, step_kernel=kernel, **kw) for m in modes}
        counts = torch.zeros((batch, 8), dtype=torch.int32, device="cuda")
        cause = torch.zeros((args.steps, batch), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        run_kw = {"plain": {}, "plain_kind": {}, "counts": dict(cause_counts=counts),
                  "per_step": dict(cause_counts=counts, out={"block_cause": cause})}

        def launch(m):
            if m == "plain_kind":   # (the library reads its tooling variables at every launch)
                os.environ["ORLG_NO_DEFER"] = "1"
            try:
                envs[m].run(args.policy, args.steps, auto_reset=True, **run_kw[m])
                envs[m].synchronize()
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
        if has_cause:
            for m in ("counts", "per_step"):
                res[m]["relative_to_plain"] = res[m]["value"] / res["plain"]["value"]
                res[m]["relative_to_plain_kind"] = res[m]["value"] / res["plain_kind"]["value"]
            launch("per_step")   # (not timed: the steady state the timed launches ran in)
            c = cause.cpu().numpy()
            refused = c != 0
            res["share_steps_refused"] = float(refused.mean())
            rows = 4 if kernel == "group" else 1
            res["share_wave_steps_classified"] = float(refused[:, :batch - batch % rows].reshape(args.steps, -1, rows).any(axis=2).mean())
            res["cause_counts"] = np.bincount(c.ravel(), minlength=8).tolist()
        for env in envs.values():
            env.close()
        out[kernel] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
